"""(CPU) nlls_solve_pcg_rhs and nlls_marginal_cov through every layer: declared in include/nlls_amd.h with their signatures, exported by the library and by the
libraries built with a user header, bound in _capi with ten argtypes each, forwarded by the linear system, on N.Solver / N.marginalcovariance / HessianOperator,
named by the shim -- and refused without a context.  The pattern of tests/test_pcg_abi.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import _capi, linearsystem, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nllssolver.jl_amd", "csrc")
RHS = r"\bint\s+nlls_solve_pcg_rhs\s*\(nlls_ctx\* ctx, int32_t which, double lambda, int32_t precond, int32_t maxiters, double rtol,\s*int32_t nrhs, const double\* B, double\* X_out, double\* stats_out\)"
COV = r"\bint\s+nlls_marginal_cov\s*\(nlls_ctx\* ctx, int32_t which, double lambda, int64_t nsel, const int64_t\* varindices,\s*int32_t precond, int32_t maxiters, double rtol, double\* cov_out, double\* stats_out\)"


def test_header_declares_both_with_their_signatures():
    h = open(os.path.join(ROOT, "include", "nlls_amd.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(RHS, bare) and re.search(COV, bare)
    for name in ("nlls_solve_pcg_rhs(nlls_ctx*", "nlls_marginal_cov(nlls_ctx*"):
        decl = h.index(name)
        assert decl > h.index("nlls_solve_pcg(nlls_ctx*") and "replaces:" in h[h.rindex("/*", 0, decl):decl], name
    cov = h[h.rindex("/*", 0, h.index("nlls_marginal_cov(nlls_ctx*")):h.index("nlls_marginal_cov(nlls_ctx*")]
    assert "NO covariance routine" in cov and "src/linearsystem.jl:91-118" in cov and "fixed variables" in cov and "lambda" in cov
    assert "src/linearsolver.jl:20-32" in h
    # nlls_get_solve_stats and nlls_get_phase_times gained no index: the counters keep describing the last nlls_solve_pcg
    assert "[53] iterations made" in h and "[14] milliseconds of the last nlls_solve_pcg" in h and "[56]" not in h


def test_library_and_binding_carry_both_names():
    L = _capi.lib()
    for name in ("nlls_solve_pcg_rhs", "nlls_marginal_cov"):
        assert hasattr(L, name) and name in _capi.SYMBOLS and len(getattr(L, name).argtypes) == 10, name
    i32, i64, dbl, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
    assert L.nlls_solve_pcg_rhs.argtypes == [vp, i32, dbl, i32, i32, dbl, i32, vp, vp, vp]
    assert L.nlls_marginal_cov.argtypes == [vp, i32, dbl, i64, vp, i32, i32, dbl, vp, vp]


def test_a_null_context_is_an_argument_error_and_writes_nothing():
    L = _capi.lib(); P = _capi._p
    B = np.ones(4); out = np.full(4, 7.25); st = np.full(12, 7.25); vi = np.array([1], np.int64)
    assert L.nlls_solve_pcg_rhs(None, 0, 0.0, 1, 10, 1e-8, 1, P(B), P(out), P(st)) == _capi.ERR_INVALID_ARG
    assert L.nlls_marginal_cov(None, 0, 0.0, 1, P(vi), 1, 10, 1e-8, P(out), P(st)) == _capi.ERR_INVALID_ARG
    assert np.all(out == 7.25) and np.all(st == 7.25)


def test_entry_points_sit_between_the_guard_pair():
    src = open(os.path.join(CSRC, "nlls_capi.cpp")).read()
    heads = dict(re.findall(r"^int\s+(nlls_\w+)\([^\n]*\)\s*\{([^\n]*)$", src, flags=re.M))
    for name in ("nlls_solve_pcg_rhs", "nlls_marginal_cov"):
        assert "NLLS_API_BEGIN" in heads[name], name
        body = src[src.index(f"int {name}("):]; body = body[:body.index("\n}\n")]
        assert body.rstrip().endswith("NLLS_API_END(ctx)"), name
    hip = open(os.path.join(CSRC, "nlls_pcg.hip")).read()
    assert "getenv" not in hip and "atomicAdd" not in hip and "__hip_atomic" not in hip and "hipFuncSetAttribute" not in hip
    assert "blockIdx.y" in hip and "hipHostMalloc" not in hip          # (the pinned mirror is PcgState's, nlls_ctx.hpp)
    assert "PinnedBuf h_scal" in open(os.path.join(CSRC, "nlls_ctx.hpp")).read()


def test_user_libraries_export_both():
    for name in ("userdemo", "uservar", "userrobust"):
        lib = os.path.join(CSRC, f"libnlls_amd_{name}.so")
        assert os.path.exists(lib), "run __graft_entry__.build()"
        L = ctypes.CDLL(lib)
        assert hasattr(L, "nlls_solve_pcg_rhs") and hasattr(L, "nlls_marginal_cov"), name


def test_python_signatures_and_defaults():
    for cls in (_capi.Context, linearsystem.MultiVariateLSgpu):
        par = inspect.signature(cls.solve_pcg_rhs).parameters
        assert list(par) == ["self", "B", "lam", "which", "precond", "maxiters", "rtol"], cls
        assert (par["lam"].default, par["which"].default, par["maxiters"].default, par["rtol"].default) == (0.0, _capi.VARS_CURRENT, None, 1e-8)
        par = inspect.signature(cls.marginal_cov).parameters
        assert list(par)[:3] == ["self", "varindices", "lam"] and par["lam"].default == 0.0 and par["maxiters"].default is None
    assert inspect.signature(_capi.Context.solve_pcg_rhs).parameters["precond"].default == 1
    assert "4 * int(self.info.ndof)" in inspect.getsource(_capi.Context.solve_pcg_rhs) and "last_pcg_rhs" in inspect.getsource(_capi.Context.solve_pcg_rhs)
    assert "last_pcg_rhs" in inspect.getsource(_capi.Context.marginal_cov)
    par = inspect.signature(N.Solver.solve_rhs).parameters
    assert list(par) == ["self", "B", "lam", "precond", "maxiters", "rtol"] and par["lam"].default == 0.0
    par = inspect.signature(N.Solver.covariance).parameters
    assert list(par) == ["self", "variables", "lam", "precond", "maxiters", "rtol", "strict"]
    assert (par["lam"].default, par["precond"].default, par["maxiters"].default, par["rtol"].default, par["strict"].default) == (0.0, "blockjacobi", None, 1e-10, True)
    par = inspect.signature(N.marginalcovariance).parameters
    assert list(par)[:5] == ["problem", "variables", "lam", "unfixed", "device"] and (par["lam"].default, par["unfixed"].default, par["device"].default) == (0.0, None, 0)
    assert N.marginalcovariance is optimizer.marginalcovariance
    assert list(inspect.signature(N.HessianOperator.solve).parameters)[:2] == ["self", "B"]


def test_stats_are_split_per_column():
    st = np.arange(16.0)                                            # three columns and the call's four
    d = _capi.Context._pcg_rhs_stats(st, 3)
    assert d["iterations"].tolist() == [0, 4, 8] and d["status"].tolist() == [1, 5, 9] and d["bnorm"].tolist() == [2.0, 6.0, 10.0] and d["rnorm"].tolist() == [3.0, 7.0, 11.0]
    assert (d["synchronisations"], d["launches"], d["product_vectors"], d["batches"]) == (12, 13, 14, 15)


class _FakeLS:
    """a linear system whose covariance solve ends one column on maxiters"""

    def __init__(self, status):
        self.status = np.asarray(status); self.calls = []

    def marginal_cov(self, varindices, lam, which, precond, maxiters, rtol):
        self.calls.append((list(varindices), lam, which, precond, maxiters, rtol)); m = self.status.size
        return np.eye(m), dict(iterations=np.full(m, 5), status=self.status, bnorm=np.ones(m), rnorm=np.full(m, 1e-3), synchronisations=1, launches=1, product_vectors=1, batches=1)


def _solver_on(ls):
    s = N.Solver.__new__(N.Solver); s.ls = ls; s._start = lambda: None
    return s


def test_covariance_is_strict_about_unconverged_columns():
    s = _solver_on(_FakeLS([0, 1, 0]))
    with pytest.raises(ValueError) as e:
        s.covariance([3, 1])
    assert "did not converge" in str(e.value) and "column 1" in str(e.value)
    assert s.ls.calls[0] == ([3, 1], 0.0, _capi.VARS_CURRENT, "blockjacobi", None, 1e-10)
    cov, st = s.covariance([3, 1], strict=False)
    assert cov.shape == (3, 3) and st["status"].tolist() == [0, 1, 0]
    cov, st = _solver_on(_FakeLS([0, 0, 0])).covariance([3, 1], lam=0.5, rtol=1e-9)
    assert cov.shape == (3, 3)


def test_julia_shim_names_both_entry_points():
    jl = open(os.path.join(ROOT, "nllssolver.jl_amd", "julia", "NLLSsolverAMD.jl")).read()
    for name in (":nlls_solve_pcg_rhs", ":nlls_marginal_cov", "function solvepcgrhs!(", "function marginalcov("):
        assert name in jl, name
