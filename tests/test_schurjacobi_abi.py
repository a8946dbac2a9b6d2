"""(CPU) NLLS_PCG_PRECOND_SCHUR_JACOBI and nlls_schur_block_diag through every layer: declared in include/nlls_amd.h, exported by the library and by the libraries built
with a user header, bound in _capi, forwarded by the linear system, on N.SchurOperator, selected by N.PCG(precond="schurjacobi", schur=True), named by the shim -- and
refused without a context.  The pattern of tests/test_schur_abi.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import _capi, iterators, linearsystem, optimizer
from nllssolver_jl_amd.callbacks import nullcallback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nllssolver.jl_amd", "csrc")


def test_header_declares_the_constant_and_the_function():
    h = open(os.path.join(ROOT, "include", "nlls_amd.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"^#define\s+NLLS_PCG_PRECOND_SCHUR_JACOBI\s+3\s*$", bare, flags=re.M)
    assert not re.search(r"^#define\s+NLLS_PCG_PRECOND_\w+\s+2\s*$", bare, flags=re.M), "2 stays unassigned: the refusal tests of the four entry points hold it"
    assert re.search(r"\bint\s+nlls_schur_block_diag\s*\(nlls_ctx\* ctx, int32_t which, double lambda, double\* d_out\s*\)", bare)
    assert "unassigned" in h[h.index("NLLS_PCG_PRECOND_BLOCK_JACOBI  1"):h.index("NLLS_PCG_PRECOND_SCHUR_JACOBI  3")]
    doc = h[h.rindex("/* ----", 0, h.index("nlls_schur_block_diag(nlls_ctx*")):h.index("nlls_schur_block_diag(nlls_ctx*")]
    assert "S_ii = B_ii + lambda I - sum_e E_ie (C_e + lambda I)^-1 E_ie'" in doc and "NLLS_ERR_NOT_SPD" in doc and "unfactored" in doc
    assert ctypes.sizeof(_capi.Info) == 112 and "[56]" not in h          # nlls_info keeps its size, nlls_get_solve_stats gained no index


def test_library_and_binding_carry_the_name():
    L = _capi.lib(); i32, dbl, vp = ctypes.c_int32, ctypes.c_double, ctypes.c_void_p
    assert hasattr(L, "nlls_schur_block_diag") and "nlls_schur_block_diag" in _capi.SYMBOLS
    assert L.nlls_schur_block_diag.argtypes == [vp, i32, dbl, vp]
    assert _capi.PCG_PRECOND_SCHUR_JACOBI == 3 and _capi.PCG_PRECONDS["schurjacobi"] == 3
    assert _capi.PCG_PRECONDS["blockjacobi"] == 1 and _capi.PCG_PRECONDS["none"] == 0 and 2 not in _capi.PCG_PRECONDS.values()
    for name in ("userdemo", "uservar", "userrobust"):
        lib = os.path.join(CSRC, f"libnlls_amd_{name}.so")
        assert os.path.exists(lib), "run __graft_entry__.build()"
        assert hasattr(ctypes.CDLL(lib), "nlls_schur_block_diag"), name


def test_a_null_context_is_an_argument_error_and_writes_nothing():
    L = _capi.lib(); out = np.full(4, 7.25); st = np.full(8, 7.25)
    assert L.nlls_schur_block_diag(None, 0, 0.0, _capi._p(out)) == _capi.ERR_INVALID_ARG
    assert L.nlls_solve_pcg_schur(None, _capi.PCG_PRECOND_SCHUR_JACOBI, 10, 1e-8, _capi._p(out), _capi._p(st)) == _capi.ERR_INVALID_ARG
    assert np.all(out == 7.25) and np.all(st == 7.25)


def test_the_entry_point_sits_between_the_guard_pair():
    src = open(os.path.join(CSRC, "nlls_capi.cpp")).read()
    heads = dict(re.findall(r"^int\s+(nlls_\w+)\([^\n]*\)\s*\{([^\n]*)$", src, flags=re.M))
    assert "NLLS_API_BEGIN" in heads["nlls_schur_block_diag"]
    body = src[src.index("int nlls_schur_block_diag("):]; body = body[:body.index("\n}\n")]
    assert "NLLS_API_END(" in body.rstrip().splitlines()[-1]
    assert "schur_check(ctx" in body and "NLLS_ERR_NOT_SPD" in body


def test_python_layers():
    for cls in (_capi.Context, linearsystem.MultiVariateLSgpu):
        par = inspect.signature(cls.schur_block_diag).parameters
        assert list(par) == ["self", "lam", "which"] and par["lam"].default == 0.0 and par["which"].default == _capi.VARS_CURRENT, cls
    assert callable(N.SchurOperator.schur_diag_blocks) and callable(N.SchurOperator.diag_blocks)
    assert "hess_block_diag" in inspect.getsource(N.SchurOperator.diag_blocks), "diag_blocks keeps returning B's blocks"
    assert "schur_block_diag" in inspect.getsource(N.SchurOperator.schur_diag_blocks)
    doc = N.SchurOperator.__doc__
    assert "NOT S's" in doc and "schur_diag_blocks()" in doc and "a block-Jacobi preconditioner for S" not in doc
    assert "schurjacobi" in inspect.getsource(_capi.Context.solve_pcg_schur)


def test_pcg_accepts_the_name_on_the_reduced_system_only():
    with pytest.raises(ValueError):
        N.PCG(precond="schurjacobi")
    with pytest.raises(ValueError):
        N.PCG(precond="schurjacobi", schur=False)
    pc = N.PCG(precond="schurjacobi", schur=True)
    assert pc.precond == "schurjacobi" and pc.schur is True
    assert N.PCG().precond == "blockjacobi" and N.PCG(schur=True).precond == "blockjacobi"          # the default does not change


class _FakeContext:
    def lm_iterations(self, *a):
        raise AssertionError("the library's own loop has no conjugate gradients")


class _FakeLS:
    def __init__(self):
        self.ctx = _FakeContext(); self.calls = []; self.b = np.ones(2)

    def initlambda(self): return 1.0
    def uniformscaling(self, k): self.calls.append(("damp", k))
    def solve_pcg_schur(self, precond, maxiters, rtol): self.calls.append(("solve_pcg_schur", precond, maxiters, rtol))
    def update(self, to, frm): self.calls.append(("update",))
    def cost(self, which): return 0.5
    def step_maxabs(self): return 1.0
    def quadform(self): return 1.0, -1.0


def test_the_iterators_pass_the_name_on():
    data = optimizer.NLLSInternal(_FakeLS(), 0); data.bestcost = 1.0
    opt = N.NLLSOptions(linearsolver=N.PCG(rtol=1e-6, maxiters=9, schur=True, precond="schurjacobi"))
    iterators.iterate_levmar(iterators.LevMarData(), data, None, opt)
    assert data.linsystem.calls[1] == ("solve_pcg_schur", "schurjacobi", 9, 1e-6)
    with pytest.raises(ValueError):          # the trust region keeps refusing the reduced system
        iterators.iterate_steihaug(iterators.SteihaugData(), data, None, opt)


def test_julia_shim_and_tool_name_it():
    jl = open(os.path.join(ROOT, "nllssolver.jl_amd", "julia", "NLLSsolverAMD.jl")).read()
    for name in (":nlls_schur_block_diag", "function schurblockdiag!(", "PCG_PRECOND_SCHUR_JACOBI = 3"):
        assert name in jl, name
    tool = open(os.path.join(ROOT, "tools", "pcg_only.py")).read()
    assert "schurjacobi" in tool and "--precond" in tool
