"""(CPU) nlls_solve_pcg_tr through every layer: declared in include/nlls_amd.h behind nlls_solve_pcg_schur, exported by the library and by the libraries built with a
user header, bound in _capi with its argtypes, forwarded by the linear system, driven by the fifth iterator N.steihaug, named by the shim -- and refused without a
context.  The pattern of tests/test_schur_abi.py."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import _capi, iterators, linearsystem, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nllssolver.jl_amd", "csrc")
NAME = "nlls_solve_pcg_tr"
DECL = r"\bint\s+nlls_solve_pcg_tr\s*\(nlls_ctx\* ctx, int32_t precond, int32_t maxiters, double rtol, double radius, double\* x_out, double\* stats_out\)"


def test_header_declares_it_behind_the_reduced_solve():
    h = open(os.path.join(ROOT, "include", "nlls_amd.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(DECL, bare)
    assert h.index(NAME + "(") > h.index("nlls_solve_pcg_schur(nlls_ctx*")
    doc = h[h.rindex("/* ----", 0, h.index(NAME + "(")):h.index(NAME + "(")]
    assert "replaces:" in doc and "src/iterators.jl:47-115" in doc and "NLLS_ERR_NOT_SPD" in doc and "NLLS_ERR_INVALID_ARG" in doc and "+inf" in doc
    for status in range(6):                                    # the six statuses, a line each
        assert re.search(rf"^ \*   {status}  \S", doc, flags=re.M), status
    # nlls_info keeps its size and nlls_get_solve_stats gained no index: the counters keep describing the last nlls_solve_pcg
    assert ctypes.sizeof(_capi.Info) == 112 and "[56]" not in h


def test_library_and_binding_carry_the_name():
    L = _capi.lib(); i32, dbl, vp = ctypes.c_int32, ctypes.c_double, ctypes.c_void_p
    assert hasattr(L, NAME) and NAME in _capi.SYMBOLS
    assert L.nlls_solve_pcg_tr.argtypes == [vp, i32, i32, dbl, dbl, vp, vp]
    for name in ("userdemo", "uservar", "userrobust"):
        lib = os.path.join(CSRC, f"libnlls_amd_{name}.so")
        assert os.path.exists(lib), "run __graft_entry__.build()"
        assert hasattr(ctypes.CDLL(lib), NAME), name


def test_a_null_context_is_an_argument_error_and_writes_nothing():
    L = _capi.lib(); P = _capi._p
    out = np.full(4, 7.25); st = np.full(8, 7.25)
    for radius in (1.0, np.inf, 0.0, -1.0, np.nan):
        assert L.nlls_solve_pcg_tr(None, 1, 10, 1e-8, radius, P(out), P(st)) == _capi.ERR_INVALID_ARG
    assert np.all(out == 7.25) and np.all(st == 7.25)


def test_entry_point_sits_between_the_guard_pair():
    src = open(os.path.join(CSRC, "nlls_capi.cpp")).read()
    heads = dict(re.findall(r"^int\s+(nlls_\w+)\([^\n]*\)\s*\{([^\n]*)$", src, flags=re.M))
    assert "NLLS_API_BEGIN" in heads[NAME]
    body = src[src.index(f"int {NAME}("):]; body = body[:body.index("\n}\n")]
    assert "NLLS_API_END(" in body.rstrip().splitlines()[-1]
    assert src.index(f"int {NAME}(") > src.index("int nlls_solve_pcg_schur(")
    assert "radius > 0.0" in body and body.index("radius > 0.0") < body.index("NEED_GRAD_LAZY")      # the radius is refused before anything is looked at or enqueued


def test_the_kernels_keep_their_launches_and_their_sums():
    """no new launch, no new partial sum, no atomics: the trust region lives in pcg_step_kernel and pcg_dir_kernel, and the stop flag is raised by the second"""
    pcg = open(os.path.join(CSRC, "nlls_pcg.hip")).read()
    assert len(re.findall(r"^__global__", pcg, flags=re.M)) == 10 and "atomic" not in pcg.replace("atomics", "") and "getenv" not in pcg
    step = pcg[pcg.index("void pcg_step_kernel("):pcg.index("void pcg_dir_kernel(")]; drv = pcg[pcg.index("void pcg_dir_kernel("):pcg.index("void pcg_finish_kernel(")]
    assert "PCG_EXIT" in step and "PCG_TAU" in step and "a.radius" in step
    boundary = step[step.rindex("if (ex) {"):]; boundary = boundary[:boundary.index("return;")]
    assert "PCG_STOP" not in boundary, "a late workgroup of the step launch would leave its share of y unwritten"
    assert "a.scal[PCG_STATUS] = a.scal[PCG_EXIT]; a.scal[PCG_STOP] = 1.0;" in drv
    ctxh = open(os.path.join(CSRC, "nlls_ctx.hpp")).read()
    for scalar in ("PCG_YY", "PCG_YP", "PCG_PP", "PCG_MODEL"):
        assert scalar in ctxh and scalar in drv, scalar
    assert ".radius = radius" in pcg and "double radius = INFINITY" in open(os.path.join(CSRC, "nlls_internal.hpp")).read()


def test_python_signatures_and_defaults():
    for cls in (_capi.Context, linearsystem.MultiVariateLSgpu):
        par = inspect.signature(cls.solve_pcg_tr).parameters
        assert list(par) == ["self", "radius", "precond", "maxiters", "rtol", "want_x"], cls
        assert par["maxiters"].default is None and par["rtol"].default == 1e-8 and par["want_x"].default is False
    assert inspect.signature(_capi.Context.solve_pcg_tr).parameters["precond"].default == 1
    assert "self._x = None" in inspect.getsource(linearsystem.MultiVariateLSgpu.solve_pcg_tr)
    src = inspect.getsource(_capi.Context.solve_pcg_tr)
    assert "last_pcg_tr" in src and "self.last_pcg =" not in src and "mnorm" in src and "model" in src and "4 * int(self.info.ndof)" in src
    assert _capi.PCG_STATUS[4] and _capi.PCG_STATUS[5]


def test_steihaug_is_the_fifth_iterator():
    assert N.steihaug is optimizer.steihaug and int(N.NLLSIterator.steihaug) == 4 and len(N.NLLSIterator) == 5
    assert [int(i) for i in (N.newton, N.levenbergmarquardt, N.dogleg, N.gradientdescent)] == [0, 1, 2, 3]
    mk, it = optimizer._ITER[N.steihaug]
    assert mk is iterators.SteihaugData and it is iterators.iterate_steihaug
    sd = iterators.SteihaugData(2.5); assert sd.trustradius == 2.5 and sd.printable() == 2.5
    sd.reset(); assert sd.trustradius == 0.0 and iterators.SteihaugData().trustradius == 0.0
    assert N.NLLSOptions(iterator=N.steihaug).iterator is N.steihaug and N.NLLSOptions(iterator=4).iterator is N.steihaug


class _FakeLS:
    """a linear system with H = diag(h) that records what the iterator calls; its solve_pcg_tr is the exact Steihaug step of a diagonal model under M = I"""

    def __init__(self, h, b, costs):
        self.h, self.b, self.costs, self.calls = np.asarray(h, float), np.asarray(b, float), list(costs), []

    def hess_apply(self, v, lam=0.0): self.calls.append(("hess_apply",)); return self.h * v
    def hess_block_diag(self, lam=0.0): self.calls.append(("hess_block_diag",)); return [np.array([[v]]) for v in self.h]
    def solve_pcg_schur(self, *a): raise AssertionError("the reduced solve has no trust region")
    def solve_pcg(self, *a): raise AssertionError("the plain solve has no trust region")
    def solve(self): raise AssertionError("no factorisation")

    def solve_pcg_tr(self, radius, precond, maxiters, rtol):
        self.calls.append(("solve_pcg_tr", radius, precond, maxiters, rtol))
        return None, dict(iterations=1, status=4, mnorm=radius, model=0.5)

    def update(self, to, frm): self.calls.append(("update",))
    def cost(self, which): self.calls.append(("cost",)); return self.costs.pop(0)
    def step_maxabs(self): return 1.0


def test_iterate_steihaug_on_a_recording_linear_system():
    ls = _FakeLS([2.0, 4.0], [1.0, 1.0], [2.0, 0.9]); data = optimizer.NLLSInternal(ls, 0); data.bestcost = 1.0
    sd = iterators.SteihaugData(); opt = N.NLLSOptions(iterator=N.steihaug, linearsolver=N.PCG(rtol=1e-2, precond="none"))
    cost = iterators.iterate_steihaug(sd, data, None, opt)
    names = [c[0] for c in ls.calls]
    # the first radius: M = I, z = b, b'z = 2, z'Hz = 6 -> (2 / 6) sqrt(2); the first trial raises the cost (mu < 0.125: halved), the second lowers it by 0.1 of a
    # predicted 0.5 (mu = 0.2: kept)
    r0 = (2.0 / 6.0) * np.sqrt(2.0)
    assert names == ["hess_apply", "solve_pcg_tr", "update", "cost", "solve_pcg_tr", "update", "cost"] and cost == 0.9
    assert ls.calls[1][1] == pytest.approx(r0, rel=1e-15) and ls.calls[1][2:] == ("none", None, 1e-2)
    assert ls.calls[4][1] == 0.5 * ls.calls[1][1] and sd.trustradius == 0.5 * ls.calls[1][1]
    assert data.linearsolvers == 2 and data.costcomputations == 2 and sd.statuses == [4, 4]
    # a good trial: mu = (1 - 0.5) / 0.5 = 1 > 0.375 -> the radius triples from the step's norm; the options' solver is taken as it is
    ls = _FakeLS([2.0, 4.0], [1.0, 1.0], [0.5]); data = optimizer.NLLSInternal(ls, 0); data.bestcost = 1.0; sd = iterators.SteihaugData(0.25)
    iterators.iterate_steihaug(sd, data, None, N.NLLSOptions(iterator=N.steihaug, linearsolver=N.PCG(rtol=1e-3, maxiters=7, precond="none")))
    assert ls.calls == [("solve_pcg_tr", 0.25, "none", 7, 1e-3), ("update",), ("cost",)] and sd.trustradius == 0.75
    # z'Hz <= 0: the first radius is sqrt(b'z)
    ls = _FakeLS([-1.0, -1.0], [3.0, 4.0], [0.5]); data = optimizer.NLLSInternal(ls, 0); data.bestcost = 1.0; sd = iterators.SteihaugData()
    iterators.iterate_steihaug(sd, data, None, N.NLLSOptions(iterator=N.steihaug, linearsolver=N.PCG(rtol=1e-2, precond="none")))
    assert ls.calls[1][1] == 5.0


def test_the_default_solver_is_block_jacobi_at_1e_2():
    ls = _FakeLS([2.0, 4.0], [1.0, 1.0], [0.5]); data = optimizer.NLLSInternal(ls, 0); data.bestcost = 1.0; sd = iterators.SteihaugData()
    iterators.iterate_steihaug(sd, data, None, N.NLLSOptions(iterator=N.steihaug))
    call = [c for c in ls.calls if c[0] == "solve_pcg_tr"][0]
    # z = M^-1 b = (1/2, 1/4): b'z = 3/4, z'Hz = 3/4 -> sqrt(3/4)
    assert call[2:] == ("blockjacobi", None, 1e-2) and call[1] == pytest.approx(np.sqrt(0.75), rel=1e-15)
    assert [c[0] for c in ls.calls][:2] == ["hess_block_diag", "hess_apply"]


def test_iterate_steihaug_refuses_the_reduced_system():
    ls = _FakeLS([2.0], [1.0], [0.5]); data = optimizer.NLLSInternal(ls, 0); data.bestcost = 1.0
    with pytest.raises(ValueError):
        iterators.iterate_steihaug(iterators.SteihaugData(), data, None, N.NLLSOptions(iterator=N.steihaug, linearsolver=N.PCG(schur=True)))
    assert ls.calls == []


def test_julia_shim_names_the_entry_point():
    jl = open(os.path.join(ROOT, "nllssolver.jl_amd", "julia", "NLLSsolverAMD.jl")).read()
    for name in (":nlls_solve_pcg_tr", "function solvepcgtr!("):
        assert name in jl, name
    call = jl[jl.index(":nlls_solve_pcg_tr"):]; call = call[:call.index("\n")]
    assert "(Ptr{Cvoid}, Int32, Int32, Float64, Float64, Ptr{Float64}, Ptr{Float64})" in call
