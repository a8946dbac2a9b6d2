"""(CPU) nlls_solve_pcg through every layer: declared in include/nlls_amd.h, exported by the library and by the libraries built with a user header, bound in _capi,
forwarded by the linear system, selected by NLLSOptions(linearsolver=N.PCG(...)), on N.Solver, named by the shim -- and refused without a context."""
import ctypes
import inspect
import os
import re

import numpy as np

import nllssolver_jl_amd as N
from nllssolver_jl_amd import _capi, iterators, linearsystem, optimizer
from nllssolver_jl_amd.callbacks import nullcallback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nllssolver.jl_amd", "csrc")


def test_header_library_and_binding_carry_the_name():
    h = open(os.path.join(ROOT, "include", "nlls_amd.h")).read()
    decl = h.index("nlls_solve_pcg(nlls_ctx*")
    assert decl > h.index("nlls_hess_block_diag(nlls_ctx*") and "replaces:" in h[h.rindex("/* ----", 0, decl):decl]
    for line in ("#define NLLS_PCG_PRECOND_NONE          0", "#define NLLS_PCG_PRECOND_BLOCK_JACOBI  1", "#define NLLS_OPT_PCG_ROUND     6", "#define NLLS_OPT_PCG_GRID_MAX  7"):
        assert line in h, line
    assert "[53] iterations made" in h and "[14] milliseconds of the last nlls_solve_pcg" in h and "[47..50] then describe the last product" in h
    bare = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    assert re.search(r"\bint\s+nlls_solve_pcg\s*\(nlls_ctx\* ctx, int32_t precond, int32_t maxiters, double rtol, double\* x_out, double\* stats_out\)", bare)
    L = _capi.lib()
    assert hasattr(L, "nlls_solve_pcg") and "nlls_solve_pcg" in _capi.SYMBOLS and len(L.nlls_solve_pcg.argtypes) == 6
    assert (_capi.OPT_PCG_ROUND, _capi.OPT_PCG_GRID_MAX, _capi.PCG_PRECOND_NONE, _capi.PCG_PRECOND_BLOCK_JACOBI) == (6, 7, 0, 1)
    out = np.full(4, 7.25); st = np.full(8, 7.25)                 # a null context is an argument error, not a crash, and writes nothing
    assert L.nlls_solve_pcg(None, 1, 10, 1e-8, _capi._p(out), _capi._p(st)) == _capi.ERR_INVALID_ARG
    assert np.all(out == 7.25) and np.all(st == 7.25)
    assert L.nlls_set_option(None, _capi.OPT_PCG_ROUND, 4) == _capi.ERR_INVALID_ARG


def test_entry_point_sits_between_the_guard_pair_and_reads_no_environment():
    src = open(os.path.join(CSRC, "nlls_capi.cpp")).read()
    heads = dict(re.findall(r"^int\s+(nlls_\w+)\([^\n]*\)\s*\{([^\n]*)$", src, flags=re.M))
    assert "NLLS_API_BEGIN" in heads["nlls_solve_pcg"]
    hip = open(os.path.join(CSRC, "nlls_pcg.hip")).read()
    assert "getenv" not in hip and "hipFuncSetAttribute" not in hip and "#define HIPCHK" not in hip and "atomicAdd" not in hip and "__hip_atomic" not in hip
    assert "block_sum" in hip and "enqueue_hess_block_diag" in hip
    # the product is the driver's ONE call, and nlls_solve_pcg is that driver on one column: H at CURRENT, the context's damping, b where the sweep left it
    assert hip.count("enqueue_hess_apply(c,") == 1 and "enqueue_hess_apply(c, k.which, k.lambda, active, p, q)" in hip
    assert ".which = NLLS_VARS_CURRENT, .lambda = c->lambda" in hip and ".ncols = 1, .d_b = c->b.p" in hip
    assert hip.count("for (;;)") == 1 and hip.count("PcgArgs a{}") == 1 and hip.count("hipLaunchKernelGGL(pcg_step_kernel") == 1


def test_makefile_builds_it_like_the_products_and_into_the_user_libraries():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^OBJS = .*\bnlls_pcg\.o\b", mk, flags=re.M) and "$(UFLAGS) -c nlls_pcg.hip" in mk and "$(OBJDIR)/nlls_pcg.o" in mk.split("-shared")[-1]
    rule = mk[mk.index("nlls_pcg.o: nlls_pcg.hip"):].split("\n")[1]
    assert "-fno-honor-nans" not in rule and "-fno-signed-zeros" not in rule      # a NaN must reach the breakdown test
    for name in ("userdemo", "uservar", "userrobust"):
        lib = os.path.join(CSRC, f"libnlls_amd_{name}.so")
        assert os.path.exists(lib), "run __graft_entry__.build()"
        assert hasattr(ctypes.CDLL(lib), "nlls_solve_pcg"), name


def test_host_layers():
    for cls in (_capi.Context, linearsystem.MultiVariateLSgpu):
        par = inspect.signature(cls.solve_pcg).parameters
        assert list(par) == ["self", "precond", "maxiters", "rtol", "want_x"]
        assert par["maxiters"].default is None and par["rtol"].default == 1e-8 and par["want_x"].default is False
    assert inspect.signature(_capi.Context.solve_pcg).parameters["precond"].default == 1
    assert "self._x = None" in inspect.getsource(linearsystem.MultiVariateLSgpu.solve_pcg)
    assert "4 * int(self.info.ndof)" in inspect.getsource(_capi.Context.solve_pcg)
    for key in ("pcg_iterations", "pcg_status", "pcg_rounds"):
        assert key in inspect.getsource(_capi.Context.solve_stats)
    par = inspect.signature(N.Solver.solve_pcg).parameters
    assert list(par) == ["self", "lam", "precond", "maxiters", "rtol"]
    assert N.PCG is iterators.PCG
    s = N.PCG(); assert (s.rtol, s.maxiters, s.precond) == (1e-8, None, "blockjacobi")
    s = N.PCG(rtol=1e-6, maxiters=7, precond="none"); assert (s.rtol, s.maxiters, s.precond) == (1e-6, 7, "none")
    assert N.NLLSOptions().linearsolver is None and N.NLLSOptions(linearsolver=s).linearsolver is s


class _FakeContext:
    def lm_iterations(self, *a):
        raise AssertionError("the library's own loop has no conjugate gradients")


class _FakeLS:
    """a linear system that records what the iterators call"""

    def __init__(self):
        self.ctx = _FakeContext(); self.calls = []; self.b = np.ones(2)

    def initlambda(self): return 1.0
    def uniformscaling(self, k): self.calls.append(("damp", k))
    def solve(self): self.calls.append(("solve",))
    def solve_pcg(self, precond, maxiters, rtol): self.calls.append(("solve_pcg", precond, maxiters, rtol))
    def lm_trial(self, d): self.calls.append(("lm_trial", d)); return 0.5
    def update(self, to, frm): self.calls.append(("update",))
    def cost(self, which): return 0.5
    def step_maxabs(self): return 1.0
    def quadform(self): return 1.0, -1.0


def test_the_iterators_take_the_unfused_branch_with_a_pcg():
    data = optimizer.NLLSInternal(_FakeLS(), 0); data.bestcost = 1.0
    opt = N.NLLSOptions(linearsolver=N.PCG(rtol=1e-6, maxiters=9))
    loop = optimizer.OuterLoop(None, opt, data, iterators.LevMarData(), iterators.iterate_levmar, nullcallback)
    assert loop.native is False
    assert optimizer.OuterLoop(None, N.NLLSOptions(), data, iterators.LevMarData(), iterators.iterate_levmar, nullcallback).native is True
    iterators.iterate_levmar(iterators.LevMarData(), data, None, opt)
    names = [c[0] for c in data.linsystem.calls]
    assert names[:3] == ["damp", "solve_pcg", "update"] and "lm_trial" not in names and "solve" not in names
    assert data.linsystem.calls[1] == ("solve_pcg", "blockjacobi", 9, 1e-6) and data.linearsolvers == 1
    data.linsystem.calls.clear(); iterators.iterate_newton(iterators.NewtonData(), data, None, opt)
    assert [c[0] for c in data.linsystem.calls] == ["solve_pcg", "update"]
    data.linsystem.calls.clear(); iterators.iterate_levmar(iterators.LevMarData(), data, None, N.NLLSOptions())       # linearsolver=None changes nothing
    assert [c[0] for c in data.linsystem.calls][0] == "lm_trial"
    data.linsystem.calls.clear(); iterators.iterate_newton(iterators.NewtonData(), data, None, N.NLLSOptions())
    assert [c[0] for c in data.linsystem.calls] == ["solve", "update"]


def test_julia_shim_names_the_entry_point():
    jl = open(os.path.join(ROOT, "nllssolver.jl_amd", "julia", "NLLSsolverAMD.jl")).read()
    assert ":nlls_solve_pcg" in jl and "function solvepcg!(" in jl
