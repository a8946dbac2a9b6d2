"""(CPU) nlls_schur_info / nlls_schur_apply / nlls_schur_reduce / nlls_schur_expand / nlls_solve_pcg_schur through every layer: declared in include/nlls_amd.h behind
nlls_marginal_cov, exported by the library and by the libraries built with a user header, bound in _capi with their argtypes, forwarded by the linear system, on
N.Solver.schur_operator, selected by N.PCG(schur=True), named by the shim -- and refused without a context.  The pattern of tests/test_pcg_abi.py."""
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
NAMES = ("nlls_schur_info", "nlls_schur_apply", "nlls_schur_reduce", "nlls_schur_expand", "nlls_solve_pcg_schur")
DECLS = (r"\bint\s+nlls_schur_info\s*\(const nlls_ctx\* ctx, int64_t\* nred_out, int64_t\* nelim_out, uint8_t\* is_elim_out\s*\)",
         r"\bint\s+nlls_schur_apply\s*\(nlls_ctx\* ctx, int32_t which, double lambda, int32_t nvec, const double\* v\s*, double\* y_out\s*\)",
         r"\bint\s+nlls_schur_reduce\s*\(nlls_ctx\* ctx, int32_t which, double lambda, int32_t nvec, const double\* b\s*, double\* s_out\s*\)",
         r"\bint\s+nlls_schur_expand\s*\(nlls_ctx\* ctx, int32_t which, double lambda, int32_t nvec, const double\* b\s*, const double\* yr\s*, double\* y_out\s*\)",
         r"\bint\s+nlls_solve_pcg_schur\s*\(nlls_ctx\* ctx, int32_t precond, int32_t maxiters, double rtol, double\* x_out, double\* stats_out\)")


def test_header_declares_the_five_behind_the_covariances():
    h = open(os.path.join(ROOT, "include", "nlls_amd.h")).read()
    bare = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    for name, decl in zip(NAMES, DECLS):
        assert re.search(decl, bare), name
        assert h.index(name + "(") > h.index("nlls_marginal_cov(nlls_ctx*"), name
    doc = h[h.rindex("/* ----", 0, h.index("nlls_schur_info(")):h.index("nlls_schur_info(")]
    assert "replaces:" in doc and "src/linearsolver.jl:20-32" in doc and "NLLS_ERR_NOT_SPD" in doc and "eliminated nothing" in doc
    # nlls_info keeps its size and nlls_get_solve_stats gained no index: the counters keep describing the last nlls_solve_pcg
    assert ctypes.sizeof(_capi.Info) == 112 and "[56]" not in h


def test_library_and_binding_carry_the_names():
    L = _capi.lib(); i32, i64, dbl, vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_double, ctypes.c_void_p
    for name in NAMES:
        assert hasattr(L, name) and name in _capi.SYMBOLS, name
    assert L.nlls_schur_info.argtypes == [vp, vp, vp, vp]
    assert L.nlls_schur_apply.argtypes == [vp, i32, dbl, i32, vp, vp] and L.nlls_schur_reduce.argtypes == [vp, i32, dbl, i32, vp, vp]
    assert L.nlls_schur_expand.argtypes == [vp, i32, dbl, i32, vp, vp, vp]
    assert L.nlls_solve_pcg_schur.argtypes == [vp, i32, i32, dbl, vp, vp]


def test_a_null_context_is_an_argument_error_and_writes_nothing():
    L = _capi.lib(); P = _capi._p
    v = np.ones(4); out = np.full(4, 7.25); st = np.full(8, 7.25); n = np.full(2, -5, np.int64); mask = np.full(4, 9, np.uint8)
    assert L.nlls_schur_info(None, P(n[:1]), P(n[1:]), P(mask)) == _capi.ERR_INVALID_ARG
    assert L.nlls_schur_apply(None, 0, 0.0, 1, P(v), P(out)) == _capi.ERR_INVALID_ARG
    assert L.nlls_schur_reduce(None, 0, 0.0, 1, P(v), P(out)) == _capi.ERR_INVALID_ARG
    assert L.nlls_schur_expand(None, 0, 0.0, 1, P(v), P(v), P(out)) == _capi.ERR_INVALID_ARG
    assert L.nlls_solve_pcg_schur(None, 1, 10, 1e-8, P(out), P(st)) == _capi.ERR_INVALID_ARG
    assert np.all(out == 7.25) and np.all(st == 7.25) and np.all(n == -5) and np.all(mask == 9)


def test_entry_points_sit_between_the_guard_pair():
    src = open(os.path.join(CSRC, "nlls_capi.cpp")).read()
    heads = dict(re.findall(r"^int\s+(nlls_\w+)\([^\n]*\)\s*\{([^\n]*)$", src, flags=re.M))
    for name in NAMES:
        assert "NLLS_API_BEGIN" in heads[name], name
        body = src[src.index(f"int {name}("):]; body = body[:body.index("\n}\n")]
        assert "NLLS_API_END(" in body.rstrip().splitlines()[-1], name
        assert src.index(f"int {name}(") > src.index("int nlls_marginal_cov("), name       # a section behind the conjugate gradients


def test_makefile_builds_it_like_the_products_and_into_the_user_libraries():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^OBJS = .*\bnlls_schur_apply\.o\b", mk, flags=re.M) and "$(UFLAGS) -c nlls_schur_apply.hip" in mk and "$(OBJDIR)/nlls_schur_apply.o" in mk.split("-shared")[-1]
    rule = mk[mk.index("nlls_schur_apply.o: nlls_schur_apply.hip"):].split("\n")[1]
    assert "-fno-honor-nans" not in rule and "-fno-signed-zeros" not in rule
    user = [l for l in mk.splitlines() if "$(UFLAGS) -c nlls_schur_apply.hip" in l]
    assert len(user) == 1 and "-fno-honor-nans" not in user[0] and "-fno-signed-zeros" not in user[0]
    for name in ("userdemo", "uservar", "userrobust"):
        lib = os.path.join(CSRC, f"libnlls_amd_{name}.so")
        assert os.path.exists(lib), "run __graft_entry__.build()"
        U = ctypes.CDLL(lib)
        assert all(hasattr(U, n) for n in NAMES), name


def test_the_kernel_file_reads_no_environment_and_adds_with_no_atomics():
    hip = open(os.path.join(CSRC, "nlls_schur_apply.hip")).read()
    assert "getenv" not in hip and "atomicAdd" not in hip and "__hip_atomic" not in hip and "atomic" not in hip.replace("No atomics", "")
    assert "schur_rows_kernel" in hip and "schur_wave_kernel" in hip and "schur_cut_kernel" in hip and "wave_sum" in hip
    pcg = open(os.path.join(CSRC, "nlls_pcg.hip")).read()
    assert ".schur = true" in pcg and "enqueue_schur_op(c, SCHUR_APPLY" in pcg          # the driver's one loop, a branch beside its one product call


def test_python_signatures_and_defaults():
    for cls in (_capi.Context, linearsystem.MultiVariateLSgpu):
        par = inspect.signature(cls.solve_pcg_schur).parameters
        assert list(par) == ["self", "precond", "maxiters", "rtol", "want_x"], cls
        assert par["maxiters"].default is None and par["rtol"].default == 1e-8 and par["want_x"].default is False
        assert list(inspect.signature(cls.schur_info).parameters) == ["self"]
        for name, head in (("schur_apply", ["self", "v"]), ("schur_reduce", ["self", "b"]), ("schur_expand", ["self", "b", "yr"])):
            par = inspect.signature(getattr(cls, name)).parameters
            assert list(par) == head + ["lam", "which"] and par["lam"].default == 0.0 and par["which"].default == _capi.VARS_CURRENT, (cls, name)
    assert inspect.signature(_capi.Context.solve_pcg_schur).parameters["precond"].default == 1
    assert "self._x = None" in inspect.getsource(linearsystem.MultiVariateLSgpu.solve_pcg_schur)
    assert "last_pcg_schur" in inspect.getsource(_capi.Context.solve_pcg_schur) and "4 * int(self.info.ndof)" in inspect.getsource(_capi.Context.solve_pcg_schur)
    par = inspect.signature(N.Solver.schur_operator).parameters
    assert list(par) == ["self", "lam"] and par["lam"].default == 0.0
    assert N.SchurOperator is optimizer.SchurOperator
    for member in ("matvec", "reduce", "expand", "diag_blocks"):
        assert callable(getattr(N.SchurOperator, member)), member
    src = inspect.getsource(N.SchurOperator.__init__)
    assert "self.shape" in src and "self.index" in src
    par = inspect.signature(N.PCG.__init__).parameters
    assert list(par) == ["self", "rtol", "maxiters", "precond", "schur"] and par["schur"].default is False
    assert N.PCG().schur is False and N.PCG(schur=True).schur is True


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
    def solve_pcg_schur(self, precond, maxiters, rtol): self.calls.append(("solve_pcg_schur", precond, maxiters, rtol))
    def lm_trial(self, d): self.calls.append(("lm_trial", d)); return 0.5
    def update(self, to, frm): self.calls.append(("update",))
    def cost(self, which): return 0.5
    def step_maxabs(self): return 1.0
    def quadform(self): return 1.0, -1.0


def test_pcg_with_schur_drives_the_reduced_solve():
    data = optimizer.NLLSInternal(_FakeLS(), 0); data.bestcost = 1.0
    opt = N.NLLSOptions(linearsolver=N.PCG(rtol=1e-6, maxiters=9, schur=True))
    loop = optimizer.OuterLoop(None, opt, data, iterators.LevMarData(), iterators.iterate_levmar, nullcallback)
    assert loop.native is False
    iterators.iterate_levmar(iterators.LevMarData(), data, None, opt)
    names = [c[0] for c in data.linsystem.calls]
    assert names[:3] == ["damp", "solve_pcg_schur", "update"] and "lm_trial" not in names and "solve" not in names and "solve_pcg" not in names
    assert data.linsystem.calls[1] == ("solve_pcg_schur", "blockjacobi", 9, 1e-6) and data.linearsolvers == 1
    data.linsystem.calls.clear(); iterators.iterate_newton(iterators.NewtonData(), data, None, opt)
    assert [c[0] for c in data.linsystem.calls] == ["solve_pcg_schur", "update"]
    data.linsystem.calls.clear(); iterators.iterate_newton(iterators.NewtonData(), data, None, N.NLLSOptions(linearsolver=N.PCG()))       # schur=False: as before
    assert [c[0] for c in data.linsystem.calls] == ["solve_pcg", "update"]


def test_julia_shim_names_the_entry_points():
    jl = open(os.path.join(ROOT, "nllssolver.jl_amd", "julia", "NLLSsolverAMD.jl")).read()
    for name in (":nlls_schur_info", ":nlls_schur_apply", ":nlls_schur_reduce", ":nlls_schur_expand", ":nlls_solve_pcg_schur",
                 "function schurapply!(", "function schurreduce!(", "function schurexpand!(", "function solvepcgschur!("):
        assert name in jl, name
