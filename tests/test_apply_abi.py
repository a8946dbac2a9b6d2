"""(CPU) nlls_hess_apply / nlls_jac_apply / nlls_jact_apply / nlls_hess_block_diag through every layer: declared in include/nlls_amd.h, exported by the library and by
the libraries built with a user header, bound in _capi, forwarded by the linear system, public as N.hessvec / N.jacvec / N.jactvec and on N.Solver, named by the shim."""
import ctypes
import inspect
import os
import re

import nllssolver_jl_amd as N
from nllssolver_jl_amd import _capi, linearsystem, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nlls_hess_apply", "nlls_jac_apply", "nlls_jact_apply", "nlls_hess_block_diag")
NARGS = {"nlls_hess_apply": 6, "nlls_jac_apply": 6, "nlls_jact_apply": 6, "nlls_hess_block_diag": 4}


def test_header_library_and_binding_carry_the_four_names():
    h = open(os.path.join(ROOT, "include", "nlls_amd.h")).read()
    section = h.index("matrix-free products with the linearisation ---")
    assert section > h.index("the linearisation of single cost blocks ---"), "the section sits behind the per-block linearisation"
    assert "#define NLLS_APPLY_MAX_VEC 8" in h and "#define NLLS_OPT_APPLY_SCRATCH" in h and "#define NLLS_OPT_APPLY_WAVE_MIN" in h
    assert "only while `which` still" in h                        # (equal to the sweep's A only while the set still holds what the sweep saw)
    for n in NAMES:                                               # each declaration cites what it replaces
        decl = h.index(n + "(nlls_ctx*")
        assert decl > section and "replaces:" in h[h.rindex("/*", 0, decl):decl], n
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    L = _capi.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", h), n
        assert hasattr(L, n) and n in _capi.SYMBOLS
        assert len(getattr(L, n).argtypes) == NARGS[n], n
    assert _capi.APPLY_MAX_VEC == 8 and (_capi.OPT_APPLY_SCRATCH, _capi.OPT_APPLY_WAVE_MIN) == (4, 5)
    # a null context is an argument error, not a crash
    buf = (ctypes.c_double * 4)()
    assert L.nlls_hess_apply(None, 0, 0.0, 1, buf, buf) == _capi.ERR_INVALID_ARG
    assert L.nlls_jac_apply(None, 0, 0, 1, buf, buf) == _capi.ERR_INVALID_ARG
    assert L.nlls_jact_apply(None, 0, 0, 1, buf, buf) == _capi.ERR_INVALID_ARG
    assert L.nlls_hess_block_diag(None, 0, 0.0, buf) == _capi.ERR_INVALID_ARG


def test_entry_points_sit_between_the_guard_pair():
    src = open(os.path.join(ROOT, "nllssolver.jl_amd", "csrc", "nlls_capi.cpp")).read()
    heads = dict(re.findall(r"^int\s+(nlls_\w+)\([^\n]*\)\s*\{([^\n]*)$", src, flags=re.M))
    for n in NAMES:
        assert n in heads and "NLLS_API_BEGIN" in heads[n], n


def test_user_libraries_get_them_through_the_kind_list():
    """`make user` compiles nlls_apply.hip with the header: the kernels are instantiated for its residual kinds by dispatch_res, no code in the header"""
    for name in ("userdemo", "uservar", "userrobust"):
        lib = os.path.join(ROOT, "nllssolver.jl_amd", "csrc", f"libnlls_amd_{name}.so")
        assert os.path.exists(lib), "run __graft_entry__.build()"
        U = ctypes.CDLL(lib)
        assert all(hasattr(U, n) for n in NAMES), name
    for hdr in ("radial_ba.hpp", "manifold_ba.hpp", "robust_kernels.hpp"):
        src = open(os.path.join(ROOT, "tests", "user_kinds", hdr)).read()
        assert not any(w in src for w in ("hess_apply", "jac_apply", "jact_apply", "hess_block_diag", "nlls_apply")), hdr
    mk = open(os.path.join(ROOT, "nllssolver.jl_amd", "csrc", "Makefile")).read()
    assert "$(UFLAGS) -c nlls_apply.hip" in mk and re.search(r"^OBJS = .*\bnlls_apply\.o\b", mk, flags=re.M)
    rule = mk[mk.index("nlls_apply.o: nlls_apply.hip"):].split("\n")[1]
    assert "-fno-honor-nans" not in rule and "-fno-signed-zeros" not in rule      # a NaN residual shows as NaN


def test_host_layers():
    for cls in (_capi.Context, linearsystem.MultiVariateLSgpu):
        par = inspect.signature(cls.hess_apply).parameters
        assert list(par) == ["self", "v", "lam", "which"] and par["lam"].default == 0.0 and par["which"].default == _capi.VARS_CURRENT
        par = inspect.signature(cls.jac_apply).parameters
        assert list(par) == ["self", "group", "v", "which"] and par["which"].default == _capi.VARS_CURRENT
        par = inspect.signature(cls.jact_apply).parameters
        assert list(par) == ["self", "group", "u", "which"] and par["which"].default == _capi.VARS_CURRENT
        par = inspect.signature(cls.hess_block_diag).parameters
        assert list(par) == ["self", "lam", "which"] and par["lam"].default == 0.0 and par["which"].default == _capi.VARS_CURRENT
    assert N.hessvec is optimizer.hessvec and N.jacvec is optimizer.jacvec and N.jactvec is optimizer.jactvec
    par = inspect.signature(N.hessvec).parameters
    assert list(par)[:4] == ["problem", "v", "lam", "unfixed"] and par["lam"].default == 0.0 and par["unfixed"].default is None
    par = inspect.signature(N.jacvec).parameters
    assert list(par)[:4] == ["problem", "group", "v", "unfixed"] and par["unfixed"].default is None
    par = inspect.signature(N.jactvec).parameters
    assert list(par)[:4] == ["problem", "group", "u", "unfixed"] and par["unfixed"].default is None
    assert list(inspect.signature(N.Solver.hessvec).parameters) == ["self", "v", "lam"] and inspect.signature(N.Solver.hessvec).parameters["lam"].default == 0.0
    assert list(inspect.signature(N.Solver.jacvec).parameters) == ["self", "group", "v"]
    assert list(inspect.signature(N.Solver.jactvec).parameters) == ["self", "group", "u"]
    assert list(inspect.signature(N.Solver.hessblockdiag).parameters) == ["self", "lam"]
    assert list(inspect.signature(N.Solver.operator).parameters) == ["self", "lam"]
    for member in ("matvec", "diag_blocks"):
        assert callable(getattr(optimizer.HessianOperator, member))
    src = inspect.getsource(optimizer.HessianOperator)
    assert "self.shape" in src and "import scipy" not in inspect.getsource(optimizer) and "from scipy" not in inspect.getsource(optimizer)      # needs no scipy


def test_julia_shim_names_the_three_entry_points():
    jl = open(os.path.join(ROOT, "nllssolver.jl_amd", "julia", "NLLSsolverAMD.jl")).read()
    assert ":nlls_hess_apply" in jl and ":nlls_jac_apply" in jl and ":nlls_jact_apply" in jl
    assert "function hessvec!(y" in jl and "function jacvec!(u" in jl and "function jactvec!(y" in jl
