"""(CPU) nlls_eval_jacobians / nlls_eval_gradhess and their two static helpers through every layer: declared in include/nlls_amd.h, exported by the library and by the
libraries built with a user header, bound in _capi, forwarded by the linear system, public as N.computeresjac / N.computecostgradhess / N.jacobian and on N.Solver."""
import ctypes
import inspect
import os
import re

import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import _capi, kinds as K, linearsystem, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nlls_eval_jacobians", "nlls_eval_gradhess", "nlls_res_jac_cols", "nlls_res_gh_dim")
DYNAMIC = (K.RES_DYN_LINEAR, K.RES_DYN_NORM, K.RES_DYN_LINEARSQ, K.COST_DYN_LINEAR)


def test_header_library_and_binding_carry_the_four_names():
    h = open(os.path.join(ROOT, "include", "nlls_amd.h")).read()
    for n in NAMES[:2]:                                               # each declaration cites the reference function it replaces, and says what it refuses
        decl = h.index("nlls_" + n[5:] + "(nlls_ctx*")
        assert "replaces:" in h[h.rindex("/*", 0, decl):decl], n
    assert "NLLS_ERR_UNSUPPORTED: nlls_eval_jacobians on a non-squared cost" in h
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    L = _capi.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", h), n
        assert hasattr(L, n) and n in _capi.SYMBOLS
    assert len(L.nlls_eval_jacobians.argtypes) == 7 and len(L.nlls_eval_gradhess.argtypes) == 8
    assert len(L.nlls_res_jac_cols.argtypes) == 1 and len(L.nlls_res_gh_dim.argtypes) == 1
    # a null context is an argument error, not a crash
    assert L.nlls_eval_jacobians(None, 0, 0, 0, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.nlls_eval_gradhess(None, 0, 0, 0, None, None, None, None) == _capi.ERR_INVALID_ARG


def test_user_libraries_get_them_through_the_kind_list():
    """`make user` instantiates the kernel for the header's residual kinds (NLLS_FOR_EACH_RES): no extra code in the header"""
    for name in ("userdemo", "uservar", "userrobust"):
        lib = os.path.join(ROOT, "nllssolver.jl_amd", "csrc", f"libnlls_amd_{name}.so")
        assert os.path.exists(lib), "run __graft_entry__.build()"
        U = ctypes.CDLL(lib)
        assert all(hasattr(U, n) for n in NAMES), name
    for hdr in ("radial_ba.hpp", "manifold_ba.hpp", "robust_kernels.hpp"):
        src = open(os.path.join(ROOT, "tests", "user_kinds", hdr)).read()
        assert "eval_jacobians" not in src and "eval_gradhess" not in src and "linearize" not in src
    # the user demo's kind (two slots: a camera of 7 unknowns and a point) is sized from its header alone
    U = ctypes.CDLL(os.path.join(ROOT, "nllssolver.jl_amd", "csrc", "libnlls_amd_userdemo.so"))
    for fn in (U.nlls_res_jac_cols, U.nlls_res_gh_dim, U.nlls_res_ndeps):
        fn.argtypes = [ctypes.c_int32]
    user0 = 100                                                       # NLLS_RES_USER0
    assert U.nlls_res_ndeps(user0) == 2 and U.nlls_res_jac_cols(user0) == 10 and U.nlls_res_gh_dim(user0) == 10
    assert _capi.lib().nlls_res_jac_cols(user0) < 0


def test_static_helpers_match_registry():
    L = _capi.lib()
    seen = 0
    for kind, (ndeps, nres, ndata, adaptive, slots) in K.RES_TABLE.items():
        if kind in DYNAMIC:
            assert L.nlls_res_jac_cols(kind) < 0 and L.nlls_res_gh_dim(kind) < 0, kind
            continue
        nj = sum(K.var_dof(vk, vd) for vk, vd in slots[1 if adaptive else 0:])
        assert L.nlls_res_jac_cols(kind) == nj, (kind, L.nlls_res_jac_cols(kind), nj)
        assert L.nlls_res_gh_dim(kind) == nj + (3 if adaptive else 0), kind
        assert adaptive == (kind in K.ADAPTIVE_KINDS)
        seen += 1
    assert seen >= 11
    assert L.nlls_res_jac_cols(K.RES_BA_AFFINE) == 9 and L.nlls_res_gh_dim(K.RES_BA_SO3_ADAPTIVE) == 12 and L.nlls_res_gh_dim(K.COST_LINEAR3) == 3
    assert L.nlls_res_jac_cols(999) < 0 and L.nlls_res_gh_dim(999) < 0
    for kind in DYNAMIC:
        assert L.nlls_res_jac_cols(kind) < 0 and L.nlls_res_gh_dim(kind) < 0


def test_host_layers():
    for cls in (_capi.Context, linearsystem.MultiVariateLSgpu):
        sj = inspect.signature(cls.eval_jacobians).parameters; sg = inspect.signature(cls.eval_gradhess).parameters
        assert list(sj) == ["self", "group", "which", "index", "want"] and list(sg) == ["self", "group", "which", "index", "want"]
        assert sj["which"].default == _capi.VARS_CURRENT and sj["index"].default is None and tuple(sj["want"].default) == ("r", "J")
        assert tuple(sg["want"].default) == ("cost", "g", "H")
    assert N.computeresjac is optimizer.computeresjac and N.computecostgradhess is optimizer.computecostgradhess and N.jacobian is optimizer.jacobian
    for fn in (N.computeresjac, N.computecostgradhess):
        par = inspect.signature(fn).parameters
        assert list(par)[:4] == ["problem", "group", "index", "unfixed"] and par["group"].default == 0 and par["index"].default is None and par["unfixed"].default is None
    par = inspect.signature(N.jacobian).parameters
    assert list(par)[:3] == ["problem", "unfixed", "weighted"] and par["weighted"].default is False
    for name in ("jacobians", "gradhess"):
        par = inspect.signature(getattr(N.Solver, name)).parameters
        assert list(par) == ["self", "group", "index"] and par["index"].default is None


def test_jacobian_refuses_groups_without_one():
    """before anything is built on the device: an adaptive, a non-squared and a dynamic-size group"""
    from nllssolver_jl_amd.variables import contaminated_gaussian
    p = N.NLLSProblem(); p.addvariable(contaminated_gaussian(0.5, 5.0, 0.6), K.VAR_CONTAMINATED_GAUSSIAN); p.addvariable(0.0)
    p.addcosts(K.RES_ADAPTIVE_MEAN, [[1, 2]], [[0.5]])
    q = N.NLLSProblem(); q.addvariable([0.1, 0.2, 0.3]); q.addcosts(K.COST_LINEAR3, [[1]], [[1.0, 2.0, 3.0]])
    d = N.NLLSProblem(); d.addvariable([1.0, 2.0], K.VAR_DYNAMIC); d.addcosts(K.RES_DYN_NORM, [[1]], [[]])
    for prob in (p, q, d):
        with pytest.raises(ValueError):
            N.jacobian(prob)


def test_julia_shim_calls_both_entry_points():
    jl = open(os.path.join(ROOT, "nllssolver.jl_amd", "julia", "NLLSsolverAMD.jl")).read()
    assert ":nlls_eval_jacobians" in jl and ":nlls_eval_gradhess" in jl and "NLLSsolver.computeresjac(ls::MultiVariateLSgpu" in jl and "NLLSsolver.computecostgradhess(ls::MultiVariateLSgpu" in jl
