"""(CPU) nlls_eval_blocks and nlls_adaptive_em through every layer: declared in include/nlls_amd.h, exported by the library and by a library built with a user header,
bound in _capi, forwarded by the linear system, public as N.residuals / N.squarederrors / N.emcallback."""
import ctypes
import inspect
import os
import re

import nllssolver_jl_amd as N
from nllssolver_jl_amd import _capi, callbacks, linearsystem, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nlls_eval_blocks", "nlls_adaptive_em")


def test_header_library_and_binding_carry_both_entry_points():
    h = open(os.path.join(ROOT, "include", "nlls_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    L = _capi.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", h), n
        assert hasattr(L, n) and n in _capi.SYMBOLS
    assert L.nlls_eval_blocks.argtypes is not None and len(L.nlls_eval_blocks.argtypes) == 7
    assert L.nlls_adaptive_em.argtypes is not None and len(L.nlls_adaptive_em.argtypes) == 6
    # a null context is an argument error, not a crash
    assert L.nlls_eval_blocks(None, 0, 0, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.nlls_adaptive_em(None, 0, 1, 1, None, None) == _capi.ERR_INVALID_ARG


def test_user_libraries_get_them_through_the_kind_list():
    """`make user` instantiates both for the header's residual kinds (NLLS_FOR_EACH_RES): no extra code in the header"""
    for name in ("userdemo", "uservar", "userrobust"):
        lib = os.path.join(ROOT, "nllssolver.jl_amd", "csrc", f"libnlls_amd_{name}.so")
        assert os.path.exists(lib), "run __graft_entry__.build()"
        U = ctypes.CDLL(lib)
        assert all(hasattr(U, n) for n in NAMES), name
    for hdr in ("radial_ba.hpp", "manifold_ba.hpp", "robust_kernels.hpp"):
        src = open(os.path.join(ROOT, "tests", "user_kinds", hdr)).read()
        assert "eval_blocks" not in src and "adaptive_em" not in src


def test_host_layers():
    assert callable(callbacks.emcallback) and N.emcallback is callbacks.emcallback
    assert N.residuals is optimizer.residuals and N.squarederrors is optimizer.squarederrors
    assert list(inspect.signature(callbacks.emcallback).parameters) == ["kernel_var", "maxiters"]
    assert inspect.signature(callbacks.emcallback).parameters["maxiters"].default == 10
    assert list(inspect.signature(N.residuals).parameters)[:2] == ["problem", "group"]
    for cls, names in ((_capi.Context, ("eval_blocks", "adaptive_em")), (linearsystem.MultiVariateLSgpu, ("eval_blocks", "adaptive_em"))):
        assert all(callable(getattr(cls, n)) for n in names)
    cb = N.emcallback(kernel_var=1, maxiters=3)
    assert callable(cb)
