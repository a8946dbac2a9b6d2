"""(CPU) nlls_set_cost_data and nlls_set_robust_params through every layer: declared in include/nlls_amd.h, exported by the library and by the libraries built with a
user header, bound in _capi, forwarded by the linear system, public as N.Solver."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import _capi, kinds as K, linearsystem, optimizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("nlls_set_cost_data", "nlls_set_robust_params")


def test_header_library_and_binding_carry_both_entry_points():
    h = open(os.path.join(ROOT, "include", "nlls_amd.h")).read()
    h = re.sub(r"/\*.*?\*/", "", h, flags=re.S)
    L = _capi.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", h), n
        assert hasattr(L, n) and n in _capi.SYMBOLS
    assert L.nlls_set_cost_data.argtypes is not None and len(L.nlls_set_cost_data.argtypes) == 5
    assert L.nlls_set_robust_params.argtypes is not None and len(L.nlls_set_robust_params.argtypes) == 3
    # a null context is an argument error, not a crash
    assert L.nlls_set_cost_data(None, 0, 0, None, None) == _capi.ERR_INVALID_ARG
    assert L.nlls_set_robust_params(None, 0, None) == _capi.ERR_INVALID_ARG


def test_user_libraries_export_them_without_a_word_in_the_header():
    """the scatter is kind-agnostic (the record length is a run-time argument): `make user` compiles nlls_update.hip as it stands"""
    for name in ("userdemo", "uservar", "userrobust"):
        lib = os.path.join(ROOT, "nllssolver.jl_amd", "csrc", f"libnlls_amd_{name}.so")
        assert os.path.exists(lib), "run __graft_entry__.build()"
        U = ctypes.CDLL(lib)
        assert all(hasattr(U, n) for n in NAMES), name
    for hdr in ("radial_ba.hpp", "manifold_ba.hpp", "robust_kernels.hpp"):
        src = open(os.path.join(ROOT, "tests", "user_kinds", hdr)).read()
        assert "set_cost_data" not in src and "set_robust_params" not in src


def test_host_layers():
    for cls in (_capi.Context, linearsystem.MultiVariateLSgpu):
        assert list(inspect.signature(cls.set_cost_data).parameters) == ["self", "group", "data", "index"]
        assert inspect.signature(cls.set_cost_data).parameters["index"].default is None
        assert list(inspect.signature(cls.set_robust_params).parameters) == ["self", "group", "params"]
    assert N.Solver is optimizer.Solver
    assert list(inspect.signature(N.Solver.__init__).parameters) == ["self", "problem", "unfixed", "flags", "device", "stream"]
    assert list(inspect.signature(N.Solver.optimize).parameters) == ["self", "options", "callback", "native"]
    assert list(inspect.signature(N.Solver.set_data).parameters) == ["self", "group", "data", "index"]
    assert list(inspect.signature(N.Solver.set_robust).parameters) == ["self", "group", "params_or_kernel"]
    for n in ("cost", "residuals", "squarederrors", "close", "__enter__", "__exit__"):
        assert callable(getattr(N.Solver, n)), n
    # the module functions keep their signatures
    assert list(inspect.signature(N.optimize).parameters) == ["problem", "options", "unfixed", "callback", "flags", "device", "stream", "native"]


def test_solver_fails_loudly_without_a_device():
    probe = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True, text=True, timeout=300)
    assert probe.returncode == 0, probe.stderr[-2000:]
    if probe.stdout.strip().splitlines()[-1] == "True":
        pytest.skip("a GPU is visible here")
    p = N.NLLSProblem(); p.addvariable(0.0); p.addcosts(K.RES_ROSENBROCK_A, [[1]], [[1.0]])
    with pytest.raises(_capi.NllsError) as e:
        N.Solver(p)
    assert e.value.code == _capi.ERR_NO_DEVICE
