"""USER robust kernels (include/nlls_amd.h, NLLS_ROBUST_USER0 .. 7): the reference robustifies with any AbstractRobustifier -- robustify(kernel, cost), robustifydcost by
second-order autodiff of it unless the kernel has a closed form (src/robust.jl, src/autodiff.jl:163).  Here they reach the device at BUILD time, like the user residual
and variable kinds: a header specialises nlls::Robust<> with NPARAM and ONE templated robustify<T>, optionally a dcost().  __graft_entry__.build() builds the example
(tests/user_kinds/robust_kernels.hpp -> csrc/libnlls_amd_userrobust.so); the checks on the device run in a process of their own (tests/userrobust_worker.py), because
the library is chosen by NLLS_AMD_LIB before it is loaded."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nllssolver.jl_amd", "csrc")
USERLIB = os.path.join(CSRC, "libnlls_amd_userrobust.so")
DEFAULTLIB = os.path.join(CSRC, "libnlls_amd.so")
BUILTIN = {0: 0, 1: 1, 2: 1, 3: 1}                          # NONE, HUBER, HUBER2O, GEMAN_MCCLURE
USER = {8: 1, 9: 1, 10: 1, 11: 1, 12: 2, 13: 1}              # USER0 .. 5 of robust_kernels.hpp


def _lib(path):
    assert os.path.exists(path), "run __graft_entry__.build()"
    return ctypes.CDLL(path)


def test_userrobust_library_exports_the_same_abi():
    """(CPU) the library with user robust kernels is the same C ABI: every symbol of include/nlls_amd.h"""
    from nllssolver_jl_amd import _capi
    L = _lib(USERLIB)
    assert not [s for s in _capi.SYMBOLS if not hasattr(L, s)]
    assert "nlls_robust_nparams" in _capi.SYMBOLS and "nlls_robustify" in _capi.SYMBOLS


def test_robust_nparams_of_the_user_library():
    """(CPU) nlls_robust_nparams gives NPARAM of the built-in kernels and of the header's, negative for ids the header does not declare"""
    L = _lib(USERLIB)
    for k, n in {**BUILTIN, **USER}.items():
        assert L.nlls_robust_nparams(k) == n, k
    for k in (14, 15, 4, 7, 16, 0x10 | 8, -1):
        assert L.nlls_robust_nparams(k) < 0, k


def test_default_library_has_no_user_robust_kernels():
    """(CPU) a library built without a user header keeps the built-in kernels and declines ids 8 .. 15"""
    L = _lib(DEFAULTLIB)
    for k, n in BUILTIN.items():
        assert L.nlls_robust_nparams(k) == n, k
    for k in range(8, 16):
        assert L.nlls_robust_nparams(k) < 0, k


def test_user_robust_params_layout():
    """(CPU) UserRobust places its parameters at robust_params[0] and [2]; Scaled keeps [2] and puts its height at [1]"""
    from nllssolver_jl_amd import kinds as K
    import nllssolver_jl_amd as N
    c, a, h = 0.3, -1.5, 2.0
    r = N.UserRobust(K.ROBUST_USER0 + 4, c, a)
    assert r.kind == 12 and r.params == (c, 0.0, a, 0.0)
    s = N.Scaled(r, h)
    assert s.kind == 12 | K.ROBUST_SCALED and s.params == (c, h, a, 0.0)
    assert N.Scaled(N.HuberKernel(0.1), h).params == (0.1, h, 0.0, 0.0)
    assert N.UserRobust(8, 0.1).params == (0.1, 0.0, 0.0, 0.0)
    for bad in ((7, 0.1), (16, 0.1), (8, 1.0, 2.0, 3.0)):
        with pytest.raises(ValueError):
            N.UserRobust(*bad)


def test_register_user_robust_cross_checks_the_library():
    """(CPU) kinds.register_user_robust raises on an NPARAM the loaded library does not declare -- in the default library (no user kernels) and in the example's
    (another NPARAM) -- and records the declared ones"""
    from nllssolver_jl_amd import kinds as K
    if not os.environ.get("NLLS_AMD_LIB"):
        with pytest.raises(ValueError):
            K.register_user_robust(8, 1)
        assert 8 not in K.USER_ROBUST
    code = ("import sys; sys.path.insert(0, sys.argv[1])\n"
            "import nllssolver_jl_amd as N\n"
            "from nllssolver_jl_amd import kinds as K\n"
            "for bad in ((8, 2), (12, 1), (14, 1), (15, 0), (7, 1), (9, 3)):\n"
            "    try: K.register_user_robust(*bad)\n"
            "    except ValueError: pass\n"
            "    else: raise SystemExit(f'accepted {bad}')\n"
            "K.register_user_robust(12, 2); K.register_user_robust(8, 1)\n"
            "assert K.USER_ROBUST == {12: 2, 8: 1}\n"
            "try: N.UserRobust(12, 0.5)\n"
            "except ValueError: pass\n"
            "else: raise SystemExit('UserRobust accepted one parameter for a kernel of two')\n"
            "p = N.NLLSProblem(); p.addvariables([[1.0, 0, 0, 0, 1, 0]]); p.addvariables([[0.0, 0, 10]])\n"
            "p.addcosts(K.RES_BA_AFFINE, [[1, 2]], [[0.1, 0.2]], N.Scaled(N.UserRobust(12, 0.5, -2.0), 3.0))\n"
            "(g,) = p.groups(); assert g['robust_kind'] == 0x1C and tuple(g['robust_params']) == (0.5, 3.0, -2.0, 0.0), g\n"
            "print('register ok')\n")
    _lib(USERLIB)
    env = dict(os.environ, NLLS_AMD_LIB=USERLIB)
    out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "register ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_user_robust_kernels_on_the_device():
    env = dict(os.environ, NLLS_AMD_LIB=USERLIB)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "userrobust_worker.py")], capture_output=True, text=True, env=env, timeout=1500)
    print(out.stdout[-4000:])
    assert out.returncode == 0 and "user robust kernels ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
