"""USER variable kinds (include/nlls_amd.h, NLLS_VAR_USER0 .. 7): the reference's variable blocks are any type with nvars() and update() (src/variable.jl), its Jacobian
taken through update(var, dualzeros) (src/autodiff.jl:57-61).  Here they reach the device at BUILD time, like the user residual kinds: a header specialises nlls::Var<> with
STORAGE, DOF and ONE templated update<T>.  __graft_entry__.build() builds the example (tests/user_kinds/manifold_ba.hpp -> csrc/libnlls_amd_uservar.so); the checks on
the device run in a process of their own (tests/uservar_worker.py), because the library is chosen by NLLS_AMD_LIB before it is loaded."""
import ctypes
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nllssolver.jl_amd", "csrc")
USERLIB = os.path.join(CSRC, "libnlls_amd_uservar.so")
DEFAULTLIB = os.path.join(CSRC, "libnlls_amd.so")
SIZES = {100: (12, 6), 101: (7, 6), 102: (3, 2)}        # (storage, dof) of USERVAR0 .. 2 in manifold_ba.hpp


def _lib(path):
    assert os.path.exists(path), "run __graft_entry__.build()"
    return ctypes.CDLL(path)


def test_uservar_library_exports_the_same_abi():
    """(CPU) the library with user variable kinds is the same C ABI: every symbol of include/nlls_amd.h"""
    from nllssolver_jl_amd import _capi
    L = _lib(USERLIB)
    assert not [s for s in _capi.SYMBOLS if not hasattr(L, s)]


def test_uservar_sizes_are_reported():
    """(CPU) nlls_var_storage / nlls_var_dof give the header's STORAGE / DOF for the user ids, whatever the dim argument"""
    L = _lib(USERLIB)
    for k, (st, dof) in SIZES.items():
        for dim in (0, dof):
            assert (L.nlls_var_storage(k, dim), L.nlls_var_dof(k, dim)) == (st, dof), k
    assert L.nlls_var_storage(103, 6) < 0 and L.nlls_var_dof(103, 6) < 0          # (ids the header does not declare)
    assert (L.nlls_var_storage(5, 6), L.nlls_var_dof(5, 6)) == (12, 6)            # (the built-in kinds are unchanged)


def test_uservar_res_slot_kinds():
    """(CPU) nlls_res_slot_kind names the user variable kinds in the user residual kinds' slots"""
    L = _lib(USERLIB)
    vk, vd = ctypes.c_int32(), ctypes.c_int32()
    for rk, slots in {100: [(100, 6), (1, 3)], 101: [(101, 6), (1, 3)], 102: [(102, 2)]}.items():
        assert L.nlls_res_ndeps(rk) == len(slots)
        for s, want in enumerate(slots):
            assert L.nlls_res_slot_kind(rk, s, ctypes.byref(vk), ctypes.byref(vd)) == 0
            assert (vk.value, vd.value) == want, (rk, s)


def test_default_library_has_no_user_variable_kinds():
    """(CPU) a library built without a user header declines the user ids, as before"""
    L = _lib(DEFAULTLIB)
    for k in range(100, 108):
        assert L.nlls_var_storage(k, 6) < 0 and L.nlls_var_dof(k, 6) < 0


def test_register_user_var_cross_checks_the_library():
    """(CPU) kinds.register_user_var raises on sizes the loaded library does not declare -- in the default library (no user kinds) and in the example's
    (other sizes) -- and records the declared ones, which var_storage / var_dof / addvariable then use"""
    from nllssolver_jl_amd import kinds as K
    if not os.environ.get("NLLS_AMD_LIB"):
        with pytest.raises(ValueError):
            K.register_user_var(100, 12, 6)
        assert 100 not in K.USER_VARS
    code = ("import sys; sys.path.insert(0, sys.argv[1])\n"
            "import nllssolver_jl_amd as N\n"
            "from nllssolver_jl_amd import kinds as K\n"
            "for bad in ((100, 7, 6), (101, 7, 3), (102, 12, 6)):\n"
            "    try: K.register_user_var(*bad)\n"
            "    except ValueError: pass\n"
            "    else: raise SystemExit(f'accepted {bad}')\n"
            "K.register_user_var(100, 12, 6); K.register_user_var(102, 3, 2)\n"
            "assert (K.var_storage(100, 6), K.var_dof(100, 6), K.var_storage(102, 2), K.var_dof(102, 2)) == (12, 6, 3, 2)\n"
            "p = N.NLLSProblem(); i = p.addvariable([1.0, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], 100); j = p.addvariable([0.0, 0.6, 0.8], 102)\n"
            "assert list(p.var_kind) == [100, 102] and list(p.var_dim) == [6, 2] and list(p.var_offsets) == [0, 12, 15]\n"
            "print('register ok')\n")
    _lib(USERLIB)
    env = dict(os.environ, NLLS_AMD_LIB=USERLIB)
    out = subprocess.run([sys.executable, "-c", code, ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0 and "register ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


@pytest.mark.gpu
def test_user_variable_kinds_on_the_device():
    env = dict(os.environ, NLLS_AMD_LIB=USERLIB)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "uservar_worker.py")], capture_output=True, text=True, env=env, timeout=1200)
    print(out.stdout[-4000:])
    assert out.returncode == 0 and "user variable kinds ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
