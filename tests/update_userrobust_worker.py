"""Worker of tests/test_gpu_update.py::test_user_robust_kernel_in_a_process_of_its_own (NLLS_AMD_LIB must be set before the library is loaded): nlls_set_robust_params on a
group whose kernel comes from a user header (tests/user_kinds/robust_kernels.hpp: USER1 = Huber with its own dcost, a twin of the built-in kernel).  The width changed on
the uploaded structure, matrix-free and materialised, against the oracle's built-in Huber of the new width and against a fresh upload with the new width."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K, _capi
import tests.test_gpu_update as T

assert os.environ.get("NLLS_AMD_LIB") and os.environ.get("NLLS_SUPERNODE_PIECE") == "128", "run through tests/test_gpu_update.py"
U1 = K.ROBUST_USER0 + 1
K.register_user_robust(U1, 1)
W0, W1 = 0.05, 0.01


class Env:          # (the worker's environment is already set: mf_problem's monkeypatch has nothing to do)
    def setenv(self, *a): pass


oracle_of = T.oracle_of
def oracle_with_builtin_huber(p, groups, bi, flags, lam_scale):
    """the oracle has no user kernels: USER1 is Huber, so it takes the built-in one with the same width"""
    return oracle_of(p, [dict(g, robust_kind=K.ROBUST_HUBER) if g["robust_kind"] == U1 else g for g in groups], bi, flags, lam_scale)
T.oracle_of = oracle_with_builtin_huber

for flags, expect_mf in ((0, 1), (_capi.FLAG_MATERIALIZE, 0)):
    T.run_robust_case(T.mf_problem(Env(), robust=N.UserRobust(U1, W0), noise=0.05), N.UserRobust(U1, W1), flags, expect_mf)
    # ... and the data of a group with a user kernel: the scatter knows nothing of kinds
    T.run_case(T.mf_problem(Env(), robust=N.UserRobust(U1, W0), noise=0.05), flags=flags, a_moves=True, expect_mf=expect_mf)
print("update user robust ok")
