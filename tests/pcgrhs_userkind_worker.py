"""Worker of tests/test_gpu_pcgrhs.py::test_user_kind_in_a_process_of_its_own (NLLS_AMD_LIB must be set before the library is loaded): nlls_solve_pcg_rhs and
nlls_marginal_cov on a residual kind that exists only as a device template of a USER header (tests/user_kinds/radial_ba.hpp, NLLS_RES_USER0) -- the problem of
tests/pcg_userkind_worker.py -- two columns against numpy.linalg.solve on that library's own A, to 1e-7 of the column's largest entry as tests/test_gpu_pcgrhs.py
holds the built-in kinds, and a camera's covariance block against numpy.linalg.inv."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K, _capi

assert os.environ.get("NLLS_AMD_LIB"), "run through tests/test_gpu_pcgrhs.py"
USER0 = 100
K.register_user_kind(USER0, 2, 2, 2, ((K.VAR_EUCLIDEAN, 7), (K.VAR_EUCLIDEAN, 3)))


def main():
    from tests.helpers import bsm_to_csr
    rng = np.random.default_rng(21); ncam, npts, percam = 12, 80, 4
    p = N.NLLSProblem()
    cams = [p.addvariable(np.concatenate([rng.standard_normal(6) * 0.3 + np.array([1, 0, 0, 0, 1, 0.0]), [0.02 * rng.standard_normal()]])) for _ in range(ncam)]
    pts = [p.addvariable(rng.uniform(-0.5, 0.5, 3) + np.array([0, 0, 2.0])) for _ in range(npts)]
    vi = np.array([[cams[(j + k) % ncam], pts[j]] for j in range(npts) for k in range(percam)], np.int64)
    off = p.var_offsets; v = p.variables
    c = v[off[vi[:, 0] - 1][:, None] + np.arange(7)]; X = v[off[vi[:, 1] - 1][:, None] + np.arange(3)]
    u = (c[:, 0:3] * X).sum(1); w = (c[:, 3:6] * X).sum(1); s = c[:, 6] * (u * u + w * w) + 1.0
    meas = np.stack([s * u, s * w], 1) + 1e-3 * rng.standard_normal((vi.shape[0], 2))
    p.addcosts(USER0, vi, meas)
    unfixed = np.ones(p.nvariables, bool); unfixed[[0, ncam + 3, ncam + 4]] = False
    bi = np.zeros(p.nvariables, np.uint64); bi[unfixed] = np.arange(1, int(unfixed.sum()) + 1, dtype=np.uint64)
    ctx = _capi.Context(0)
    ctx.upload(p.var_kind, p.var_dim, bi, p.groups()); ctx.set_variables(p.variables)
    ctx.sweep_gradhess(); ndof = ctx.info.ndof
    A = bsm_to_csr(ctx.bsm_index(), ctx.get_bsm_data(), ndof).toarray(); b = ctx.get_grad()
    lam = 1e-2 * np.max(np.abs(np.diag(A))); Al = A + lam * np.eye(ndof)
    np.linalg.cholesky(Al)                                              # (the input: positive definite at this damping)
    B = np.stack([b, rng.standard_normal(ndof)]); ref = np.linalg.solve(Al, B.T).T
    Xd, st = ctx.solve_pcg_rhs(B, lam, _capi.VARS_CURRENT, _capi.PCG_PRECOND_BLOCK_JACOBI, None, 1e-10)
    err = max(np.max(np.abs(Xd[k] - ref[k])) / np.max(np.abs(ref[k])) for k in range(2))
    print(f"PCGRHS user0: ndof {ndof} iterations {st['iterations'].tolist()} status {st['status'].tolist()} against numpy {err:.3e} (of 1e-7)")
    assert np.all(st["status"] == 0) and err <= 1e-7
    assert ctx.solve_pcg_rhs(B, lam, _capi.VARS_CURRENT, _capi.PCG_PRECOND_BLOCK_JACOBI, None, 1e-10)[0].tobytes() == Xd.tobytes()
    cov, cs = ctx.marginal_cov([2], lam, _capi.VARS_CURRENT, _capi.PCG_PRECOND_BLOCK_JACOBI, None, 1e-10)      # camera 2: the first unfixed block, 7 unknowns
    cref = np.linalg.inv(Al)[:7, :7]
    cerr = max(np.max(np.abs(cov[:, j] - cref[:, j])) / np.max(np.abs(cref[:, j])) for j in range(7))
    print(f"PCGRHS user0 covariance: against numpy.linalg.inv {cerr:.3e} (of 1e-7)")
    assert cov.shape == (7, 7) and np.all(cs["status"] == 0) and cerr <= 1e-7
    ctx.close()
    print("user kind pcg rhs ok")


if __name__ == "__main__":
    main()
