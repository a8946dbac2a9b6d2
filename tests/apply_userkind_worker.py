"""Worker of tests/test_gpu_apply.py::test_user_kind_in_a_process_of_its_own (NLLS_AMD_LIB must be set before the library is loaded): nlls_hess_apply and its siblings
for a residual kind that exists only as a device template of a USER header (tests/user_kinds/radial_ba.hpp, NLLS_RES_USER0), against that library's own sweep: A from
nlls_get_bsm_data, b from nlls_get_grad.  The problem of tests/linearize_userkind_worker.py with some variables fixed; H v and the diagonal blocks to 1e-11 of the
largest entry, as tests/test_gpu_apply.py holds the built-in kinds."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K, _capi

assert os.environ.get("NLLS_AMD_LIB"), "run through tests/test_gpu_apply.py"
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
    meas[rng.random(vi.shape[0]) < 0.1] += 0.1
    p.addcosts(USER0, vi, meas, N.Huber2oKernel(0.004))
    unfixed = np.ones(p.nvariables, bool); unfixed[[0, ncam + 3, ncam + 4]] = False
    bi = np.zeros(p.nvariables, np.uint64); bi[unfixed] = np.arange(1, int(unfixed.sum()) + 1, dtype=np.uint64)
    ctx = _capi.Context(0)
    ctx.upload(p.var_kind, p.var_dim, bi, p.groups()); ctx.set_variables(p.variables)
    ctx.sweep_gradhess(); ndof = ctx.info.ndof
    assert ctx.info.is_sparse and ndof == 7 * (ncam - 1) + 3 * (npts - 2)
    A = bsm_to_csr(ctx.bsm_index(), ctx.get_bsm_data(), ndof).toarray()
    V = rng.standard_normal((3, ndof)); lam = 1e-3 * np.max(np.abs(np.diag(A)))
    rel = lambda a, b: np.max(np.abs(a - b)) / np.max(np.abs(b))
    Y = ctx.hess_apply(V, lam); e_h = rel(Y, V @ A + lam * V)
    bo = np.asarray(ctx.bsm_index()[3], np.int64) - 1; D = ctx.hess_block_diag(lam)
    e_d = max(rel(d, A[bo[k]:bo[k] + d.shape[0], bo[k]:bo[k] + d.shape[0]] + lam * np.eye(d.shape[0])) for k, d in enumerate(D))
    assert sorted({d.shape[0] for d in D}) == [3, 7]
    print(f"APPLY user0: ndof {ndof} H v {e_h:.3e} diagonal blocks {e_d:.3e} (of 1e-11)")
    assert e_h < 1e-11 and e_d < 1e-11
    assert ctx.hess_apply(V[1], lam).tobytes() == Y[1].tobytes()
    x = rng.standard_normal(ndof)
    assert ctx.jac_apply(0, x).shape == (2 * vi.shape[0],) and ctx.jact_apply(0, np.ones(2 * vi.shape[0])).shape == (ndof,)
    ctx.close()
    print("user kind products ok")


if __name__ == "__main__":
    main()
