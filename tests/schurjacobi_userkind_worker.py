"""Worker of tests/test_gpu_schurjacobi.py::test_user_kind_in_a_process_of_its_own (NLLS_AMD_LIB must be set before the library is loaded): nlls_schur_block_diag and
nlls_solve_pcg_schur under NLLS_PCG_PRECOND_SCHUR_JACOBI on a residual kind that exists only as a device template of a USER header (tests/user_kinds/radial_ba.hpp,
NLLS_RES_USER0: 7-dof cameras, 3-dof points) -- the problem of tests/schur_userkind_worker.py -- so that the off-diagonal records of the block launch are those of a
`make user` build.  The blocks are held against the host's reduced system of that library's own sweep to 1e-11 * max(1, kappa) of a block's largest entry, the step
against its direct solve to 1e-7 of its largest entry, as tests/test_gpu_schurjacobi.py holds the built-in kinds."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K, _capi

assert os.environ.get("NLLS_AMD_LIB"), "run through tests/test_gpu_schurjacobi.py"
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
    lam = 1e-2 * np.max(np.abs(np.diag(A)))
    np.linalg.cholesky(A + lam * np.eye(ndof))                          # (the input: positive definite at this damping)
    nred, nelim, is_elim, index = ctx.schur_info(); bs = ctx.block_sizes()
    assert nelim == npts - 2 and nred == 7 * (ncam - 1), "the upload should eliminate the free points: the input is at fault"
    e = np.repeat(is_elim, bs); r = ~e; M = A + lam * np.eye(ndof)
    C = M[np.ix_(e, e)]; E = M[np.ix_(r, e)]; S = M[np.ix_(r, r)] - E @ np.linalg.solve(C, E.T)
    kappa = max(np.linalg.cond(C[k:k + 3, k:k + 3]) for k in range(0, C.shape[0], 3)); tol = 1e-11 * max(1.0, kappa)
    rbs = bs[~is_elim]; rbo = np.concatenate(([0], np.cumsum(rbs)))
    assert np.all(rbs == 7) and np.all(bs[is_elim] == 3), "7-dof cameras should stay, 3-dof points go: the input is at fault"
    D = ctx.schur_block_diag(lam); assert len(D) == rbs.size
    worst = max(np.max(np.abs(d - S[o:o + 7, o:o + 7])) / np.max(np.abs(S[o:o + 7, o:o + 7])) for d, o in zip(D, rbo))
    print(f"SCHURJACOBI user0: ndof {ndof} nred {nred} kappa {kappa:.3e}: worst block {worst:.3e} (of {tol:.3e})")
    assert worst <= tol and all(d.tobytes() == e2.tobytes() for d, e2 in zip(D, ctx.schur_block_diag(lam)))
    ctx.damp(lam); xs = ctx.solve(want_x=True)
    _, sb = ctx.solve_pcg_schur(_capi.PCG_PRECOND_BLOCK_JACOBI, None, 1e-10)
    x, st = ctx.solve_pcg_schur(_capi.PCG_PRECOND_SCHUR_JACOBI, None, 1e-10, want_x=True)
    err = np.max(np.abs(x - xs)) / np.max(np.abs(xs))
    print(f"SCHURJACOBI PCG user0: iterations {st['iterations']} (block Jacobi {sb['iterations']}) status {st['status']} against nlls_solve {err:.3e} (of 1e-7)")
    assert st["status"] == 0 and err <= 1e-7 and x.tobytes() == ctx.get_step().tobytes()
    assert ctx.solve_pcg_schur("schurjacobi", None, 1e-10, want_x=True)[0].tobytes() == x.tobytes()
    ctx.close()
    print("user kind schurjacobi ok")


if __name__ == "__main__":
    main()
