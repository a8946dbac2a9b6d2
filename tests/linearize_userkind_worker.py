"""Worker of tests/test_gpu_linearize.py::test_user_kind_in_a_process_of_its_own (NLLS_AMD_LIB must be set before the library is loaded): nlls_eval_jacobians /
nlls_eval_gradhess for a residual kind that exists only as a device template of a USER header (tests/user_kinds/radial_ba.hpp, NLLS_RES_USER0).  No oracle has the kind:
J is held against central differences of nlls_eval_blocks' r, taken through nlls_set_step + nlls_retract into VARS_NEXT with h = 1e-6, to rtol 1e-6, atol 1e-7 (what
tests/test_oracle_pins.py::test_so3_kinds_against_finite_differences uses for that comparison); g and H against rho' J'r and rho' J'J + 2 rho'' (J'r)(J'r)' formed from
the device's own J and r and the closed-form Huber derivatives (src/robust.jl:48-55), to 1e-11 of the block's largest entry."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K, _capi

assert os.environ.get("NLLS_AMD_LIB"), "run through tests/test_gpu_linearize.py"
USER0 = 100
K.register_user_kind(USER0, 2, 2, 2, ((K.VAR_EUCLIDEAN, 7), (K.VAR_EUCLIDEAN, 3)))


def main():
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
    width = 0.004; n = vi.shape[0]
    p.addcosts(USER0, vi, meas, N.Huber2oKernel(width))
    ctx = _capi.Context(0)
    ctx.upload(p.var_kind, p.var_dim, np.arange(1, p.nvariables + 1, dtype=np.uint64), p.groups()); ctx.set_variables(p.variables)
    assert ctx.L.nlls_res_jac_cols(USER0) == 10 and ctx.L.nlls_res_gh_dim(USER0) == 10
    jac = ctx.eval_jacobians(0); gh = ctx.eval_gradhess(0); J, r = jac["J"], jac["r"]
    assert J.shape == (n, 2, 10) and gh["H"].shape == (n, 10, 10)
    assert r.tobytes() == ctx.eval_blocks(0, want="r")["r"].tobytes()
    # central differences: every block depends on ONE camera and ONE point, so a step that moves tangent entry q of every camera (or point) at once moves each block along
    # its own column q
    bo = np.asarray(ctx.bsm_index()[3], np.int64) - 1; ndof = ctx.info.ndof; h = 1e-6
    Jfd = np.zeros_like(J)
    for first, dof, col0 in ((0, 7, 0), (ncam, 3, 7)):
        nv = ncam if first == 0 else npts
        for q in range(dof):
            rr = []
            for sgn in (1.0, -1.0):
                x = np.zeros(ndof); x[bo[first:first + nv] + q] = sgn * h
                ctx.set_step(x); ctx.retract(_capi.VARS_NEXT, _capi.VARS_CURRENT)
                rr.append(ctx.eval_blocks(0, _capi.VARS_NEXT, want="r")["r"])
            Jfd[:, :, col0 + q] = (rr[0] - rr[1]) / (2 * h)
    efd = np.max(np.abs(J - Jfd) - 1e-6 * np.abs(Jfd))
    print(f"LINEARIZE user0: n={n} J against central differences: largest |J - Jfd| - 1e-6 |Jfd| = {efd:.3e} (of 1e-7), max |J| {np.max(np.abs(J)):.3e}")
    assert np.allclose(J, Jfd, rtol=1e-6, atol=1e-7)
    assert np.max(np.abs(J[:, :, 6])) > 0 and np.max(np.abs(J[:, :, 7:])) > 0
    # g == rho' J'r and H == rho' J'J + 2 rho'' (J'r)(J'r)' from the device's own J and r; Huber2oKernel in closed form
    sq = (r * r).sum(1); hi = sq >= width * width; root = np.sqrt(np.maximum(sq, 1e-300))
    assert 0 < hi.sum() < n and np.min(np.abs(sq - width * width)) > 1e-9 * width * width
    rho = np.where(hi, 2 * width * root - width * width, sq); d1 = np.where(hi, width / root, 1.0); d2 = np.where(hi, (-0.5 * width) / (sq * root), 0.0)
    Jtr = np.einsum("nmj,nm->nj", J, r); JtJ = np.einsum("nmi,nmj->nij", J, J)
    g_ref = d1[:, None] * Jtr; H_ref = d1[:, None, None] * JtJ + 2.0 * d2[:, None, None] * Jtr[:, :, None] * Jtr[:, None, :]
    bm = lambda a: np.max(np.abs(a.reshape(n, -1)), axis=1)
    ec = np.max(np.abs(gh["cost"] - 0.5 * rho) / (0.5 * rho)); eg = np.max(bm(gh["g"] - g_ref) / bm(g_ref)); eh = np.max(bm(gh["H"] - H_ref) / bm(H_ref))
    print(f"LINEARIZE user0: cost {ec:.3e} g {eg:.3e} H {eh:.3e} (of 1e-11)")
    assert ec <= 1e-11 and eg <= 1e-11 and eh <= 1e-11
    ctx.close()
    print("user kind linearisation ok")


if __name__ == "__main__":
    main()
