"""Worker of tests/test_uservar.py (its own process: NLLS_AMD_LIB must be set before the library is loaded).  A library built with a user header of USER VARIABLE kinds
(tests/user_kinds/manifold_ba.hpp: `make user USER_KINDS=...`) runs three variable types the registry does not have, each under a user residual kind over it:
  a. USERVAR0 / USER0, the SO(3) pose and its pinhole restated generically: the twin of POSE_SO3 / BA_SO3, so the oracle holds it (the same numbers as the built-in problem);
  b. USERVAR1 / USER1, a unit-quaternion pose: cost against numpy, gradient against central differences through a numpy update(), a noise-free problem to its optimum;
  c. USERVAR2 / USER2, a unit 3-vector (storage 3, dof 2): optimize and optimizesingles converge, the norm stays 1, nlls_retract = the numpy update()."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K, synthetic, _capi
from oracle import oracle as O
from tests.helpers import oracle_problem, blockindices

assert os.environ.get("NLLS_AMD_LIB"), "run through tests/test_uservar.py"
USERVAR0, USERVAR1, USERVAR2 = 100, 101, 102
USER0, USER1, USER2 = 100, 101, 102
try:
    K.register_user_var(USERVAR0, 7, 6); raise AssertionError("register_user_var accepted sizes the library does not declare")
except ValueError:
    pass
K.register_user_var(USERVAR0, 12, 6); K.register_user_var(USERVAR1, 7, 6); K.register_user_var(USERVAR2, 3, 2)
K.register_user_kind(USER0, 2, 2, 2, ((USERVAR0, 6), (K.VAR_EUCLIDEAN, 3)))
K.register_user_kind(USER1, 2, 2, 2, ((USERVAR1, 6), (K.VAR_EUCLIDEAN, 3)))
K.register_user_kind(USER2, 1, 3, 3, ((USERVAR2, 2),))
RTOL, RTOL_X = 1e-11, 1e-7          # tests/test_gpu_parity.py's check_problem: sweeps, damped step


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


# ---- a. the twin of the built-in SO(3) bundle adjustment -------------------------------------------------------------------------------------------------
def so3_problem(ncam, npts, prop, seed=3, noise=1e-3):
    return synthetic.perturb_ba_problem(synthetic.create_so3_ba_problem(ncam, npts, prop, seed=seed, adaptive=False, noise=noise, outlier_frac=0.0), 1e-3, 1e-3)


def twin(p):
    """the same variables, costs and data with the poses as USERVAR0 and the blocks as USER0"""
    t = N.NLLSProblem(); v = p.variables; npose = int((p.var_kind == K.VAR_POSE_SO3).sum())
    assert np.all(p.var_kind[:npose] == K.VAR_POSE_SO3)
    t.addvariables(v[:12 * npose].reshape(npose, 12), USERVAR0)
    t.addvariables(v[12 * npose:].reshape(-1, 3))
    (g,) = p.costs.values(); vi, da = g.arrays()
    t.addcosts(USER0, vi, da, g.robust)
    return t


def check_twin():
    p = so3_problem(40, 1500, 0.15); t = twin(p)
    bi = blockindices(p); op = oracle_problem(p); ols = op.linear_system(bi)
    cb, ct = _capi.Context(0), _capi.Context(0)
    ib = cb.upload(p.var_kind, p.var_dim, bi, p.groups()); it = ct.upload(t.var_kind, t.var_dim, bi, t.groups())
    assert it.is_sparse and it.has_schur and it.ndof == ib.ndof and it.nnz_data == ib.nnz_data, (it.is_sparse, it.has_schur)
    for g_, o_ in zip(ct.bsm_index(), ols.bsm_index()):
        assert np.array_equal(g_, o_)
    cb.set_variables(p.variables); ct.set_variables(t.variables)
    c_b, c_t, c_o = cb.sweep_gradhess(), ct.sweep_gradhess(), ols.costgradhess()
    assert np.isclose(c_t, c_b, rtol=1e-13, atol=0) and np.isclose(c_t, c_o, rtol=RTOL), (c_t, c_b, c_o)
    assert np.isclose(ct.sweep_cost(), c_b, rtol=1e-13, atol=0)
    assert rel(ct.get_bsm_data(), ols.data) < RTOL, "A.data"
    assert rel(ct.get_grad(), ols.b) < RTOL, "b"
    # the LM trial on both paths: matrix-free (reduced USERVAR0 cameras next to Euclidean points), then materialised
    lam = ols.max_abs_diag() * 1e-6; assert ols.solve(lam) == 0
    n0 = ct.solve_stats()["mf_trials"]
    c_mf = ct.lm_trial(lam); st = ct.solve_stats()
    assert st["mf_trials"] == n0 + 1 and st["status"] == 0 and st["dropped_pivots"] == 0, st
    x_mf = ct.get_step(); assert rel(x_mf, ols.x) < RTOL_X, ("mf step", rel(x_mf, ols.x))
    v_mf = ct.get_variables(_capi.VARS_NEXT)
    ct.set_option(_capi.OPT_MATERIALIZE, 1)
    c_mat = ct.lm_trial(0.0)
    assert ct.solve_stats()["mf_trials"] == n0 + 1
    x_mat = ct.get_step(); assert rel(x_mat, ols.x) < RTOL_X, ("materialised step", rel(x_mat, ols.x))
    assert rel(x_mf, x_mat) < 1e-9 and rel(v_mf, ct.get_variables(_capi.VARS_NEXT)) < 1e-11 and np.isclose(c_mf, c_mat, rtol=1e-9), (rel(x_mf, x_mat), c_mf, c_mat)
    # the retraction: update() of USERVAR0 against the built-in POSE_SO3's (the oracle's) with the same step
    ct.retract(_capi.VARS_NEXT, _capi.VARS_CURRENT)
    op.set_variables(p.variables, O.VARS_NEXT); op.update(ols, O.VARS_NEXT, O.VARS_CURRENT, step=x_mat)
    assert rel(ct.get_variables(_capi.VARS_NEXT), op.get_variables(O.VARS_NEXT)) < 1e-13
    # the trial point's cost against the oracle's cost of the same point
    assert np.isclose(ct.sweep_cost(_capi.VARS_NEXT), op.cost(O.VARS_NEXT), rtol=RTOL)
    cb.close()
    # ten iterations of the library's own LM loop (nlls_lm_iterations) from the start, against the oracle's optimize
    ores = oracle_problem(p).optimize(maxiters=10)
    ct.set_option(_capi.OPT_MATERIALIZE, 0); ct.set_variables(t.variables); c0 = ct.sweep_gradhess()
    opt = _capi.LmOptions(reldcost=1e-15, absdcost=1e-15, dstep=1e-15, maxfails=3, maxiters=10, stoptime_ns=0)
    lst = _capi.LmState(); lst.bestcost = c0; lst.cost = c0
    ct.lm_iterations(opt, lst, 10)
    assert np.isclose(lst.bestcost, ores.bestcost, rtol=1e-8), (lst.bestcost, ores.bestcost)
    ct.close()
    t2 = twin(p); res = N.optimize(t2, N.NLLSOptions(maxiters=10))
    assert np.isclose(res.bestcost, ores.bestcost, rtol=1e-8), (res.bestcost, ores.bestcost)
    print(f"twin: cost {c_t:.6e} = built-in, A / b / both trial steps = oracle (mf trials {st['mf_trials']}), retraction = POSE_SO3's, "
          f"10 LM iterations -> {lst.bestcost:.6e} (lm_iterations) / {res.bestcost:.6e} (optimize) = oracle {ores.bestcost:.6e}")
    # optimizesingles on the cameras: the per-variable kernel retracts with USERVAR0's update<double>
    pb, pt = so3_problem(40, 1500, 0.15), twin(so3_problem(40, 1500, 0.15))
    cams = np.arange(1, 41)
    ib_ = N.optimizesingles(pb, N.NLLSOptions(), cams); it_ = N.optimizesingles(pt, N.NLLSOptions(), cams)
    assert rel(pt.variables, pb.variables) < 1e-9 and np.isclose(N.cost(pt), N.cost(pb), rtol=1e-9), (rel(pt.variables, pb.variables), N.cost(pt), N.cost(pb))
    print(f"twin: optimizesingles on the cameras = built-in ({int(it_.sum())} / {int(ib_.sum())} iterations)")
    # the reduced system by each solver: the band, the dense reduced system (NLLS_FLAG_NO_BAND), the small dense route (< 64 reduced dof)
    for (ncam, npts, prop, flags, mode) in ((40, 1500, 0.15, 0, 2), (40, 1500, 0.15, _capi.FLAG_NO_BAND, 1), (8, 400, 0.5, 0, 0)):
        q = so3_problem(ncam, npts, prop); tq = twin(q); bq = blockindices(q)
        oq = oracle_problem(q).linear_system(bq); oq.costgradhess()
        c = _capi.Context(0); info = c.upload(tq.var_kind, tq.var_dim, bq, tq.groups(), flags)
        c.set_variables(tq.variables); c.sweep_gradhess()
        lam = oq.max_abs_diag() * 1e-6; c.damp(lam); x = c.solve(want_x=True); assert oq.solve(lam) == 0
        s = c.solve_stats(); c.close()
        assert info.solve_mode == mode and s["dropped_pivots"] == 0, (flags, info.solve_mode, mode)
        assert rel(x, oq.x) < RTOL_X, (flags, rel(x, oq.x))
        print(f"twin: reduced solve mode {info.solve_mode} (bcr launches {s['bcr_launches']}) = oracle, {info.nreduced_dof} reduced dof")


# ---- b. unit-quaternion bundle adjustment -----------------------------------------------------------------------------------------------------------------
def quat_update(q, w):
    """numpy statement of USERVAR1's update: q * exp(w[:3] / 2) normalised, t + w[3:]"""
    w = np.asarray(w, np.float64); th2 = float(w[:3] @ w[:3])
    if th2 < 1e-12: c, s = 1.0 - th2 / 8.0, 0.5 - th2 / 48.0
    else: th = np.sqrt(th2); c, s = np.cos(th / 2), np.sin(th / 2) / th
    e = np.r_[c, s * w[:3]]; a = q[:4]
    r = np.array([a[0] * e[0] - a[1] * e[1] - a[2] * e[2] - a[3] * e[3], a[0] * e[1] + a[1] * e[0] + a[2] * e[3] - a[3] * e[2],
                  a[0] * e[2] - a[1] * e[3] + a[2] * e[0] + a[3] * e[1], a[0] * e[3] + a[1] * e[2] - a[2] * e[1] + a[3] * e[0]])
    return np.r_[r / np.linalg.norm(r), q[4:] + w[3:]]


def quat_project(P, X):
    """(n, 7) poses, (n, 3) points -> (n, 2) projections"""
    qw, u, t = P[:, 0:1], P[:, 1:4], P[:, 4:7]
    c = np.cross(u, X); Y = X + 2.0 * (qw * c + np.cross(u, c)) + t
    return Y[:, :2] / Y[:, 2:3]


def quat_problem(ncam, npts, prop, seed=4):
    rng = np.random.default_rng(seed)
    poses = np.zeros((ncam, 7))
    for i in range(ncam):
        poses[i] = quat_update(np.r_[1.0, 0, 0, 0, 0, 0, 0], np.r_[0.05 * rng.standard_normal(), -0.3 + 0.6 * i / max(ncam - 1, 1), 0.05 * rng.standard_normal(),
                                                                    0.2 * rng.standard_normal(2), 0.1 * rng.standard_normal()])
    pts = rng.random((npts, 3)) + np.array([-0.5, -0.5, 5.0])
    cam, lm = synthetic.ba_visibility(ncam, npts, prop)
    p = N.NLLSProblem(); p.addvariables(poses, USERVAR1); p.addvariables(pts)
    vi = np.stack([cam, lm + ncam], 1)
    p.addcosts(USER1, vi, quat_project(poses[cam - 1], pts[lm - 1]))
    return p, vi, ncam


def quat_cost(p, vi, ncam, v):
    P = v[:7 * ncam].reshape(ncam, 7); X = v[7 * ncam:].reshape(-1, 3)
    (g,) = p.costs.values(); meas = g.arrays()[1]
    r = quat_project(P[vi[:, 0] - 1], X[vi[:, 1] - 1 - ncam]) - meas
    return 0.5 * float((r * r).sum())


def quat_perturb(v, ncam, rng, sp=1e-3, sx=1e-3):
    v = v.copy()
    for i in range(ncam): v[7 * i:7 * i + 7] = quat_update(v[7 * i:7 * i + 7], sp * rng.standard_normal(6))
    v[7 * ncam:] += sx * rng.standard_normal(v.size - 7 * ncam)
    return v


def check_quaternion():
    p, vi, ncam = quat_problem(40, 1500, 0.15); rng = np.random.default_rng(6)
    start = quat_perturb(p.variables, ncam, rng)
    ctx = _capi.Context(0); bi = blockindices(p)
    info = ctx.upload(p.var_kind, p.var_dim, bi, p.groups()); assert info.is_sparse and info.has_schur
    ctx.set_variables(start)
    c_dev, c_np = ctx.sweep_gradhess(), quat_cost(p, vi, ncam, start)
    assert np.isclose(c_dev, c_np, rtol=1e-11), (c_dev, c_np)
    b = ctx.get_grad()
    # the gradient against central differences of the numpy cost, taken in the tangent through the numpy update(): camera i's dof 6 i .. 6 i + 5, point j's after them
    for k in np.r_[rng.choice(6 * ncam, 16, replace=False), 6 * ncam + rng.choice(b.size - 6 * ncam, 8, replace=False)]:
        h = 1e-6; vp, vm = start.copy(), start.copy()
        if k < 6 * ncam:
            i, j = divmod(int(k), 6); e = np.zeros(6); e[j] = h
            vp[7 * i:7 * i + 7] = quat_update(start[7 * i:7 * i + 7], e); vm[7 * i:7 * i + 7] = quat_update(start[7 * i:7 * i + 7], -e)
        else:
            o = 7 * ncam + (int(k) - 6 * ncam); vp[o] += h; vm[o] -= h
        fd = (quat_cost(p, vi, ncam, vp) - quat_cost(p, vi, ncam, vm)) / (2 * h)
        assert abs(fd - b[k]) <= 1e-6 * max(1.0, np.max(np.abs(b))), (k, fd, b[k])
    # the matrix-free and the materialised trial agree
    lam = 1e-6 * ctx.max_abs_diag(); n0 = ctx.solve_stats()["mf_trials"]
    c_mf = ctx.lm_trial(lam); st = ctx.solve_stats(); x_mf = ctx.get_step()
    assert st["mf_trials"] == n0 + 1 and st["status"] == 0, st
    ctx.set_option(_capi.OPT_MATERIALIZE, 1); c_mat = ctx.lm_trial(0.0); x_mat = ctx.get_step()
    assert rel(x_mf, x_mat) < 1e-9 and np.isclose(c_mf, c_mat, rtol=1e-9), (rel(x_mf, x_mat), c_mf, c_mat)
    ctx.close()
    # noise-free: to the zero-residual optimum, every quaternion of unit length
    p.variables[:] = start
    res = N.optimize(p, N.NLLSOptions(maxiters=60))
    assert res.bestcost < 1e-15 * len(vi), (res.bestcost, res.niterations)
    qn = np.linalg.norm(p.variables[:7 * ncam].reshape(ncam, 7)[:, :4], axis=1)
    assert np.max(np.abs(qn - 1.0)) <= 1e-14, np.max(np.abs(qn - 1.0))
    print(f"quaternion BA: cost = numpy, gradient = central differences through update(), mf step = materialised, optimize -> {res.bestcost:.2e} in {res.niterations} iterations, |q| = 1")


# ---- c. unit 3-vectors ------------------------------------------------------------------------------------------------------------------------------------
def dir_update(v, d):
    """numpy statement of USERVAR2's update"""
    b1 = np.array([v[2], 0.0, -v[0]]) if abs(v[0]) > 0.5 else np.array([0.0, -v[2], v[1]])
    b1 = b1 * (1.0 / np.sqrt(b1 @ b1)); b2 = np.cross(v, b1)
    u = d[0] * b1 + d[1] * b2 + v
    return u * (1.0 / np.sqrt(u @ u))


def dir_problem(nv, nmeas, seed=8):
    rng = np.random.default_rng(seed)
    truth = rng.standard_normal((nv, 3)); truth /= np.linalg.norm(truth, axis=1, keepdims=True)
    p = N.NLLSProblem()
    start = np.array([dir_update(t, 0.3 * rng.standard_normal(2)) for t in truth])
    p.addvariables(start, USERVAR2)
    vi = np.repeat(np.arange(1, nv + 1), nmeas)
    meas = truth[vi - 1] + 0.05 * rng.standard_normal((vi.size, 3))
    p.addcosts(USER2, vi[:, None], meas)
    opt = np.array([m / np.linalg.norm(m) for m in (meas.reshape(nv, nmeas, 3).sum(1))])     # the optimum on the sphere: the normalised sum
    return p, opt


def check_direction():
    p, opt = dir_problem(300, 5)
    # nlls_retract against the numpy update
    # (NLLS_FLAG_NO_SCHUR: with every block eliminated and no reduced system left, the Schur path returns a zero step -- for built-in Euclidean blocks as well)
    ctx = _capi.Context(0); bi = blockindices(p); ctx.upload(p.var_kind, p.var_dim, bi, p.groups(), _capi.FLAG_NO_SCHUR)
    v0 = p.variables.copy(); ctx.set_variables(v0); ctx.sweep_gradhess()
    ctx.damp(1e-3 * ctx.max_abs_diag()); x = ctx.solve(want_x=True); ctx.retract(_capi.VARS_NEXT, _capi.VARS_CURRENT)
    assert np.max(np.abs(x)) > 0.1, np.max(np.abs(x))
    want = np.concatenate([dir_update(v0[3 * i:3 * i + 3], x[2 * i:2 * i + 2]) for i in range(300)])
    assert rel(ctx.get_variables(_capi.VARS_NEXT), want) < 1e-13, rel(ctx.get_variables(_capi.VARS_NEXT), want)
    ctx.close()
    res = N.optimize(p, N.NLLSOptions(maxiters=50), flags=_capi.FLAG_NO_SCHUR)
    V = p.variables.reshape(-1, 3)
    assert np.max(np.abs(V - opt)) < 1e-9 and np.max(np.abs(np.linalg.norm(V, axis=1) - 1.0)) <= 1e-14, (np.max(np.abs(V - opt)), res.niterations)
    q, opt2 = dir_problem(300, 5)
    it = N.optimizesingles(q, N.NLLSOptions(), np.arange(1, 301))
    V2 = q.variables.reshape(-1, 3)
    assert it.min() >= 1 and np.max(np.abs(V2 - opt2)) < 1e-7 and np.max(np.abs(np.linalg.norm(V2, axis=1) - 1.0)) <= 1e-14, np.max(np.abs(V2 - opt2))
    print(f"unit 3-vectors: retraction = numpy update(), optimize ({res.niterations} iterations) and optimizesingles reach the normalised mean, |v| = 1")


if __name__ == "__main__":
    check_twin(); check_quaternion(); check_direction()
    print("user variable kinds ok")
