"""Worker of tests/test_userrobust.py (its own process: NLLS_AMD_LIB must be set before the library is loaded).  A library built with a user header of USER ROBUST
kernels (tests/user_kinds/robust_kernels.hpp: `make user USER_KINDS=...`) runs six robustifiers, three of them twins of the built-in ones:
  a. kernel values: nlls_robustify (the device functions every kernel calls) against numpy closed forms, with and without Scaled, built-in kernels included;
  b. twins (USER0 = Huber2o by autodiff, USER1 = Huber with its own dcost, USER2 = Geman-McClure by autodiff, and Scaled): cost, b and A.data equal the built-in's,
     LM through both trial paths and optimizesingles equal the oracle's run with the built-in kernel;
  c. Cauchy, Barron and Tukey: cost against numpy, b and H against central differences, optimize converges with the cost never rising, both trial paths agree;
     a point whose observations all lie beyond Tukey's width (rho' = 0) stays finite; an id the build lacks is refused at upload."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K, synthetic, _capi
from tests.helpers import oracle_problem, blockindices, bsm_to_csr
from tests.test_gpu_functional import _oracle_optimizesingles

assert os.environ.get("NLLS_AMD_LIB"), "run through tests/test_userrobust.py"
U0, U1, U2, U3, U4, U5 = range(K.ROBUST_USER0, K.ROBUST_USER0 + 6)
NPARAM = {U0: 1, U1: 1, U2: 1, U3: 1, U4: 2, U5: 1}
try:
    K.register_user_robust(U4, 1); raise AssertionError("register_user_robust accepted an NPARAM the library does not declare")
except ValueError:
    pass
for k, n in NPARAM.items():
    K.register_user_robust(k, n)
RTOL, RTOL_X = 1e-11, 1e-7          # tests/test_gpu_parity.py's check_problem: sweeps, damped step
CONVERGED = (1 << 2) | (1 << 3) | (1 << 6)                              # optimizer.py: the reference's relative / absolute cost decrease and step-size flags
BAD = (1 << 0) | (1 << 1) | (1 << 4) | (1 << 5)                         # inf / NaN cost or step


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def close(a, b, rtol=1e-13):
    """|a - b| <= rtol |b| elementwise (an exact zero must be met exactly)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.isfinite(a)) and np.all(np.abs(a - b) <= rtol * np.abs(b)))


# ---- a. kernel values --------------------------------------------------------------------------------------------------------------------------------------
def closed_form(rob, s):
    """(robustify, rho', rho'') of a Robustifier at costs s, in closed form (src/robust.jl; the header's formulas)"""
    base, p = rob.kind & 0xF, rob.params
    s = np.asarray(s, np.float64); w = p[0]; w2 = w * w
    with np.errstate(all="ignore"):
        if base == K.ROBUST_NONE:
            rho, d1, d2 = s, np.ones_like(s), np.zeros_like(s)
        elif base in (K.ROBUST_HUBER, K.ROBUST_HUBER2O, U0, U1):
            sq = np.sqrt(s); hi = s >= w2; second = base in (K.ROBUST_HUBER2O, U0)
            rho = np.where(hi, sq * (w * 2) - w2, s); d1 = np.where(hi, w / sq, 1.0); d2 = np.where(hi & second, (-0.5 * w) / (s * sq), 0.0)
        elif base in (K.ROBUST_GEMAN_MCCLURE, U2):
            rho = s * w2 / (s + w2); d1 = (w2 / (s + w2)) ** 2; d2 = -2.0 * d1 / (s + w2)
        elif base == U3:                                            # Cauchy
            t = s / w2; rho = w2 * np.log1p(t); d1 = 1.0 / (1.0 + t); d2 = -1.0 / (w2 * (1.0 + t) ** 2)
        elif base == U4:                                            # Barron: c = p[0], alpha = p[2]
            c, a = p[0], p[2]; b = c * c * abs(a - 2.0); x = 1.0 + s / b
            rho = 2.0 * b / a * np.expm1(0.5 * a * np.log1p(s / b)); d1 = x ** (0.5 * a - 1.0); d2 = (0.5 * a - 1.0) / b * x ** (0.5 * a - 2.0)
        elif base == U5:                                            # Tukey
            u = 1.0 - s / w2; lo = s < w2
            rho = np.where(lo, w2 / 3.0 * (1.0 - u ** 3), w2 / 3.0); d1 = np.where(lo, u * u, 0.0); d2 = np.where(lo, -2.0 * u / w2, 0.0)
        else:
            raise ValueError(rob.kind)
    if rob.kind & K.ROBUST_SCALED:
        rho, d1, d2 = rho * p[1], d1 * p[1], d2 * p[1]
    return rho, d1, d2


def grid(scale2):
    return np.array([0.0, 1e-300, 0.75 * scale2, scale2, 1.25 * scale2, 1e6])


def check_values():
    ctx = _capi.Context(0)
    w, h, c = 0.7, 2.5, 0.5
    kernels = [N.NoRobust(), N.HuberKernel(w), N.Huber2oKernel(w), N.GemanMcclureKernel(w)] + [N.UserRobust(k, w) for k in (U0, U1, U2, U3, U5)] + \
              [N.UserRobust(U4, c, a) for a in (1.0, -2.0, 0.5, 4.0)]
    n = 0
    for rob in kernels:
        for r in (rob, N.Scaled(rob, h)):
            s = grid(c * c if (r.kind & 0xF) == U4 else w * w)
            out = ctx.robustify(r, s); rho, d1, d2 = closed_form(r, s)
            for q, (name, want) in enumerate((("robustify", rho), ("rho", rho), ("rho'", d1), ("rho''", d2))):
                assert close(out[:, q], want), (r.kind, r.params, name, out[:, q], want)
            n += 1
    # Barron with alpha = -2 is Geman-McClure with w = 2 c
    s = grid(c * c)
    assert close(ctx.robustify(N.UserRobust(U4, c, -2.0), s), ctx.robustify(N.GemanMcclureKernel(2 * c), s)), "Barron(alpha = -2) != Geman-McClure(2 c)"
    # an id the build does not have
    try:
        ctx.robustify(K.Robustifier(U5 + 1, (w,)), s); raise AssertionError("nlls_robustify accepted id 14")
    except _capi.NllsError as e:
        assert e.code == _capi.ERR_UNSUPPORTED, e.code
    ctx.close()
    print(f"kernel values: {n} kernels (built-in and USER0 .. 5, with and without Scaled) = numpy closed forms to 1e-13; Barron(-2) = Geman-McClure(2c); id 14 refused")


# ---- b. the twins of the built-in kernels --------------------------------------------------------------------------------------------------------------------
W = 0.02
FAMILIES = {
    "affine": lambda rob: synthetic.perturb_ba_problem(synthetic.create_ba_problem(40, 1500, 0.15, seed=7, robust=rob, outlier_frac=0.1, outlier_sigma=0.05), 1e-3, 1e-3),
    "so3": lambda rob: synthetic.perturb_ba_problem(synthetic.create_so3_ba_problem(40, 1500, 0.15, seed=3, adaptive=False, robust=rob, outlier_frac=0.1,
                                                                                    outlier_sigma=0.05, noise=1e-3), 1e-3, 1e-3),
}
PAIRS = [("Huber2o", N.Huber2oKernel(W), N.UserRobust(U0, W)), ("Huber", N.HuberKernel(W), N.UserRobust(U1, W)),
         ("GemanMcclure", N.GemanMcclureKernel(W), N.UserRobust(U2, W)), ("Scaled(Huber2o)", N.Scaled(N.Huber2oKernel(W), 2.5), N.Scaled(N.UserRobust(U0, W), 2.5))]


def optimize_tracked(p, flags, maxiters):
    """N.optimize with a callback that records the trial costs and the matrix-free trial count of the linear system"""
    costs, mf = [], [0]
    def cb(cost, problem, data, *unused):
        costs.append(cost); mf[0] = data.linsystem.ctx.solve_stats()["mf_trials"]; return cost, 0
    res = N.optimize(p, N.NLLSOptions(maxiters=maxiters), callback=cb, flags=flags)
    return res, costs, mf[0]


def check_twins():
    for fam, mk in FAMILIES.items():
        for name, builtin, user in PAIRS:
            pb, pt = mk(builtin), mk(user)
            assert np.array_equal(pb.variables, pt.variables)
            bi = blockindices(pb)
            cb, ct = _capi.Context(0), _capi.Context(0)
            ib = cb.upload(pb.var_kind, pb.var_dim, bi, pb.groups()); it = ct.upload(pt.var_kind, pt.var_dim, bi, pt.groups())
            assert it.is_sparse and it.has_schur and it.ndof == ib.ndof and it.nnz_data == ib.nnz_data
            cb.set_variables(pb.variables); ct.set_variables(pt.variables)
            c_b, c_t = cb.sweep_gradhess(), ct.sweep_gradhess()
            assert close(c_t, c_b), (fam, name, c_t, c_b)
            assert close(ct.sweep_cost(), c_b), (fam, name)
            assert rel(ct.get_grad(), cb.get_grad()) <= 1e-13, (fam, name, "b", rel(ct.get_grad(), cb.get_grad()))
            assert rel(ct.get_bsm_data(), cb.get_bsm_data()) <= 1e-13, (fam, name, "A.data", rel(ct.get_bsm_data(), cb.get_bsm_data()))
            cb.close(); ct.close()
            # optimize with the twin, matrix-free trial and materialised trial, against the oracle's run with the built-in kernel
            maxiters = 10
            ores = oracle_problem(mk(builtin)).optimize(maxiters=maxiters)
            got = []
            for flags, want_mf in ((0, True), (_capi.FLAG_MATERIALIZE, False)):
                q = mk(user); res, costs, mf = optimize_tracked(q, flags, maxiters)
                assert (mf > 0) == want_mf, (fam, name, flags, mf)
                assert np.isclose(res.bestcost, ores.bestcost, rtol=RTOL_X), (fam, name, flags, res.bestcost, ores.bestcost)
                got.append(res.bestcost)
            print(f"twin {name} ({fam}): cost / b / A.data = built-in, optimize -> {got[0]:.9e} (mf) / {got[1]:.9e} (materialised) = oracle {ores.bestcost:.9e}")
        # optimizesingles of the points with a twin against the oracle's with the built-in kernel (affine: Euclidean points next to affine cameras)
        if fam == "affine":
            for name, builtin, user in PAIRS:
                pb, pt = mk(builtin), mk(user)
                pts = np.nonzero((pb.var_kind == K.VAR_EUCLIDEAN) & (pb.var_dim == 3))[0] + 1
                expect = _oracle_optimizesingles(pb, pts)
                it_ = N.optimizesingles(pt, N.NLLSOptions(), indices=pts)
                assert it_.min() >= 1 and np.max(np.abs(pt.variables - expect)) < 1e-7, (name, np.max(np.abs(pt.variables - expect)))
            print(f"twins: optimizesingles of the {pts.size} points = oracle with the built-in kernels")


# ---- c. Cauchy, Barron, Tukey ---------------------------------------------------------------------------------------------------------------------------
def affine_cost(p, rob, v):
    """0.5 sum rho(|r|^2) of the affine BA of synthetic.create_ba_problem at packed variables v (numpy)"""
    (g,) = p.costs.values(); vi, meas = g.arrays()
    ncam = int(np.sum(p.var_dim == 6)); C = v[:6 * ncam].reshape(ncam, 6); X = v[6 * ncam:].reshape(-1, 3)
    c, x = C[vi[:, 0] - 1], X[vi[:, 1] - 1 - ncam]
    r = np.stack([(c[:, 0:3] * x).sum(1), (c[:, 3:6] * x).sum(1)], 1) - meas
    return 0.5 * float(np.sum(closed_form(rob, (r * r).sum(1))[0]))


def contaminated(rob, far_point=False, seed=21):
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(40, 1500, 0.15, seed=seed, robust=rob, outlier_frac=0.1, outlier_sigma=0.05), 1e-3, 1e-3)
    if far_point:                                                   # every observation of one point far beyond the kernel's width: rho' = 0 on all of them
        (g,) = p.costs.values(); vi, meas = g.arrays(); ncam = 40
        j = int(np.bincount(vi[:, 1]).argmax())
        meas = meas.copy(); meas[vi[:, 1] == j] += 1.0
        g.set_arrays(vi, meas); p._gpu = None
        return p, j
    return p, None


def check_new_kernels():
    rng = np.random.default_rng(9)
    for name, rob, far in (("Cauchy", N.UserRobust(U3, 0.02), False), ("Barron(1)", N.UserRobust(U4, 0.02, 1.0), False),
                           ("Barron(-3)", N.UserRobust(U4, 0.02, -3.0), False), ("Tukey", N.UserRobust(U5, 0.05), True)):
        p, jfar = contaminated(rob, far)
        bi = blockindices(p); ctx = _capi.Context(0); info = ctx.upload(p.var_kind, p.var_dim, bi, p.groups())
        v0 = p.variables.copy(); ctx.set_variables(v0)
        c_dev = ctx.sweep_gradhess(); c_np = affine_cost(p, rob, v0)
        assert np.isclose(c_dev, c_np, rtol=RTOL), (name, c_dev, c_np)
        b = ctx.get_grad(); H = bsm_to_csr(ctx.bsm_index(), ctx.get_bsm_data(), info.ndof)
        assert np.all(np.isfinite(b)) and np.all(np.isfinite(H.data)), name
        ncd = 6 * 40
        # b against central differences of the device cost (the variables are Euclidean: dof k is packed entry k)
        def dcost(k, hh):
            vp, vm = v0.copy(), v0.copy(); vp[k] += hh; vm[k] -= hh
            ctx.set_variables(vp); cp_ = ctx.sweep_cost(); ctx.set_variables(vm); cm_ = ctx.sweep_cost()
            return (cp_ - cm_) / (2 * hh)
        for k in np.r_[rng.choice(ncd, 10, replace=False), ncd + rng.choice(b.size - ncd, 10, replace=False)]:
            fd = dcost(int(k), 1e-6)
            assert abs(fd - b[k]) <= 1e-6 * np.max(np.abs(b)), (name, k, fd, b[k])
        # H v against central differences of b, along cameras only and along points only, on the rows of the same kind (the residual is bilinear in a camera and a
        # point: its second derivatives couple the two kinds only, so these rows of the Gauss-Newton H with the robust correction are the exact Hessian's)
        for sel in (np.arange(ncd), np.arange(ncd, b.size)):
            vdir = np.zeros(b.size); vdir[sel] = rng.standard_normal(sel.size)
            def db(hh):
                ctx.set_variables(v0 + hh * vdir); ctx.sweep_gradhess(); bp = ctx.get_grad()
                ctx.set_variables(v0 - hh * vdir); ctx.sweep_gradhess(); bm = ctx.get_grad()
                return (bp - bm) / (2 * hh)
            fd = (4.0 * db(5e-7) - db(1e-6)) / 3.0; Hv = H @ vdir         # (Richardson: b bends on the kernels' scale, w^2 = 4e-4 in the cost)
            assert rel(Hv[sel], fd[sel]) <= 1e-6, (name, "H v", rel(Hv[sel], fd[sel]))
        ctx.set_variables(v0); ctx.sweep_gradhess()
        if jfar is not None:                                        # the far point: no gradient, an H block of zeros
            o = ncd + 3 * (jfar - 1 - 40)
            assert np.all(b[o:o + 3] == 0.0), (name, b[o:o + 3])
        # one LM trial from the same point: matrix-free and materialised agree
        lam = 1e-6 * ctx.max_abs_diag(); n0 = ctx.solve_stats()["mf_trials"]
        c_mf = ctx.lm_trial(lam); st = ctx.solve_stats(); x_mf = ctx.get_step()
        assert st["mf_trials"] == n0 + 1 and st["status"] == 0, (name, st)
        ctx.set_option(_capi.OPT_MATERIALIZE, 1); c_mat = ctx.lm_trial(0.0); x_mat = ctx.get_step()
        assert ctx.solve_stats()["mf_trials"] == n0 + 1
        assert np.all(np.isfinite(x_mf)) and rel(x_mf, x_mat) < 1e-9 and np.isclose(c_mf, c_mat, rtol=1e-9), (name, rel(x_mf, x_mat), c_mf, c_mat)
        ctx.close()
        # optimize: both trial paths, each ends on a convergence flag of the reference with the accepted cost never rising, and the two agree
        fin = []
        for flags, want_mf in ((0, True), (_capi.FLAG_MATERIALIZE, False)):
            q, _ = contaminated(rob, far); res, costs, mf = optimize_tracked(q, flags, 200)
            assert (mf > 0) == want_mf, (name, flags, mf)
            assert (res.termination & CONVERGED) and not (res.termination & BAD), (name, flags, bin(res.termination))
            assert np.all(np.isfinite(costs)) and np.all(np.isfinite(q.variables)), (name, flags, costs)
            acc = [res.startcost]                                   # the accepted trials: LM keeps a trial whose cost does not exceed the best so far
            for c_ in costs:
                if c_ <= acc[-1]: acc.append(c_)
            assert acc[-1] == res.bestcost and res.bestcost < 0.5 * res.startcost, (name, flags, res.startcost, res.bestcost, acc[-1])
            assert np.isclose(N.cost(q), res.bestcost, rtol=1e-12), (name, flags, N.cost(q), res.bestcost)     # the returned variables have the cost the loop accepted
            fin.append((res.bestcost, q.variables.copy(), res.niterations))
        assert np.isclose(fin[0][0], fin[1][0], rtol=1e-12), (name, fin[0][0], fin[1][0])
        print(f"{name}: cost = numpy, b / H v = central differences, mf step = materialised, optimize {fin[0][0]:.6e} ({fin[0][2]} it, mf) = {fin[1][0]:.6e} "
              f"({fin[1][2]} it, materialised)" + (f", point {jfar} beyond the width: b = 0, all finite" if jfar is not None else ""))
    # an id the build does not declare is refused at upload
    p, _ = contaminated(K.Robustifier(U5 + 1, (0.02,)))
    ctx = _capi.Context(0)
    try:
        ctx.upload(p.var_kind, p.var_dim, blockindices(p), p.groups()); raise AssertionError("upload accepted robust id 14")
    except _capi.NllsError as e:
        assert e.code == _capi.ERR_UNSUPPORTED, e.code
    ctx.close()
    print("id 14: NLLS_ERR_UNSUPPORTED at upload")


if __name__ == "__main__":
    check_values(); check_twins(); check_new_kernels()
    print("user robust kernels ok")
