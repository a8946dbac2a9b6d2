"""Worker of tests/test_gpu_singles_wave.py: the cases whose environment must be set before the library is loaded (NLLS_SINGLES_WAVE_MIN is read when a context is created,
NLLS_AMD_LIB when the library is loaded).
  partial     NLLS_SINGLES_WAVE_MIN=1: points of a few blocks each and a variable without any block through the wavefront kernel, against the oracle and the thread kernel
  wide        NLLS_AMD_LIB = the library with tests/user_kinds/radial_ba.hpp: 7-dof cameras (RES_USER0) relaxed by nlls_optimize_singles
  wide_huge   the same with NLLS_SINGLES_WAVE_MIN huge: more than 6 dof still means a wavefront, a 3-dof point of many blocks a thread"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K, synthetic, _capi


def relax(p, sel, cl=None, **opts):
    sel = np.asarray(sel, np.int64)
    cptr, cgroup, cindex, cslot = cl if cl is not None else p.costlists(sel)
    ctx = _capi.Context(0)
    ctx.upload(p.var_kind, p.var_dim, np.arange(1, p.nvariables + 1, dtype=np.uint64), p.groups(), 0)
    ctx.set_variables(p.variables)
    it = ctx.optimize_singles(sel, cptr, cgroup, cindex, cslot, **opts)
    out = ctx.get_variables(), it, ctx.solve_stats(), ctx.sweep_cost()
    ctx.close()
    return out


def partial():
    from tests.test_gpu_functional import _oracle_optimizesingles
    assert os.environ.get("NLLS_SINGLES_WAVE_MIN") == "1"
    p = synthetic.create_ba_problem(8, 600, 0.5, seed=12, robust=N.HuberKernel(0.02), outlier_frac=0.1, outlier_sigma=0.05)
    lone = p.addvariable(np.array([0.3, -0.2, 0.1]))               # a variable no cost block depends on
    p = synthetic.perturb_ba_problem(p, 3e-3, 0.0)
    pts = np.nonzero((p.var_kind == K.VAR_EUCLIDEAN) & (p.var_dim == 3))[0] + 1
    assert lone in pts
    cl = p.costlists(pts); nb = np.diff(cl[0])
    assert nb[pts == lone][0] == 0 and 0 < nb[pts != lone].max() < 64, (nb.min(), nb.max())
    got, it, st, cost = relax(p, pts, cl)
    assert st["singles_wave"] == pts.size and st["singles_thread"] == 0, st
    has = pts != lone
    expect = _oracle_optimizesingles(p, pts[has])
    off = p.var_offsets; lo = off[lone - 1]
    keep = np.ones(got.size, bool); keep[lo:lo + 3] = False
    err = np.max(np.abs(got[keep] - expect[keep]))
    print(f"partial: {pts.size} points of {nb[has].min()}..{nb[has].max()} blocks, iterations {it[has].min()}..{it[has].max()}, cost {cost:.6e}, max |variables - oracle| {err:.3e}")
    assert err < 1e-7, err
    # the empty variable: exactly what the thread kernel leaves (a context whose threshold no variable reaches)
    os.environ["NLLS_SINGLES_WAVE_MIN"] = "1000000000"
    got_t, it_t, st_t, _ = relax(p, pts, cl)
    os.environ["NLLS_SINGLES_WAVE_MIN"] = "1"
    assert st_t["singles_thread"] == pts.size and st_t["singles_wave"] == 0, st_t
    print(f"partial: empty variable {got[lo:lo + 3]} after {it[pts == lone][0]} iterations; thread kernel {got_t[lo:lo + 3]} after {it_t[pts == lone][0]}")
    assert got[lo:lo + 3].tobytes() == got_t[lo:lo + 3].tobytes() and it[pts == lone][0] == it_t[pts == lone][0]
    # (What both kernels leave is NOT the variable's old storage, as one might suppose: the subproblem without a block has H = 0 and g = 0, the LDL' of
    #  src/linearsolver.jl:20-32 divides 0 by 0, and the loop of src/optimize.jl accepts the NaN step at cost 0 -- measured: [nan nan nan] after 1 iteration from
    #  the thread kernel of the parent commit and from both kernels here.  The thread kernel's arithmetic is not this test's to change; the yardstick is its bits.)
    assert np.max(np.abs(got - got_t)[keep]) < 1e-7


USER0 = 100


def radial_model(c, X):
    u, v = (c[:, 0:3] * X).sum(1), (c[:, 3:6] * X).sum(1); s = 1.0 + c[:, 6] * (u * u + v * v)
    return np.stack([s * u, s * v], 1)


def make_radial(ncam, npts, seed, robust=None, outlier_frac=0.0):
    """every 7-dof camera sees every point (npts >= 64 blocks per camera); returns the problem at the truth"""
    rng = np.random.default_rng(seed)
    p = N.NLLSProblem()
    cv = np.concatenate([rng.standard_normal((ncam, 6)) * 0.3 + np.array([1, 0, 0, 0, 1, 0.0]), 0.02 * rng.standard_normal((ncam, 1))], 1)
    pv = rng.uniform(-0.5, 0.5, (npts, 3)) + np.array([0, 0, 2.0])
    cams = p.addvariables(cv) + np.arange(ncam); pts = p.addvariables(pv) + np.arange(npts)
    vi = np.stack([np.repeat(cams, npts), np.tile(pts, ncam)], 1).astype(np.int64)
    meas = radial_model(cv[vi[:, 0] - cams[0]], pv[vi[:, 1] - pts[0]])
    if outlier_frac > 0:
        bad = rng.random(len(meas)) < outlier_frac
        meas[bad] += 0.05 * rng.standard_normal((int(bad.sum()), 2))
    p.addcosts(USER0, vi, meas, robust)
    return p, cams, pts, vi


def perturb_cameras(p, cams, sigma, seed):
    rng = np.random.default_rng(seed); off = p.var_offsets
    for c in cams:
        p.variables[off[c - 1]:off[c - 1] + 7] += sigma * rng.standard_normal(7)
    p._gpu = None


def wide(huge):
    assert os.environ.get("NLLS_AMD_LIB")
    K.register_user_kind(USER0, 2, 2, 2, ((K.VAR_EUCLIDEAN, 7), (K.VAR_EUCLIDEAN, 3)))
    # a. noise-free: from perturbed cameras and true points back to the zero-residual optimum
    p, cams, pts, vi = make_radial(5, 96, seed=21)
    perturb_cameras(p, cams, 2e-3, seed=22)
    got, it, st, cost = relax(p, cams)                              # (the parent: NLLS_ERR_UNSUPPORTED, more than 6 degrees of freedom)
    print(f"wide: 5 cameras of 7 dof, 96 blocks each: iterations {it.tolist()}, cost {cost:.3e}, stats {st['singles_wave']}/{st['singles_thread']}")
    assert st["singles_wave"] == 5 and st["singles_thread"] == 0, st
    assert it.min() >= 1 and cost < 1e-15 * len(vi), cost
    if huge:
        # more than 6 dof: a wavefront whatever the threshold; a 3-dof point of 5 blocks (or of any number): a thread
        assert os.environ.get("NLLS_SINGLES_WAVE_MIN") == "1000000000"
        _, _, st2, _ = relax(p, pts[:7])
        assert st2["singles_wave"] == 0 and st2["singles_thread"] == 7, st2
        q = synthetic.perturb_ba_problem(synthetic.create_ba_problem(8, 600, 0.5, seed=11), 0.0, 2e-3)
        _, _, st3, c3 = relax(q, np.arange(1, 9))
        assert st3["singles_wave"] == 0 and st3["singles_thread"] == 8 and c3 < 1e-15 * 8 * 600, (st3, c3)
        return
    # b. Huber and outliers: against the route the host takes for a variable the kernel declines -- each camera's sub-problem through N.optimize, only that camera free
    p, cams, pts, vi = make_radial(5, 96, seed=23, robust=N.HuberKernel(0.02), outlier_frac=0.1)
    perturb_cameras(p, cams, 2e-3, seed=24)
    opts = N.NLLSOptions()
    expect = p.variables.copy(); off = p.var_offsets
    (g,) = list(p.costs.values()); gvi, gda = g.arrays()
    for c in cams:
        sub = N.NLLSProblem(); sub.copy_variables_from(p, p.variables)
        sel = np.nonzero(gvi[:, 0] == c)[0]
        sub.addcosts(g.res_kind, gvi[sel], gda[sel], g.robust)
        unfixed = np.zeros(p.nvariables, bool); unfixed[c - 1] = True
        N.optimize(sub, opts, unfixed)
        expect[off[c - 1]:off[c - 1] + 7] = sub.variables[off[c - 1]:off[c - 1] + 7]
    c0 = N.cost(p)
    got, it, st, cost = relax(p, cams, maxiters=opts.maxiters, maxfails=opts.maxfails, reldcost=opts.reldcost, absdcost=opts.absdcost, dstep=opts.dstep, iterator=int(opts.iterator))
    err = np.max(np.abs(got - expect))
    print(f"wide, Huber: iterations {it.tolist()}, cost {c0:.6e} -> {cost:.6e}, max |variables - sub-problem route| {err:.3e}")
    assert st["singles_wave"] == 5 and cost < c0
    assert err < 1e-7, err
    # ... and through the public entry point: the 7-dof cameras join the runs that go to the kernel
    from nllssolver_jl_amd import optimizer
    it2 = N.optimizesingles(p, opts, indices=cams)
    assert optimizer.last_singles_stats == dict(singles_wave=5, singles_thread=0) and np.array_equal(it2, it)
    assert np.max(np.abs(p.variables - got)) == 0.0


if __name__ == "__main__":
    mode = sys.argv[1]
    {"partial": partial, "wide": lambda: wide(False), "wide_huge": lambda: wide(True)}[mode]()
    print(f"singles wave {mode} ok")
