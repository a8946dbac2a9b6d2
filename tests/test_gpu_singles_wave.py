"""nlls_optimize_singles with one WAVEFRONT per variable (singles_wave_kernel, csrc/nlls_cost.hip): a variable of at least 64 cost blocks (a camera against fixed
points: resection) or of 7 .. 12 degrees of freedom gets 64 lanes that deal its blocks; every other one keeps its thread.  Against the CPU oracle's optimizesingles
(tests/test_gpu_functional._oracle_optimizesingles) at the tolerance that comparison has everywhere: 1e-7, 1e-6 for gradient descent with maxiters = 40.
The cases that need an environment of their own (NLLS_SINGLES_WAVE_MIN, the library with user kinds) run in tests/singles_wave_worker.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import synthetic, _capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
USERLIB = os.path.join(ROOT, "nllssolver.jl_amd", "csrc", "libnlls_amd_userdemo.so")
WORKER = os.path.join(ROOT, "tests", "singles_wave_worker.py")


def _cameras_problem(robust):
    """8 affine cameras over 600 fixed points, the cameras moved off their optimum (perturb_ba_problem(p, 0, s) moves the cameras only)"""
    if robust:
        p = synthetic.create_ba_problem(8, 600, 0.5, seed=12, robust=N.HuberKernel(0.02), outlier_frac=0.1, outlier_sigma=0.05)
    else:
        p = synthetic.create_ba_problem(8, 600, 0.5, seed=11)
    return synthetic.perturb_ba_problem(p, 0.0, 2e-3)


def _relax(p, sel, start=None, **opts):
    """ctx.optimize_singles of `sel` on a fresh context: (variables, iterations, solve_stats, cost)"""
    sel = np.asarray(sel, np.int64)
    cptr, cgroup, cindex, cslot = p.costlists(sel)
    ctx = _capi.Context(0)
    ctx.upload(p.var_kind, p.var_dim, np.arange(1, p.nvariables + 1, dtype=np.uint64), p.groups(), 0)
    ctx.set_variables(p.variables if start is None else start)
    it = ctx.optimize_singles(sel, cptr, cgroup, cindex, cslot, **opts)
    out = ctx.get_variables(), it, ctx.solve_stats(), ctx.sweep_cost()
    ctx.close()
    return out


def _ncosts(p):
    return sum(len(g["varind"]) for g in p.groups())


@pytest.mark.parametrize("robust", [False, True])
@pytest.mark.parametrize("iterator", ["newton", "levenbergmarquardt", "dogleg", "gradientdescent"])
def test_cameras_through_the_wave_kernel(iterator, robust):
    from tests.test_gpu_functional import _oracle_optimizesingles
    itv = getattr(N, iterator); maxit = 40 if iterator == "gradientdescent" else 100
    p = _cameras_problem(robust)
    cams = np.nonzero((p.var_kind == K.VAR_EUCLIDEAN) & (p.var_dim == 6))[0] + 1
    cptr = p.costlists(cams)[0]; nb = np.diff(cptr)
    assert cams.size == 8 and nb.min() >= 64, nb
    expect = _oracle_optimizesingles(p, cams, iterator=int(itv), maxiters=maxit)
    got, it, st, cost = _relax(p, cams, iterator=int(itv), maxiters=maxit)
    err = np.max(np.abs(got - expect))
    print(f"{iterator} robust={robust}: blocks per camera {nb.min()}..{nb.max()}, iterations {it.tolist()}, cost {cost:.3e}, max |variables - oracle| {err:.3e}, stats {st['singles_wave']}/{st['singles_thread']}")
    assert st["singles_wave"] == 8 and st["singles_thread"] == 0, st
    assert it.min() >= 1
    assert err < (1e-6 if iterator == "gradientdescent" else 1e-7), err
    if not robust and iterator != "gradientdescent":
        # the bound of test_randomized_optimize_matches_oracle: noise-free, the optimum is a zero residual (the oracle ends at 1e-26 .. 1e-29 with these three iterators,
        # and at 9e-4 after 40 steps of gradient descent)
        assert cost < 1e-15 * _ncosts(p), cost


def test_so3_cameras_through_the_wave_kernel():
    """storage 12, 6 dof, a retraction that is not an addition (R <- R expm([w]x)) inside the kernel"""
    from tests.test_gpu_functional import _oracle_optimizesingles
    for robust in (None, N.HuberKernel(0.02)):
        p = synthetic.create_so3_ba_problem(6, 400, 0.6, seed=3, adaptive=False, outlier_frac=0.1 if robust else 0.0, noise=1e-3 if robust else 0.0, robust=robust)
        p = synthetic.perturb_ba_problem(p, 0.0, 2e-3)
        cams = np.nonzero(p.var_kind == K.VAR_POSE_SO3)[0] + 1
        nb = np.diff(p.costlists(cams)[0])
        assert cams.size == 6 and nb.min() >= 64, nb
        expect = _oracle_optimizesingles(p, cams)
        got, it, st, cost = _relax(p, cams)
        err = np.max(np.abs(got - expect))
        print(f"so3 robust={robust is not None}: blocks per camera {nb.min()}..{nb.max()}, iterations {it.tolist()}, cost {cost:.3e}, max |variables - oracle| {err:.3e}")
        assert st["singles_wave"] == 6 and st["singles_thread"] == 0, st
        assert err < 1e-7, err
        if robust is None:
            assert cost < 1e-15 * _ncosts(p), cost


def test_points_and_cameras_listed_together():
    """N.optimizesingles of everything: the points first (one launch, one thread each), then the cameras, which see the moved points -- where the sequential oracle lands"""
    from tests.test_gpu_functional import _oracle_optimizesingles
    from nllssolver_jl_amd import optimizer
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(8, 600, 0.5, seed=12, robust=N.HuberKernel(0.02), outlier_frac=0.1, outlier_sigma=0.05), 2e-3, 2e-3)
    allv = np.arange(1, p.nvariables + 1)
    c0 = N.cost(p)
    expect = _oracle_optimizesingles(p, allv)
    iters = N.optimizesingles(p, N.NLLSOptions(), indices=allv)
    err = np.max(np.abs(p.variables - expect))
    print(f"mixed: cost {c0:.3e} -> {N.cost(p):.3e}, max |variables - oracle| {err:.3e}, last call {optimizer.last_singles_stats}")
    assert iters.shape == (p.nvariables,) and iters.min() >= 1 and N.cost(p) < c0
    assert err < 1e-7, err
    assert optimizer.last_singles_stats == dict(singles_wave=8, singles_thread=0)      # (singles_levels: the call before it held the points)


def test_class_boundary():
    """one 3-dof variable of 63 blocks and one of 64: a thread and a wavefront in one call"""
    from tests.test_gpu_functional import _oracle_optimizesingles
    rng = np.random.default_rng(7)
    p = N.NLLSProblem()
    cv = rng.standard_normal((64, 6)) + np.array([1.0, 0, 0, 0, 1.0, 0])
    truth = rng.random((2, 3)) + np.array([-0.5, -0.5, 10.0])
    cams = p.addvariables(cv) + np.arange(64); pts = p.addvariables(truth + 1e-2 * rng.standard_normal((2, 3))) + np.arange(2)
    vi = np.concatenate([np.stack([cams[:63], np.full(63, pts[0])], 1), np.stack([cams, np.full(64, pts[1])], 1)]).astype(np.int64)
    C = cv[vi[:, 0] - cams[0]]; X = truth[vi[:, 1] - pts[0]]
    meas = np.stack([(C[:, 0:3] * X).sum(1), (C[:, 3:6] * X).sum(1)], 1)
    p.addcosts(K.RES_BA_AFFINE, vi, meas + 1e-3 * rng.standard_normal(meas.shape), N.HuberKernel(0.02))
    assert np.diff(p.costlists(pts)[0]).tolist() == [63, 64]
    expect = _oracle_optimizesingles(p, pts)
    got, it, st, cost = _relax(p, pts)
    err = np.max(np.abs(got - expect))
    print(f"boundary: iterations {it.tolist()}, max |variables - oracle| {err:.3e}, stats {st['singles_wave']}/{st['singles_thread']}")
    assert (st["singles_wave"], st["singles_thread"]) == (1, 1), st
    assert it.min() >= 1 and err < 1e-7, err


def test_bit_reproducible_and_independent_of_the_rest_of_the_launch():
    p = _cameras_problem(True)
    cams = np.nonzero((p.var_kind == K.VAR_EUCLIDEAN) & (p.var_dim == 6))[0] + 1
    a, ita, _, _ = _relax(p, cams)
    b, itb, _, _ = _relax(p, cams)
    assert a.tobytes() == b.tobytes() and np.array_equal(ita, itb)
    c, itc, st, _ = _relax(p, cams[2:3])
    assert st["singles_wave"] == 1 and itc[0] == ita[2]
    lo, hi = p.var_offsets[cams[2] - 1], p.var_offsets[cams[2] - 1] + 6
    assert c[lo:hi].tobytes() == a[lo:hi].tobytes()
    assert c[:lo].tobytes() == np.asarray(p.variables)[:lo].tobytes()       # (nothing else moved)


def test_wave_kernel_invalidates_a_lookahead_sweep():
    """tests/test_gpu_parity.py::test_optimize_singles_invalidates_a_lookahead_sweep with the CAMERAS relaxed (one wavefront each): LM trial + accept + optimize_singles +
    sweep(NULL) + trial, the same with and without the look-ahead sweep"""
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(60, 1500, 0.12, seed=5, robust=N.HuberKernel(0.02), outlier_frac=0.05, outlier_sigma=0.05), 1e-3, 1e-3)
    bi = np.arange(1, p.nvariables + 1, dtype=np.uint64)
    cams = np.arange(1, 61, dtype=np.int64)
    cptr, cgroup, cindex, cslot = p.costlists(cams)
    assert np.diff(cptr).min() >= 64
    out = {}
    for la in (1, 0):
        for mat in (0, 1):
            ctx = _capi.Context(); ctx.upload(p.var_kind, p.var_dim, bi, p.groups())
            ctx.set_option(_capi.OPT_LOOKAHEAD, la); ctx.set_option(_capi.OPT_MATERIALIZE, mat)
            ctx.set_variables(p.variables); ctx.sweep_gradhess(); lam = 1e-5 * ctx.max_abs_diag()
            ctx.copy_variables(_capi.VARS_NEXT, _capi.VARS_CURRENT)
            ctx.sweep_gradhess(want_cost=False); ctx.lm_trial(lam)            # (the second sweep of the set arms the look-ahead)
            ctx.damp(-lam); ctx.swap_variables(_capi.VARS_CURRENT, _capi.VARS_NEXT)
            ctx.optimize_singles(cams, cptr, cgroup, cindex, cslot, maxiters=3)
            assert ctx.solve_stats()["singles_wave"] == 60
            ctx.sweep_gradhess(want_cost=False)
            c = ctx.lm_trial(lam)
            out[(la, mat)] = (c, ctx.get_step()); ctx.close()
    rel = lambda a, b: np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)
    for mat in (0, 1):
        assert np.isclose(out[(1, mat)][0], out[(0, mat)][0], rtol=1e-10), (mat, out[(1, mat)][0], out[(0, mat)][0])
        assert rel(out[(1, mat)][1], out[(0, mat)][1]) < 1e-6


def _worker(mode, **env):
    out = subprocess.run([sys.executable, WORKER, mode], capture_output=True, text=True, env=dict(os.environ, **env), timeout=900)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and f"singles wave {mode} ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


def test_partial_wavefronts_and_an_empty_variable():
    """NLLS_SINGLES_WAVE_MIN=1: the points (a few blocks each: most lanes idle) and a variable without any block through the wave kernel"""
    _worker("partial", NLLS_SINGLES_WAVE_MIN="1")


def test_wide_variables():
    """7-dof cameras of tests/user_kinds/radial_ba.hpp (RES_USER0): the parent answers NLLS_ERR_UNSUPPORTED"""
    _worker("wide", NLLS_AMD_LIB=USERLIB)


def test_wide_variables_ignore_the_block_threshold():
    _worker("wide_huge", NLLS_AMD_LIB=USERLIB, NLLS_SINGLES_WAVE_MIN="1000000000")
