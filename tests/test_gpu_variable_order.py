"""Every solver path under variable orders other than "reduced variables first".

Every generator lists cameras / poses / the adaptive kernel variable before the points, so every coupling block lies in a POINT's block row.  The C ABI takes
any order and the reference does not care (tests/test_variable_order.py pins that on the CPU oracle); the device code does.  A point listed before one of its
cameras finds that coupling block in the camera's row, stored transposed (SchurNbr::trans): the strided gather of schur_elim_kernel, the transposed branch of
schur_backsub_kernel, the generic (LDS-staged) supernodes for every point, neighbour lists sorted by reduced column instead of memory offset, and an
accumulate sweep whose camera rows own hundreds of off-diagonal blocks.  The problems here are the other tests' problems re-indexed by
tests/helpers.permute_variables and run through tests/test_gpu_parity.check_problem at that file's tolerances (exact structure; cost, A.data, b; the damped
solve and its long-double backward error; quadratic form, retraction, nlls_lm_trial).  Each case asserts the branch it was written for through the counters
of nlls_get_solve_stats [29..42] and prints them (COUNTERS ...)."""
import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import synthetic, _capi
from tests.helpers import (oracle_problem, blockindices, structured_problem, longdouble_schur_step, permute_variables, to_original_order, variable_sizes,
                           eliminated_mask, NAMED_ORDERS, order_elim_first, order_random, order_var_last, order_var_middle)
from tests.test_gpu_parity import check_problem, rel, RTOL

pytestmark = pytest.mark.gpu

U = np.finfo(np.float64).eps / 2
F = _capi
COUNTERS = ("elim_fast60", "elim_fast_narrow", "elim_fast_wide", "elim_slow_acc", "elim_slow_noacc", "elim_nbrs_transposed", "elim_nbrs", "elim_slab",
            "sweep_light_tiles", "sweep_image_tiles", "sweep_direct_tiles", "sweep_partial_tiles", "sweep_fold_groups", "sweep_fused_groups", "mf_trials")


def branch_stats(q, where, unfixed=None, flags=0, lam_scale=1e-4):
    """What the upload of `q` chose, and whether its LM trial ran matrix-free: one upload, one accumulate sweep, one trial; the counters printed."""
    ctx = _capi.Context(); info = ctx.upload(q.var_kind, q.var_dim, blockindices(q, unfixed), q.groups(), flags)
    try:
        ctx.set_variables(q.variables); ctx.set_variables(q.variables, _capi.VARS_NEXT)
        ctx.sweep_gradhess(); ctx.lm_trial(lam_scale * ctx.max_abs_diag())
        st = ctx.solve_stats()
    finally:
        ctx.close()
    print(f"COUNTERS {where} solve_mode={info.solve_mode} nred={info.nreduced_dof} " + " ".join(f"{k}={st[k]}" for k in COUNTERS))
    st["fast"] = st["elim_fast60"] + st["elim_fast_narrow"] + st["elim_fast_wide"]; st["slow"] = st["elim_slow_acc"] + st["elim_slow_noacc"]
    return info, st


def assert_order_branch(order, st, schur=True):
    """the elimination branch each named order exists for"""
    nb, tr = st["elim_nbrs"], st["elim_nbrs_transposed"]
    if not schur:
        assert nb == 0 and st["fast"] == 0 and st["slow"] == 0, st
        return
    assert nb > 0 and st["fast"] + st["slow"] == st["elim_supernodes"], st
    if order == "identity":
        assert tr == 0 and st["slow"] == 0 and st["fast"] > 0, st
    elif order in ("elim_first", "reversed"):            # every point before every camera: every neighbour transposed, nothing on the fast path, no matrix-free trial,
        assert tr == nb and st["fast"] == 0 and st["slow"] > 0 and st["mf_trials"] == 0 and st["elim_slab"] == 0, st     # no slab assembly (NLLS_FLAG_DETERMINISTIC has no effect)
    elif order == "interleaved":
        assert 0 < tr < nb and st["slow"] > 0, st
    else:
        assert tr > 0 and st["slow"] > 0, st


def permuted(p, order, elim=None):
    f = NAMED_ORDERS[order] if isinstance(order, str) else order
    return permute_variables(p, f(eliminated_mask(p) if elim is None else elim))


# ---- elimination, affine bundle adjustment ---------------------------------------------------------------------------------------------------------
BA_SHAPES = {"small": (12, 80, 0.3, 5), "band": (30, 400, 0.12, 6)}          # dense / small reduced system (72 dof); band reduced system (180 dof >= 128)
BA_FLAGS = {"default": 0, "no_bcr": F.FLAG_NO_BCR, "no_bcr_no_twist": F.FLAG_NO_BCR | F.FLAG_NO_TWIST, "no_band": F.FLAG_NO_BAND, "force_atomic": F.FLAG_FORCE_ATOMIC,
            "no_schur": F.FLAG_NO_SCHUR, "deterministic": F.FLAG_DETERMINISTIC}
_problems = {}


def ba_problem(shape):
    if shape not in _problems:
        ncam, npts, prop, seed = BA_SHAPES[shape]
        _problems[shape] = synthetic.perturb_ba_problem(synthetic.create_ba_problem(ncam, npts, prop, seed=seed, robust=N.HuberKernel(0.05), outlier_frac=0.1, outlier_sigma=0.05), 1e-3, 1e-3)
    return _problems[shape]


@pytest.mark.parametrize("flags", list(BA_FLAGS))
@pytest.mark.parametrize("order", list(NAMED_ORDERS))
@pytest.mark.parametrize("shape", list(BA_SHAPES))
def test_ba_affine_elimination_under_every_order(shape, order, flags):
    q, _ = permuted(ba_problem(shape), order)
    fl = BA_FLAGS[flags]; schur = flags != "no_schur"
    info = check_problem(q, flags=fl, expect_sparse=1, expect_schur=int(schur), lam_scale=1e-4)
    assert info.nreduced_dof == (6 * BA_SHAPES[shape][0] if schur else info.ndof)
    if shape == "band": assert info.nreduced_dof >= 128
    _, st = branch_stats(q, f"ba_{shape}-{order}-{flags}", flags=fl)
    assert_order_branch(order, st, schur)


# ---- the generic supernodes' two classes: pair accumulators in LDS, or every product straight into S -----------------------------------------------
@pytest.mark.parametrize("ncam,npts,prop,acc", [(20, 150, 0.2, True), (40, 300, 0.1, False)])
def test_slow_path_widths_under_elim_first(ncam, npts, prop, acc):
    """Points seen by ALL cameras (nd = 120: the accumulators fit the 150 KB budget; nd = 240: they do not) beside the ordinary ones and one point seen by a
    single camera, every one of them listed before the cameras."""
    p = synthetic.create_ba_problem(ncam, npts, prop, seed=21, robust=N.HuberKernel(0.05), outlier_frac=0.05, outlier_sigma=0.05)
    wide = [7, npts // 2, npts - 3]; lonely = 11
    p = synthetic.widen_visibility(p, ncam, {l: ncam for l in wide})
    g = next(iter(p.costs.values())); vi, da = g.arrays()
    first = np.nonzero(vi[:, 1] == ncam + lonely)[0]; keep = np.ones(len(vi), bool); keep[first[1:]] = False       # the lonely point keeps its first observation
    g.set_arrays(np.ascontiguousarray(vi[keep]), np.ascontiguousarray(da[keep]))
    p = synthetic.perturb_ba_problem(p, 1e-3, 1e-3)
    per_point = np.bincount(g.arrays()[0][:, 1] - ncam - 1, minlength=npts)
    assert np.all(per_point[np.array(wide) - 1] == ncam) and per_point[lonely - 1] == 1
    q, _ = permuted(p, "elim_first")
    info = check_problem(q, expect_sparse=1, expect_schur=1, lam_scale=1e-4)
    assert info.nreduced_dof == 6 * ncam and info.nschur_blocks == npts
    _, st = branch_stats(q, f"slow_widths-{ncam}cam")
    assert_order_branch("elim_first", st)
    if acc: assert st["elim_slow_noacc"] == 0 and st["elim_slow_acc"] > 0, st
    else: assert st["elim_slow_noacc"] >= 1 and st["elim_slow_acc"] > 0, st        # (the ordinary points' supernodes keep their accumulators)


# ---- one-dof blocks: DV = 1, the transposed neighbour a 1 x 1 block -------------------------------------------------------------------------------
@pytest.mark.parametrize("ps", [0, 1])
def test_one_dof_blocks_under_elim_first(ps):
    p, meta = structured_problem(K.RES_ROSENBROCK_B, [(3, 20), (2, 5)], 40, ps)
    q, new_of_old = permuted(p, "elim_first", meta["elim_blocks"])
    elim_q = meta["elim_blocks"][np.argsort(new_of_old)]
    info = check_problem(q, expect_sparse=1, expect_schur=1, lam_scale=1e-4)
    assert info.nschur_blocks == int(elim_q.sum())
    _, st = branch_stats(q, f"one_dof-ps{ps}")
    assert_order_branch("elim_first", st)
    # the step against the long-double Schur step, at the bound of tests/test_gpu_mf_shapes.py
    bi = blockindices(q); ols = oracle_problem(q).linear_system(bi); ols.costgradhess(); lam = ols.max_abs_diag() * 1e-6
    ctx = _capi.Context(); ctx.upload(q.var_kind, q.var_dim, bi, q.groups(), 0)
    try:
        ctx.set_variables(q.variables); ctx.sweep_gradhess(); ctx.damp(lam); x = ctx.solve(want_x=True)
    finally:
        ctx.close()
    x_ref, S = longdouble_schur_step(ols.data, ols.bsm_index(), ols.b, lam, elim_q)
    bound = max(1e-12, 1e2 * U * np.linalg.cond(S)); err = rel(x, x_ref.astype(np.float64))
    print(f"one_dof-ps{ps}: step against the long-double Schur step {err:.3e} (bound {bound:.3e})")
    assert err <= bound, (err, bound)


# ---- the accumulate sweep's tile classes with the roles swapped: camera rows own the off-diagonal blocks -------------------------------------------
@pytest.mark.parametrize("npts,cls", [(100, "light"), (200, "image"), (400, "direct"), (1100, "split")])
def test_sweep_tile_classes_under_elim_first(npts, cls):
    """8 cameras that see every point, the points listed first: a camera row holds 18 npts + 36 doubles and npts entries -- a light row (<= 128 entries), a heavy
    tile with an LDS image, a TILE_DIRECT tile (18 npts + 36 + 6 > 6144), two TILE_PARTIAL pieces (> 1024 entries)."""
    ncam = 8
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(ncam, npts, 1.0, seed=40 + npts, robust=N.HuberKernel(0.05), outlier_frac=0.05, outlier_sigma=0.05), 1e-3, 1e-3)
    assert p.ncosts() == ncam * npts
    q, _ = permuted(p, "elim_first")
    check_problem(q, expect_sparse=1, expect_schur=1, lam_scale=1e-4)
    _, st = branch_stats(q, f"sweep_tiles-{npts}")
    assert_order_branch("elim_first", st)
    assert st["sweep_fold_groups"] == 0 and st["sweep_light_tiles"] > 0, st                 # (the point rows, a diagonal block each, are light everywhere)
    image, direct, partial = st["sweep_image_tiles"], st["sweep_direct_tiles"], st["sweep_partial_tiles"]
    if cls == "light": assert (image, direct, partial) == (0, 0, 0), st
    elif cls == "image": assert (image, direct, partial) == (ncam, 0, 0), st
    elif cls == "direct": assert (image, direct) == (0, ncam) and partial == ncam, st
    else: assert (image, direct) == (0, 2 * ncam) and partial == 2 * ncam, st
    # two sweeps of one upload.  Heavy tiles with an image sum a row in registers, in a fixed order: the same bits.  A light row's DIAGONAL block and its part of b are
    # summed with LDS atomics into a few accumulators (gh_light_kernel) -- with 100 entries to a row in an order that varies -- but its off-diagonal blocks have one
    # writer each: the same bits there, rounding on the diagonal blocks and b.  DIRECT / PARTIAL tiles add to memory with atomics: rounding everywhere.
    ctx = _capi.Context(); ctx.upload(q.var_kind, q.var_dim, blockindices(q), q.groups(), 0)
    try:
        ctx.set_variables(q.variables); cp, rv, nz, bo = (np.asarray(a, np.int64) for a in ctx.bsm_index())
        c1 = ctx.sweep_gradhess(); A1, b1 = ctx.get_bsm_data().copy(), ctx.get_grad().copy()
        c2 = ctx.sweep_gradhess(); A2, b2 = ctx.get_bsm_data(), ctx.get_grad()
    finally:
        ctx.close()
    assert np.isclose(c1, c2, rtol=RTOL) and rel(A2, A1) < RTOL and rel(b2, b1) < RTOL
    if cls == "image": assert c1 == c2 and np.array_equal(A1, A2) and np.array_equal(b1, b2)
    if cls == "light":
        bs = np.diff(np.r_[bo - 1, len(b1)]); rows = np.repeat(np.arange(len(cp) - 1), np.diff(cp)); dg = np.nonzero(rv - 1 == rows)[0]
        offdiag = np.ones(A1.size, bool)
        for o, n in zip(nz[dg] - 1, bs[rows[dg]] ** 2): offdiag[o:o + n] = False
        assert offdiag.sum() == 18 * ncam * npts and np.array_equal(A1[offdiag], A2[offdiag])


@pytest.mark.parametrize("order", ["identity", "elim_first"])
def test_fused_launch_eligibility_follows_the_order(order):
    """8 cameras that see all 200 points.  Cameras first: their rows are heavy tiles that own a diagonal block, the points' rows light -- one fused launch
    (launch_gh_fused).  Points first: a camera row owns its 200 off-diagonal blocks too (an LDS image of 18 x 200 + 36 doubles, within the 6144 of an image tile but
    far more than the light role needs): not fused, one launch per slot."""
    ncam, npts = 8, 200
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(ncam, npts, 1.0, seed=8, robust=N.HuberKernel(0.05), outlier_frac=0.05, outlier_sigma=0.05), 1e-3, 1e-3)
    assert p.ncosts() == ncam * npts
    q, _ = permuted(p, order)
    check_problem(q, expect_sparse=1, expect_schur=1, lam_scale=1e-4)
    _, st = branch_stats(q, f"fused-{order}")
    assert_order_branch(order, st)
    assert st["sweep_image_tiles"] == ncam and st["sweep_direct_tiles"] == 0 and st["sweep_partial_tiles"] == 0, st
    assert st["sweep_fused_groups"] == (1 if order == "identity" else 0), st


# ---- three-slot groups: (kernel variable, pose, point) ------------------------------------------------------------------------------------------------
SO3_ORDERS = {"elim_first": order_elim_first, "random": order_random(11), "kernel_last": order_var_last(0), "kernel_middle": order_var_middle(0)}


@pytest.mark.parametrize("order", list(SO3_ORDERS))
@pytest.mark.parametrize("ncam,npts,prop", [(8, 60, 0.5), (20, 400, 0.25)])
def test_so3_adaptive_under_every_order(ncam, npts, prop, order):
    p = synthetic.perturb_ba_problem(synthetic.create_so3_ba_problem(ncam, npts, prop, seed=2, adaptive=True), 1e-3, 1e-3)
    q, _ = permuted(p, SO3_ORDERS[order])
    info = check_problem(q, expect_sparse=1, expect_schur=1, lam_scale=1e-4)
    assert info.nreduced_dof == 6 * ncam + 3 and info.nschur_blocks == npts
    _, st = branch_stats(q, f"so3_adaptive-{ncam}x{npts}-{order}")
    nb, tr = st["elim_nbrs"], st["elim_nbrs_transposed"]
    if order == "elim_first": assert tr == nb > 0 and st["fast"] == 0 and st["sweep_fold_groups"] == 0, st
    elif order == "kernel_last": assert tr == npts and nb > tr and st["slow"] > 0, st        # (every point's block with the kernel variable, and only that one)
    else: assert 0 < tr < nb and st["slow"] > 0, st


@pytest.mark.parametrize("order", ["identity", "elim_first"])
def test_folded_sweep_eligibility_follows_the_order(order):
    """10 poses with 136 .. 442 observations each under the adaptive kernel.  Poses first: the pose rows and the kernel variable's row are heavy, every block lies
    in a point's light row -- the group is swept folded (build_fold).  Points first: the pose rows own their off-diagonal blocks, one writer each (and the longest
    are TILE_DIRECT): build_fold declines, one launch per slot."""
    p = synthetic.perturb_ba_problem(synthetic.create_so3_ba_problem(10, 600, 0.5, seed=2, adaptive=True), 1e-3, 1e-3)
    q, _ = permuted(p, order)
    info = check_problem(q, expect_sparse=1, expect_schur=1, lam_scale=1e-4)
    assert info.nreduced_dof == 63 and info.nschur_blocks == 600
    _, st = branch_stats(q, f"fold-{order}")
    assert_order_branch(order, st)
    assert st["sweep_fold_groups"] == (1 if order == "identity" else 0), st
    if order == "elim_first": assert st["sweep_direct_tiles"] > 0 and st["sweep_image_tiles"] > 0, st


def test_so3_adaptive_kernel_fixed_under_elim_first():
    p = synthetic.perturb_ba_problem(synthetic.create_so3_ba_problem(8, 60, 0.5, seed=2, adaptive=True), 1e-3, 1e-3)
    q, new_of_old = permuted(p, "elim_first")
    unfixed = np.ones(q.nvariables, bool); unfixed[new_of_old[0]] = False
    info = check_problem(q, unfixed=unfixed, expect_sparse=1, lam_scale=1e-4)
    assert info.nreduced_dof == 6 * 8
    _, st = branch_stats(q, "so3_adaptive-kernel_fixed", unfixed=unfixed)
    assert st["elim_nbrs_transposed"] == st["elim_nbrs"] > 0 and st["fast"] == 0, st


def test_so3_huber_under_elim_first():
    p = synthetic.perturb_ba_problem(synthetic.create_so3_ba_problem(8, 60, 0.5, seed=2, adaptive=False, robust=N.HuberKernel(0.05)), 1e-3, 1e-3)
    q, _ = permuted(p, "elim_first")
    check_problem(q, expect_sparse=1, expect_schur=1, lam_scale=1e-4)
    _, st = branch_stats(q, "so3_huber-elim_first")
    assert_order_branch("elim_first", st)


# ---- fixed variables ------------------------------------------------------------------------------------------------------------------------------------
def test_fixed_variables_under_a_random_order():
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 60, 0.4, seed=6), 1e-3, 1e-3)
    unfixed = np.ones(p.nvariables, bool); unfixed[[0, 3, 15, 16, 40]] = False            # (two cameras, three points: tests/test_gpu_parity.test_ba_fixed_variables)
    perm = order_random(3)(eliminated_mask(p)); q, _ = permute_variables(p, perm)
    check_problem(q, unfixed=unfixed[perm], expect_sparse=1)
    _, st = branch_stats(q, "fixed-random", unfixed=unfixed[perm])
    assert 0 < st["elim_nbrs_transposed"] < st["elim_nbrs"], st


# ---- seeded random ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", list(range(700, 716)))
def test_randomized_ba_under_a_random_order(seed):
    """tests/test_gpu_parity.test_randomized_ba_against_oracle (shape, kernel, outliers, fixed variables, flags drawn per seed) with the variables in a random
    order; at most 40 cameras and 600 points."""
    rng = np.random.default_rng(seed)
    ncam = int(rng.integers(4, 41)); npts = int(rng.integers(20, 601)); prop = max(float(rng.uniform(0.05, 0.6)), 3.5 / ncam)
    kind = int(rng.integers(0, 4))
    robust = [None, N.HuberKernel(float(rng.uniform(0.005, 0.1))), N.GemanMcclureKernel(float(rng.uniform(0.02, 0.2))),
              N.Scaled(N.Huber2oKernel(float(rng.uniform(0.005, 0.1))), float(rng.uniform(0.5, 3.0)))][kind]
    kw = dict(robust=robust, outlier_frac=float(rng.uniform(0.0, 0.3)), outlier_sigma=0.1) if robust is not None else {}
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(ncam, npts, prop, seed=seed, **kw), 1e-3, 1e-3)
    perm = rng.permutation(p.nvariables); q, _ = permute_variables(p, perm)
    unfixed = None
    if rng.random() < 0.5:
        unfixed = np.ones(q.nvariables, bool); unfixed[rng.choice(q.nvariables, size=max(1, q.nvariables // 20), replace=False)] = False
    flags = [0, F.FLAG_NO_BCR, F.FLAG_FORCE_ATOMIC, F.FLAG_NO_BAND, F.FLAG_NO_BCR | F.FLAG_NO_TWIST, F.FLAG_FORCE_SPARSE][int(rng.integers(0, 6))]
    if seed % 3 == 0: flags |= F.FLAG_DETERMINISTIC
    info = check_problem(q, unfixed=unfixed, flags=flags, lam_scale=[1e-6, 1e-4, 1e-1, 1e-2][kind])
    if info.is_sparse:
        _, st = branch_stats(q, f"random-{seed}", unfixed=unfixed, flags=flags)
        assert st["elim_nbrs"] == 0 or st["elim_nbrs_transposed"] > 0, st


# ---- the layers above the solve, on one points-first problem each ----------------------------------------------------------------------------------------
def _layers_problem(pose_noise=1e-3):
    return synthetic.perturb_ba_problem(synthetic.create_ba_problem(12, 120, 0.4, seed=5, robust=N.HuberKernel(0.01), outlier_frac=0.1, outlier_sigma=0.05), 3e-3, pose_noise)


def test_optimize_under_elim_first():
    p = _layers_problem(); q, _ = permuted(p, "elim_first")
    ro = oracle_problem(q).optimize(iterator=1, maxiters=8)
    rg = N.optimize(q, N.NLLSOptions(maxiters=8)); r0 = N.optimize(p, N.NLLSOptions(maxiters=8))
    assert np.isclose(rg.bestcost, ro.bestcost, rtol=1e-8), (rg.bestcost, ro.bestcost)
    assert np.isclose(rg.bestcost, r0.bestcost, rtol=1e-8), (rg.bestcost, r0.bestcost)      # ... and the identity order's


def test_optimizesingles_under_elim_first():
    from tests.test_gpu_functional import _oracle_optimizesingles
    p = _layers_problem(0.0); q, new_of_old = permuted(p, "elim_first")
    pts_p = np.nonzero(eliminated_mask(p))[0] + 1; pts_q = np.nonzero(eliminated_mask(q))[0] + 1
    assert np.array_equal(pts_q, np.arange(1, pts_p.size + 1))                              # (the points come first)
    expect = _oracle_optimizesingles(p, pts_p)                                              # the oracle on the identity order
    c0 = N.cost(q)
    N.optimizesingles(q, N.NLLSOptions(), indices=pts_q)
    assert N.cost(q) < c0
    back = to_original_order(q.variables, variable_sizes(p)[0], new_of_old)
    assert np.max(np.abs(back - expect)) < 1e-7, np.max(np.abs(back - expect))


def test_eval_blocks_under_elim_first():
    p = _layers_problem(); q, _ = permuted(p, "elim_first")
    out = []
    for pr in (p, q):
        ctx = _capi.Context(); ctx.upload(pr.var_kind, pr.var_dim, blockindices(pr), pr.groups(), 0)
        try:
            ctx.set_variables(pr.variables); out.append(ctx.eval_blocks(0))
        finally:
            ctx.close()
    # the same blocks in the same upload order, evaluated from the same numbers: per-block arithmetic only
    for k in ("r", "sqerr", "rho", "weight"):
        assert out[0][k].shape == out[1][k].shape and np.allclose(out[1][k], out[0][k], rtol=1e-13, atol=1e-13 * np.max(np.abs(out[0][k]))), k


def test_set_cost_data_under_elim_first():
    p = _layers_problem(); q, _ = permuted(p, "elim_first")
    g = q.groups(); da = g[0]["data"].copy(); n = da.shape[0]
    idx = np.array([1, 2, n // 3, n // 2, n - 1, n], np.int64)                              # (1-based blocks of the group, its first and last among them)
    new = da[idx - 1] + np.random.default_rng(9).uniform(-0.02, 0.02, (idx.size, da.shape[1]))
    da2 = da.copy(); da2[idx - 1] = new
    g2 = [dict(g[0], data=np.ascontiguousarray(da2))]
    bi = blockindices(q); res = []
    for groups, update in ((g, True), (g2, False)):
        ctx = _capi.Context(); ctx.upload(q.var_kind, q.var_dim, bi, groups, 0)
        try:
            ctx.set_variables(q.variables)
            if update: ctx.sweep_gradhess(); ctx.set_cost_data(0, new, idx)
            res.append((ctx.sweep_gradhess(), ctx.get_bsm_data().copy(), ctx.get_grad().copy(), ctx.sweep_cost()))
        finally:
            ctx.close()
    (c_u, A_u, b_u, k_u), (c_f, A_f, b_f, k_f) = res
    assert np.isclose(c_u, c_f, rtol=RTOL) and np.isclose(k_u, k_f, rtol=RTOL) and rel(A_u, A_f) < RTOL and rel(b_u, b_f) < RTOL
    ols = _oracle_ls(q, g2, bi)
    assert np.isclose(c_u, ols.costgradhess(), rtol=RTOL) and rel(A_u, ols.data) < RTOL and rel(b_u, ols.b) < RTOL      # ... and the oracle on the new data


def _oracle_ls(q, groups, bi):
    from oracle import oracle as O
    op = O.OracleProblem(q.var_kind, q.var_dim, groups); op.set_variables(q.variables)
    return op.linear_system(bi, 0)
