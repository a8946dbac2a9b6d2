"""The matrix-free back-substitution (csrc/nlls_mfb.hip) packs the supernodes of ONE batch four to a workgroup, one wavefront each, behind the workgroups of the
supernodes of several batches.  These are the smallest structures at which the packing can go wrong: a last packed workgroup with 1, 2, 3 and 4 live wavefronts, a grid
without any packed workgroup, single-batch supernodes of one member and of a full batch (8 members at six neighbour blocks), with none and with two several-batch
supernodes in front -- built from explicit visibility lists.

Which supernodes are which is build_mf's rule (csrc/nlls_structure.cpp), written out in _supernodes below: a run of eliminated variables with the same neighbours is a
supernode; it is of one batch where its members fit one wavefront, one lane per cost block: nmem <= min(64 // ncb, 8) (the LDS bound does not bind at ncb <= 7).  The
library reports no count of either class, so every case asserts the count of supernodes (solve_stats) and that the trial ran matrix-free.

What the structure does not admit: a matrix-free trial needs a reduced band of at least 128 unknowns (22 cameras) and at least as many eliminated blocks as reduced
ones, and a single-batch supernode holds at most 8 members -- so ONE or THREE single-batch supernodes WITHOUT a several-batch one cannot be built: one holds 8 points; three
hold 24 only at 8 members each, which needs windows of at most seven cameras -- at ncb = 8 (nd = 48, four tile rows) a member's slab is 3 (16 * 4 + 8) + 2 = 218 doubles and
a wavefront's LDS region 218 B + 72 + 745, within build_mf's 2446 only up to B = 7 -- and three windows of seven see 21 of the 22 cameras.  4, 5, 6 and 9 can.  With two several-batch supernodes in front every count is there: 0, 1, 2, 3, 4, 5, 6, 9.

The eliminated slot: 1 in both bundle-adjustment kinds (slots: camera, point); 0 -- the eliminated variable first -- in b (x^2 - y) with x eliminated, the one built-in
kind whose slot 0 can be eliminated (one-dof blocks; many single-batch supernodes of one to eight members).

Every case: the checks of tests/test_gpu_mf_shapes.py at its tolerances, two identical trials byte for byte (step, trial variables, the scalars the finishing workgroup
publishes), nlls_sweep_cost of the trial point == the trial's cost.

Four cases on a dyadic grid (below: the sweep's sums are exact there, so A and b do not depend on the order of its atomics): step and scalars against the bytes of the
commit BEFORE the packing (tests/golden/mfb_pack/*.bin, written once on the GPU by tools/mfb_pack_golden.py)."""
import os

import numpy as np
import pytest

from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import _capi
from oracle import oracle as O
from tests.helpers import oracle_problem, blockindices, structured_problem, check_structure, longdouble_backward_error, LD, bsm_coo, _ld_sym_matvec

pytestmark = pytest.mark.gpu

BA, SO3, RB = K.RES_BA_AFFINE, K.RES_BA_SO3, K.RES_ROSENBROCK_B
NCAM = 22                                       # 132 reduced unknowns: the narrow band the block cyclic reduction takes (128 at least)
BIG_NCB = 11                                    # a several-batch supernode: 12 or 6 points seen by 11 cameras (3 members per batch: four or two batches); two of them see every camera
TINY_MEMBERS = (8, 1, 8, 8, 3, 8, 1, 8, 5)      # members of the k-th single-batch supernode (six cameras each): a full batch, one member, in between
SCALARS_WRITTEN = (0, 1, 2, 4, 5, 8, 9, 10)     # what mf_finish_body writes of the eleven scalars: cost, max|x|, x'x, x'(H + lambda I)x, g'x, x'Hx, x'x, status


def windows_of(nbig, ntiny):
    """Per eliminated variable its cameras (0-based): nbig runs of 12 or 6 points seen by BIG_NCB cameras, then ntiny runs of TINY_MEMBERS[k] points seen by six cameras, the windows spread so that every
    camera is seen and neighbouring runs differ."""
    # (more points than cameras, or the points are not the eliminated class; fewer than 64, or a camera seen by a quarter of them leaves the band for the border and the band
    #  falls below the 128 unknowns of the block cyclic reduction)
    w, big_members = [], 12 if ntiny <= 3 else 6
    for b in range(nbig):
        w += [tuple(range(BIG_NCB * b, BIG_NCB * (b + 1)))] * big_members
    for k in range(ntiny):
        start = NCAM - 6 if ntiny == 1 else int(round(k * (NCAM - 6) / (ntiny - 1)))
        w += [tuple(range(start, start + 6))] * TINY_MEMBERS[k]
    cover = np.zeros(NCAM, int)
    for win in w: cover[list(win)] += 1
    assert cover.min() > 0, "a camera nobody sees"
    assert NCAM < len(w) < 64, "the points must be the most numerous block size, and no camera a border block"
    return w


def _supernodes(windows):
    """(several-batch, single-batch) supernodes of a list of windows, by build_mf's rule at ncb <= 7 or one-dof blocks."""
    runs, prev = [], None
    for w in windows:
        if w != prev or runs[-1][1] == 128: runs.append([len(w), 0])
        runs[-1][1] += 1; prev = w
    tiny = sum(1 for ncb, nmem in runs if nmem <= min(64 // ncb, 8))
    return len(runs) - tiny, tiny


def ba_problem(kind, windows, seed=0, noise=1e-3):
    """Cameras first, then the points; one cost block per (point, camera of its window), in point order."""
    from nllssolver_jl_amd import NLLSProblem, synthetic
    nelim = len(windows)
    cam = np.concatenate([np.asarray(w) for w in windows]); pt = np.repeat(np.arange(nelim), [len(w) for w in windows])
    if kind == BA:
        rng = np.random.default_rng(seed)
        cams = rng.standard_normal((NCAM, 6)) + np.array([1.0, 0, 0, 0, 1.0, 0]); pts = rng.random((nelim, 3)) + np.array([-0.5, -0.5, 10.0])
        p = NLLSProblem(); p.addvariables(cams); p.addvariables(pts)
        c, X = cams[cam], pts[pt]
        p.addcosts(BA, np.stack([cam + 1, pt + NCAM + 1], axis=1), np.stack([(c[:, 0:3] * X).sum(1), (c[:, 3:6] * X).sum(1)], axis=1))
    else:
        p = synthetic.create_so3_ba_problem(NCAM, nelim, 0.0, seed=seed + 1, adaptive=False, outlier_frac=0.0, noise=0.0, visibility=(cam + 1, pt + 1))
    synthetic.perturb_ba_problem(p, noise, noise, seed=seed + 1)
    return p, dict(elim_blocks=np.r_[np.zeros(NCAM, bool), np.ones(nelim, bool)], supernodes=sum(_supernodes(windows)), windows=windows, nred=NCAM)


# (id, kind, several-batch supernodes, single-batch supernodes)
CASES = ([(f"ba_big2_tiny{t}", BA, 2, t) for t in (0, 1, 2, 3, 4, 5, 6, 9)] + [(f"ba_big0_tiny{t}", BA, 0, t) for t in (4, 5, 6, 9)]
         + [(f"so3_big2_tiny{t}", SO3, 2, t) for t in (1, 3, 5)] + [("so3_big0_tiny4", SO3, 0, 4), ("so3_big0_tiny9", SO3, 0, 9)])
RB_RUNS = [(2, 40), (2, 3), (3, 1), (2, 8), (4, 5), (16, 4), (3, 2)]


def build_case(kind, nbig, ntiny):
    windows = windows_of(nbig, ntiny)
    assert _supernodes(windows) == (nbig, ntiny), _supernodes(windows)
    return ba_problem(kind, windows)


# ---- golden bytes ------------------------------------------------------------------------------------------------------------------------------------
# The camera rows of A and b come from the accumulate sweep, whose tiles at these sizes sum with atomics: with the generic problems above two processes of ONE library give
# different bytes of the step (notes/r16.md).  The golden cases therefore live on a dyadic grid: truth on multiples of 1/16, perturbations and hence residuals on multiples
# of 2^-8 and 2^-16, all magnitudes below 2^7 -- every product and every sum of the sweep (J'J: 24 bits, J'r: 35 bits + 6 for the sums) is EXACT in float64, so A and b are
# the same bits in whatever order the atomics land, and everything behind them (the matrix-free trial) has no atomics.
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mfb_pack")
GOLDEN_CASES = ((2, 1), (2, 5), (0, 4), (0, 5))       # (several-batch, single-batch): 1 and 5 with, 4 and 5 without (1 without cannot be built: 4, one full packed workgroup, stands for it)


def golden_name(nbig, ntiny):
    return f"ba_dyadic_big{nbig}_tiny{ntiny}"


def dyadic_ba_problem(windows, seed=5):
    from nllssolver_jl_amd import NLLSProblem
    rng = np.random.default_rng(seed); nelim = len(windows)
    cam = np.concatenate([np.asarray(w) for w in windows]); pt = np.repeat(np.arange(nelim), [len(w) for w in windows])
    cams = np.round(16 * (rng.standard_normal((NCAM, 6)).clip(-3, 3) + np.array([1.0, 0, 0, 0, 1.0, 0]))) / 16
    pts = np.round(16 * (rng.random((nelim, 3)) + np.array([-0.5, -0.5, 10.0]))) / 16
    c, X = cams[cam], pts[pt]
    meas = np.stack([(c[:, 0:3] * X).sum(1), (c[:, 3:6] * X).sum(1)], axis=1)                  # exact: multiples of 2^-8 below 2^7
    p = NLLSProblem()
    p.addvariables(cams + rng.integers(-3, 4, cams.shape) / 256); p.addvariables(pts + rng.integers(-3, 4, pts.shape) / 256)
    p.addcosts(BA, np.stack([cam + 1, pt + NCAM + 1], axis=1), meas)
    return p, dict(elim_blocks=np.r_[np.zeros(NCAM, bool), np.ones(nelim, bool)], supernodes=sum(_supernodes(windows)), windows=windows, nred=NCAM)


def golden_trial(nbig, ntiny):
    """(step, scalars) of the first damped trial of a golden case; NLLS_SUPERNODE_PIECE=128 is the caller's to set"""
    windows = windows_of(nbig, ntiny)
    assert _supernodes(windows) == (nbig, ntiny)
    p, meta = dyadic_ba_problem(windows)
    ols = oracle_problem(p).linear_system(blockindices(p)); ols.costgradhess()
    ctx = upload(p, meta)
    try:
        lam, c_t, x, sc, nmf = first_trial(ctx, ols)
        assert nmf == 1, "the trial did not run matrix-free"
        assert ctx.solve_stats()["elim_supernodes"] == meta["supernodes"]
    finally:
        ctx.close()
    return x, sc


def scalars_of(ctx):
    """the trial's scalars as the finishing workgroup left them on the device (nlls_lm_trial has synchronised): a plain hipMemcpy by the runtime the library itself uses"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    ptr, n = ctx.reduce_buffer(3); out = np.zeros(n)
    rc = hip.hipMemcpy(C.c_void_p(out.ctypes.data), C.c_void_p(ptr), C.c_size_t(8 * n), C.c_int(2))      # hipMemcpyDeviceToHost
    assert rc == 0, f"hipMemcpy: {rc}"
    return out[list(SCALARS_WRITTEN)].copy()


def upload(p, meta):
    """(NLLS_SUPERNODE_PIECE=128 is the caller's to set: runs are then never cut into pieces)"""
    bi = blockindices(p)
    ctx = _capi.Context(); info = ctx.upload(p.var_kind, p.var_dim, bi, p.groups(), 0)
    assert info.is_sparse and info.has_schur and info.nschur_blocks == int(meta["elim_blocks"].sum()) and info.solve_mode == 2, (info.solve_mode, info.nschur_blocks)
    ctx.set_variables(p.variables); ctx.set_variables(p.variables, _capi.VARS_NEXT)
    return ctx


def first_trial(ctx, ols):
    """sweep + one damped trial (lambda from the ORACLE's diagonal: the same number wherever this runs): (lambda, cost, step, scalars, mf trials it took)"""
    ctx.sweep_gradhess(); lam = ols.max_abs_diag() * 1e-6
    n0 = ctx.solve_stats()["mf_trials"]; c_t = ctx.lm_trial(lam)
    return lam, c_t, ctx.get_step(), scalars_of(ctx), ctx.solve_stats()["mf_trials"] - n0


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _check(p, meta, monkeypatch):
    op = oracle_problem(p); ols = op.linear_system(blockindices(p)); c0 = ols.costgradhess()
    check_structure(ols, meta)
    monkeypatch.setenv("NLLS_SUPERNODE_PIECE", "128")
    ctx = upload(p, meta)
    try:
        lam, c_t, x, sc, nmf = first_trial(ctx, ols)
        st = ctx.solve_stats()
        assert nmf == 1, "the trial did not run matrix-free"
        assert st["elim_supernodes"] == meta["supernodes"] and st["dropped_pivots"] == 0 and st["status"] == 0, st
        v = ctx.get_variables(_capi.VARS_NEXT); xHx, gx = ctx.quadform(); mx, nrm = ctx.step_maxabs(), ctx.step_norm()
        # two identical trials: the same bytes
        c_t2 = ctx.lm_trial(0.0)
        assert c_t2 == c_t and ctx.get_step().tobytes() == x.tobytes() and ctx.get_variables(_capi.VARS_NEXT).tobytes() == v.tobytes() and scalars_of(ctx).tobytes() == sc.tobytes()
        # the cost sweep of the trial point: the trial's own sum
        c_s = ctx.sweep_cost(_capi.VARS_NEXT)
        assert c_s == c_t, (c_s, c_t)
        # the step against the oracle's H and g (backward error) and against the materialised trial
        idx = ols.bsm_index()
        eta = longdouble_backward_error(ols.data, idx, ols.b, lam, x)
        assert eta <= 1e-13, f"backward error {eta:.3e}"
        ctx.set_option(_capi.OPT_MATERIALIZE, 1)
        n1 = ctx.solve_stats()["mf_trials"]; c_m = ctx.lm_trial(0.0)
        assert ctx.solve_stats()["mf_trials"] == n1
        assert rel(x, ctx.get_step()) < 1e-9 and np.isclose(c_m, c_t, rtol=1e-9, atol=1e-13 * c0), (rel(x, ctx.get_step()), c_m, c_t)
        ctx.set_option(_capi.OPT_MATERIALIZE, 0)
        # the trial's point, cost and statistics against the oracle
        op.set_variables(p.variables, O.VARS_NEXT); op.update(ols, O.VARS_NEXT, O.VARS_CURRENT, step=x)
        assert rel(v, op.get_variables(O.VARS_NEXT)) < 1e-13
        assert np.isclose(c_t, op.cost(O.VARS_NEXT), rtol=1e-11, atol=1e-13 * c0), (c_t, op.cost(O.VARS_NEXT))
        I, J, V = bsm_coo(idx, ols.data, len(ols.b)); xl = x.astype(LD)
        xHx_ref = float(xl @ _ld_sym_matvec(I, J, V, xl, len(xl)) + LD(lam) * (xl @ xl)); gx_ref = float(ols.b.astype(LD) @ xl)
        assert np.isclose(xHx, xHx_ref, rtol=1e-11) and np.isclose(gx, gx_ref, rtol=1e-11), (xHx, xHx_ref, gx, gx_ref)
        assert mx == np.max(np.abs(x)) and np.isclose(nrm, np.linalg.norm(x), rtol=1e-12)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind,nbig,ntiny", [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_packed_backsub(kind, nbig, ntiny, monkeypatch):
    p, meta = build_case(kind, nbig, ntiny)
    _check(p, meta, monkeypatch)


def test_packed_backsub_eliminated_slot_first(monkeypatch):
    """b (x^2 - y) with x -- slot 0 -- eliminated: the other instantiation (PS = 0), single-batch supernodes of one to eight members beside several-batch ones.  (One-dof
    blocks: the kind at which the stored trial point was not old + x before the packing -- the step's one product contracted into the retraction's sum -- and the cost
    sweep of the trial point missed the trial's cost in the last place: 31.38720306348433 against 31.387203063484325.)"""
    p, meta = structured_problem(RB, RB_RUNS, 160, 0)
    nbig, ntiny = _supernodes(meta["windows"])
    assert nbig >= 1 and ntiny >= 9 and nbig + ntiny == meta["supernodes"], (nbig, ntiny)
    _check(p, meta, monkeypatch)


@pytest.mark.parametrize("nbig,ntiny", GOLDEN_CASES, ids=[golden_name(*c) for c in GOLDEN_CASES])
def test_packed_backsub_golden_bytes(nbig, ntiny, monkeypatch):
    """The step and the published scalars of the first trial, byte for byte against the commit before the packing (tests/golden/mfb_pack, tools/mfb_pack_golden.py)."""
    monkeypatch.setenv("NLLS_SUPERNODE_PIECE", "128")
    x, sc = golden_trial(nbig, ntiny)
    ref = np.fromfile(os.path.join(GOLDEN, golden_name(nbig, ntiny) + ".bin"), np.float64)
    assert ref.size == x.size + sc.size, (ref.size, x.size)
    bad = np.nonzero(ref[:x.size].view(np.uint64) != x.view(np.uint64))[0]
    assert bad.size == 0, f"{bad.size} of {x.size} entries of the step differ from the golden bytes, the first at {bad[:5]}"
    assert ref[x.size:].tobytes() == sc.tobytes(), (ref[x.size:], sc)
