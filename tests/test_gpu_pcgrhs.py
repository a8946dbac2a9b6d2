"""nlls_solve_pcg_rhs and nlls_marginal_cov: conjugate gradients on the device for right-hand sides of the caller's, eight columns at a time, and the blocks of
(H + lambda I)^-1 that are marginal covariances (include/nlls_amd.h).

Every test first runs the host mirror `pcg_mirror` of tests/test_gpu_pcg.py on the device's own A and asserts the input condition it relies on -- convergence inside
the cap of 4 ndof iterations, or the breakdown -- so that a bad input blames the input and not the kernel.

Tolerances are those of tests/test_gpu_pcg.py:
  a column against numpy.linalg.solve / numpy.linalg.inv on the device's A + lambda I: 1e-7 of the column's largest entry, at rtol 1e-10 (a covariance column IS a
         solve with a unit right-hand side);
  true residual ||(A + lambda I) x_k - b_k|| <= 2 rtol ||b_k|| at rtol 1e-8;
  the grid caps against the default, ||b_k||: 1e-11 -- the same sums in another order;
  the trial behind a call: 1e-9, the pattern of tests/test_gpu_pcg.py::test_a_trial_behind_a_solve_runs_as_before.
The byte rules are exact: two calls, a column among other columns, in another order, across the batch boundary at eight, under another round length, and nrhs = 1
with the gradient against nlls_solve_pcg."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import synthetic, _capi
from tests.helpers import blockindices
from tests.test_gpu_blockeval import chain_problem
from tests.test_gpu_linearize import affine_two_groups, device_system, upload, rel
from tests.test_gpu_apply import PROBLEMS, block_sizes
from tests.test_gpu_pcg import pcg_mirror, host_blocks, pd_lambda, swept, system_state, rosenbrock_two, hub65, dense_curve_rosenbrock

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, JACOBI = _capi.PCG_PRECOND_NONE, _capi.PCG_PRECOND_BLOCK_JACOBI
CUR, NEXT, BEST = _capi.VARS_CURRENT, _capi.VARS_NEXT, _capi.VARS_BEST
COLKEYS = ("iterations", "status", "bnorm", "rnorm")


def colstats(st, k):
    return tuple(st[key][k].item() for key in COLKEYS)


def mirror_converges(A, lam, bo, bs, cols, blocks=True, rtol=1e-10):
    """the input condition: the host mirror on the device's A converges on every column within 4 ndof iterations -> its iteration counts"""
    n = A.shape[0]; Al = A + lam * np.eye(n); its = []
    for k, col in enumerate(cols):
        _, it, status, _ = pcg_mirror(lambda v: Al @ v, host_blocks(A, lam, bo, bs) if blocks else None, bo, col, 4 * n, rtol)
        assert status == 0, f"column {k}: the host mirror did not converge in {4 * n} iterations (status {status}): the input is at fault"
        its.append(it)
    return its


# ---- 1. against numpy ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, _capi.FLAG_MATERIALIZE], ids=["default", "materialize"])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_against_numpy(name, flags):
    p, unfixed = PROBLEMS[name]()
    ctx, A, b, bo, bs = swept(p, unfixed, flags); ndof = ctx.info.ndof
    lam = pd_lambda(A); Al = A + lam * np.eye(ndof)
    Ball = np.random.default_rng(23).standard_normal((17, ndof))
    mirror_converges(A, lam, bo, bs, Ball[:3])
    blocks = ctx.hess_block_diag(lam)
    for nrhs in (1, 3, 8, 9, 17):
        B = Ball[:nrhs]; ref = np.linalg.solve(Al, B.T).T
        X, st = ctx.solve_pcg_rhs(B, lam, CUR, JACOBI, None, 1e-10)
        assert X.shape == (nrhs, ndof) and np.all(st["status"] == 0) and np.all(st["iterations"] >= 1), (name, nrhs, st)
        err = max(np.max(np.abs(X[k] - ref[k])) / np.max(np.abs(ref[k])) for k in range(nrhs))
        X8, st8 = ctx.solve_pcg_rhs(B, lam, CUR, JACOBI, None, 1e-8)
        res = max(np.linalg.norm(Al @ X8[k] - B[k]) / np.linalg.norm(B[k]) for k in range(nrhs))
        bn = max(abs(st["bnorm"][k] - np.linalg.norm(B[k])) / np.linalg.norm(B[k]) for k in range(nrhs))
        print(f"PCGRHS {name} flags {flags} nrhs {nrhs}: ndof {ndof} lambda {lam:.3e} iterations {st['iterations'].min()}..{st['iterations'].max()}; against numpy {err:.3e} (of 1e-7); "
              f"true residual at rtol 1e-8 {res:.3e} (of 2e-8); ||b|| {bn:.3e} (of 1e-11); synchronisations {st['synchronisations']} launches {st['launches']} "
              f"product vectors {st['product_vectors']} batches {st['batches']}")
        assert err <= 1e-7 and np.all(st8["status"] == 0) and res <= 2e-8 and bn <= 1e-11, (name, nrhs)
        assert np.all(st["rnorm"] <= 1e-10 * st["bnorm"]) and st["batches"] == -(-nrhs // 8)
        if nrhs == 3:                                                   # the mirror on the device's own products
            for k in range(3):
                _, kd, sd, _ = pcg_mirror(lambda v: ctx.hess_apply(v, lam), blocks, bo, B[k], 4 * ndof, 1e-10)
                assert sd == 0 and abs(st["iterations"][k] - kd) <= 1, (name, k, st["iterations"][k], kd)
    x1, s1 = ctx.solve_pcg_rhs(Ball[0], lam, CUR, JACOBI, None, 1e-10)  # 1-D in, 1-D out
    assert x1.shape == (ndof,) and s1["iterations"].shape == (1,)
    ctx.close()


# ---- 2. equal to nlls_solve_pcg -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", [JACOBI, NONE], ids=["blockjacobi", "none"])
def test_equal_to_solve_pcg(pc):
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed)
    lam = 1e-2 * np.max(np.abs(np.diag(A)))
    (k,) = mirror_converges(A, lam, bo, bs, [b], blocks=pc == JACOBI); assert k > 4
    ctx.damp(lam)
    for mi in (None, 4):                                                # converged; the cap reached: status 1 on both
        x, s = ctx.solve_pcg(pc, mi, 1e-10, want_x=True)
        X, st = ctx.solve_pcg_rhs(ctx.get_grad(), lam, CUR, pc, mi, 1e-10)
        assert s["status"] == (0 if mi is None else 1)
        assert X.tobytes() == (-x).tobytes(), (pc, mi)
        assert colstats(st, 0) == (s["iterations"], s["status"], s["bnorm"], s["rnorm"]), (pc, mi, st, s)
    ctx.close()


def test_interleaved_calls_share_buffers():
    """The three entry points share one driver and one set of buffers, regrown between calls, laid out by each call's own cap = min(columns, 8), with Minv left behind at
    another call's lambda.  558 unknowns: three workgroups of 256 per column, blocks of two sizes.  Every call of the sequence on ONE context returns, byte for byte and in
    every statistic, what the FIRST call on a fresh context of the same problem returns.

    For nlls_solve_pcg_rhs and nlls_marginal_cov the fresh context makes the same call.  nlls_solve_pcg reads the gradient of the context's own sweep, and two sweeps
    of this problem (two cost groups share rows: the accumulate sweep adds them with atomics) differ in the last bits -- on the MI355X the first solve_pcg of two fresh
    contexts differed in x from byte 8 on.  Its reference is therefore the call that takes that gradient as an ARGUMENT, nlls_solve_pcg_rhs(b, lambda = the damping,
    CURRENT, one column) as the first call of a fresh context: -X and the four statistics, byte for byte (the rule of test_equal_to_solve_pcg), the synchronisations
    ceil(k / round) + 1; and the second solve_pcg of the sequence, behind the two column calls, equals the first one of the same context in every byte and statistic."""
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed); ndof = b.size
    lam = 1e-2 * np.max(np.abs(np.diag(A))); lam2 = 0.5 * lam
    B9 = np.random.default_rng(29).standard_normal((9, ndof)); sel = [57, 4]                  # a point and a camera: m = 9, two batches of unit columns
    assert ndof == 558 and sorted(set(bs.tolist())) == [3, 6]
    (k,) = mirror_converges(A, lam, bo, bs, [b]); assert k > 4                                  # (maxiters = 4 below ends on the cap)
    mirror_converges(A, lam2, bo, bs, B9[:2])
    ctx.damp(lam); g = ctx.get_grad()
    step = lambda mi: ((lambda c: c.solve_pcg(JACOBI, mi, 1e-10, want_x=True)), (lambda c: c.solve_pcg_rhs(g, lam, CUR, JACOBI, mi, 1e-10)))
    cols = lambda f: (f, f)
    calls = [("solve_pcg", *step(None)),                                                        # (on the one context, as the first call of a fresh one)
             ("solve_pcg_rhs, 9 columns at another lambda", *cols(lambda c: c.solve_pcg_rhs(B9, lam2, CUR, JACOBI, None, 1e-10))),
             ("marginal_cov of two variables", *cols(lambda c: c.marginal_cov(sel, lam, CUR, JACOBI, None, 1e-10))),
             ("solve_pcg again", *step(None)),
             ("solve_pcg_rhs, one column", *cols(lambda c: c.solve_pcg_rhs(B9[3], lam2, CUR, JACOBI, None, 1e-10))),
             ("solve_pcg, maxiters 4", *step(4))]

    def same(u, v):
        return type(u) is type(v) and (u.tobytes() == v.tobytes() if isinstance(u, np.ndarray) else u == v)

    seen = {}
    for what, call, first in calls:
        got, gs = call(ctx)
        fresh = swept(p, unfixed)[0]; fresh.damp(lam); ref, rs = first(fresh); fresh.close()
        print(f"PCGRHS interleaved, {what}: iterations {np.asarray(gs['iterations']).tolist()} status {np.asarray(gs['status']).tolist()} launches {gs['launches']}")
        assert np.all(rs["status"] == (1 if "maxiters" in what else 0)), (what, rs)
        if call is first:
            assert got.shape == ref.shape and got.tobytes() == ref.tobytes(), what
            assert gs.keys() == rs.keys() and all(same(gs[key], rs[key]) for key in rs), (what, gs, rs)
            continue
        assert got.shape == ref.shape == (ndof,) and got.tobytes() == (-ref).tobytes() and ctx.get_step().tobytes() == got.tobytes(), what
        assert (gs["iterations"], gs["status"], gs["bnorm"], gs["rnorm"]) == colstats(rs, 0), (what, gs, rs)
        assert gs["rounds"] == gs["iterations"] + 1, (what, gs)                               # (round length 1)
        seen[what] = (got.tobytes(), dict(gs))
    assert seen["solve_pcg again"] == seen["solve_pcg"] and seen["solve_pcg, maxiters 4"][1]["iterations"] == 4
    assert ctx.get_grad().tobytes() == g.tobytes()
    ctx.close()


# ---- 3. column independence ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", [JACOBI, NONE], ids=["blockjacobi", "none"])
def test_column_independence(pc):
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed); ndof = b.size
    lam = 1e-2 * np.max(np.abs(np.diag(A))); Al = A + lam * np.eye(ndof)
    unit = np.zeros(ndof); unit[ndof // 3] = 1.0
    cols = [b, unit, np.zeros(ndof)]
    if pc == NONE:
        w, V = np.linalg.eigh(Al); ev = V[:, ndof // 2].copy()
        _, kev, sev, _ = pcg_mirror(lambda v: Al @ v, None, bo, ev, 4 * ndof, 1e-8)
        assert (kev, sev) == (1, 0), "the mirror should finish an eigenvector in one iteration: the input is at fault"
        cols.append(ev)
    rtol = 1e-8
    mirror_converges(A, lam, bo, bs, [c for c in cols if np.any(c)], blocks=pc == JACOBI, rtol=rtol)
    C = np.stack(cols); n = len(cols); filler = np.random.default_rng(5).standard_normal((17, ndof))
    call = lambda B: ctx.solve_pcg_rhs(B, lam, CUR, pc, None, rtol)
    X0, s0 = call(C)
    assert np.all(s0["status"] == 0) and s0["batches"] == 1
    assert colstats(s0, 2)[:2] == (0, 0) and s0["bnorm"][2] == 0.0 and not np.any(X0[2]) and X0[2].tobytes() == np.zeros(ndof).tobytes()      # the zero column ends at once
    if pc == NONE:
        assert s0["iterations"][3] == 1
    assert s0["product_vectors"] == s0["iterations"].sum(), s0       # (round length 1, the default: a finished column pays for no product)
    X1, s1 = call(C)                                                    # two identical calls
    assert X1.tobytes() == X0.tobytes() and all(np.array_equal(s0[key], s1[key]) for key in s0)
    Xr, sr = call(C[::-1])                                              # reversed
    for k in range(n):
        assert Xr[n - 1 - k].tobytes() == X0[k].tobytes() and colstats(sr, n - 1 - k) == colstats(s0, k), ("reversed", k)
    for k in range(n):                                                  # each alone
        xa, sa = call(C[k]); assert xa.tobytes() == X0[k].tobytes() and colstats(sa, 0) == colstats(s0, k), ("alone", k)
    for r in range(n):                                                  # at positions 7, 8 and 9 of 17 columns, across the batch boundary: every column at each of them once
        B = filler.copy(); ks = [(r + j) % n for j in range(3)]; B[7:10] = C[ks]; Xe, se = call(B)
        assert se["batches"] == 3
        for pos, k in zip((7, 8, 9), ks):
            assert Xe[pos].tobytes() == X0[k].tobytes() and colstats(se, pos) == colstats(s0, k), ("embedded", pos, k)
    for rnd in (3, 1000, 1):
        ctx.set_option(_capi.OPT_PCG_ROUND, rnd); Xn, sn = call(C)
        print(f"PCGRHS precond {pc} round {rnd}: iterations {sn['iterations'].tolist()} synchronisations {sn['synchronisations']} product vectors {sn['product_vectors']}")
        assert Xn.tobytes() == X0.tobytes() and all(np.array_equal(sn[key], s0[key]) for key in COLKEYS), rnd
        assert sn["product_vectors"] >= s0["product_vectors"] and (rnd != 1 or sn["product_vectors"] == sn["iterations"].sum())
    B17 = filler.copy(); _, s17 = call(B17)
    assert s17["batches"] == 3 and s17["product_vectors"] == s17["iterations"].sum()
    ctx.close()


# ---- 4. grid caps -------------------------------------------------------------------------------------------------------------------------------------
def test_grid_caps():
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed); ndof = b.size
    lam = 1e-2 * np.max(np.abs(np.diag(A)))
    B = np.stack([b, np.random.default_rng(3).standard_normal(ndof), np.eye(ndof)[5]])
    mirror_converges(A, lam, bo, bs, B)
    X0, s0 = ctx.solve_pcg_rhs(B, lam, CUR, JACOBI, None, 1e-10)
    assert ndof == 558 and np.all(s0["status"] == 0)                    # three workgroups of 256 per column by default: the caps 1 and 2 stride, 3 is the default grid
    for g in (1, 2, 3):
        ctx.set_option(_capi.OPT_PCG_GRID_MAX, g)
        X, st = ctx.solve_pcg_rhs(B, lam, CUR, JACOBI, None, 1e-10); e = max(rel(X[k], X0[k]) for k in range(3))
        print(f"PCGRHS grid cap {g}: iterations {st['iterations'].tolist()} (default {s0['iterations'].tolist()}) against the default grid {e:.3e} (of 1e-11)")
        assert np.all(st["status"] == 0) and e <= 1e-11, g
        assert ctx.solve_pcg_rhs(B, lam, CUR, JACOBI, None, 1e-10)[0].tobytes() == X.tobytes()
    ctx.set_option(_capi.OPT_PCG_GRID_MAX, 1024)
    assert ctx.solve_pcg_rhs(B, lam, CUR, JACOBI, None, 1e-10)[0].tobytes() == X0.tobytes()
    ctx.close()


# ---- 5. ragged sizes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,make", [("dense curve + rosenbrock", dense_curve_rosenbrock), ("two-variable rosenbrock", rosenbrock_two), ("hub of 65", hub65)])
def test_ragged_sizes(name, make):
    ctx, A, b, bo, bs = swept(make()); ndof = ctx.info.ndof; lam = pd_lambda(A); Al = A + lam * np.eye(ndof)
    Ball = np.random.default_rng(11).standard_normal((9, ndof)); Ball[0] = b
    mirror_converges(A, lam, bo, bs, Ball[:2])
    for nrhs in (7, 9):
        for pc in (JACOBI, NONE):
            B = Ball[:nrhs]; ref = np.linalg.solve(Al, B.T).T
            X, st = ctx.solve_pcg_rhs(B, lam, CUR, pc, None, 1e-10)
            err = max(np.max(np.abs(X[k] - ref[k])) / np.max(np.abs(ref[k])) for k in range(nrhs))
            print(f"PCGRHS {name} nrhs {nrhs} precond {pc}: ndof {ndof} blocks of {sorted(set(bs.tolist()))} iterations {st['iterations'].tolist()}; against numpy {err:.3e} (of 1e-7)")
            assert np.all(st["status"] == 0) and err <= 1e-7 and st["batches"] == -(-nrhs // 8), (name, nrhs, pc)
    ctx.close()


# ---- 6. another variable set --------------------------------------------------------------------------------------------------------------------------
def test_another_variable_set_without_a_sweep():
    p, unfixed = affine_two_groups()
    # the input: the system at the moved point, from a context of its own that sweeps there
    moved = p.variables + 1e-3 * np.random.default_rng(9).standard_normal(p.variables.size)
    ref = upload(p, unfixed); ref.set_variables(moved); ref.sweep_gradhess(); A, _ = device_system(ref); bo, bs = block_sizes(ref); ref.close()
    ctx = upload(p, unfixed); ctx.set_variables(moved, NEXT); ndof = ctx.info.ndof      # a fresh upload, no sweep; CURRENT holds other values
    lam = pd_lambda(A); B = np.random.default_rng(10).standard_normal((3, ndof))
    mirror_converges(A, lam, bo, bs, B, rtol=1e-8)
    X, st = ctx.solve_pcg_rhs(B, lam, NEXT, JACOBI, None, 1e-8)
    Y = ctx.hess_apply(X, lam, which=NEXT)
    res = max(np.linalg.norm(Y[k] - B[k]) / np.linalg.norm(B[k]) for k in range(3))
    Xc, _ = ctx.solve_pcg_rhs(B, lam, CUR, JACOBI, None, 1e-8)
    print(f"PCGRHS which = NEXT without a sweep: residual through hess_apply {res:.3e} (of 2e-8); against the solve at CURRENT {rel(X, Xc):.3e}")
    assert np.all(st["status"] == 0) and res <= 2e-8 and X.tobytes() != Xc.tobytes()
    ctx.close()


# ---- 7. breakdowns ------------------------------------------------------------------------------------------------------------------------------------
def raw_rhs(ctx, B, lam, pc, mi, rtol, which=CUR):
    """the entry itself on the rows of B, its outputs behind sentinels -> (return value, X_out, stats_out)"""
    B = np.ascontiguousarray(B, np.float64); n = B.shape[0]
    out = np.full(B.shape, 7.25); st = np.full(4 * n + 4, -1.0)
    rc = ctx.L.nlls_solve_pcg_rhs(ctx.h, which, lam, pc, mi, rtol, n, _capi._p(B), _capi._p(out), _capi._p(st))
    return rc, out, st


def test_breakdown_on_an_indefinite_system():
    """the system of tests/test_gpu_pcg.py::test_breakdown_on_an_indefinite_system at lambda 0, as column 1 of 3"""
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(3, 5, 1.0, seed=2, robust=N.GemanMcclureKernel(0.01), outlier_frac=0.3, outlier_sigma=0.2), 1e-2, 1e-2)
    ctx, A, b, bo, bs = swept(p); ndof = ctx.info.ndof
    assert pcg_mirror(lambda v: A @ v, None, bo, b, 4 * ndof, 1e-10)[1:3] == (1, 2) and b @ A @ b <= 0, "b'Hb should be <= 0: the input is at fault"
    w, V = np.linalg.eigh(A); good = [V[:, -1].copy(), V[:, -2].copy()]      # harmless: eigenvectors of positive eigenvalues end in one iteration, p'Hp > 0
    assert w[-2] > 0 and all(pcg_mirror(lambda v: A @ v, None, bo, g, 4 * ndof, 1e-8)[1:3] == (1, 0) for g in good), "the input is at fault"
    rc, out, st = raw_rhs(ctx, np.stack([good[0], b, good[1]]), 0.0, NONE, 4 * ndof, 1e-8)
    assert rc == _capi.ERR_NOT_SPD and np.all(out == 7.25), (rc, st)
    assert (int(st[4]), int(st[5])) == (1, 2), st                       # column 1: iteration 1, status 2
    rc2, out2, st2 = raw_rhs(ctx, np.stack([good[0], good[1]]), 0.0, NONE, 4 * ndof, 1e-8)
    assert rc2 == _capi.OK and st[0:4].tobytes() == st2[0:4].tobytes() and st[8:12].tobytes() == st2[4:8].tobytes() and int(st2[1]) == 0
    with pytest.raises(_capi.NllsError) as e:
        ctx.solve_pcg_rhs(np.stack([good[0], b, good[1]]), 0.0, CUR, NONE, None, 1e-8)
    assert e.value.code == _capi.ERR_NOT_SPD and ctx.last_pcg_rhs["status"].tolist() == [0, 2, 0]
    ctx.close()


def test_breakdown_of_the_preconditioner_at_lambda_zero():
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed, _capi.FLAG_MATERIALIZE); ndof = b.size
    assert pcg_mirror(lambda v: A @ v, host_blocks(A, 0.0, bo, bs), bo, b, 4 * ndof, 1e-10)[2] == 3, "a diagonal block should be indefinite at lambda 0: the input is at fault"
    B = np.random.default_rng(2).standard_normal((10, ndof))
    rc, out, st = raw_rhs(ctx, B, 0.0, JACOBI, 4 * ndof, 1e-10)
    assert rc == _capi.ERR_NOT_SPD and np.all(out == 7.25)
    assert np.all(st[:40].reshape(10, 4)[:, 1] == 3) and np.all(st[:40].reshape(10, 4)[:, 0] == 0) and st[42] == 0, st      # every column, no iteration, no product
    cov = np.full((6, 6), 7.25); cs = np.full(28, -1.0); vi = np.array([3], np.int64)
    rc = ctx.L.nlls_marginal_cov(ctx.h, CUR, 0.0, 1, _capi._p(vi), JACOBI, 4 * ndof, 1e-10, _capi._p(cov), _capi._p(cs))
    assert rc == _capi.ERR_NOT_SPD and np.all(cov == 7.25) and np.all(cs[:24].reshape(6, 4)[:, 1] == 3)
    ctx.close()


def test_a_nan_in_one_column():
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed); ndof = b.size
    lam = 1e-2 * np.max(np.abs(np.diag(A)))
    B = np.random.default_rng(4).standard_normal((3, ndof)); mirror_converges(A, lam, bo, bs, B[[0, 2]], rtol=1e-8)
    good = ctx.solve_pcg_rhs(B[[0, 2]], lam, CUR, JACOBI, None, 1e-8)[1]
    B[1, 17] = np.nan
    rc, out, st = raw_rhs(ctx, B, lam, JACOBI, 4 * ndof, 1e-8)
    assert rc == _capi.ERR_NOT_SPD and np.all(out == 7.25) and int(st[5]) == 2 and int(st[4]) == 1, st
    assert (int(st[1]), int(st[9])) == (0, 0) and (st[0], st[8]) == (good["iterations"][0], good["iterations"][1]) and (st[3], st[11]) == (good["rnorm"][0], good["rnorm"][1])
    ctx.close()


# ---- 8. nothing else moves ----------------------------------------------------------------------------------------------------------------------------
def test_state_is_untouched():
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed, _capi.FLAG_MATERIALIZE); ndof = b.size
    lam = 1e-2 * np.max(np.abs(np.diag(A))); ctx.damp(lam)
    ctx.solve_pcg(JACOBI, 3, 1e-10); ctx.set_step(np.linspace(-1.0, 2.0, ndof))
    ctx.set_variables(ctx.get_variables(CUR) * (1 + 1e-6), NEXT)
    pcg = lambda: {k: v for k, v in ctx.solve_stats().items() if k.startswith("pcg")}
    before = system_state(ctx) + [ctx.get_step().tobytes()]; pb = pcg()
    assert pb["pcg_iterations"] == 3 and pb["pcg_status"] == 1
    X, st = ctx.solve_pcg_rhs(np.random.default_rng(1).standard_normal((9, ndof)), 0.5 * lam, NEXT, JACOBI, None, 1e-8)
    assert system_state(ctx) + [ctx.get_step().tobytes()] == before and pcg() == pb
    cov, cs = ctx.marginal_cov([3, 41], 0.5 * lam, BEST, JACOBI, None, 1e-8)
    assert system_state(ctx) + [ctx.get_step().tobytes()] == before and pcg() == pb
    x = ctx.solve(want_x=True)                                          # the damping is the context's, not the calls'
    assert rel(x, -np.linalg.solve(A + lam * np.eye(ndof), b)) <= 1e-7
    ctx.close()


def _trial_run(p, call, materialise):
    ctx = upload(p, None, _capi.FLAG_DETERMINISTIC)
    if materialise:
        ctx.set_option(_capi.OPT_MATERIALIZE, 1)
    ctx.copy_variables(NEXT, CUR)
    c0 = ctx.sweep_gradhess(); lam = 1e-3
    if call:
        big = 1e-2 * ctx.max_abs_diag(); ndof = ctx.info.ndof
        _, st = ctx.solve_pcg_rhs(np.random.default_rng(6).standard_normal((9, ndof)), big, CUR, JACOBI, 4, 1e-10); assert st["batches"] == 2 and np.all(st["iterations"] >= 1)
        _, st = ctx.marginal_cov([2], big, CUR, JACOBI, 4, 1e-10); assert np.all(st["iterations"] >= 1)
    c1 = ctx.lm_trial(lam); mf = ctx.solve_stats()["mf_trials"]
    out = (c0, c1, ctx.get_step().tobytes(), ctx.get_variables(NEXT).tobytes()); ctx.close()
    return out, mf


@pytest.mark.parametrize("materialise", [False, True], ids=["matrix-free", "materialised"])
def test_a_trial_behind_the_calls_runs_as_before(materialise):
    """the pattern of tests/test_gpu_pcg.py::test_a_trial_behind_a_solve_runs_as_before: bytes cannot be compared across runs on these two paths"""
    p = chain_problem()
    (a, mfa), (c, mfc) = (_trial_run(p, call, materialise) for call in (False, True))
    assert mfa == mfc == (0 if materialise else 1), "the trial did not take the path the case was written for"
    print(f"PCGRHS trial behind the calls, materialise={materialise}: costs {a[:2]} / {c[:2]}")
    assert np.allclose(c[:2], a[:2], rtol=1e-9, atol=0.0)
    assert np.allclose(np.frombuffer(c[2]), np.frombuffer(a[2]), rtol=1e-9, atol=1e-12) and np.allclose(np.frombuffer(c[3]), np.frombuffer(a[3]), rtol=1e-9, atol=1e-12)


# ---- 9. covariance ------------------------------------------------------------------------------------------------------------------------------------
def cov_case(name):
    """(problem, unfixed, the listed variables -- 1-based, NOT ascending: an eliminated point, the kernel's variable where there is one, a reduced camera)"""
    if name == "affine two groups":
        p, unfixed = affine_two_groups(); return p, unfixed, [57, 4, 120]         # a point, camera 4, another point: m = 12
    p = synthetic.create_so3_ba_problem(4, 30, 0.5, seed=6, adaptive=True); return p, None, [9, 1, 3]      # a point, the kernel's variable, a camera: m = 12


@pytest.mark.parametrize("name", ["affine two groups", "so3 adaptive"])
def test_covariance(name):
    p, unfixed, sel = cov_case(name)
    ctx, A, b, bo, bs = swept(p, unfixed); ndof = ctx.info.ndof; lam = pd_lambda(A); Al = A + lam * np.eye(ndof)
    bi = blockindices(p, unfixed).astype(np.int64)
    assert all(bi[v - 1] > 0 for v in sel) and sel != sorted(sel)
    rows = np.concatenate([bo[bi[v - 1] - 1] + np.arange(bs[bi[v - 1] - 1]) for v in sel]); m = rows.size
    assert m > 8 and (name != "so3 adaptive" or p.var_kind[0] == K.VAR_CONTAMINATED_GAUSSIAN)
    E = np.zeros((m, ndof)); E[np.arange(m), rows] = 1.0
    mirror_converges(A, lam, bo, bs, E[[0, m - 1]])
    ref = np.linalg.inv(Al)[np.ix_(rows, rows)]
    cov, st = ctx.marginal_cov(sel, lam, CUR, JACOBI, None, 1e-10)
    assert cov.shape == (m, m) and np.all(st["status"] == 0) and st["batches"] == 2
    err = max(np.max(np.abs(cov[:, j] - ref[:, j])) / np.max(np.abs(ref[:, j])) for j in range(m))
    print(f"PCGRHS covariance {name}: ndof {ndof} m {m} lambda {lam:.3e} iterations {st['iterations'].tolist()}; against numpy.linalg.inv {err:.3e} (of 1e-7); "
          f"asymmetry {np.max(np.abs(cov - cov.T)) / np.max(np.abs(cov)):.3e}; synchronisations {st['synchronisations']} product vectors {st['product_vectors']}")
    assert err <= 1e-7 and np.all(np.diag(cov) > 0)
    X, sx = ctx.solve_pcg_rhs(E, lam, CUR, JACOBI, None, 1e-10)        # the same unit columns through the other entry, picked at the same rows
    assert cov.tobytes() == np.ascontiguousarray(X[:, rows].T).tobytes() and all(np.array_equal(st[key], sx[key]) for key in COLKEYS)
    assert ctx.marginal_cov(sel, lam, CUR, JACOBI, None, 1e-10)[0].tobytes() == cov.tobytes()
    # refusals: a fixed variable, a repeated index, index 0, index nvar + 1 -- nothing written
    fixed = int(np.flatnonzero(bi == 0)[0]) + 1 if np.any(bi == 0) else None
    for bad in ([sel[0], fixed] if fixed else []), [sel[0], sel[1], sel[0]], [0], [p.nvariables + 1]:
        if not bad:
            continue
        vi = np.array(bad, np.int64); out = np.full(36 * 36, 7.25); s = np.full(4 * 36 + 4, 7.25)
        rc = ctx.L.nlls_marginal_cov(ctx.h, CUR, lam, vi.size, _capi._p(vi), JACOBI, 10, 1e-8, _capi._p(out), _capi._p(s))
        assert rc == _capi.ERR_INVALID_ARG and np.all(out == 7.25) and np.all(s == 7.25), bad
    ctx.close()
    # the layers above, on contexts of their own: the same matrix from both (the same kernels on the same values), held to the same bound
    with N.Solver(p, unfixed) as s:
        cs, ss = s.covariance(sel, lam)
        Xs, _ = s.solve_rhs(E[:2], lam, rtol=1e-8); Xo, _ = s.operator(lam).solve(E[:2], rtol=1e-8)
        res = max(np.linalg.norm(s.hessvec(Xs[k], lam) - E[k]) for k in range(2))       # (||e_k|| = 1)
    cm, sm = N.marginalcovariance(p, sel, lam, unfixed)
    assert cs.tobytes() == cm.tobytes() and np.all(ss["status"] == 0) and np.all(sm["status"] == 0)
    assert max(np.max(np.abs(cs[:, j] - ref[:, j])) / np.max(np.abs(ref[:, j])) for j in range(m)) <= 1e-7
    assert Xo.tobytes() == Xs.tobytes() and res <= 2e-8
    with N.Solver(p, unfixed) as s, pytest.raises(ValueError):
        s.covariance(sel, lam, maxiters=2)                              # strict: a column that ended on maxiters is no covariance


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = _capi.lib(); ctx = _capi.Context(); P = _capi._p
    B = np.ones((2, 6)); out = np.full((2, 6), 7.25); cov = np.full((3, 3), 7.25); vi = np.array([1], np.int64)
    st = np.full(16, 7.25)                                              # (4 * 2 + 4 of the two columns, 4 * 3 + 4 of a three-dof variable's covariance)
    rhs = lambda which=CUR, lam=0.0, pc=JACOBI, mi=10, rtol=1e-8, nrhs=2, b=B, o=out: L.nlls_solve_pcg_rhs(ctx.h, which, lam, pc, mi, rtol, nrhs, P(b), P(o), P(st))
    mc = lambda which=CUR, lam=0.0, nsel=1, v=vi, pc=JACOBI, mi=10, rtol=1e-8, o=cov: L.nlls_marginal_cov(ctx.h, which, lam, nsel, P(v), pc, mi, rtol, P(o), P(st))
    assert rhs() == _capi.ERR_NOT_READY and mc() == _capi.ERR_NOT_READY                                          # no upload yet
    p = N.NLLSProblem(); a = p.addvariable([0.1, 0.2, 0.3]); b = p.addvariable([0.3, -0.2, 0.5]); rng = np.random.default_rng(2)
    p.addcosts(K.RES_LINEAR3, [[a], [b], [a], [b]], rng.standard_normal((4, 12)))
    ctx.upload(p.var_kind, p.var_dim, blockindices(p), p.groups()); ctx.set_variables(p.variables)
    for call in (rhs, mc):
        for which in (-1, 3):
            assert call(which=which) == _capi.ERR_INVALID_ARG
        for pc in (-1, 2):
            assert call(pc=pc) == _capi.ERR_INVALID_ARG
        for mi in (0, -3):
            assert call(mi=mi) == _capi.ERR_INVALID_ARG
        for rtol in (np.nan, np.inf, -1e-3):
            assert call(rtol=rtol) == _capi.ERR_INVALID_ARG
        for lam in (np.nan, np.inf):
            assert call(lam=lam) == _capi.ERR_INVALID_ARG
        assert call(o=None) == _capi.ERR_INVALID_ARG
    for nrhs in (0, -1):
        assert rhs(nrhs=nrhs) == _capi.ERR_INVALID_ARG
    assert rhs(b=None) == _capi.ERR_INVALID_ARG
    for nsel in (0, -1):
        assert mc(nsel=nsel) == _capi.ERR_INVALID_ARG
    assert mc(v=None) == _capi.ERR_INVALID_ARG
    for bad in ([0], [3], [1, 1]):
        v = np.array(bad, np.int64); assert mc(nsel=v.size, v=v) == _capi.ERR_INVALID_ARG
    assert L.nlls_solve_pcg_rhs(None, CUR, 0.0, JACOBI, 10, 1e-8, 2, P(B), P(out), P(st)) == _capi.ERR_INVALID_ARG
    assert L.nlls_marginal_cov(None, CUR, 0.0, 1, P(vi), JACOBI, 10, 1e-8, P(cov), P(st)) == _capi.ERR_INVALID_ARG
    assert np.all(out == 7.25) and np.all(st == 7.25) and np.all(cov == 7.25), "a refused call wrote to an output"
    # no sweep is needed, and stats_out may be NULL
    assert L.nlls_solve_pcg_rhs(ctx.h, CUR, 0.0, JACOBI, 100, 1e-12, 2, P(B), P(out), None) == _capi.OK and np.all(out != 7.25)
    assert L.nlls_marginal_cov(ctx.h, CUR, 0.0, 1, P(vi), JACOBI, 100, 1e-12, P(cov), None) == _capi.OK and np.all(np.diag(cov) > 0)
    assert rhs(mi=100, rtol=1e-12) == _capi.OK and (int(st[1]), int(st[5]), int(st[11])) == (0, 0, 1)
    ctx.sweep_gradhess(); A, g = device_system(ctx)
    assert rel(out[0], np.linalg.solve(A, B[0])) <= 1e-9 and rel(cov.T, np.linalg.inv(A)[:3, :3]) <= 1e-9
    ctx.close()
    # a fixed variable has no row in H
    q = N.NLLSProblem(); a = q.addvariable([0.1, 0.2, 0.3]); b = q.addvariable([0.3, -0.2, 0.5]); q.addcosts(K.RES_LINEAR3, [[a], [b], [a], [b]], rng.standard_normal((4, 12)))
    ctx = upload(q, np.array([True, False])); st[:] = 7.25; cov[:] = 7.25
    v2 = np.array([2], np.int64); assert mc(v=v2) == _capi.ERR_INVALID_ARG and mc() == _capi.OK
    ctx.close()
    # a dynamic-size group: no per-block Hessian
    ctx = _capi.Context(); out[:] = 7.25; st[:] = 7.25; cov[:] = 7.25
    d = p.addvariable([1.0, 2.0, 3.0, 4.0], K.VAR_DYNAMIC)
    p.addcosts(K.COST_DYN_LINEAR, [[d]], rng.standard_normal((1, 4))); p.addcosts(K.RES_DYN_NORM, [[d]], np.zeros((1, 0)))
    ctx.upload(p.var_kind, p.var_dim, blockindices(p), p.groups()); ctx.set_variables(p.variables)
    B10 = np.ones((2, ctx.info.ndof)); o10 = np.full((2, ctx.info.ndof), 7.25)
    assert rhs(b=B10, o=o10) == _capi.ERR_UNSUPPORTED and mc() == _capi.ERR_UNSUPPORTED and np.all(o10 == 7.25) and np.all(st == 7.25) and np.all(cov == 7.25)
    ctx.close()
    # every variable fixed: ndof == 0
    q = N.NLLSProblem(); a = q.addvariable([0.1, 0.2, 0.3]); q.addcosts(K.RES_LINEAR3, [[a]], rng.standard_normal((1, 12)))
    ctx = upload(q, np.zeros(1, bool)); out[:] = 7.25; st[:] = 7.25
    assert ctx.info.ndof == 0 and rhs() == _capi.OK and np.all(out == 7.25) and np.all(st[:12] == 0.0) and np.all(st[12:] == 7.25)
    assert mc() == _capi.ERR_INVALID_ARG                                # (its one variable is fixed)
    ctx.close()


def test_sharded_contexts_are_refused():
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3), 1e-3, 1e-3)
    c = _capi.Context()
    try:
        c.set_shard(0, 2); c.upload(p.var_kind, p.var_dim, blockindices(p), p.groups(), _capi.FLAG_FORCE_SPARSE); c.set_variables(p.variables)
        assert c.shard_info()["nranks"] == 2 and c.shard_info()["replicated"] == 0
        ndof = c.info.ndof; B = np.ones((2, ndof)); out = np.full((2, ndof), 7.25); cov = np.full((6, 6), 7.25); vi = np.array([1], np.int64)
        assert c.L.nlls_solve_pcg_rhs(c.h, CUR, 1.0, JACOBI, 10, 1e-8, 2, _capi._p(B), _capi._p(out), None) == _capi.ERR_UNSUPPORTED and np.all(out == 7.25)
        assert c.L.nlls_marginal_cov(c.h, CUR, 1.0, 1, _capi._p(vi), JACOBI, 10, 1e-8, _capi._p(cov), None) == _capi.ERR_UNSUPPORTED and np.all(cov == 7.25)
    finally:
        c.close()


# ---- 11. a user kind ----------------------------------------------------------------------------------------------------------------------------------
def test_user_kind_in_a_process_of_its_own():
    userlib = os.path.join(ROOT, "nllssolver.jl_amd", "csrc", "libnlls_amd_userdemo.so")
    env = dict(os.environ, NLLS_AMD_LIB=userlib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pcgrhs_userkind_worker.py")], capture_output=True, text=True, env=env, timeout=600)
    print(out.stdout[-1500:])
    assert out.returncode == 0 and "user kind pcg rhs ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
