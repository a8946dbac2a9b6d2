"""The dense blocked LDL' (enqueue_reduced_solve in csrc/nlls_solve.hip; the panel and backward kernels in csrc/nlls_bcr.hip) and its windowed form at the sizes
their launches branch on: the reduced solver behind solve_mode 1 -- every band wider than the band kernels take, every structure the tile-sparse solver declines,
every system stored densely, everything under NLLS_FLAG_NO_BAND -- and the one-wavefront solve (solve_mode 0) on the other side of its edge n 63 | 64.

  full      npad = 64 ceil((n + 1) / 64) (the right-hand side rides along as row n): 128-column panels k = 0, 2, ... while two 64-blocks are left, each followed by one
            trailing update of the T = npad / 64 - k - 2 blocks behind it (syrk_update2_kernel on 64 x 64 tiles, or syrk_update128_kernel on T128 = ceil(T / 2)
            tiles of 128 x 128 when T128 >= dense_t128_min, 16 by default: never below n = 2111, so only NLLS_DENSE_T128_MIN=1 reaches it here, the half-empty last
            tile included whenever T is odd); an odd last 64-column panel with nothing behind it; then the backward substitution, fused or one launch per block.
  windowed  (`dense_window`: sparse, a Schur complement, n_band >= 1024, 2 (bw + 256) < n_band, no NLLS_FLAG_NO_BAND) npad = 128 ceil((n + 1) / 128); panel p
            touches the nwin = (127 + bw) / 128 blocks of 128 rows below it that the band reaches and the strip of blocks from n_band / 128 on (the border's and the
            right-hand side's rows; the last band rows too unless n_band is a multiple of 128).
  storage   a system without a Schur complement that the upload stores densely is copied into S by dense_to_S_kernel; one with a Schur complement is assembled
            into S by the elimination kernels.

Every case: on the CPU, before anything is uploaded, the half bandwidth from the problem's pairs (the chain tests' generators and their `_half_bandwidth`), the
solver and the window the upload must choose, npad and the launch counts that follow from it -- from the formulas of csrc/nlls_structure.cpp and
enqueue_reduced_solve, the table below holding npad and nwin as literals beside them; then what the upload reports; then the project's bar for this solver: x of a
damped solve against the oracle at RTOL_X, the long-double backward error at ETA_BOUND["dense"] (check_step), status 0, one nlls_lm_trial against the separate calls,
and a SECOND solve on the same context at 100 lambda against the oracle's second solve (the factored diagonal slots, inv(L_JJ)' and the zero-fill flags carry over).

The tile-sparse solver is offered every Schur complement of n >= 512 without NLLS_FLAG_NO_BAND; whether it takes one is a cost model's decision over a nested
dissection -- a formula over counts that the host-only nlls_nd_tiles gives on the CPU, restated and held to the upload in tests/test_gpu_tsp_shapes.py (`_expected`),
not here.  The windowed cases switch it off (NLLS_FLAG_NO_TILE_SPARSE); rb_130_1023 and rb_256_1024 are uploaded at default flags
and assert that it declines them (solve_mode 1).

Where the border comes from: the generators' own border variables (rb, so3), and on ba_43_180 the upload's rule that a reduced block coupled to more than a quarter of
the eliminated ones goes behind the band (`_quarter_rule_border` restates it): two of its cameras, twelve rows.

The NaN cases: dense_panel_kernel's loops are fixed-count (the `while` loops in it are index arithmetic on the thread's number), as are the update kernels', the
one-launch-per-block backward kernels' and small_solve_kernel's.  dense_bwd_fused_kernel polls x for a sentinel (a NaN of a payload no arithmetic produces: a NaN that
the factorisation left is published like any number and ends the poll) under a clock bound of half a second per hop: a NaN cannot stall it."""
import functools

import numpy as np
import pytest

from nllssolver_jl_amd import NLLSProblem, kinds as K
from nllssolver_jl_amd import _capi
from tests.helpers import oracle_problem, blockindices, longdouble_backward_error
from tests.test_gpu_parity import RTOL_X, ETA_BOUND, rel, check_step, solver_of      # (ETA_BOUND["dense"] = ETA_BOUND["small"] = 1e-13 is applied inside check_step)
# the chain tests' problems, formed once per process and shared with them: structured_problem / check_structure / _half_bandwidth / _camera_windows are used there
from tests.test_gpu_chain_shapes import _reference as _chain_reference, _half_bandwidth

pytestmark = pytest.mark.gpu

NO_BAND, NTS = _capi.FLAG_NO_BAND, _capi.FLAG_NO_TILE_SPARSE
assert ETA_BOUND["dense"] == 1e-13 and ETA_BOUND["small"] == 1e-13 and RTOL_X == 1e-7


# ---- problems --------------------------------------------------------------------------------------------------------------------------------------
def _all_pairs_problem(n):
    """n one-dof variables, one b (x^2 - y) block on every pair (which of the two is x drawn per pair, b uniform in 0.5 .. 2): every block of H is filled, the upload
    stores the system densely, nothing is eliminated"""
    rng = np.random.default_rng(n)
    p = NLLSProblem(); p.addvariables(rng.uniform(0.5, 1.5, (n, 1)))
    i, j = np.triu_indices(n, 1); vi = np.stack([i, j], axis=1) + 1
    flip = rng.random(len(vi)) < 0.5; vi[flip] = vi[flip][:, ::-1]
    p.addcosts(K.RES_ROSENBROCK_B, vi, rng.uniform(0.5, 2.0, (len(vi), 1)))
    return p


def _quarter_rule_border(red, el, dof, nred):
    """the reduced blocks the upload orders behind the band as border rows (build_schur, "reduced ordering"): with 64 eliminated blocks or more, a reduced block coupled
    to more than a quarter of them, taken in block order while the border stays within 15 unknowns.  red / el: per cost block, the 0-based reduced block and the
    eliminated variable's number; all reduced blocks of `dof` unknowns.  (No problem of this file stores a block between two reduced variables: the rule's other half.)"""
    pairs = np.unique(np.stack([np.asarray(red, np.int64), np.asarray(el, np.int64)], axis=1), axis=0)
    cnt = np.bincount(pairs[:, 0], minlength=nred); nelim = np.unique(pairs[:, 1]).size
    border, bd = [], 0
    for k in range(nred):
        if nelim >= 64 and 4 * cnt[k] > nelim and bd + dof <= 15: border.append(k); bd += dof
    return border


@functools.lru_cache(maxsize=None)
def _reference(spec):
    """spec -> dict(p, bi, ols, A, lam, x, x100, bw, n_band, nbd, sparse, schur): the oracle side, formed once per problem, shared by the flag and switch variants,
    left unchanged.  x / x100: the oracle's damped steps at lam and at 100 lam.
      ("ap", n): _all_pairs_problem;   ("rb", bw, n_band, border), ("ba", window cameras, cameras, members), ("so3", window cameras, cameras): the chain tests'"""
    if spec[0] == "ap":
        n = spec[1]; p = _all_pairs_problem(n); bi = blockindices(p)
        ols = oracle_problem(p).linear_system(bi, 0); ols.costgradhess()
        assert not ols.info.is_sparse and ols.info.ndof == n
        M = ols.data.copy().reshape(n, n).T; M = np.tril(M) + np.tril(M, -1).T; A = M.T.ravel()         # (mirrored as check_problem does: the device's A.data holds both halves)
        lam = ols.max_abs_diag() * 1e-6
        assert ols.solve(lam) == 0
        x = ols.x.copy(); bw, n_band, nbd, sparse, schur = 0, n, 0, False, False                        # (nothing eliminated: no Schur fill to bound, the statistic stays 0)
    else:
        p, bi, ols, A, lam, x, bw, n_band, nbd = _chain_reference(spec); sparse = schur = True
        assert ols.info.is_sparse
        if spec[0] != "so3":                                                                            # (so3: three-slot blocks; its quarter rule is asserted by the chain tests' generator)
            vi, _ = next(iter(p.costs.values())).arrays(); dof = 6 if spec[0] == "ba" else 1; nred = (n_band + nbd) // dof
            border = _quarter_rule_border(vi[:, 0] - 1, vi[:, 1], dof, nred)
            if spec[0] == "rb": assert border == list(range(n_band, n_band + nbd)), (spec, border)      # (the generator's border variables, nothing else)
            elif border:
                # a window of many cameras over few points: the rule takes cameras out of the band.  The band is what is left, in the caller's order
                pos = np.cumsum(~np.isin(np.arange(nred), border)) - 1; inband = ~np.isin(vi[:, 0] - 1, border)
                bw = _half_bandwidth(pos[vi[inband, 0] - 1], vi[inband, 1], dof); nbd = dof * len(border); n_band -= nbd
    assert ols.solve(100.0 * lam) == 0
    x100 = ols.x.copy()
    for a in (A, x, x100): a.setflags(write=False)
    return dict(p=p, bi=bi, ols=ols, A=A, lam=lam, x=x, x100=x100, bw=bw, n_band=n_band, nbd=nbd, sparse=sparse, schur=schur)


# ---- what the upload and the launch arithmetic must come to, restated from the code ------------------------------------------------------------------------
def _expected(ref, flags):
    """-> dict(mode, window, npad, nb128, ...) from nlls_structure.cpp ("choose the reduced-system solver") and enqueue_reduced_solve"""
    n_band, nbd, bw = ref["n_band"], ref["nbd"], ref["bw"]; n = n_band + nbd
    # (the band kernels are offered every sparse system of n_band >= 128 with bw <= 127 unless NLLS_FLAG_NO_BAND is set: no case of this file may be one of those)
    assert not ref["sparse"] or (flags & NO_BAND) or bw > 127 or n_band < 128
    mode = 0 if n < 64 else 1
    window = bool(mode == 1 and ref["sparse"] and ref["schur"] and n_band >= 1024 and not (flags & NO_BAND) and 2 * (bw + 256) < n_band)
    npad = 128 * ((n + 1 + 127) // 128) if window else 64 * ((n + 1 + 63) // 64)
    e = dict(mode=mode, window=int(window), npad=npad, nb128=(npad + 127) // 128, n=n)
    if window:
        e.update(nwin=(127 + bw) // 128, strip=n_band // 128, strip_shared=n_band % 128 != 0, rhs_fills_npad=n + 1 == npad)
    else:
        nblk = npad // 64; e.update(panels128=nblk // 2, odd_last_panel=nblk % 2, first_T=max(nblk - 2, 0))
    return e


def _solve_and_trial(ctx, info, ref, exp, cid):
    """the damped solve, one LM trial and the second solve at 100 lambda of an uploaded context against the oracle; prints the case's lines; returns x"""
    p, ols, A, lam = ref["p"], ref["ols"], ref["A"], ref["lam"]; index = ols.bsm_index() if info.is_sparse else None
    ctx.set_variables(p.variables); ctx.sweep_gradhess(); ctx.damp(lam)
    x = ctx.solve(want_x=True).copy(); st = ctx.solve_stats()
    r = rel(x, ref["x"]); eta = longdouble_backward_error(A, index, ols.b, lam, x)
    print(f"DENSE {cid} mode {info.solve_mode} window {st['dense_window']} npad {exp['npad']} rel {r:.3e} eta {eta:.3e}")
    assert st["status"] == 0, (cid, st["status"])
    assert r < RTOL_X, f"{cid}: x mismatch {r}"
    check_step(ctx, info, ols, A, lam, x, cid)
    # the same trial in one call against the separate entry points (check_problem's comparison and tolerances)
    xHx, gx = ctx.quadform()
    ctx.retract(_capi.VARS_NEXT, _capi.VARS_CURRENT)
    v = ctx.get_variables(_capi.VARS_NEXT); c_next = ctx.sweep_cost(_capi.VARS_NEXT)
    ctx.set_variables(np.zeros_like(v), _capi.VARS_NEXT)
    c_trial = ctx.lm_trial(0.0)
    assert np.isclose(c_trial, c_next, rtol=1e-9, atol=1e-300), (cid, c_trial, c_next)
    assert rel(ctx.get_variables(_capi.VARS_NEXT), v) < 1e-9
    xHx2, gx2 = ctx.quadform()
    assert np.isclose(xHx2, xHx, rtol=1e-8) and np.isclose(gx2, gx, rtol=1e-8), (cid, xHx2, xHx, gx2, gx)
    assert np.isclose(ctx.step_maxabs(), np.max(np.abs(x)), rtol=1e-8)
    x_trial = ctx.get_step()
    assert ctx.solve_stats()["status"] == 0
    assert rel(x_trial, ref["x"]) < RTOL_X, f"{cid}: trial step vs oracle {rel(x_trial, ref['x'])}"
    check_step(ctx, info, ols, A, lam, x_trial, cid + " trial")
    # the second solve of the same context: lambda + 99 lambda (nlls_damp accumulates; the sum's rounding, 1e-16 lambda, is far below either bound)
    ctx.damp(99.0 * lam)
    x2 = ctx.solve(want_x=True).copy()
    r2 = rel(x2, ref["x100"]); eta2 = longdouble_backward_error(A, index, ols.b, 100.0 * lam, x2)
    print(f"DENSE {cid}@100lam mode {info.solve_mode} window {st['dense_window']} npad {exp['npad']} rel {r2:.3e} eta {eta2:.3e}")
    assert ctx.solve_stats()["status"] == 0
    assert r2 < RTOL_X, f"{cid}: x mismatch {r2} of the second solve"
    check_step(ctx, info, ols, A, 100.0 * lam, x2, cid + " 100 lam")
    return x


def _upload(ctx, ref, flags, cid):
    """upload under `flags` and assert the path against _expected -> (info, expected)"""
    p, bi = ref["p"], ref["bi"]; exp = _expected(ref, flags)                     # (on the CPU, before the upload)
    info = ctx.upload(p.var_kind, p.var_dim, bi, p.groups(), flags); st = ctx.solve_stats()
    print(f"DENSE {cid} upload: solve_mode {info.solve_mode} window {st['dense_window']} bw {st['bandwidth']} n_band {st['band_dof']} nbd {info.nborder_dof} reordered {st['reordered']} expected {exp}")
    assert bool(info.is_sparse) == ref["sparse"] and bool(info.has_schur) == ref["schur"], (cid, info.is_sparse, info.has_schur)
    assert info.solve_mode == exp["mode"], (cid, info.solve_mode, exp)
    assert st["dense_window"] == exp["window"], (cid, st["dense_window"], exp)
    assert st["bandwidth"] == ref["bw"] and st["band_dof"] == ref["n_band"], (cid, st["bandwidth"], ref["bw"], st["band_dof"], ref["n_band"])
    assert info.nborder_dof == ref["nbd"] and info.nreduced_dof == exp["n"], (cid, info.nborder_dof, info.nreduced_dof)
    assert solver_of(info, st) == ("dense" if exp["mode"] else "small"), (cid, solver_of(info, st))
    return info, exp


def _run(cid, spec, flags, npad=None, nwin=None, window=None):
    """upload, assert the path and the table's literals (npad; nwin: windowed expected), solve and compare -> (x, expected)"""
    ref = _reference(spec)
    ctx = _capi.Context()
    try:
        info, exp = _upload(ctx, ref, flags, cid)
        if npad is not None: assert exp["npad"] == npad, (cid, exp, npad)
        if window is not None: assert exp["window"] == window, (cid, exp)
        if nwin is not None: assert exp["window"] == 1 and exp["nwin"] == nwin, (cid, exp, nwin)
        return _solve_and_trial(ctx, info, ref, exp, cid), exp
    finally:
        ctx.close()


# ---- A. dense storage: dense_to_S_kernel, no elimination ----------------------------------------------------------------------------------------------------
# (n, npad, 128-column panels, odd last 64-column panel)
STORAGE = [
    (63, 64, 0, 1),        # SOLVE_SMALL: the last size of the one-wavefront solve (the small dense system's own route by default; small_solve_kernel under NLLS_TINY_DENSE=0)
    (64, 128, 1, 0),       # the first dense size: one 128-column panel, rows 64 .. 127 padding and the right-hand side
    (126, 128, 1, 0),      # (the size at which full-visibility bundle adjustment turns block-sparse)
    (127, 128, 1, 0),      # n + 1 = npad = 128: one panel, nothing behind it
    (128, 192, 1, 1),      # n + 1 = 129: the odd last 64-column panel, and a trailing update with T = 1
    (191, 192, 1, 1),      # n + 1 = npad = 192
    (192, 256, 2, 0),      # two panels, T = 2
    (255, 256, 2, 0),
    (256, 320, 2, 1),      # T = 3, 1 and the odd last panel
    (257, 320, 2, 1),
    (320, 384, 3, 0),      # three panels: T = 4, 2
]


def _storage_case(n, npad, panels, odd, cid):
    x, exp = _run(cid, ("ap", n), 0, npad=npad, window=0)
    if n >= 64: assert (exp["panels128"], exp["odd_last_panel"]) == (panels, odd), (cid, exp)
    assert exp["mode"] == (0 if n < 64 else 1)
    return x


@pytest.mark.parametrize("n,npad,panels,odd", STORAGE, ids=[f"ap_{c[0]}" for c in STORAGE])
def test_dense_storage_sizes(n, npad, panels, odd):
    """a densely stored system (all pairs of n scalars coupled) at n on both sides of every multiple of 64 up to 320: the edge of the one-wavefront solve, and npad's steps
    -- which change the number of 128-column panels and whether an odd 64-column panel ends the factorisation"""
    _storage_case(n, npad, panels, odd, f"ap_{n}")


def test_small_solve_kernel_at_its_last_size(monkeypatch):
    """n = 63 under NLLS_TINY_DENSE=0: the general route's small_solve_kernel itself, at the largest system it is handed"""
    monkeypatch.setenv("NLLS_TINY_DENSE", "0")
    _storage_case(63, 64, 0, 1, "ap_63_general")


# ---- B. a Schur complement into the full dense LDL' -------------------------------------------------------------------------------------------------------
# (id, spec, flags, npad)
FULL = [
    ("rb_8_64", ("rb", 8, 64, 0), NO_BAND, 128),               # the first size past the one-wavefront solve, assembled by the elimination
    ("rb_8_127", ("rb", 8, 127, 0), NO_BAND, 128),             # n + 1 = npad
    ("rb_8_128", ("rb", 8, 128, 0), NO_BAND, 192),             # the odd last panel
    ("rb_8_191", ("rb", 8, 191, 0), NO_BAND, 192),
    ("rb_8_192", ("rb", 8, 192, 0), NO_BAND, 256),
    ("rb_8_193", ("rb", 8, 193, 0), NO_BAND, 256),
    ("rb_130_1023", ("rb", 130, 1023, 0), 0, 1024),            # default flags.  The largest n_band that is not windowed; n + 1 = npad = 1024 by blocks of 64
    ("rb_256_1024", ("rb", 256, 1024, 0), 0, 1088),            # default flags.  2 (256 + 256) < 1024 is false: not windowed
]


@pytest.mark.parametrize("cid,spec,flags,npad", FULL, ids=[c[0] for c in FULL])
def test_schur_complement_into_the_full_factorisation(cid, spec, flags, npad):
    """a band of half bandwidth 8 under NLLS_FLAG_NO_BAND around n = 64, 128, 192; and the false sides of both window edges (n_band 1023; 2 (bw + 256) = n_band)"""
    _run(cid, spec, flags, npad=npad, window=0)


# ---- C. windowed ----------------------------------------------------------------------------------------------------------------------------------------
# (id, spec, npad, nwin)
WINDOWED = [
    ("rb_130_1024", ("rb", 130, 1024, 0), 1152, 2),            # the smallest windowed system; the strip's block holds the right-hand side's row alone
    ("rb_255_1024", ("rb", 255, 1024, 0), 1152, 2),            # the true side of 2 (bw + 256) < n_band
    ("rb_128_1024", ("rb", 128, 1024, 0), 1152, 1),            # nwin 1 ...
    ("rb_129_1150", ("rb", 129, 1150, 0), 1152, 2),            # ... nwin 2; the strip's block 8 also holds the band rows 1024 .. 1149
    ("rb_129_1151", ("rb", 129, 1151, 0), 1152, 2),            # n + 1 = npad
    ("rb_129_1153", ("rb", 129, 1153, 0), 1280, 2),            # one band row alone in block 9 beside the right-hand side
    ("rb_256_1025", ("rb", 256, 1025, 0), 1152, 2),            # nwin 2 at its step ...
    ("ba_43_180", ("ba", 43, 180, 2), 1152, 3),                # ... nwin 3: bw 257; six-dof blocks.  Cameras 34 and 35 see more than a quarter of the 276 points: border, 12 rows
    #     (with six-dof blocks no coupled pair of unknowns lies 257 apart from a column that ends a panel -- 128 p + 127 is odd -- so this band never reaches its third block)
    ("rb_257_1027", ("rb", 257, 1027, 0), 1152, 3),            # nwin 3 with one-dof variables: the third block below every panel is reached; 2 (257 + 256) < 1027 by one
    ("ba_22_171", ("ba", 22, 171, 4), 1152, 2),                # bw 131, n_band 1026
    ("rb_129_1024_b1", ("rb", 129, 1024, 1), 1152, 2),         # a border row in the strip
    ("rb_129_1030_b3", ("rb", 129, 1030, 3), 1152, 2),         # three, behind six band rows
    ("so3_22_176", ("so3", 22, 176), 1152, 2),                 # bw 131, the adaptive kernel's three border rows, n_band 1056
]
WINDOWED_SPEC = {c[0]: c[1] for c in WINDOWED}


@pytest.mark.parametrize("cid,spec,npad,nwin", WINDOWED, ids=[c[0] for c in WINDOWED])
def test_windowed_factorisation(cid, spec, npad, nwin):
    """the window's decision edges, nwin on both sides of its steps, the strip alone in its block, sharing it with band rows and filling npad exactly, border rows; and
    the same system by the full LDL' (NLLS_FLAG_NO_BAND: not windowed, npad by blocks of 64)"""
    ref = _reference(spec); exp = _expected(ref, NTS)
    if cid == "rb_129_1150": assert exp["strip_shared"] and exp["strip"] == 8
    if cid == "rb_129_1151": assert exp["rhs_fills_npad"]
    if cid == "rb_129_1153": assert exp["strip"] == 9 and ref["n_band"] - 128 * exp["strip"] == 1
    if cid == "rb_130_1024": assert not exp["strip_shared"] and exp["strip"] == 8 and exp["nb128"] == 9
    x, _ = _run(cid, spec, NTS, npad=npad, nwin=nwin)
    x1, _ = _run(cid + " full", spec, NO_BAND, window=0)
    assert rel(x, x1) < RTOL_X, (cid, rel(x, x1))


# ---- D. switches on the window ------------------------------------------------------------------------------------------------------------------------------
# (rb_130_1023: npad / 64 = 16, every T even; rb_256_1024 and ap_256: 17 and 5, every T odd -- T128 = ceil(T / 2) with a half-empty last tile, down to T = 1)
SWITCHED = [("rb_129_1153", ("rb", 129, 1153, 0), NTS, 1), ("so3_22_176", ("so3", 22, 176), NTS, 1), ("rb_130_1023", ("rb", 130, 1023, 0), 0, 0),
            ("rb_256_1024", ("rb", 256, 1024, 0), 0, 0), ("ap_256", ("ap", 256), 0, 0)]
SWITCHES = [("NLLS_DENSE_T128_MIN", "1"), ("NLLS_DENSE_STEP_BACKWARD", "1"), ("NLLS_DENSE_DCH1", "0")]
_default_x = {}


@pytest.mark.parametrize("name,value", SWITCHES, ids=[f"{n}={v}" for n, v in SWITCHES])
@pytest.mark.parametrize("cid,spec,flags,window", SWITCHED, ids=[c[0] for c in SWITCHED])
def test_switches_on_the_window(cid, spec, flags, window, name, value, monkeypatch):
    """NLLS_DENSE_T128_MIN=1: syrk_update128_kernel from the first pass on -- with its window arguments (wq, wstrip) on the windowed systems, with the half-empty last
    tile of an odd T on the full one; NLLS_DENSE_STEP_BACKWARD=1: one backward launch per block; NLLS_DENSE_DCH1=0: two X tile rows per panel workgroup (the windowed panels
    always take one: there the switch must change nothing).  The switches are read when the context is created."""
    monkeypatch.delenv(name, raising=False)
    if cid not in _default_x: _default_x[cid] = _run(cid + " default", spec, flags, window=window)[0]
    monkeypatch.setenv(name, value)
    x, _ = _run(f"{cid} {name}={value}", spec, flags, window=window)
    assert rel(x, _default_x[cid]) < RTOL_X, (cid, name, rel(x, _default_x[cid]))


# ---- E. error return and recovery --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,spec,flags", [("rb_129_1153", ("rb", 129, 1153, 0), NTS), ("ap_128", ("ap", 128), 0)], ids=["rb_129_1153", "ap_128"])
def test_nan_is_an_error_return_and_the_context_recovers(cid, spec, flags):
    """A NaN measurement on a windowed system and on a densely stored one: whichever kernel meets it first (the elimination's block, or the panel's test on the pivots
    of a tile -- no loop of the factorisation or the substitution depends on the data: module docstring) the solve returns NLLS_ERR_NOT_SPD; the same context, the clean
    data restored, then passes the full check"""
    ref = _reference(spec); p = ref["p"]
    g = next(iter(p.costs.values())); vi, da = g.arrays(); bad = da.copy(); bad[len(bad) // 3, 0] = np.nan
    ctx = _capi.Context()
    try:
        info, exp = _upload(ctx, ref, flags, cid + " NaN")
        ctx.set_variables(p.variables)
        ctx.set_cost_data(0, bad); ctx.sweep_gradhess(); ctx.damp(ref["lam"])
        with pytest.raises(_capi.NllsError) as e:
            ctx.solve()
        assert e.value.code == _capi.ERR_NOT_SPD
        ctx.set_cost_data(0, da)
        _solve_and_trial(ctx, info, ref, exp, cid + " behind the NaN")
    finally:
        ctx.close()
