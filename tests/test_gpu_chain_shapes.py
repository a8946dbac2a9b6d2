"""The chain band solvers (csrc/nlls_chain.hip) at the widths and lengths they branch on: the reduced solvers behind solve_mode 2 whenever block cyclic
reduction does not take the band -- by default every band of half bandwidth 81 .. 126, and every band under NLLS_FLAG_NO_BCR.

  form 1  band_ldlt_solve_kernel<SEG, NSLOT>: one persistent workgroup, the band window in registers.  Branches: the window 12/4 (bw <= 107) or 16/4; the chunk
          CH of the HBM -> LDS ring of RC = (PFC + 1) CH columns -- 32 while H = bw + nbd + 2 <= 96, 16 above, and 8 where the ring of CH 16 would not fit the
          150 KB of LDS the upload allows (bw >= 114 without a border: the LDS budget, not the CH H <= 3072 rule, is what reaches CH 8); the ring longer than,
          equal to and shorter than the band; the backward pass's three 64-row register blocks, rotated at every multiple of 64; border rows (0, 3, 15).
  form 2  band_blocked_factor_kernel + band_backward_tiles_kernel from one end;  form 3  twisted: from both ends, a separator of ws columns solved by the same
          kernels at NBWs = ceil((ws - 1) / 16) -- chosen when nbd == 0, ws <= 16 NBW and kk >= 4 (NBW + 2), kk = (n_band - bw) / 16, ws = n_band - 16 kk.

Every case: the half bandwidth asserted on the CPU from the problem's (reduced, eliminated) pairs before anything is uploaded; then what the upload reports --
solve_mode, bandwidth, border and band unknowns, no cyclic reduction, and the chain form and window of nlls_get_solve_stats [51], [52]; then the project's bar
for this solver: x of a damped solve against the oracle's sparse LDL' at RTOL_X, the long-double backward error at ETA_BOUND["chain"] (check_step), status 0,
and one nlls_lm_trial against the separate calls at check_problem's tolerances.  Repeated solves are not compared byte for byte: without the cyclic reduction
there is no slab gather, and the assembly in front of the solve sums with atomics.

What the upload routes elsewhere (asserted as such, with x still held to the oracle):
  * bw 127 without a border, bw 125 with any: no chunk length fits the ring into 150 KB (CH 8 at bw 127: 154,328 B), so the widest band the register window
    takes is 126 (nbd 0), 124 (nbd 1), 120 (nbd 3), 111 (nbd 15); wider bands go to the dense LDL'.  A window of 21 six-dof cameras with the adaptive kernel's
    border (bw 125, nbd 3) is therefore no band solve; 19 cameras (bw 113) is, at CH 8.
  * bw 128: never a band solve (the decision edge bw <= 127).
What the upload cannot reach at all: the windows 8/1, 10/2, 12/2 (bw <= 72, where H <= 89 <= 96 with the border's 15 dof at most: always the blocked chain)."""
import functools

import numpy as np
import pytest

from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import synthetic, _capi
from tests.helpers import oracle_problem, blockindices, structured_problem, check_structure, longdouble_backward_error
from tests.test_gpu_parity import RTOL_X, ETA_BOUND, rel, check_step, solver_of      # (ETA_BOUND["chain"] = 1e-13 is applied inside check_step)

pytestmark = pytest.mark.gpu

NO_BCR, NO_TWIST = _capi.FLAG_NO_BCR, _capi.FLAG_NO_TWIST


# ---- problems --------------------------------------------------------------------------------------------------------------------------------------
def _half_bandwidth(red, el, dof):
    """half bandwidth (dof) of the reduced system that eliminating `el` leaves: an eliminated variable couples all its reduced neighbours `red` (0-based
    positions in the band, blocks of `dof` unknowns) pairwise -- the farthest pair, first unknown of the one to the last of the other"""
    red, el = np.asarray(red, np.int64), np.asarray(el, np.int64); el = el - el.min()
    lo = np.full(el.max() + 1, np.iinfo(np.int64).max); hi = np.full(el.max() + 1, -1)
    np.minimum.at(lo, el, red); np.maximum.at(hi, el, red)
    return int(dof * ((hi - lo).max() + 1) - 1)


def _camera_windows(ncam, wide, k_wide, k_narrow):
    """(camera, landmark) pairs, 1-based, camera-major: k_wide landmarks on every window of `wide` consecutive cameras and k_narrow on every pair of
    neighbours.  The narrow ones keep every camera under a quarter of all landmarks -- a camera that sees more is ordered into the border by the upload."""
    wins = [range(s, s + wide) for s in range(ncam - wide + 1) for _ in range(k_wide)] + [range(s, s + 2) for s in range(ncam - 1) for _ in range(k_narrow)]
    cam = np.concatenate([np.asarray(w) for w in wins]); lm = np.repeat(np.arange(len(wins)), [len(w) for w in wins])
    o = np.lexsort((lm, cam))
    return cam[o] + 1, lm[o] + 1, len(wins)


@functools.lru_cache(maxsize=None)
def _reference(spec):
    """spec -> (problem, blockindices, oracle system, its A.data, lambda, the oracle's damped x, half bandwidth from the pairs, band unknowns, border unknowns):
    formed once per problem, shared by the flag variants, left unchanged.
      ("rb", bw, n_band, border): b (x^2 - y), one-dof variables, every window of bw + 1 consecutive band variables once; `border` variables on every block
      ("ba", window cameras, cameras, members): affine cameras, `members` points on every window
      ("so3", window cameras, cameras): SO(3) poses under the adaptive kernel, whose variable (3 dof) couples to every block: the border"""
    kind = spec[0]
    if kind == "rb":
        _, bw, n_band, border = spec
        p, meta = structured_problem(K.RES_ROSENBROCK_B, [(bw + 1, 1)] * (n_band - bw), n_band + border, ps=1, seed=bw + n_band, border=border)
        vi, _ = next(iter(p.costs.values())).arrays(); red = vi[:, 0] - 1; inband = red < n_band
        bw_cpu = _half_bandwidth(red[inband], vi[inband, 1], 1); nbd = border; lam_scale = 1e-6
    elif kind == "ba":
        _, w, ncam, nmem = spec
        p, meta = structured_problem(K.RES_BA_AFFINE, [(w, nmem)] * (ncam - w + 1), ncam, seed=w + ncam)
        vi, _ = next(iter(p.costs.values())).arrays()
        bw_cpu = _half_bandwidth(vi[:, 0] - 1, vi[:, 1], 6); n_band, nbd = 6 * ncam, 0; lam_scale = 1e-6
    else:
        _, w, ncam = spec
        cam, lm, npts = _camera_windows(ncam, w, 3, 8)
        assert 4 * np.bincount(cam).max() <= npts, "a camera sees more than a quarter of the landmarks: the upload would order it into the border"
        p = synthetic.perturb_ba_problem(synthetic.create_so3_ba_problem(ncam, npts, 0.0, seed=w + ncam, adaptive=True, visibility=(cam, lm)), 1e-3, 1e-3)
        bw_cpu = _half_bandwidth(cam - 1, lm, 6); n_band, nbd = 6 * ncam, 3; meta = None; lam_scale = 1e-4
    bi = blockindices(p)
    ols = oracle_problem(p).linear_system(bi, 0); ols.costgradhess()
    if meta is not None: check_structure(ols, meta)
    A = ols.data.copy(); lam = ols.max_abs_diag() * lam_scale
    assert ols.solve(lam) == 0
    x = ols.x.copy(); x.setflags(write=False); A.setflags(write=False)
    return p, bi, ols, A, lam, x, bw_cpu, n_band, nbd


def _window(seg, nslot, ch):
    return 1000 * seg + 10 * nslot + ch // 8


def _solve_and_trial(ctx, info, ref, cid):
    """the damped solve and one LM trial of an uploaded context against the oracle; prints the case's line; returns x"""
    p, bi, ols, A, lam, x_ora = ref[:6]
    ctx.set_variables(p.variables); ctx.sweep_gradhess(); ctx.damp(lam)
    x = ctx.solve(want_x=True).copy(); st = ctx.solve_stats()
    r = rel(x, x_ora); eta = longdouble_backward_error(A, ols.bsm_index(), ols.b, lam, x)
    print(f"CHAIN {cid} form {st['chain_form']} window {st['chain_window']} bw {st['bandwidth']} nbd {info.nborder_dof} n_band {st['band_dof']} rel {r:.3e} eta {eta:.3e}")
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
    assert rel(x_trial, x_ora) < RTOL_X, f"{cid}: trial step vs oracle {rel(x_trial, x_ora)}"
    check_step(ctx, info, ols, A, lam, x_trial, cid + " trial")
    return x


def _run(cid, spec, flags, form, window):
    """upload under `flags`, assert the path (form 0: the upload is expected NOT to hand the band to the chain kernels), solve and compare"""
    ref = _reference(spec); p, bi = ref[:2]; bw_cpu, n_band, nbd = ref[6:]
    ctx = _capi.Context()
    try:
        info = ctx.upload(p.var_kind, p.var_dim, bi, p.groups(), flags); st = ctx.solve_stats()
        assert info.is_sparse and info.has_schur and info.nreduced_dof == n_band + nbd, (cid, info.nreduced_dof)
        assert st["bandwidth"] == bw_cpu and info.nborder_dof == nbd and st["band_dof"] == n_band, (cid, st["bandwidth"], bw_cpu, info.nborder_dof, st["band_dof"])
        if form == 0:
            print(f"CHAIN {cid}: no band solve, solve_mode {info.solve_mode}")
            assert info.solve_mode != 2 and (st["chain_form"], st["chain_window"]) == (0, 0), (cid, info.solve_mode, st["chain_form"])
        else:
            assert info.solve_mode == 2 and st["bcr_launches"] == 0 and solver_of(info, st) == "chain", (cid, info.solve_mode, st["bcr_launches"])
            assert (st["chain_form"], st["chain_window"]) == (form, window), (cid, st["chain_form"], st["chain_window"], form, window)
        return _solve_and_trial(ctx, info, ref, cid), st
    finally:
        ctx.close()


# ---- form 1: the register window, default flags ----------------------------------------------------------------------------------------------------------
W12_32, W12_16, W16_16, W16_8 = _window(12, 4, 32), _window(12, 4, 16), _window(16, 4, 16), _window(16, 4, 8)
# (id, spec, flags, window; 0: the upload does not take the band path).  PFC = ceil((bw + 1) / CH) + 1, RC = (PFC + 1) CH.
FORM1 = [
    ("rb_bw81_n160", ("rb", 81, 160, 0), 0, W12_32),            # the narrowest band the cyclic reduction does not take; H 83: CH 32, RC 160 = n_band
    ("rb_bw107_n192", ("rb", 107, 192, 0), 0, W12_16),          # the last band of the 12/4 window ...
    ("rb_bw108_n192", ("rb", 108, 192, 0), 0, W16_16),          # ... the first of 16/4
    ("rb_bw113_n192", ("rb", 113, 192, 0), 0, W16_16),          # the last band whose ring fits at CH 16 ...
    ("rb_bw114_n192", ("rb", 114, 192, 0), 0, W16_8),           # ... the first at CH 8 (the LDS budget)
    ("rb_bw126_n192", ("rb", 126, 192, 0), 0, W16_8),           # the widest band the upload hands over: the backward window spans three 64-row blocks; rotation at 192
    ("rb_bw126_n193", ("rb", 126, 193, 0), 0, W16_8),
    ("rb_bw127_n192", ("rb", 127, 192, 0), 0, 0),               # no chunk length fits the ring (module docstring): dense
    ("rb_bw127_n193", ("rb", 127, 193, 0), 0, 0),
    ("rb_bw128_n192", ("rb", 128, 192, 0), 0, 0),               # the decision edge bw <= 127, nothing else
    ("rb_bw94_n192", ("rb", 94, 192, 0), 0, W12_32),            # H 96: CH 32 ...
    ("rb_bw95_n192", ("rb", 95, 192, 0), 0, W12_16),            # ... H 97: CH 16
    # bw 125: CH 8, PFC 17, RC 144 -- the ring longer than the band (128, 129), a column short of it, equal, a column over (143, 144, 145), and wrapped (159, 160);
    # 128 is the smallest n_band the band path takes
    ("rb_bw125_n128", ("rb", 125, 128, 0), 0, W16_8),
    ("rb_bw125_n129", ("rb", 125, 129, 0), 0, W16_8),
    ("rb_bw125_n143", ("rb", 125, 143, 0), 0, W16_8),
    ("rb_bw125_n144", ("rb", 125, 144, 0), 0, W16_8),
    ("rb_bw125_n145", ("rb", 125, 145, 0), 0, W16_8),
    ("rb_bw125_n159", ("rb", 125, 159, 0), 0, W16_8),
    ("rb_bw125_n160", ("rb", 125, 160, 0), 0, W16_8),
    # bw 113 at CH 16: PFC 9, RC 160 -- the same three positions of the ring at the chunk length the wider bands do not get
    ("rb_bw113_n159", ("rb", 113, 159, 0), 0, W16_16),
    ("rb_bw113_n160", ("rb", 113, 160, 0), 0, W16_16),
    ("rb_bw113_n161", ("rb", 113, 161, 0), 0, W16_16),
    # the za / zb / zc rotation of the backward pass around multiples of 64; n_band no multiple of CH
    ("rb_bw101_n191", ("rb", 101, 191, 0), 0, W12_16),
    ("rb_bw101_n192", ("rb", 101, 192, 0), 0, W12_16),
    ("rb_bw101_n193", ("rb", 101, 193, 0), 0, W12_16),
    ("rb_bw101_n255", ("rb", 101, 255, 0), 0, W12_16),
    ("rb_bw101_n257", ("rb", 101, 257, 0), 0, W12_16),
    # the workload: 200 six-dof cameras, every point seen by 14, 18, 21 of them -- a band of 1200 that wraps the ring six times and more
    ("ba_w14_c200", ("ba", 14, 200, 4), 0, W12_32),             # bw 83
    ("ba_w18_c200", ("ba", 18, 200, 4), 0, W12_16),             # bw 107
    ("ba_w21_c200", ("ba", 21, 200, 4), 0, W16_8),              # bw 125
    # the adaptive kernel's three border rows through every pivot and the corner
    ("so3_w14_c40", ("so3", 14, 40), 0, W12_32),                # bw 83, H 88
    ("so3_w16_c40", ("so3", 16, 40), 0, W12_16),                # bw 95, H 100: CH 16 with a border
    ("so3_w19_c40", ("so3", 19, 40), 0, W16_8),                 # bw 113, H 118: the 16/4 window with a border; its ring fits at CH 8 only
    ("so3_w20_c40", ("so3", 20, 40), 0, W16_8),                 # bw 119: the widest camera window the register window takes with three border rows (the limit is bw 120)
    ("so3_w21_c40", ("so3", 21, 40), 0, 0),                     # bw 125 with a border: not a band solve
    # the one shape at bw <= 80 that leaves the blocked chain: H = 80 + 15 + 2 = 97 > 96
    ("rb_bw80_n192_b15", ("rb", 80, 192, 15), NO_BCR, W12_16),
    ("rb_bw79_n192_b15", ("rb", 79, 192, 15), NO_BCR, None),    # H 96: still blocked, one-sided (a border switches the twist off)
]


@pytest.mark.parametrize("cid,spec,flags,window", FORM1, ids=[c[0] for c in FORM1])
def test_register_window_shapes(cid, spec, flags, window):
    if window is None: _run(cid, spec, flags, 2, 0)
    else: _run(cid, spec, flags, 1 if window else 0, window)


def test_window_boundary_changes_the_instantiation():
    """bw 107 | 108 are the two sides of the 12/4 -> 16/4 boundary, bw 94 | 95 of CH 32 -> 16, bw 113 | 114 of CH 16 -> 8: the statistic must tell them apart"""
    assert len({W12_32, W12_16, W16_16, W16_8}) == 4
    got = {}
    for bw in (94, 95, 107, 108, 113, 114):
        p, bi = _reference(("rb", bw, 192, 0))[:2]
        ctx = _capi.Context(); ctx.upload(p.var_kind, p.var_dim, bi, p.groups(), 0); got[bw] = ctx.solve_stats()["chain_window"]; ctx.close()
    assert got[107] != got[108] and got[94] != got[95] and got[113] != got[114], got
    assert got[95] == got[107] and got[108] == got[113], got


def test_nan_pivot_is_an_error_return_and_the_context_recovers():
    """A NaN measurement on a form-1 band: whichever kernel meets it first (the elimination's block, or the band kernel's `d != d` test on the pivot it reaches --
    its loops are fixed-count) the solve returns NLLS_ERR_NOT_SPD; the same context then solves the clean problem to tolerance."""
    cid = "rb_bw101_n192"; ref = _reference(("rb", 101, 192, 0)); p, bi = ref[:2]
    g = next(iter(p.costs.values())); vi, da = g.arrays(); bad = da.copy(); bad[len(bad) // 3, 0] = np.nan
    ctx = _capi.Context()
    try:
        info = ctx.upload(p.var_kind, p.var_dim, bi, p.groups(), 0)
        assert info.solve_mode == 2 and ctx.solve_stats()["chain_form"] == 1
        ctx.set_variables(p.variables)
        ctx.set_cost_data(0, bad); ctx.sweep_gradhess(); ctx.damp(ref[4])
        with pytest.raises(_capi.NllsError) as e:
            ctx.solve()
        assert e.value.code == _capi.ERR_NOT_SPD
        ctx.set_cost_data(0, da)
        _solve_and_trial(ctx, info, ref, cid + " behind the NaN")
    finally:
        ctx.close()


# ---- forms 2 and 3: the blocked chain under NLLS_FLAG_NO_BCR ---------------------------------------------------------------------------------------------------
# (id, spec, twisted expected, NBW); kk = (n_band - bw) / 16, ws = n_band - 16 kk; twisted: nbd == 0 and ws <= 16 NBW and kk >= 4 (NBW + 2)
BLOCKED = [
    ("ba_w3_c45", ("ba", 3, 45, 4), False, 2),                  # bw 17, n_band 270: kk 15 < 16
    ("ba_w3_c46", ("ba", 3, 46, 4), True, 2),                   # 276: kk 16, ws 20: separator NBWs 2
    ("ba_w8_c63", ("ba", 8, 63, 4), False, 3),                  # bw 47, 378: kk 20, ws 58 > 48
    ("ba_w8_c64", ("ba", 8, 64, 4), True, 3),                   # 384: kk 21, ws 48: NBWs 3
    ("rb_bw80_n528", ("rb", 80, 528, 0), True, 5),              # kk 28, ws 80 = 16 NBW: NBWs 5
    ("rb_bw80_n529", ("rb", 80, 529, 0), False, 5),             # ws 81
    ("rb_bw80_n543", ("rb", 80, 543, 0), False, 5),             # ws 95
    ("so3_w3_c50", ("so3", 3, 50), False, 2),                   # bw 17, 300: kk 17, ws 28 -- long and short enough, but a border switches the twist off
]


@pytest.mark.parametrize("cid,spec,twisted,NBW", BLOCKED, ids=[c[0] for c in BLOCKED])
def test_blocked_chain_twisted_condition(cid, spec, twisted, NBW):
    bw_cpu, n_band, nbd = _reference(spec)[6:]
    kk = (n_band - bw_cpu) // 16; ws = n_band - 16 * kk
    assert (bw_cpu + 15) // 16 == NBW and twisted == (nbd == 0 and ws <= 16 * NBW and kk >= 4 * (NBW + 2)), (cid, bw_cpu, kk, ws)
    if twisted: assert (ws - 1 + 15) // 16 == {"ba_w3_c46": 2, "ba_w8_c64": 3, "rb_bw80_n528": 5}[cid], (cid, ws)      # the separator's own width class
    x, _ = _run(cid, spec, NO_BCR, 3 if twisted else 2, 0)
    x1, _ = _run(cid + " no_twist", spec, NO_BCR | NO_TWIST, 2, 0)
    assert rel(x, x1) < RTOL_X, (cid, rel(x, x1))
