"""The block cyclic reduction's panel and backward kernels over the shapes their code branches on (round 13: the from-LDS and the from-register entry of
bcr_factor, the root block's factor pre-multiplied inside the backward launch, no update launch for the root), at the smallest problems that reach them.

Tiles per block NT = 1 .. 5 (NLLS_BCR_NT_FULL=1: the block is ceil(bandwidth / 16) tiles, so the camera window of the generator picks NT), chains of
N = 2, 3, 4, 5, 8 and 9 blocks (both parities of the first level, a last level with a single survivor), with the SO(3) kind's three border rows (the
adaptive kernel's variable) and with affine cameras, and both forms of the backward pass.  Every case: the NT, N and launch count the upload reports;
x against the oracle's LDL' of the same linearisation at check_problem's tolerance; status 0 (no hand-off timed out); and, where the reduced system is assembled
without atomics (NLLS_FLAG_DETERMINISTIC), a second solve byte-identical.

What the library cannot reach from here: a band solve needs 128 band unknowns, the largest block is 80, so N = 1 (the root with no level in front of it)
exists only below the C API; NT = 1 starts at N = 9; and the generator's chains of two and three blocks (24 cameras) always come with 12 border unknowns,
the two end cameras of so short a chain.  The default assembly in front of the reduced solve sums with atomics, so two ctx.solve() calls differ in the last
bits whatever the reduced solver does.  All of that -- N = 1, 2, 3 with and without border rows in both backward forms, and the byte-identity of repeated solves
on the band-storage (default) path -- is asserted through the stand-alone harness over nlls_bcr.hip: test_harness_chains_both_backward_forms."""
import functools
import os
import subprocess

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import synthetic, _capi
from tests.helpers import oracle_problem, blockindices
from tests.test_gpu_parity import RTOL_X, rel, check_step

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name: (cameras, cameras per point, NT, N, border unknowns of the affine variant -- the SO(3) variant has the kernel's three more).  12 points per camera.
# Border 12: the generator's chains of 24 cameras order their two end cameras last; every other affine variant is asserted to have NO border.
SHAPES = {
    "nt1_n9": (22, None, 1, 9, 0),        # every point seen by two neighbouring cameras exactly (bandwidth 11; a window of the generator that narrow leaves points unseen): SO(3) cameras in both variants
    "nt2_n5": (22, 2.6, 2, 5, 0),
    "nt2_n8": (40, 2.6, 2, 8, 0),
    "nt3_n4": (26, 5.2, 3, 4, 0),
    "nt4_n3": (24, 7.9, 4, 3, 12),
    "nt4_n4": (36, 7.9, 4, 4, 0),
    "nt5_n2": (24, 10.5, 5, 2, 12),
    "nt5_n5": (54, 10.5, 5, 5, 0),
}


@functools.lru_cache(maxsize=None)
def _reference(shape, so3):
    """the problem, its oracle linearisation and the oracle's damped x: formed once per shape, shared by both backward forms"""
    ncam, cpp = SHAPES[shape][:2]
    if cpp is None:
        lm = np.arange(12 * ncam); c0 = lm % (ncam - 1); cam = np.concatenate([c0, c0 + 1]); lm = np.concatenate([lm, lm]); o = np.lexsort((lm, cam))
        p = synthetic.create_so3_ba_problem(ncam, 12 * ncam, 0.0, seed=5, adaptive=bool(so3), visibility=(cam[o] + 1, lm[o] + 1))
    elif so3: p = synthetic.create_so3_ba_problem(ncam, 12 * ncam, cpp / ncam, seed=5, adaptive=True)
    else: p = synthetic.create_ba_problem(ncam, 12 * ncam, cpp / ncam, seed=5)
    p = synthetic.perturb_ba_problem(p, 1e-3, 1e-3)
    bi = blockindices(p)
    ols = oracle_problem(p).linear_system(bi, 0); ols.costgradhess()
    A = ols.data.copy(); lam = ols.max_abs_diag() * 1e-4
    assert ols.solve(lam) == 0
    x = ols.x.copy(); x.setflags(write=False); A.setflags(write=False)
    return p, bi, ols, A, lam, x


def _solve_and_check(ctx, info, ols, A, lam, x_ora, where, identical):
    """identical: the context assembles the reduced system without atomics (NLLS_FLAG_DETERMINISTIC), so a second solve must give the same bytes; the default
    assembly flushes with atomics, and its x moves in the last bits from one solve to the next whatever the reduced solver does"""
    ctx.damp(lam)
    x = ctx.solve(want_x=True).copy()
    st = ctx.solve_stats()
    print(f"X {where} rel {rel(x, x_ora):.3e} status {st['status']}")
    assert st["status"] == 0, (where, st["status"])
    if identical:
        assert np.array_equal(ctx.solve(want_x=True).view(np.uint64), x.view(np.uint64)), f"{where}: two solves of one system differ"
        assert ctx.solve_stats()["status"] == 0
    assert rel(x, x_ora) < RTOL_X, f"{where}: x mismatch {rel(x, x_ora)}"
    check_step(ctx, info, ols, A, lam, x, where)
    return x


@pytest.mark.parametrize("level_backward", [0, 1], ids=["fused", "per_level"])
@pytest.mark.parametrize("so3", [0, 1], ids=["affine", "so3_border"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_panel_and_backward_shapes(shape, so3, level_backward, monkeypatch):
    ncam, cpp, NT, NB, border = SHAPES[shape]
    p, bi, ols, A, lam, x_ora = _reference(shape, so3)
    monkeypatch.setenv("NLLS_BCR_NT_FULL", "1")
    if level_backward: monkeypatch.setenv("NLLS_BCR_LEVEL_BACKWARD", "1")
    # the default assembly (band storage, converted to tiles in front of the levels) and the deterministic one (tiles gathered in place, no atomics anywhere:
    # the solve is bit-reproducible, tests/test_gpu_parity.py test_deterministic_flag_is_bit_reproducible)
    for flags in (0, _capi.FLAG_DETERMINISTIC):
        ctx = _capi.Context()
        info = ctx.upload(p.var_kind, p.var_dim, bi, p.groups(), flags)
        st = ctx.solve_stats()
        assert info.solve_mode == 2 and st["bcr_launches"] > 0, (info.solve_mode, st["bcr_launches"])
        assert st["bcr_block"] == 16 * NT, (st["bcr_block"], st["bandwidth"])
        assert (st["band_dof"] + 16 * NT - 1) // (16 * NT) == NB, (st["band_dof"], st["bcr_block"])
        assert info.nborder_dof == border + (3 if so3 else 0), info.nborder_dof      # (so3: the kernel's variable; 12: the two cameras a short chain orders last)
        # levels: the root and one per halving in front of it; launches: the conversion, a panel per level, an update per level BUT the root's,
        # and one backward launch (fused) or one per level
        L = st["bcr_levels"]; m, lv = NB, 1
        while m > 1: m = (m - 1) // 2 if m & 1 else m // 2; lv += 1
        assert L == lv and st["bcr_launches"] == (3 * L if level_backward else 2 * L + 1), (L, lv, st["bcr_launches"])
        ctx.set_variables(p.variables); ctx.sweep_gradhess()
        slab = bool(flags) and st["elim_slab"] > 0
        if flags and shape != "nt5_n2": assert slab, "every chain but the two-block one qualifies for the ordered gather"      # (two-block chains: test_harness_chains_both_backward_forms compares their bytes)
        _solve_and_check(ctx, info, ols, A, lam, x_ora, f"{shape} so3={so3} level_backward={level_backward} flags={flags} slab={int(slab)}", identical=slab)
        ctx.close()


@pytest.mark.parametrize("shape", ["nt4_n4", "nt5_n5"])
def test_guarded_refactorisation_and_the_floorless_instantiation(shape, monkeypatch):
    """A gauge-free problem (affine cameras, nothing fixed) solved UNDAMPED: the reduced system is singular, the pivots of the gauge directions fall below their
    floors, the tile that met one is factored again from the kept copy with the guard in the chain (bcr_factor), and the solve counts them (stats [10]).
    The oracle's x is no reference for that solve -- along the null space an exact LDL' returns (rounding) / (rounding) -- so the step is held to what it is
    for: on this noise-free problem, 1e-3 from its zero-residual optimum, the Gauss-Newton step leaves residuals of second order in the perturbation (the
    cost falls by about 1e-6; below 1e-2 is asserted).  The same context then solves DAMPED, floor on, against the oracle; and a context with
    NLLS_FLAG_NO_PIVOT_FLOOR (the panel's <false> instantiation) does."""
    p, bi, ols, A, lam, x_ora = _reference(shape, 0)
    monkeypatch.setenv("NLLS_BCR_NT_FULL", "1")
    ctx = _capi.Context(); info = ctx.upload(p.var_kind, p.var_dim, bi, p.groups(), _capi.FLAG_DETERMINISTIC)      # (no atomics in the assembly: two solves, the same bytes)
    assert info.solve_mode == 2 and ctx.solve_stats()["bcr_block"] == 16 * SHAPES[shape][2] and ctx.solve_stats()["elim_slab"] > 0
    ctx.set_variables(p.variables); c0 = ctx.sweep_gradhess()
    ctx.damp(0.0); x = ctx.solve(want_x=True).copy(); st = ctx.solve_stats()
    assert st["status"] == 0 and st["dropped_pivots"] > 0, st
    assert np.all(np.isfinite(x))
    assert np.array_equal(ctx.solve(want_x=True).view(np.uint64), x.view(np.uint64))
    ctx.retract(_capi.VARS_NEXT, _capi.VARS_CURRENT); c1 = ctx.sweep_cost(_capi.VARS_NEXT)
    print(f"GUARD {shape} dropped {st['dropped_pivots']} cost {c0:.3e} -> {c1:.3e}")
    assert c1 < 1e-2 * c0, (c0, c1)
    _solve_and_check(ctx, info, ols, A, lam, x_ora, f"{shape} damped behind the undamped solve", identical=True)
    ctx.close()
    ctx = _capi.Context(); info = ctx.upload(p.var_kind, p.var_dim, bi, p.groups(), _capi.FLAG_NO_PIVOT_FLOOR)
    assert info.solve_mode == 2 and ctx.solve_stats()["bcr_block"] == 16 * SHAPES[shape][2]
    ctx.set_variables(p.variables); ctx.sweep_gradhess()
    _solve_and_check(ctx, info, ols, A, lam, x_ora, f"{shape} no pivot floor", identical=False)
    ctx.close()


# (n, bandwidth, border rows) -> (NT, N) of the stand-alone harness: the chains the library cannot reach or cannot reach without border rows
HARNESS = {
    (16, 5, 0): (1, 1), (16, 5, 3): (1, 1), (48, 40, 0): (3, 1), (64, 64, 3): (4, 1), (80, 65, 0): (5, 1), (80, 65, 3): (5, 1),      # the root alone
    (32, 5, 0): (1, 2), (160, 65, 0): (5, 2), (160, 65, 3): (5, 2), (128, 64, 0): (4, 2),                                           # two blocks, without a border too
    (144, 40, 0): (3, 3), (192, 64, 0): (4, 3), (240, 65, 0): (5, 3),                                                                # three
    (256, 64, 0): (4, 4), (320, 64, 3): (4, 5), (512, 64, 0): (4, 8),
}


def test_harness_chains_both_backward_forms():
    """The chains the C API does not hand to the cyclic reduction (N = 1: a band solve needs 128 band unknowns, the largest block is 80) or only with border rows
    (N = 2, 3), through tools/bcr/bcr_test, which build() compiles: it includes csrc/nlls_bcr.hip itself -- the same source as libnlls_amd.so, a separately
    compiled copy, not the library -- and hands BcrSolver a random bordered band system in BAND STORAGE (the path through bcr_convert_kernel, the default
    assembly's).  Every case in both backward forms (fused; one launch per level, where N = 1 is the `<NT, false>` root launch with no level in front of it):
    x against a CPU bordered-band LDL' at 1e-9 of |x| (tighter than RTOL_X), status 0, and x of the sixth solve of the same system equal to x of the first BIT
    FOR BIT -- the cyclic reduction has no atomics; this is where the default path's reproducibility is asserted, since the library's own default assembly in
    front of it sums with atomics."""
    exe = os.path.join(ROOT, "tools", "bcr", "bcr_test")
    assert os.path.exists(exe), "tools/bcr/bcr_test is built by __graft_entry__.build()"
    args = []
    for (n, bw, nbd) in HARNESS:
        for form in ("fused", "level"): args += [str(n), str(bw), str(nbd), form]
    r = subprocess.run([exe, "list"] + args, capture_output=True, text=True, timeout=120)
    print(r.stdout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("case ")]
    assert r.returncode == 0 and "all ok" in r.stdout and len(lines) == 2 * len(HARNESS), (r.returncode, r.stdout, r.stderr)
    it = iter(lines)
    for (n, bw, nbd), (NT, NB) in HARNESS.items():
        for form in ("fused", "per-level"):
            l = next(it); f = l.split()
            assert f"n={n:5d} bw={bw:3d} nbd={nbd:2d} " in l and f" N={NB:4d} NT={NT} " in l and f" {form} " in l, l
            assert "status=0" in f and "repeat=identical" in f and f[-1] == "OK", l
            L = int(l.split("levels=")[1].split()[0]); launches = int(l.split("launches=")[1].split()[0])
            assert launches == (2 * L + 1 if form == "fused" else 3 * L), l          # (no update launch for the root)
