"""The panel kernel's tile column 0 (round 15: wave 0 takes its first diagonal tile and its floors from global memory straight into registers, and the barrier
behind the landing is gone), held to the bits of the commit before it.

1. Golden x.  tools/bcr/bcr_test (built by build(); it includes csrc/nlls_bcr.hip itself) solves a fixed, host-generated bordered band system; BCR_TEST_DUMP
   writes x of the first solve raw.  tests/golden/bcr_x/<n>_<bw>_<nbd>_<form>.bin is that x at the parent of round 15, made once on an MI355X.  No arithmetic
   changed, so the bytes must be equal: NT = 1 (column 0 is the only column, no look-ahead tile), NT = 3, NT = 4 with one, two and five blocks (every X-row
   count per workgroup), NT = 5 (the largest LDS footprint), with and without border rows, both backward forms.
2. The pivot floor on tile column 0 and on the last tile column of one eliminated block (`bcr_test floor`: the FLOOR instantiation, whose floors of column 0
   now come from registers and whose guarded re-factorisation starts from the register copy of the tile).  The issue asked for exactly zero rows and columns;
   an exactly zero pivot never reaches the floor -- the unguarded chain turns the tile into NaN, NaN is above no floor, the solve reports a bad pivot, at the
   parent as well -- so the two unknowns are singular by cancellation instead, as a gauge direction is (tools/bcr/bcr_test.hip, run_case).  Everything else
   is as asked: x = 0 there, the rest against a CPU LDL' of the system without them at 1e-9 |x|, the dropped count >= 1 and equal in the first and the sixth
   solve, x of the sixth solve the bytes of the first.
3. Through the library at NT = 4 and 5: a gauge-free problem undamped (guarded re-factorisation) and damped, against the oracle, byte-identical repeats, and
   the MFMA count of nlls_get_solve_stats against the launcher's formula written out again here."""
import os
import subprocess

import numpy as np
import pytest

from nllssolver_jl_amd import _capi
from tests.test_gpu_parity import RTOL_X, rel, check_step
from tests.test_gpu_bcr_panel import SHAPES, _reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "bcr", "bcr_test")
GOLDEN = os.path.join(ROOT, "tests", "golden", "bcr_x")

# (n, bandwidth, border rows) -> (NT, N)
CASES = {
    (16, 5, 0): (1, 1), (32, 5, 0): (1, 2),
    (48, 40, 0): (3, 1), (144, 40, 0): (3, 3),
    (64, 64, 3): (4, 1), (128, 64, 0): (4, 2), (320, 64, 3): (4, 5),
    (80, 65, 3): (5, 1), (160, 65, 0): (5, 2),
}


def test_x_is_the_parents_bit_for_bit(tmp_path):
    assert os.path.exists(EXE), "tools/bcr/bcr_test is built by __graft_entry__.build()"
    for (n, bw, nbd), (NT, NB) in CASES.items():
        for form in ("fused", "level"):
            dump = tmp_path / f"{n}_{bw}_{nbd}_{form}.bin"
            r = subprocess.run([EXE, str(n), str(bw), str(nbd), "2"] + (["level"] if form == "level" else []), capture_output=True, text=True, timeout=60,
                               env=dict(os.environ, BCR_TEST_DUMP=str(dump)))
            assert r.returncode == 0 and "all ok" in r.stdout, (n, bw, nbd, form, r.returncode, r.stdout, r.stderr)      # (the first failure ends the test: nothing runs behind it)
            assert f" N={NB:4d} NT={NT} " in r.stdout, r.stdout
            want = open(os.path.join(GOLDEN, f"{n}_{bw}_{nbd}_{form}.bin"), "rb").read()
            got = dump.read_bytes()
            assert len(want) == 8 * (n + nbd)
            assert got == want, f"{n} {bw} {nbd} {form}: x differs from the parent's in {int(np.sum(np.frombuffer(got, np.uint64) != np.frombuffer(want, np.uint64)))} of {n + nbd} words"


def test_floor_on_tile_column_0_and_on_the_last():
    r = subprocess.run([EXE, "floor"], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0 and "all ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    cases = [l for l in r.stdout.splitlines() if l.startswith("case ")]
    floors = [l for l in r.stdout.splitlines() if l.strip().startswith("floor ")]
    assert len(cases) == 2 and len(floors) == 2, r.stdout
    for l, form in zip(cases, ("fused", "per-level")):
        f = l.split()
        assert " N=   4 NT=4 " in l and f" {form} " in l and "status=0" in f and "repeat=identical" in f and f[-1] == "OK", l      # (OK: err <= 1e-9 |x| against the CPU without the two)
    for l in floors:
        first = int(l.split("first=")[1].split()[0]); last = int(l.split("last=")[1].split()[0])
        assert first >= 1 and first == last and l.rstrip().endswith("unknowns zero"), l
        assert first == 2, l        # (one per singular unknown: only the workgroup that holds the border row reports)


def _nchunks(NT, chrows): return (2 * NT + 1 + chrows - 1) // chrows


def _level_chrows(NT, nelim, slots):
    for c in (1, 2):
        if _nchunks(NT, c) * nelim <= slots: return c
    return 3


def mfma_formula(N, NT, nbd, slots=256):
    """BcrSolver::build's count of v_mfma_f64_16x16x4_f64 per solve, written out again: the panels (every workgroup factors its block's diagonal tiles), the
    update jobs, the backward launch's root workgroup.  No warm-up chain is in it: round 15 measured one and took it out again."""
    NO, RXT = NT * (NT - 1) // 2, 2 * NT + 1

    def panel(has_l, has_r, nelim):
        chr_, t = _level_chrows(NT, nelim, slots), 0
        for ch in range(_nchunks(NT, chr_)):
            RX = sum(1 for s in range(chr_) if chr_ * ch + s <= 2 * NT and (has_l if chr_ * ch + s < NT else (has_r if chr_ * ch + s < 2 * NT else True)))
            if not RX: continue
            for J in range(NT):
                t += 30 + (8 if J + 1 < NT else 0) + 4 * ((NT - J - 2 if J + 1 < NT else 0) + RX)
                mm = NT - 1 - J
                if mm > 0:
                    ntot = mm * (mm + 1) // 2 - 1 + RX * mm
                    t += sum(12 * ((ntot - w0 + 17) // 18) for w0 in range(min(6, ntot)))
        return t

    total, m = 0, N
    while m > 1:
        first = 0 if m & 1 else 1
        elim = [(idx >= 1, idx + 1 < m) for idx in range(first, m, 2)]
        total += sum(panel(l, r, len(elim)) for l, r in elim)
        for idx in range(1 - first, m, 2):                 # the survivors: their diagonal block's tiles and their border / rhs row
            ns = int(idx >= 1) + int(idx + 1 < m)
            total += (NT * (NT + 1) // 2 + NT) * 4 * NT * ns
        for l, r in elim:
            if l and r: total += NT * NT * 4 * NT           # the new coupling
            if nbd > 0: total += 4 * NT                     # the corner's share
            rows = sum(1 for Rg in range(RXT) if not (Rg < NT and not l) and not (NT <= Rg < 2 * NT and not r))
            total += 4 * (rows * NT + NO)                   # the pre-multiplied factor
        m = len(range(1 - first, m, 2))
    return total + panel(False, False, 1) + 4 * (NT + NO) + (4 * NT if nbd > 0 else 0)


def test_formula_is_the_launchers_on_the_benchmarks_shape():
    # (notes/r13.md: SQ_INSTS_VALU_MFMA_F64 counts 271 416 per solve of 6000 band unknowns in blocks of 64, no border, and BcrSolver::mfma_issued says so)
    assert mfma_formula(94, 4, 0) == 271416


@pytest.mark.parametrize("shape", ["nt4_n4", "nt5_n5"])
def test_library_undamped_then_damped(shape, monkeypatch):
    NT, NB = SHAPES[shape][2:4]
    p, bi, ols, A, lam, x_ora = _reference(shape, 0)
    monkeypatch.setenv("NLLS_BCR_NT_FULL", "1")
    ctx = _capi.Context(); info = ctx.upload(p.var_kind, p.var_dim, bi, p.groups(), _capi.FLAG_DETERMINISTIC)
    st = ctx.solve_stats()
    assert info.solve_mode == 2 and st["bcr_block"] == 16 * NT and st["elim_slab"] > 0 and (st["band_dof"] + 16 * NT - 1) // (16 * NT) == NB
    assert st["bcr_mfma_issued"] == mfma_formula(NB, NT, info.nborder_dof), (st["bcr_mfma_issued"], mfma_formula(NB, NT, info.nborder_dof))
    ctx.set_variables(p.variables); ctx.sweep_gradhess()
    ctx.damp(0.0); x0 = ctx.solve(want_x=True).copy(); st = ctx.solve_stats()        # undamped: the gauge directions' pivots fall below their floors
    assert st["status"] == 0 and st["dropped_pivots"] > 0 and np.all(np.isfinite(x0)), st
    assert np.array_equal(ctx.solve(want_x=True).view(np.uint64), x0.view(np.uint64))
    ctx.damp(lam); x = ctx.solve(want_x=True).copy(); st = ctx.solve_stats()
    print(f"CHAIN {shape} rel {rel(x, x_ora):.3e} status {st['status']} mfma {st['bcr_mfma_issued']}")
    assert st["status"] == 0
    assert np.array_equal(ctx.solve(want_x=True).view(np.uint64), x.view(np.uint64)), "two solves of one system differ"
    assert rel(x, x_ora) < RTOL_X, rel(x, x_ora)
    check_step(ctx, info, ols, A, lam, x, f"{shape} damped behind the undamped solve")
    ctx.close()
