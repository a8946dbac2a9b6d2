"""The accumulate and cost sweeps against an INTEGER reference, bit for bit, at every edge where their launches switch form (tests/sweep_cases.py: the cases, the
reference, the tile loop restated; DESIGN.md 4.1 lists the edges; notes/r22.md the run).

The problems live on a dyadic grid where every product and every sum of the sweep is exact in float64, so A.data, b and the cost do not depend on the order of the
atomics, the accumulator copies or the reduction trees: the device must give the reference's bits -- no tolerance, and one dropped, doubled or misplaced contribution
shows.  Every case: upload; info.is_sparse and the six tile counters against the restatement; sweep_gradhess() at `variables`, again at `variables` (a missing zero fill
in front of atomics doubles the entries) and at `variables2` (an image entry a TILE_NOZERO tile never writes keeps its old value); after each, get_bsm_data(), get_grad(),
the returned cost and sweep_cost() equal the reference in their uint64 view (a negative zero shows)."""
import time

import numpy as np
import pytest

from nllssolver_jl_amd import _capi
from tests import sweep_cases as S

pytestmark = pytest.mark.gpu
DEVICE_ERROR = []                # a case that met a device error: the cases behind it start nothing on the device


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def explain(case, tiles, what, got, ref):
    """the first differing entries of A.data (with block row, column and the tiles that write the row) or of b"""
    bad = np.nonzero(bits(got) != bits(ref))[0]; lines = [f"{what}: {bad.size} of {ref.size} entries differ"]
    for i in bad[:8]:
        where = S.owner_of_entry(tiles, int(i)) if what == "A.data" else ""
        lines.append(f"  [{i}] device {got[i]!r} reference {ref[i]!r} (device - reference = {got[i] - ref[i]!r}) {where}")
    return "\n".join(lines)


@pytest.mark.parametrize("name", list(S.CASES))
def test_sweep_exact(name, monkeypatch):
    assert not DEVICE_ERROR, f"not run: {DEVICE_ERROR[0]} met a device error"
    t0 = time.perf_counter()
    case = S.CASES[name](); sp = case.sp
    tiles = case.assert_edge()                                            # the edge the case exists for, before anything is uploaded
    refs = [case.reference(0), case.reference(0), case.reference(1)]
    for k in ("NLLS_SWEEP_FOLD", "NLLS_HEAVY_MAX_ENTRIES", "NLLS_TINY_DENSE", "NLLS_COST_GRID_MAX"): monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items(): monkeypatch.setenv(k, v)
    t1 = time.perf_counter()
    ctx = _capi.Context()
    try:
        info = ctx.upload(sp.var_kind, sp.var_dim, sp.bi, sp.groups, case.flags)
        assert bool(info.is_sparse) == tiles["sparse"] and info.ndof == tiles["st"]["ndof"]
        if info.is_sparse:
            for g, o in zip(ctx.bsm_index(), tiles["st"]["ols"].bsm_index()): assert np.array_equal(g, o)
        for which, (A, b, cost) in zip((sp.variables, sp.variables, sp.variables2), refs):
            ctx.set_variables(which)
            c_gh = ctx.sweep_gradhess()
            st = ctx.solve_stats(); got = {k: st[k] for k in S.COUNTERS}
            assert got == tiles["counters"], (got, tiles["counters"])
            A_gpu, b_gpu = ctx.get_bsm_data(), ctx.get_grad()
            assert A_gpu.shape == A.shape and np.array_equal(bits(A_gpu), bits(A)), explain(case, tiles, "A.data", A_gpu, A)
            assert np.array_equal(bits(b_gpu), bits(b)), explain(case, tiles, "b", b_gpu, b)
            c_sw = ctx.sweep_cost()
            assert bits(c_gh)[0] == bits(cost)[0] and bits(c_sw)[0] == bits(cost)[0], (c_gh, c_sw, cost)
        if not info.is_sparse:
            n = info.ndof; M = A_gpu.reshape(n, n)
            assert np.array_equal(bits(M), bits(M.T)), "the mirrored dense matrix is not symmetric in bits"
    except _capi.NllsError:
        DEVICE_ERROR.append(name); raise
    finally:
        ctx.close()
    t2 = time.perf_counter()
    print(f"SWEEP {name}: sparse={int(tiles['sparse'])} ndof={tiles['st']['ndof']} costs={sum(len(g['varind']) for g in sp.groups)} "
          + " ".join(f"{k[6:]}={v}" for k, v in tiles["counters"].items()) + f" cost_list={[G['cost_list'] for G in tiles['groups']]} host {t1 - t0:.2f} s device {t2 - t1:.2f} s")
