"""NLLS_PCG_PRECOND_SCHUR_JACOBI and nlls_schur_block_diag: the diagonal blocks of S(lambda) = B + lambda I - E (C + lambda I)^-1 E' themselves, returned and used as the
preconditioner of nlls_solve_pcg_schur (include/nlls_amd.h).

The host reference is tests/test_gpu_schur.py's: Reduced on the device's own swept A, b and the mask of schur_info; block i of the device is held against the matching
diagonal block of Reduced.S.  Every case first asserts on the host the condition it rests on, so that a bad input blames the input.

Tolerances:
  a block against the host's: Reduced.tol = 1e-11 * max(1, kappa) of the block's largest entry -- the bound the Schur products are held to, and every block carries one
         solve with C_e + lam I;
  x against damp(lambda); solve(): 1e-7 of the step's largest entry; the true residual at rtol 1e-8: 2e-8 ||b|| (both of tests/test_gpu_schur.py);
  a truncated iterate against the mirror's, expanded: 1e-11 of the largest entry;
  iteration counts: within 1 of the host mirror on the device's own operator and the device's own blocks.
"Schur-Jacobi takes no more iterations than block Jacobi" is asserted only where the float64 host mirror on Reduced.S shows it first, and at least one of the three
eliminating problems must show it (all three do: 6 / 6, 8 / 7 and 10 / 9 iterations under block Jacobi / Schur-Jacobi at rtol 1e-10 -- at the damping of pd_lambda, 1e-2
of the largest diagonal entry, both preconditioners leave little to do; no other seed was needed).
The bit rules are exact: two calls, calls that differ in the round length."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import synthetic, _capi
from tests.helpers import blockindices, expected_elimination
from tests.test_gpu_linearize import affine_two_groups, upload, rel
from tests.test_gpu_apply import PROBLEMS, HUBS, block_sizes, hub_problem, incidences
from tests.test_gpu_pcg import pcg_mirror, pd_lambda, swept
from tests.test_gpu_schur import ELIMINATING, Reduced, block_min_eigs, refused_not_spd, system_state

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, JACOBI, SJACOBI = _capi.PCG_PRECOND_NONE, _capi.PCG_PRECOND_BLOCK_JACOBI, _capi.PCG_PRECOND_SCHUR_JACOBI
FLAGS = pytest.mark.parametrize("flags", [0, _capi.FLAG_MATERIALIZE], ids=["default", "materialize"])


def pair_index(p, unfixed, is_elim):
    """from the incidence lists alone: {(reduced block, eliminated block): [(group, cost block, r slot, e slot), ..]}, the number of cost blocks that join a FIXED
    variable with an eliminated one, and the number with at least two reduced slots beside an eliminated one"""
    bi = blockindices(p, unfixed).astype(np.int64); pairs = {}; fixed_e = two_r = 0
    for gi, g in enumerate(p.costs.values()):
        for ci, row in enumerate(np.asarray(g.arrays()[0], np.int64)):
            blk = bi[row - 1]
            es = [s for s, b in enumerate(blk) if b and is_elim[b - 1]]; rs = [s for s, b in enumerate(blk) if b and not is_elim[b - 1]]
            assert len(es) <= 1, "two eliminated variables in one cost block: the eliminated set is not independent: the input is at fault"
            if es:
                fixed_e += bool(np.any(blk == 0)); two_r += len(rs) >= 2
                for s in rs:
                    pairs.setdefault((int(blk[s]) - 1, int(blk[es[0]]) - 1), []).append((gi, ci, s, es[0]))
    return pairs, fixed_e, two_r


def host_blocks_of_S(ref):
    return [ref.S[o:o + d, o:o + d] for o, d in zip(ref.rbo, ref.rbs)]


def check_blocks(ctx, ref, lam, tag, which=_capi.VARS_CURRENT):
    """every block of schur_block_diag against the matching diagonal block of Reduced.S; -> the blocks"""
    D = ctx.schur_block_diag(lam, which); want = host_blocks_of_S(ref); errs = []
    assert len(D) == len(want), tag
    for d, w in zip(D, want):
        assert d.shape == w.shape, tag
        errs.append(np.max(np.abs(d - w)) / np.max(np.abs(w)))
    print(f"SCHURJACOBI {tag} lambda {lam:.3e}: {len(D)} blocks, kappa {ref.kappa:.3e}, worst block {max(errs):.3e} (of {ref.tol:.3e})")
    assert max(errs) <= ref.tol, (tag, max(errs))
    return D


def same_bytes(a, b):
    return len(a) == len(b) and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- 1. the blocks against the host -----------------------------------------------------------------------------------------------------------------------
@FLAGS
@pytest.mark.parametrize("name", ELIMINATING)
def test_blocks_against_the_host(name, flags):
    p, unfixed = PROBLEMS[name]()
    ctx, A, b, bo, bs = swept(p, unfixed, flags); bo, bs = block_sizes(ctx)
    nred, nelim, is_elim, index = ctx.schur_info()
    assert nelim > 0, f"{name}: the upload eliminated nothing: the input is at fault"
    pairs, fixed_e, two_r = pair_index(p, unfixed, is_elim)
    # the hazard every problem is here for: where summing E behind the product, or a wrong transpose flag, shows
    if name == "affine two groups":
        assert any(len({g for g, _, _, _ in t}) == 2 for t in pairs.values()) and fixed_e > 0, "no pair joined by both groups, or no fixed camera beside a point: the input is at fault"
    elif name == "so3 adaptive":
        assert bs[0] == 3 and not is_elim[0] and any(r == 0 and len(t) > 1 and len({g for g, _, _, _ in t}) == 1 for (r, e), t in pairs.items()) and two_r > 0, \
            "the kernel should meet a point through several blocks of one group, in blocks of two reduced slots: the input is at fault"
    else:
        assert np.unique(bs[~is_elim]).size > 1 and not set(bs[~is_elim]) <= set(bs[is_elim]), "the reduced blocks should be of unequal sizes, other than the eliminated one: the input is at fault"
    lam0 = pd_lambda(A)
    for lam in (lam0, 10 * lam0):
        ref = Reduced(ctx, A, lam, bo, bs); D = check_blocks(ctx, ref, lam, f"{name} flags {flags}")
        assert same_bytes(D, ctx.schur_block_diag(lam)), "two identical calls differ"
    ctx.close()


def test_transposed_terms_are_exercised():
    """a reduced slot BEHIND its eliminated slot (the stored block is E_ie') and one in front of it: the problems whose blocks this file holds against the host -- the three
    that eliminate, the hub shapes -- must show both orders between them, or a flag is never taken"""
    seen = {}
    for name, (p, unfixed) in [(n, PROBLEMS[n]()) for n in ELIMINATING] + [(f"hub degree {d}", (hub_problem(n, k)[0], None)) for n, k, d, _ in HUBS]:
        ctx = upload(p, unfixed); is_elim = ctx.schur_info()[2]; ctx.close()
        seen[name] = {bool(s < e) for t in pair_index(p, unfixed, is_elim)[0].values() for _, _, s, e in t}
    print(f"SCHURJACOBI slot orders (True: the reduced slot first): {seen}")
    assert set().union(*seen.values()) == {True, False}, "no problem of this file stores a transposed block: the input is at fault"


# ---- 2. a block without eliminated neighbours ---------------------------------------------------------------------------------------------------------------
def test_a_block_without_eliminated_neighbours():
    """affine two groups with one more variable of two unknowns and a cost of its own: not of the eliminated size, no neighbour at all -- no lane is launched for its row,
    and its block holds the bytes nlls_hess_block_diag returns"""
    p, unfixed = affine_two_groups()
    first = p.addvariables(np.array([[0.3, 1.7]])); unfixed = np.append(unfixed, True)
    p.addcosts(K.RES_ROSENBROCK_2D, np.array([[first]]), np.array([[1.0, 10.0]]), N.GemanMcclureKernel(2.0))
    ctx, A, b, bo, bs = swept(p, unfixed); bo, bs = block_sizes(ctx)
    nred, nelim, is_elim, index = ctx.schur_info(); pairs, _, _ = pair_index(p, unfixed, is_elim)
    lone = int(blockindices(p, unfixed)[first - 1]) - 1
    assert nelim > 0 and not is_elim[lone] and bs[lone] == 2 and not any(r == lone for r, _ in pairs), "the added block should be reduced and meet no eliminated block: the input is at fault"
    lam = pd_lambda(A); ref = Reduced(ctx, A, lam, bo, bs)
    D = check_blocks(ctx, ref, lam, "a lone reduced block"); H = ctx.hess_block_diag(lam)
    i = int(np.sum(~is_elim[:lone]))
    assert D[i].tobytes() == H[lone].tobytes(), "a reduced block with nothing to subtract differs from nlls_hess_block_diag's"
    assert sum(D[j].tobytes() != H[r].tobytes() for j, r in enumerate(np.flatnonzero(~is_elim))) == len({r for r, _ in pairs}), "exactly the rows with pairs should change"
    ctx.close()


# ---- 3. row classes -----------------------------------------------------------------------------------------------------------------------------------------
def test_hub_shapes():
    """the hub's row (63, 64, 65, 197, 66 incidences) is a reduced row on either side of the wavefront threshold, its pairs the eliminated ends of its edges"""
    done = []
    for n, pendants, degree, nedges in HUBS:
        p, hub = hub_problem(n, pendants); inc = incidences(p, None)
        assert inc[hub] == degree and inc.max() == degree
        ctx, A, b, bo, bs = swept(p); bo, bs = block_sizes(ctx); nred, nelim, is_elim, index = ctx.schur_info()
        assert np.array_equal(is_elim, expected_elimination(ctx))
        if nelim == 0:
            out = np.full(max(nred, 1), 7.25)
            assert ctx.L.nlls_schur_block_diag(ctx.h, 0, 0.1, _capi._p(out)) == _capi.ERR_UNSUPPORTED and np.all(out == 7.25); ctx.close(); continue
        pairs, _, _ = pair_index(p, None, is_elim)
        assert not is_elim[hub] and sum(r == hub for r, _ in pairs) > 0, "the hub should be a reduced row with eliminated neighbours: the input is at fault"
        lam = pd_lambda(A); ref = Reduced(ctx, A, lam, bo, bs)
        D = check_blocks(ctx, ref, lam, f"hub degree {degree}")
        assert same_bytes(D, ctx.schur_block_diag(lam)), degree
        done.append(degree); ctx.close()
    assert len(done) >= 2 and any(d < 64 for d in done) and any(d >= 64 for d in done), f"hub shapes that eliminate: {done}: the input is at fault"


def test_wave_min_moves_reduced_rows():
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed); bo, bs = block_sizes(ctx); inc = incidences(p, unfixed)
    lam = pd_lambda(A); ref = Reduced(ctx, A, lam, bo, bs); rinc = inc[~ref.is_elim]
    assert rinc.max() >= 64 > rinc.min(), "by default the reduced rows should fall on both sides of the threshold: the input is at fault"
    base = check_blocks(ctx, ref, lam, "wave_min 64")
    assert same_bytes(base, ctx.schur_block_diag(lam))
    for w in (1, int(np.unique(rinc)[1]), int(rinc.max()) + 1):          # every reduced row a wavefront; all but the shortest; none
        assert (np.sum(rinc >= w) > 0) == (w <= rinc.max()) and np.sum(rinc >= w) != np.sum(rinc >= 64), "the setting should move reduced rows: the input is at fault"
        ctx.set_option(_capi.OPT_APPLY_WAVE_MIN, w)
        got = check_blocks(ctx, ref, lam, f"wave_min {w}")
        assert same_bytes(got, ctx.schur_block_diag(lam)), w
    ctx.set_option(_capi.OPT_APPLY_WAVE_MIN, 64)
    assert same_bytes(base, ctx.schur_block_diag(lam)), "back at the default the bytes of the default should return"
    ctx.close()


def test_a_cut_reduced_row():
    """the adaptive kernel's variable lies in every block of its group: 4320 incidences in 600 pairs, two segments that end at pair boundaries"""
    p = synthetic.create_so3_ba_problem(8, 600, 0.9, seed=6, adaptive=True); inc = incidences(p, None)
    ctx, A, b, bo, bs = swept(p); bo, bs = block_sizes(ctx); nred, nelim, is_elim, index = ctx.schur_info()
    pairs, _, two_r = pair_index(p, None, is_elim)
    assert inc[0] > 4096 and inc[0] == inc.max() and nelim == 600 and not is_elim[0] and bs[0] == 3, "the kernel's row should be a cut reduced row: the input is at fault"
    assert sum(r == 0 for r, _ in pairs) == 600 and sum(len(t) for (r, _), t in pairs.items() if r == 0) == inc[0] and two_r == inc[0], "the kernel should meet every point: the input is at fault"
    lam = pd_lambda(A); ref = Reduced(ctx, A, lam, bo, bs)
    D = check_blocks(ctx, ref, lam, "cut reduced row")
    assert same_bytes(D, ctx.schur_block_diag(lam))
    ctx.close()


# ---- 4. the solve -------------------------------------------------------------------------------------------------------------------------------------------
def solve_case(name, p, unfixed):
    """-> (device counts (none, block Jacobi, Schur-Jacobi), host counts on Reduced.S)"""
    ctx, A, b, bo, bs = swept(p, unfixed); bo, bs = block_sizes(ctx); ndof = ctx.info.ndof; cap = 4 * ndof
    lam = pd_lambda(A); ref = Reduced(ctx, A, lam, bo, bs); s = ref.reduce(b)
    host = [pcg_mirror(lambda v: ref.S @ v, blocks, ref.rbo, s, cap, 1e-10)[1:3] for blocks in (None, ref.rblocks(), host_blocks_of_S(ref))]
    assert all(status == 0 for _, status in host), f"{name}: the host mirrors on S: {host}: the input is at fault"
    sblocks = ctx.schur_block_diag(lam)
    _, kd, sd, _ = pcg_mirror(lambda v: ctx.schur_apply(v, lam), sblocks, ref.rbo, ctx.schur_reduce(b, lam), cap, 1e-10)
    assert sd == 0, f"{name}: the mirror on the device's operator and blocks ended with status {sd}: the input is at fault"
    ctx.damp(lam); xs = ctx.solve(want_x=True)
    _, full = ctx.solve_pcg(JACOBI, None, 1e-10); stats_full = ctx.solve_stats()
    counts = [ctx.solve_pcg_schur(pc, None, 1e-10)[1] for pc in (NONE, JACOBI)]
    x, st = ctx.solve_pcg_schur(SJACOBI, None, 1e-10, want_x=True); counts.append(st)
    assert st["status"] == 0 and st["iterations"] >= 1 and x.tobytes() == ctx.get_step().tobytes()
    assert ctx.solve_pcg_schur("schurjacobi", None, 1e-10, want_x=True)[0].tobytes() == x.tobytes()
    err = np.max(np.abs(x - xs)) / np.max(np.abs(xs))
    x8, st8 = ctx.solve_pcg_schur(SJACOBI, None, 1e-8, want_x=True)
    res = np.linalg.norm(ref.M @ (-x8) - b) / np.linalg.norm(b)
    dev = tuple(c["iterations"] for c in counts); hst = tuple(k for k, _ in host)
    print(f"SCHURJACOBI PCG {name}: ndof {ndof} nred {ref.nred} lambda {lam:.3e} iterations none / block Jacobi / Schur-Jacobi: device {dev} host on S {hst}; mirror on the device's "
          f"blocks {kd}; against nlls_solve {err:.3e} (of 1e-7); true residual at rtol 1e-8 {res:.3e} (of 2e-8); launches {tuple(c['launches'] for c in counts)}")
    assert err <= 1e-7 and st8["status"] == 0 and res <= 2e-8, name
    assert abs(st["iterations"] - kd) <= 1, (name, st, kd)
    assert abs(st["bnorm"] - np.linalg.norm(s)) <= 1e-9 * max(1.0, ref.kappa) * np.linalg.norm(s) and st["rnorm"] <= 1e-10 * st["bnorm"]
    assert st["launches"] > 0 and st["rounds"] == st["iterations"] + 1
    after = ctx.solve_stats()                                              # the counters keep describing the last nlls_solve_pcg
    assert all(after[k] == stats_full[k] for k in ("pcg_iterations", "pcg_status", "pcg_rounds")) and after["pcg_iterations"] == full["iterations"]
    ctx.close()
    return dev, hst


def test_solve_against_the_direct_solve():
    shown = []
    for name in ELIMINATING:
        dev, hst = solve_case(name, *PROBLEMS[name]())
        if hst[2] <= hst[1]:                # the host shows it first
            shown.append(name); assert dev[2] <= dev[1], (name, dev, hst)
    print(f"SCHURJACOBI PCG: the host mirror shows Schur-Jacobi ahead of block Jacobi on {shown}")
    assert shown, "on none of the three does the host mirror show Schur-Jacobi ahead of block Jacobi: the input is at fault"


# ---- 5. truncation and rounds -------------------------------------------------------------------------------------------------------------------------------
def test_truncation_and_rounds():
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed); bo, bs = block_sizes(ctx)
    lam = 1e-2 * np.max(np.abs(np.diag(A))); ref = Reduced(ctx, A, lam, bo, bs); s = ref.reduce(b)
    _, k, status, _ = pcg_mirror(lambda v: ref.S @ v, host_blocks_of_S(ref), ref.rbo, s, 4 * b.size, 1e-10)
    assert status == 0 and k > 4, f"the host mirror on S: {k} iterations, status {status}: the input is at fault"
    sblocks = ctx.schur_block_diag(lam)
    _, _, _, its = pcg_mirror(lambda v: ctx.schur_apply(v, lam), sblocks, ref.rbo, ctx.schur_reduce(b, lam), 3, 1e-10)
    assert len(its) == 3
    ctx.damp(lam)
    for m in (1, 2, 3):
        x, st = ctx.solve_pcg_schur(SJACOBI, m, 1e-10, want_x=True)
        assert (st["status"], st["iterations"]) == (1, m) and x.tobytes() == ctx.get_step().tobytes()
        e = rel(-x, ctx.schur_expand(b, its[m - 1], lam))
        print(f"SCHURJACOBI PCG truncated at {m}: against the mirror's iterate, expanded {e:.3e} (of 1e-11)")
        assert e <= 1e-11
    x0, s0 = ctx.solve_pcg_schur(SJACOBI, None, 1e-10, want_x=True); x1, s1 = ctx.solve_pcg_schur(SJACOBI, None, 1e-10, want_x=True)
    assert s0["status"] == 0 and x0.tobytes() == x1.tobytes() and s0 == s1, "two calls on the same sweep differ"
    kd = s0["iterations"]; assert abs(kd - k) <= 1
    _, sb = ctx.solve_pcg_schur(JACOBI, None, 1e-10)
    for rnd in (1, 3, 1000):
        ctx.set_option(_capi.OPT_PCG_ROUND, rnd)
        x, st = ctx.solve_pcg_schur(SJACOBI, None, 1e-10, want_x=True)
        print(f"SCHURJACOBI PCG round {rnd}: iterations {st['iterations']} synchronisations {st['rounds']} launches {st['launches']} (block Jacobi: {sb['iterations']} iterations, {sb['launches']} launches)")
        assert x.tobytes() == x0.tobytes() and st["iterations"] == kd and st["status"] == 0, rnd
        assert st["rounds"] == -(-kd // rnd) + 1, (rnd, st)
    ctx.close()


def test_set_up_launches_are_counted():
    """with maxiters 1 the two calls differ in their set-up alone: Schur-Jacobi adds one off-diagonal record launch per group and its subtraction launches"""
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed); ctx.damp(pd_lambda(A))
    _, sb = ctx.solve_pcg_schur(JACOBI, 1, 1e-10); _, ss = ctx.solve_pcg_schur(SJACOBI, 1, 1e-10)
    inc = incidences(p, unfixed)[~ctx.schur_info()[2]]
    extra = len(p.costs) + int(np.any(inc < 64)) + int(np.any(inc >= 64))
    print(f"SCHURJACOBI set-up: launches block Jacobi {sb['launches']}, Schur-Jacobi {ss['launches']} (expected {extra} more)")
    assert ss["launches"] - sb["launches"] == extra and ss["rounds"] == sb["rounds"]
    ctx.close()


# ---- 6. breakdown -------------------------------------------------------------------------------------------------------------------------------------------
def test_breakdowns():
    p, unfixed = PROBLEMS["so3 adaptive"]()
    ctx, A, b, bo, bs = swept(p, unfixed, _capi.FLAG_MATERIALIZE); bo, bs = block_sizes(ctx); ndof = b.size
    nred, nelim, is_elim, index = ctx.schur_info(); mins = block_min_eigs(A, bo, bs)
    me, mr = mins[is_elim].min(), mins[~is_elim].min()
    assert nelim > 0 and me > 0 and mr < 0.25 * me, f"smallest eigenvalues: eliminated blocks {me:.3e}, reduced blocks {mr:.3e}: the input is at fault"
    lam = -0.5 * me; ref = Reduced(ctx, A, lam, bo, bs)
    with pytest.raises(np.linalg.LinAlgError):          # some S_ii has no factor at this lambda, while every C_e + lambda I keeps its own
        for blk in host_blocks_of_S(ref):
            np.linalg.cholesky(blk)
    ctx.damp(lam)
    assert refused_not_spd(ctx, SJACOBI, 3) == 0
    assert "Schur-Jacobi" in ctx.L.nlls_last_error(ctx.h).decode()
    check_blocks(ctx, ref, lam, "indefinite blocks")                       # returned as they are
    lam2 = -2.0 * me; ctx.damp(lam2 - lam)
    with pytest.raises(np.linalg.LinAlgError):
        for o, d, e in zip(bo, bs, is_elim):
            if e:
                np.linalg.cholesky(A[o:o + d, o:o + d] + lam2 * np.eye(d))
    assert refused_not_spd(ctx, SJACOBI, 3) == 0
    out = np.full(int(np.sum(bs[~is_elim] ** 2)), 7.25)
    assert ctx.L.nlls_schur_block_diag(ctx.h, 0, lam2, _capi._p(out)) == _capi.ERR_NOT_SPD and np.all(out == 7.25), "a call without a factor wrote to its output"
    ctx.close()


# ---- 7. edges and refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_every_unfixed_block_eliminated():
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3), 1e-3, 1e-3)
    unfixed = np.ones(p.nvariables, bool); unfixed[:10] = False
    ctx, A, b, bo, bs = swept(p, unfixed, _capi.FLAG_MATERIALIZE)
    nred, nelim, is_elim, index = ctx.schur_info()
    assert (nred, nelim) == (0, 200) and is_elim.all(), "every point should be eliminated: the input is at fault"
    out = np.full(16, 7.25)
    assert ctx.L.nlls_schur_block_diag(ctx.h, 0, 0.1, _capi._p(out)) == _capi.OK and np.all(out == 7.25) and ctx.schur_block_diag(0.1) == []
    ctx.damp(pd_lambda(A))
    x, st = ctx.solve_pcg_schur(SJACOBI, None, 1e-10, want_x=True); xj, _ = ctx.solve_pcg_schur(JACOBI, None, 1e-10, want_x=True)
    assert (st["status"], st["iterations"]) == (0, 0) and x.tobytes() == ctx.get_step().tobytes() == xj.tobytes()
    ctx.close()


def test_refusals():
    L = _capi.lib(); ctx = _capi.Context(); P = _capi._p
    out = np.full(4096, 7.25); st = np.full(40, 7.25); v = np.ones(4096)
    assert L.nlls_schur_block_diag(ctx.h, 0, 0.0, P(out)) == _capi.ERR_NOT_READY                                       # no upload yet
    p, unfixed = affine_two_groups(); ctx.close(); ctx = upload(p, unfixed)
    assert L.nlls_schur_block_diag(ctx.h, 0, 0.0, None) == _capi.ERR_INVALID_ARG                                      # a null pointer
    for which, lam in ((-1, 0.0), (3, 0.0), (0, np.nan), (0, np.inf), (0, -np.inf)):
        assert L.nlls_schur_block_diag(ctx.h, which, lam, P(out)) == _capi.ERR_INVALID_ARG, (which, lam)
    assert np.all(out == 7.25), "a refused call wrote to its output"
    assert len(ctx.schur_block_diag(0.5)) == int(np.sum(~ctx.schur_info()[2]))                                        # an upload and no sweep
    ctx.sweep_gradhess(); ndof = ctx.info.ndof; sel = np.array([3], np.int64)
    refusals = (("nlls_solve_pcg", lambda: L.nlls_solve_pcg(ctx.h, SJACOBI, 10, 1e-8, P(out), P(st))),
                ("nlls_solve_pcg_rhs", lambda: L.nlls_solve_pcg_rhs(ctx.h, 0, 0.1, SJACOBI, 10, 1e-8, 1, P(v), P(out), P(st))),
                ("nlls_marginal_cov", lambda: L.nlls_marginal_cov(ctx.h, 0, 0.1, 1, P(sel), SJACOBI, 10, 1e-8, P(out), P(st))),
                ("nlls_solve_pcg_tr", lambda: L.nlls_solve_pcg_tr(ctx.h, SJACOBI, 10, 1e-8, 1.0, P(out), P(st))))
    for name, call in refusals:
        assert call() == _capi.ERR_INVALID_ARG, name
        text = L.nlls_last_error(ctx.h).decode(); assert name in text and "reduced system" in text, text
    assert np.all(out == 7.25) and np.all(st == 7.25), "a refused call wrote to an output"
    assert L.nlls_solve_pcg_schur(ctx.h, 2, 10, 1e-8, P(out), P(st)) == _capi.ERR_INVALID_ARG                           # 2 stays unassigned
    ctx.damp(1e-2 * ctx.max_abs_diag())
    assert L.nlls_solve_pcg_schur(ctx.h, SJACOBI, 1000, 1e-10, None, None) == _capi.OK                                 # both outputs may be NULL
    ctx.close()
    ctx = upload(p, unfixed, _capi.FLAG_NO_SCHUR); ctx.sweep_gradhess()                                                # nothing eliminated
    assert L.nlls_schur_block_diag(ctx.h, 0, 0.1, P(out)) == _capi.ERR_UNSUPPORTED and "eliminated nothing" in L.nlls_last_error(ctx.h).decode()
    assert L.nlls_solve_pcg_schur(ctx.h, SJACOBI, 10, 1e-8, P(out), P(st)) == _capi.ERR_UNSUPPORTED
    assert np.all(out == 7.25) and np.all(st == 7.25)
    ctx.close()


def test_sharded_contexts_are_refused():
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3), 1e-3, 1e-3)
    c = _capi.Context(); P = _capi._p
    try:
        c.set_shard(0, 2); c.upload(p.var_kind, p.var_dim, blockindices(p), p.groups(), _capi.FLAG_FORCE_SPARSE); c.set_variables(p.variables)
        assert c.shard_info()["nranks"] == 2 and c.shard_info()["replicated"] == 0
        c.sweep_gradhess_local(); out = np.full(c.info.ndof * 6, 7.25)
        assert c.L.nlls_schur_block_diag(c.h, 0, 0.0, P(out)) == _capi.ERR_UNSUPPORTED
        assert c.L.nlls_solve_pcg_schur(c.h, SJACOBI, 10, 1e-8, P(out), None) == _capi.ERR_UNSUPPORTED and np.all(out == 7.25)
    finally:
        c.close()


# ---- 8. read only -------------------------------------------------------------------------------------------------------------------------------------------
def test_the_call_leaves_everything_untouched():
    p, unfixed = affine_two_groups()
    ctx = upload(p, unfixed, _capi.FLAG_MATERIALIZE); ctx.copy_variables(_capi.VARS_NEXT, _capi.VARS_CURRENT); ctx.copy_variables(_capi.VARS_BEST, _capi.VARS_CURRENT)
    ctx.sweep_gradhess(); ctx.damp(1e-2 * ctx.max_abs_diag()); ctx.solve(); ctx.solve_pcg(JACOBI, None, 1e-8); step = ctx.get_step().tobytes()
    ctx.hess_apply(np.ones(ctx.info.ndof), 0.2)                            # (a product's statistics to keep)
    before = system_state(ctx); st0 = ctx.solve_stats()
    for which, lam in ((_capi.VARS_CURRENT, 0.3), (_capi.VARS_NEXT, 0.1), (_capi.VARS_BEST, 0.2)):
        ctx.schur_block_diag(lam, which)
    st1 = ctx.solve_stats()
    assert system_state(ctx) == before and ctx.get_step().tobytes() == step
    assert st0 == st1, {k: (st0[k], st1[k]) for k in st0 if st0[k] != st1[k]}
    ctx.close()


# ---- 9. the iterator ----------------------------------------------------------------------------------------------------------------------------------------
def test_optimize_with_schur_jacobi_steps():
    make = lambda: synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3), 1e-3, 1e-3)      # (the problem of tests/test_gpu_schur.py::test_optimize_with_reduced_pcg_steps)
    with N.Solver(make()) as s:
        res = s.optimize(N.NLLSOptions(maxiters=50, linearsolver=N.PCG(rtol=1e-6, schur=True, precond="schurjacobi"))); last = s.ls.ctx.last_pcg_schur
        print(f"SCHURJACOBI optimize: cost {res.startcost:.3e} -> {res.bestcost:.3e} in {res.niterations} iterations, {res.linearsolvers} linear solves, last of {last['iterations']} iterations")
        assert res.bestcost <= 1e-15 * res.startcost and res.linearsolvers > 0 and last["iterations"] > 0 and s.ls.ctx.solve_stats()["pcg_iterations"] == 0
        op = s.schur_operator(0.5); blocks = op.schur_diag_blocks(); plain = op.diag_blocks()
        assert len(blocks) == len(plain) and all(a.shape == c.shape for a, c in zip(blocks, plain)) and same_bytes(blocks, s.ls.schur_block_diag(0.5))
        Sd = np.array([op.matvec(e) for e in np.eye(op.shape[0])]).T; o = 0; worst = 0.0
        for blk in blocks:
            d = blk.shape[0]; worst = max(worst, np.max(np.abs(blk - Sd[o:o + d, o:o + d])) / np.max(np.abs(blk))); o += d
        print(f"SCHURJACOBI operator: schur_diag_blocks against the operator's own columns {worst:.3e} (of 1e-9)")
        assert worst <= 1e-9                                               # (two device paths to the same numbers; the bound of a trial behind the calls)
    with pytest.raises(ValueError):
        N.optimize(make(), N.NLLSOptions(maxiters=3, iterator=N.steihaug, linearsolver=N.PCG(schur=True, precond="schurjacobi")))


# ---- 10. a user kind ----------------------------------------------------------------------------------------------------------------------------------------
def test_user_kind_in_a_process_of_its_own():
    userlib = os.path.join(ROOT, "nllssolver.jl_amd", "csrc", "libnlls_amd_userdemo.so")
    env = dict(os.environ, NLLS_AMD_LIB=userlib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "schurjacobi_userkind_worker.py")], capture_output=True, text=True, env=env, timeout=600)
    print(out.stdout[-1500:])
    assert out.returncode == 0 and "user kind schurjacobi ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
