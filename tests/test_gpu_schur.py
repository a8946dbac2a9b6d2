"""nlls_schur_apply / nlls_schur_reduce / nlls_schur_expand / nlls_solve_pcg_schur: the reduced system of the upload's eliminated set, applied and never formed
(include/nlls_amd.h).

The host reference is the device's own swept A, b (device_system) and the mask of schur_info, with M = A + lam I split over (r, e):
    S = M_rr - M_re inv(M_ee) M_er,   reduce(b) = b_r - M_re inv(M_ee) b_e,   expand(b, yr) = [yr ; inv(M_ee) (b_e - M_er yr)]
Every case first asserts on the host the condition it rests on -- the eliminated set is independent (M_ee block diagonal), the mirror converges or breaks down -- so
that a bad input blames the input.

Tolerances:
  the products against the reference: 1e-11 * max(1, kappa) of the largest entry of the reference -- 1e-11 is RTOL of tests/test_gpu_apply.py (the same products summed
         in different orders), and every product carries one solve with C_e + lam I: kappa is the largest np.linalg.cond of an eliminated block on the host;
  x against damp(lambda); solve(): 1e-7 of the largest entry of the step, the bound of tests/test_gpu_pcg.py; the true residual at rtol 1e-8: 2e-8 ||b||;
  a truncated iterate against the mirror's, expanded: 1e-11 of the largest entry; the trial behind the calls: 1e-9 (tests/test_gpu_apply.py).
The bit rules are exact: two calls, vector k of eight against the call on it alone, a chunked call against the unchunked one, calls that differ in the round length."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import synthetic, _capi
from tests.helpers import expected_elimination
from tests.test_gpu_blockeval import chain_problem
from tests.test_gpu_linearize import affine_two_groups, device_system, upload, rel
from tests.test_gpu_apply import PROBLEMS, HUBS, block_sizes, hub_problem, incidences, dense_curve_rosenbrock
from tests.test_gpu_pcg import pcg_mirror, pd_lambda, swept

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-11
NONE, JACOBI = _capi.PCG_PRECOND_NONE, _capi.PCG_PRECOND_BLOCK_JACOBI
ELIMINATING = ("affine two groups", "so3 adaptive", "mixed linear3 + cost3")      # the problems of PROBLEMS whose upload eliminates (asserted in test_products_against_the_sweep)
FLAGS = pytest.mark.parametrize("flags", [0, _capi.FLAG_MATERIALIZE], ids=["default", "materialize"])


class Reduced:
    """the host reference of one swept context at one lambda"""

    def __init__(self, ctx, A, lam, bo, bs):
        self.nred, self.nelim, self.is_elim, self.index = ctx.schur_info()
        self.e = np.repeat(self.is_elim, bs); self.r = ~self.e; ndof = A.shape[0]
        assert np.array_equal(np.flatnonzero(self.r), self.index) and self.nred == int(self.r.sum()) and self.nelim == int(self.is_elim.sum())
        M = A + lam * np.eye(ndof); self.M = M
        self.C = M[np.ix_(self.e, self.e)]; self.E = M[np.ix_(self.r, self.e)]; self.B = M[np.ix_(self.r, self.r)]
        blockdiag = np.zeros_like(self.C); eb = bs[self.is_elim]; eo = np.concatenate(([0], np.cumsum(eb)))
        for k in range(eb.size):
            blockdiag[eo[k]:eo[k + 1], eo[k]:eo[k + 1]] = self.C[eo[k]:eo[k + 1], eo[k]:eo[k + 1]]
        assert np.array_equal(blockdiag, self.C), "the eliminated set is not independent: the input is at fault"
        self.kappa = max([np.linalg.cond(self.C[eo[k]:eo[k + 1], eo[k]:eo[k + 1]]) for k in range(eb.size)] + [1.0])
        self.tol = RTOL * max(1.0, self.kappa)
        self.CinvEt = np.linalg.solve(self.C, self.E.T); self.S = self.B - self.E @ self.CinvEt
        self.rbs = bs[~self.is_elim]; self.rbo = np.concatenate(([0], np.cumsum(self.rbs)))[:-1]

    def reduce(self, b):
        return b[..., self.r] - np.linalg.solve(self.C, b[..., self.e].T).T @ self.E.T

    def expand(self, b, yr):
        y = np.zeros(b.shape); y[..., self.r] = yr; y[..., self.e] = np.linalg.solve(self.C, (b[..., self.e] - yr @ self.E).T).T
        return y

    def rblocks(self):
        return [self.B[o:o + d, o:o + d] for o, d in zip(self.rbo, self.rbs)]


def refused_unsupported(ctx, tag):
    """an upload that eliminated nothing: NLLS_ERR_UNSUPPORTED from the three products and the solve, the text says why, nothing written"""
    P = _capi._p; ndof = ctx.info.ndof; v = np.ones(ndof); out = np.full(ndof, 7.25); st = np.full(8, 7.25)
    nred, nelim, is_elim, index = ctx.schur_info()
    assert nelim == 0 and nred == ndof and not is_elim.any() and ctx.info.nschur_blocks == 0, tag
    assert ctx.L.nlls_schur_apply(ctx.h, 0, 0.1, 1, P(v), P(out)) == _capi.ERR_UNSUPPORTED
    assert "eliminated nothing" in ctx.L.nlls_last_error(ctx.h).decode()
    assert ctx.L.nlls_schur_reduce(ctx.h, 0, 0.1, 1, P(v), P(out)) == _capi.ERR_UNSUPPORTED
    assert ctx.L.nlls_schur_expand(ctx.h, 0, 0.1, 1, P(v), P(v), P(out)) == _capi.ERR_UNSUPPORTED
    assert ctx.L.nlls_solve_pcg_schur(ctx.h, JACOBI, 10, 1e-8, P(out), P(st)) == _capi.ERR_UNSUPPORTED
    assert np.all(out == 7.25) and np.all(st == 7.25), tag


def check_products(ctx, ref, lam, rng, tag, nvec=3):
    """schur_apply, schur_reduce and schur_expand on nvec random vectors against the host reference; -> the largest error over the bound"""
    ndof = ref.M.shape[0]; V = rng.standard_normal((nvec, ref.nred)); Bv = rng.standard_normal((nvec, ndof))
    got = (ctx.schur_apply(V, lam), ctx.schur_reduce(Bv, lam), ctx.schur_expand(Bv, V, lam))
    want = (V @ ref.S, ref.reduce(Bv), ref.expand(Bv, V))
    errs = [rel(g, w) for g, w in zip(got, want)]
    print(f"SCHUR {tag} lambda {lam:.3e}: nred {ref.nred} of {ndof}, {ref.nelim} eliminated, kappa {ref.kappa:.3e}; apply {errs[0]:.3e} reduce {errs[1]:.3e} expand {errs[2]:.3e} (of {ref.tol:.3e})")
    assert got[0].shape == (nvec, ref.nred) and got[1].shape == (nvec, ref.nred) and got[2].shape == (nvec, ndof)
    assert got[2][:, ref.r].tobytes() == V.tobytes(), "expand does not copy yr bit for bit"
    assert max(errs) <= ref.tol, (tag, errs)
    return got


# ---- 1. the products against the sweep ------------------------------------------------------------------------------------------------------------------
@FLAGS
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_products_against_the_sweep(name, flags):
    p, unfixed = PROBLEMS[name]()
    ctx, A, b, bo, bs = swept(p, unfixed, flags); bo, bs = block_sizes(ctx)
    nred, nelim, is_elim, index = ctx.schur_info()
    assert nelim == ctx.info.nschur_blocks and np.array_equal(is_elim, expected_elimination(ctx)), name
    assert (nelim > 0) == (name in ELIMINATING) and sum(n in PROBLEMS for n in ELIMINATING) >= 3, name
    if nelim == 0:
        refused_unsupported(ctx, name); print(f"SCHUR {name} flags {flags}: the upload eliminated nothing, refused"); ctx.close(); return
    rng = np.random.default_rng(17); lam0 = pd_lambda(A)
    for lam in (lam0, 10 * lam0):
        ref = Reduced(ctx, A, lam, bo, bs); got = check_products(ctx, ref, lam, rng, f"{name} flags {flags}")
        st = ctx.solve_stats(); assert st["apply_short_rows"] + st["apply_wave_rows"] == ctx.info.nblocks and st["apply_chunks"] == 1
        v = rng.standard_normal(ref.nred); y = ctx.schur_apply(v, lam)               # 1-D in, 1-D out
        assert y.shape == (ref.nred,) and rel(y, v @ ref.S) <= ref.tol
        # expand(b, S^-1 reduce(b)) solves (H + lam I) y = b: on the device's own reduce and expand, the reduced solve on the host
        y = ctx.schur_expand(b, np.linalg.solve(ref.S, ctx.schur_reduce(b, lam)), lam)
        res = np.linalg.norm(ref.M @ y - b) / np.linalg.norm(b); print(f"      expand(b, S^-1 reduce(b)): residual {res:.3e}")
        assert res <= 1e-7 * max(1.0, ref.kappa)       # (what a step is held to against nlls_solve: the two products are within the bound above, the host's solve carries cond(S))
    ctx.close()


# ---- 2. against the full product ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ELIMINATING)
def test_against_the_full_product(name):
    """(H + lam I) expand(0, v) = [S v ; 0]"""
    p, unfixed = PROBLEMS[name]()
    ctx, A, b, bo, bs = swept(p, unfixed); bo, bs = block_sizes(ctx); lam = pd_lambda(A); ref = Reduced(ctx, A, lam, bo, bs)
    v = np.random.default_rng(5).standard_normal(ref.nred)
    full = ctx.hess_apply(ctx.schur_expand(np.zeros(b.size), v, lam), lam); sv = ctx.schur_apply(v, lam)
    top = np.max(np.abs(full[ref.r])); e_r = np.max(np.abs(full[ref.r] - sv)) / top; e_e = np.max(np.abs(full[ref.e])) / top
    print(f"SCHUR {name} against the full product: r rows {e_r:.3e}, e rows {e_e:.3e} (of {ref.tol:.3e})")
    assert e_r <= ref.tol and e_e <= ref.tol
    ctx.close()


# ---- 3. the bit rules -----------------------------------------------------------------------------------------------------------------------------------
def test_bit_rules():
    p, unfixed = affine_two_groups(); ctx = upload(p, unfixed); ndof = ctx.info.ndof; nred = ctx.schur_info()[0]; rng = np.random.default_rng(31)
    assert 0 < nred < ndof
    V = rng.standard_normal((8, nred)); B = rng.standard_normal((8, ndof)); lam = 0.37
    calls = {"apply": lambda k=slice(None): ctx.schur_apply(V[k], lam), "reduce": lambda k=slice(None): ctx.schur_reduce(B[k], lam),
             "expand": lambda k=slice(None): ctx.schur_expand(B[k], V[k], lam)}
    full = {k: f() for k, f in calls.items()}
    assert ctx.solve_stats()["apply_chunks"] == 1
    for k, f in calls.items():
        assert f().tobytes() == full[k].tobytes(), f"two identical {k} calls differ"
        for j in range(8):
            assert f(j).tobytes() == full[k][j].tobytes(), f"{k}: vector {j} of eight differs from the call on it alone"
    ctx.schur_apply(V[:1], lam); one = ctx.solve_stats()["apply_scratch"]                       # doubles of one vector's records
    ctx.set_option(_capi.OPT_APPLY_SCRATCH, 3 * 8 * one + 8)                                    # room for the records of three vectors: 8 vectors in chunks of 3, 3, 2
    for k, f in calls.items():
        chunked = f(); st = ctx.solve_stats()
        assert st["apply_chunks"] == 3 and st["apply_scratch"] == 3 * one, (k, st)
        assert chunked.tobytes() == full[k].tobytes(), f"a chunked {k} differs from the unchunked one"
    ctx.set_option(_capi.OPT_APPLY_SCRATCH, 1)                                                  # less than one vector's records: one vector at a time
    for k, f in calls.items():
        chunked = f(); assert ctx.solve_stats()["apply_chunks"] == 8 and chunked.tobytes() == full[k].tobytes(), k
    ctx.close()


# ---- 4. row classes -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,pendants,degree,nedges", HUBS, ids=[f"hub degree {d}" for _, _, d, _ in HUBS])
def test_hub_shapes(n, pendants, degree, nedges):
    """the hub's row (63, 64, 65, 66, 197 incidences) is a REDUCED row on either side of the wavefront threshold; the chain's ends and pendants are eliminated"""
    p, hub = hub_problem(n, pendants); inc = incidences(p, None)
    assert inc[hub] == degree and inc.max() == degree
    ctx, A, b, bo, bs = swept(p); bo, bs = block_sizes(ctx)
    nred, nelim, is_elim, index = ctx.schur_info()
    assert np.array_equal(is_elim, expected_elimination(ctx))
    if nelim == 0:
        refused_unsupported(ctx, f"hub {degree}"); print(f"SCHUR hub degree {degree}: the upload eliminated nothing, refused"); ctx.close(); return
    assert not is_elim[hub] and nelim >= 34, "the hub should be a reduced row of an upload that eliminates: the input is at fault"     # (all five shapes eliminate: at least two must)
    lam = pd_lambda(A); ref = Reduced(ctx, A, lam, bo, bs); rng = np.random.default_rng(degree)
    got = check_products(ctx, ref, lam, rng, f"hub degree {degree}", nvec=2); st = ctx.solve_stats()
    assert (st["apply_short_rows"], st["apply_wave_rows"]) == (int(np.sum(inc < 64)), int(np.sum(inc >= 64))), st
    again = check_products(ctx, ref, lam, np.random.default_rng(degree), f"hub degree {degree} again", nvec=2)
    assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got))
    ctx.close()


def test_at_least_two_hub_shapes_eliminate():
    """what test_hub_shapes rests on: a shape whose upload eliminates nothing only exercises the refusal"""
    counts = []
    for n, pendants, degree, nedges in HUBS:
        ctx = upload(hub_problem(n, pendants)[0]); nelim = ctx.schur_info()[1]
        assert (nelim > 0) == bool(expected_elimination(ctx).any()); counts.append(nelim); ctx.close()
    print(f"SCHUR hub shapes: eliminated blocks {counts}")
    assert sum(c > 0 for c in counts) >= 2, counts


def test_wave_min_moves_rows_of_both_classes():
    """NLLS_OPT_APPLY_WAVE_MIN 1: every row, eliminated ones included, takes a wavefront and the middle step its launch of its own; the second smallest count: the rows of
    the smallest count stay one lane per entry.  Each setting reproducible to the bit, the settings agree within the bound."""
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed); bo, bs = block_sizes(ctx); inc = incidences(p, unfixed)
    lam = pd_lambda(A); ref = Reduced(ctx, A, lam, bo, bs)
    assert inc[ref.is_elim].max() < 64 <= inc[~ref.is_elim].max(), "by default the eliminated rows should be short and a reduced row long: the input is at fault"
    base = check_products(ctx, ref, lam, np.random.default_rng(2), "wave_min 64"); st = ctx.solve_stats()
    assert (st["apply_short_rows"], st["apply_wave_rows"]) == (int(np.sum(inc < 64)), int(np.sum(inc >= 64)))
    for w in (1, int(np.unique(inc)[1])):
        ctx.set_option(_capi.OPT_APPLY_WAVE_MIN, w)
        got = check_products(ctx, ref, lam, np.random.default_rng(2), f"wave_min {w}"); st = ctx.solve_stats()
        assert (st["apply_short_rows"], st["apply_wave_rows"]) == (int(np.sum(inc < w)), int(np.sum(inc >= w))) and np.sum(inc[ref.is_elim] >= w) > 0, (w, st)
        again = check_products(ctx, ref, lam, np.random.default_rng(2), f"wave_min {w} again")
        assert all(a.tobytes() == g.tobytes() for a, g in zip(again, got)), w
        assert all(rel(g, h) <= ref.tol for g, h in zip(got, base)), w
    ctx.set_option(_capi.OPT_APPLY_WAVE_MIN, 64)
    assert all(a.tobytes() == g.tobytes() for a, g in zip(check_products(ctx, ref, lam, np.random.default_rng(2), "wave_min 64 again"), base))
    ctx.close()


# ---- 5. a cut reduced row -------------------------------------------------------------------------------------------------------------------------------
def test_a_cut_reduced_row():
    """the adaptive kernel's variable lies in every block of its group: 4320 incidences, two segments of a REDUCED row (its three unknowns); the 600 points are eliminated"""
    p = synthetic.create_so3_ba_problem(8, 600, 0.9, seed=6, adaptive=True); inc = incidences(p, None)
    assert inc[0] > 4096 and inc[0] == inc.max()
    ctx, A, b, bo, bs = swept(p); bo, bs = block_sizes(ctx); nred, nelim, is_elim, index = ctx.schur_info()
    assert nelim == 600 and not is_elim[0] and bs[0] == 3 and np.all(bs[is_elim] == 3), "the upload should eliminate the 600 points and keep the kernel: the input is at fault"
    lam = pd_lambda(A); ref = Reduced(ctx, A, lam, bo, bs)
    got = check_products(ctx, ref, lam, np.random.default_rng(9), "cut reduced row", nvec=8)
    assert ctx.schur_apply(np.ones(nred), lam).tobytes() == ctx.schur_apply(np.ones(nred), lam).tobytes()
    ctx.close()


# ---- 6. the solve against nlls_solve --------------------------------------------------------------------------------------------------------------------
@FLAGS
@pytest.mark.parametrize("name", ELIMINATING)
def test_solve_against_the_direct_solve(name, flags):
    p, unfixed = PROBLEMS[name]()
    ctx, A, b, bo, bs = swept(p, unfixed, flags); bo, bs = block_sizes(ctx); ndof = ctx.info.ndof; cap = 4 * ndof
    lam = pd_lambda(A); ref = Reduced(ctx, A, lam, bo, bs); s = ref.reduce(b)
    full_blocks = [ref.M[o:o + d, o:o + d] for o, d in zip(bo, bs)]
    _, ka, sa, _ = pcg_mirror(lambda v: ref.M @ v, full_blocks, bo, b, cap, 1e-10)
    _, ks, ss, _ = pcg_mirror(lambda v: ref.S @ v, ref.rblocks(), ref.rbo, s, cap, 1e-10)
    assert sa == 0 and ss == 0 and ks <= ka, f"{name}: the host mirrors: on A {ka} (status {sa}), on S {ks} (status {ss}): the input is at fault"
    dblocks = [d for d, e in zip(ctx.hess_block_diag(lam), ref.is_elim) if not e]
    _, kd, sd, _ = pcg_mirror(lambda v: ctx.schur_apply(v, lam), dblocks, ref.rbo, ctx.schur_reduce(b, lam), cap, 1e-10)
    assert sd == 0
    ctx.damp(lam); xs = ctx.solve(want_x=True)
    _, full = ctx.solve_pcg(JACOBI, None, 1e-10); stats_full = ctx.solve_stats()
    x, st = ctx.solve_pcg_schur(JACOBI, None, 1e-10, want_x=True)
    assert st["status"] == 0 and st["iterations"] >= 1 and x.tobytes() == ctx.get_step().tobytes()
    err = np.max(np.abs(x - xs)) / np.max(np.abs(xs))
    x8, st8 = ctx.solve_pcg_schur(JACOBI, None, 1e-8, want_x=True)
    res = np.linalg.norm(ref.M @ (-x8) - b) / np.linalg.norm(b)
    print(f"SCHUR PCG {name} flags {flags}: ndof {ndof} nred {ref.nred} lambda {lam:.3e} iterations device {st['iterations']} mirror {kd} host {ks}; full system: device {full['iterations']} "
          f"host {ka}; against nlls_solve {err:.3e} (of 1e-7); true residual at rtol 1e-8 {res:.3e} (of 2e-8) recurrence {st8['rnorm'] / st8['bnorm']:.3e}; rounds {st['rounds']} "
          f"launches {st['launches']} (full: {full['launches']})")
    assert err <= 1e-7, name
    assert st8["status"] == 0 and res <= 2e-8, name
    assert abs(st["iterations"] - kd) <= 1 and st["iterations"] <= full["iterations"], (name, st, kd, full)
    assert abs(st["bnorm"] - np.linalg.norm(s)) <= 1e-9 * max(1.0, ref.kappa) * np.linalg.norm(s) and st["rnorm"] <= 1e-10 * st["bnorm"]
    after = ctx.solve_stats()                                              # the counters keep describing the last nlls_solve_pcg
    assert all(after[k] == stats_full[k] for k in ("pcg_iterations", "pcg_status", "pcg_rounds")) and after["pcg_iterations"] == full["iterations"]
    ctx.close()


def test_every_unfixed_block_eliminated():
    """all cameras fixed: the points are isolated blocks and the upload eliminates every one of them -- the reduced system has NO unknown.  The solve is then
    x = -(C + lambda I)^-1 b with status 0 and no iteration; apply and reduce have nothing to write; expand is the block-diagonal solve"""
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3), 1e-3, 1e-3)
    unfixed = np.ones(p.nvariables, bool); unfixed[:10] = False
    ctx, A, b, bo, bs = swept(p, unfixed, _capi.FLAG_MATERIALIZE); bo, bs = block_sizes(ctx); ndof = b.size
    nred, nelim, is_elim, index = ctx.schur_info()
    assert ctx.info.is_sparse and ndof == 600 and (nred, nelim) == (0, 200) and is_elim.all() and index.size == 0, "every point should be eliminated: the input is at fault"
    lam = pd_lambda(A); ref = Reduced(ctx, A, lam, bo, bs)
    assert ctx.schur_apply(np.zeros(0), lam).shape == (0,) and ctx.schur_reduce(b, lam).shape == (0,)
    y = ctx.schur_expand(b, np.zeros(0), lam); e = rel(y, np.linalg.solve(ref.M, b))
    ctx.damp(lam); xs = -np.linalg.solve(ref.M, b)                       # (the host's solve of the device's own block-diagonal system)
    for pc in (JACOBI, NONE):
        x, st = ctx.solve_pcg_schur(pc, None, 1e-10, want_x=True)
        assert (st["status"], st["iterations"]) == (0, 0) and x.tobytes() == ctx.get_step().tobytes()
        err = np.max(np.abs(x - xs)) / np.max(np.abs(xs))
        print(f"SCHUR PCG nred 0, precond {pc}: expand {e:.3e} (of {ref.tol:.3e}); against the host's solve {err:.3e} (of 1e-7); rounds {st['rounds']} launches {st['launches']}")
        assert e <= ref.tol and err <= 1e-7
    assert ctx.L.nlls_solve_pcg_schur(ctx.h, JACOBI, 10, 1e-8, None, None) == _capi.OK
    ctx.damp(-lam - 2.0 * block_min_eigs(A, bo, bs).max())                # below every block's smallest eigenvalue: no factor
    assert refused_not_spd(ctx, JACOBI, 3) == 0
    ctx.close()


# ---- 7. truncation and rounds ---------------------------------------------------------------------------------------------------------------------------
def test_truncation_and_rounds():
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed); bo, bs = block_sizes(ctx)
    lam = 1e-2 * np.max(np.abs(np.diag(A))); ref = Reduced(ctx, A, lam, bo, bs); s = ref.reduce(b)
    _, k, status, _ = pcg_mirror(lambda v: ref.S @ v, ref.rblocks(), ref.rbo, s, 4 * b.size, 1e-10)
    assert status == 0 and k > 4, f"the host mirror on S: {k} iterations, status {status}: the input is at fault"
    dblocks = [d for d, e in zip(ctx.hess_block_diag(lam), ref.is_elim) if not e]
    _, _, _, its = pcg_mirror(lambda v: ctx.schur_apply(v, lam), dblocks, ref.rbo, ctx.schur_reduce(b, lam), 3, 1e-10)
    assert len(its) == 3
    ctx.damp(lam)
    for m in (1, 2, 3):
        x, st = ctx.solve_pcg_schur(JACOBI, m, 1e-10, want_x=True)
        assert (st["status"], st["iterations"]) == (1, m) and x.tobytes() == ctx.get_step().tobytes()
        e = rel(-x, ctx.schur_expand(b, its[m - 1], lam))
        print(f"SCHUR PCG truncated at {m}: against the mirror's iterate, expanded {e:.3e} (of 1e-11)")
        assert e <= 1e-11
    x0, s0 = ctx.solve_pcg_schur(JACOBI, None, 1e-10, want_x=True); x1, s1 = ctx.solve_pcg_schur(JACOBI, None, 1e-10, want_x=True)
    assert s0["status"] == 0 and x0.tobytes() == x1.tobytes() and s0 == s1, "two calls on the same sweep differ"
    kd = s0["iterations"]; assert abs(kd - k) <= 1
    for rnd in (1, 3, 1000):
        ctx.set_option(_capi.OPT_PCG_ROUND, rnd)
        x, st = ctx.solve_pcg_schur(JACOBI, None, 1e-10, want_x=True)
        print(f"SCHUR PCG round {rnd}: iterations {st['iterations']} synchronisations {st['rounds']} launches {st['launches']}")
        assert x.tobytes() == x0.tobytes() and st["iterations"] == kd and st["status"] == 0, rnd
        assert st["rounds"] == -(-kd // rnd) + 1, (rnd, st)
    ctx.set_option(_capi.OPT_PCG_ROUND, 1)
    _, kn, sn, _ = pcg_mirror(lambda v: ref.S @ v, None, ref.rbo, s, 4 * b.size, 1e-10)
    assert sn == 0
    xn, st = ctx.solve_pcg_schur(NONE, None, 1e-10, want_x=True)
    print(f"SCHUR PCG no preconditioner: iterations {st['iterations']} (host {kn}, block Jacobi {kd}); against block Jacobi {rel(xn, x0):.3e} (of 1e-7)")
    assert st["status"] == 0 and abs(st["iterations"] - kn) <= 1 and rel(xn, x0) <= 1e-7
    assert ctx.solve_pcg_schur("none", None, 1e-10, want_x=True)[0].tobytes() == xn.tobytes()
    ctx.close()


# ---- 8. breakdowns --------------------------------------------------------------------------------------------------------------------------------------
def system_state(ctx):
    return [ctx.get_bsm_data().tobytes(), ctx.get_grad().tobytes()] + [ctx.get_variables(w).tobytes() for w in range(3)]


def refused_not_spd(ctx, pc, status):
    """an error return of the host's look at the device's scalars: NLLS_ERR_NOT_SPD, the step, x_out and the linear system byte for byte; -> the iteration it ended in"""
    ndof = ctx.info.ndof; sentinel = np.linspace(-1.0, 2.0, ndof); ctx.set_step(sentinel); before = system_state(ctx); counters = ctx.solve_stats()
    out = np.full(ndof, 7.25); st = np.full(8, -1.0)
    rc = ctx.L.nlls_solve_pcg_schur(ctx.h, pc, 4 * ndof, 1e-10, _capi._p(out), _capi._p(st))
    assert rc == _capi.ERR_NOT_SPD and int(st[1]) == status, (rc, st)
    assert np.all(out == 7.25) and ctx.get_step().tobytes() == sentinel.tobytes() and system_state(ctx) == before
    after = ctx.solve_stats(); assert all(after[k] == counters[k] for k in ("pcg_iterations", "pcg_status", "pcg_rounds"))
    with pytest.raises(_capi.NllsError) as e:
        ctx.solve_pcg_schur(pc, None, 1e-10)
    assert e.value.code == _capi.ERR_NOT_SPD and ctx.last_pcg_schur["status"] == status
    return int(st[0])


def block_min_eigs(A, bo, bs):
    return np.array([np.linalg.eigvalsh(A[o:o + d, o:o + d])[0] for o, d in zip(bo, bs)])


def test_breakdowns():
    """negative damping, as a caller's nlls_damp leaves it: first between the smallest eigenvalues of the two classes' diagonal blocks -- every C_e + lambda I keeps its
    factor, a block of B + lambda I loses it: status 3 under block Jacobi, and S is indefinite: status 2 without a preconditioner -- then below an eliminated block's:
    status 3 under either"""
    p, unfixed = PROBLEMS["so3 adaptive"]()
    ctx, A, b, bo, bs = swept(p, unfixed, _capi.FLAG_MATERIALIZE); bo, bs = block_sizes(ctx); ndof = b.size
    nred, nelim, is_elim, index = ctx.schur_info(); mins = block_min_eigs(A, bo, bs)
    me, mr = mins[is_elim].min(), mins[~is_elim].min()
    assert nelim > 0 and me > 0 and mr < 0.25 * me, f"smallest eigenvalues: eliminated blocks {me:.3e}, reduced blocks {mr:.3e}: the input is at fault"
    lam = -0.5 * me; ref = Reduced(ctx, A, lam, bo, bs); s = ref.reduce(b)
    assert pcg_mirror(lambda v: ref.S @ v, ref.rblocks(), ref.rbo, s, 4 * ndof, 1e-10)[1:3] == (0, 3), "a reduced block should be indefinite: the input is at fault"
    kn, sn = pcg_mirror(lambda v: ref.S @ v, None, ref.rbo, s, 4 * ndof, 1e-10)[1:3]
    assert sn == 2, f"the host mirror without a preconditioner ended with status {sn}: the input is at fault"
    ctx.damp(lam)
    assert refused_not_spd(ctx, JACOBI, 3) == 0
    it = refused_not_spd(ctx, NONE, 2); print(f"SCHUR PCG breakdown: lambda {lam:.3e}, status 2 in iteration {it} (host mirror: {kn})")
    assert it >= 1
    v = np.ones(nred); out = np.full(nred, 7.25)                          # the products need only the eliminated blocks' factors: they answer at this lambda
    assert ctx.L.nlls_schur_apply(ctx.h, 0, lam, 1, _capi._p(v), _capi._p(out)) == _capi.OK and rel(out, v @ ref.S) <= ref.tol
    lam2 = -2.0 * me; ctx.damp(lam2 - lam)
    with pytest.raises(np.linalg.LinAlgError):
        for o, d, e in zip(bo, bs, is_elim):
            if e:
                np.linalg.cholesky(A[o:o + d, o:o + d] + lam2 * np.eye(d))
    assert refused_not_spd(ctx, NONE, 3) == 0 and refused_not_spd(ctx, JACOBI, 3) == 0
    out[:] = 7.25; full = np.full(ndof, 7.25); P = _capi._p
    assert ctx.L.nlls_schur_apply(ctx.h, 0, lam2, 1, P(v), P(out)) == _capi.ERR_NOT_SPD
    assert ctx.L.nlls_schur_reduce(ctx.h, 0, lam2, 1, P(b), P(out)) == _capi.ERR_NOT_SPD
    assert ctx.L.nlls_schur_expand(ctx.h, 0, lam2, 1, P(b), P(v), P(full)) == _capi.ERR_NOT_SPD
    assert np.all(out == 7.25) and np.all(full == 7.25), "a product without a factor wrote to its output"
    ctx.close()


def test_refusals():
    L = _capi.lib(); ctx = _capi.Context(); P = _capi._p
    out = np.full(4096, 7.25); v = np.ones(4096); st = np.full(8, 7.25); n = np.zeros(2, np.int64)
    assert L.nlls_schur_info(ctx.h, P(n[:1]), P(n[1:]), None) == _capi.ERR_NOT_READY                               # no upload yet
    assert L.nlls_schur_apply(ctx.h, 0, 0.0, 1, P(v), P(out)) == _capi.ERR_NOT_READY
    assert L.nlls_schur_reduce(ctx.h, 0, 0.0, 1, P(v), P(out)) == _capi.ERR_NOT_READY
    assert L.nlls_schur_expand(ctx.h, 0, 0.0, 1, P(v), P(v), P(out)) == _capi.ERR_NOT_READY
    assert L.nlls_solve_pcg_schur(ctx.h, JACOBI, 10, 1e-8, P(out), P(st)) == _capi.ERR_NOT_READY
    p, unfixed = affine_two_groups(); ctx.close(); ctx = upload(p, unfixed)
    assert L.nlls_solve_pcg_schur(ctx.h, JACOBI, 10, 1e-8, P(out), P(st)) == _capi.ERR_NOT_READY                   # no sweep yet
    assert L.nlls_schur_info(ctx.h, None, None, None) == _capi.OK                                                   # every output may be NULL
    for args in ((None, P(out)), (P(v), None)):                                                                     # a null pointer
        assert L.nlls_schur_apply(ctx.h, 0, 0.0, 1, *args) == _capi.ERR_INVALID_ARG and L.nlls_schur_reduce(ctx.h, 0, 0.0, 1, *args) == _capi.ERR_INVALID_ARG
    for args in ((None, P(v), P(out)), (P(v), None, P(out)), (P(v), P(v), None)):
        assert L.nlls_schur_expand(ctx.h, 0, 0.0, 1, *args) == _capi.ERR_INVALID_ARG
    for which, nvec, lam in ((-1, 1, 0.0), (3, 1, 0.0), (0, 0, 0.0), (0, -1, 0.0), (0, _capi.APPLY_MAX_VEC + 1, 0.0), (0, 1, np.nan), (0, 1, np.inf)):
        assert L.nlls_schur_apply(ctx.h, which, lam, nvec, P(v), P(out)) == _capi.ERR_INVALID_ARG
        assert L.nlls_schur_reduce(ctx.h, which, lam, nvec, P(v), P(out)) == _capi.ERR_INVALID_ARG
        assert L.nlls_schur_expand(ctx.h, which, lam, nvec, P(v), P(v), P(out)) == _capi.ERR_INVALID_ARG
    ctx.sweep_gradhess()
    for pc, mi, rtol in ((-1, 10, 1e-8), (2, 10, 1e-8), (1, 0, 1e-8), (1, 10, np.nan), (1, 10, -1e-3)):
        assert L.nlls_solve_pcg_schur(ctx.h, pc, mi, rtol, P(out), P(st)) == _capi.ERR_INVALID_ARG
    assert np.all(out == 7.25) and np.all(st == 7.25), "a refused call wrote to an output"
    ctx.damp(1e-2 * ctx.max_abs_diag())
    assert L.nlls_solve_pcg_schur(ctx.h, JACOBI, 1000, 1e-10, None, None) == _capi.OK                               # both outputs may be NULL
    assert ctx.schur_apply(np.ones((19, ctx.schur_info()[0])), 1.0).shape == (19, ctx.schur_info()[0])             # more than eight vectors: split into calls
    ctx.close()
    # NLLS_FLAG_NO_SCHUR: the same problem with nothing eliminated
    ctx = upload(p, unfixed, _capi.FLAG_NO_SCHUR); ctx.sweep_gradhess(); refused_unsupported(ctx, "NLLS_FLAG_NO_SCHUR"); ctx.close()


def test_sharded_contexts_are_refused():
    from tests.helpers import blockindices
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3), 1e-3, 1e-3)
    c = _capi.Context(); P = _capi._p
    try:
        c.set_shard(0, 2); c.upload(p.var_kind, p.var_dim, blockindices(p), p.groups(), _capi.FLAG_FORCE_SPARSE); c.set_variables(p.variables)
        assert c.shard_info()["nranks"] == 2 and c.shard_info()["replicated"] == 0
        c.sweep_gradhess_local(); ndof = c.info.ndof; v = np.ones(ndof); out = np.full(ndof, 7.25)
        assert c.L.nlls_schur_apply(c.h, 0, 0.0, 1, P(v), P(out)) == _capi.ERR_UNSUPPORTED and c.L.nlls_schur_reduce(c.h, 0, 0.0, 1, P(v), P(out)) == _capi.ERR_UNSUPPORTED
        assert c.L.nlls_schur_expand(c.h, 0, 0.0, 1, P(v), P(v), P(out)) == _capi.ERR_UNSUPPORTED
        assert c.L.nlls_solve_pcg_schur(c.h, JACOBI, 10, 1e-8, P(out), None) == _capi.ERR_UNSUPPORTED and np.all(out == 7.25)
    finally:
        c.close()


# ---- 9. read only ---------------------------------------------------------------------------------------------------------------------------------------
def four_calls(ctx, rng):
    nred, nelim, is_elim, index = ctx.schur_info(); ndof = ctx.info.ndof
    ctx.schur_apply(rng.standard_normal((2, nred)), 0.3, _capi.VARS_CURRENT); ctx.schur_reduce(rng.standard_normal(ndof), 0.1, _capi.VARS_NEXT)
    ctx.schur_expand(rng.standard_normal(ndof), rng.standard_normal(nred), 0.2, _capi.VARS_BEST)


def test_calls_leave_the_linear_system_untouched():
    p, unfixed = affine_two_groups()
    ctx = upload(p, unfixed, _capi.FLAG_MATERIALIZE); ctx.copy_variables(_capi.VARS_NEXT, _capi.VARS_CURRENT); ctx.copy_variables(_capi.VARS_BEST, _capi.VARS_CURRENT)
    ctx.sweep_gradhess(); ctx.solve(); step = ctx.get_step().tobytes()
    before = system_state(ctx); st0 = ctx.solve_stats()
    four_calls(ctx, np.random.default_rng(4))
    st1 = ctx.solve_stats()
    assert system_state(ctx) == before and ctx.get_step().tobytes() == step
    assert all(st0[k] == st1[k] for k in st0 if not k.startswith("apply")), (st0, st1)
    ctx.close()


def _trial_run(p, call, materialise):
    ctx = upload(p, None, _capi.FLAG_DETERMINISTIC)
    if materialise:
        ctx.set_option(_capi.OPT_MATERIALIZE, 1)
    ctx.copy_variables(_capi.VARS_NEXT, _capi.VARS_CURRENT); ctx.copy_variables(_capi.VARS_BEST, _capi.VARS_CURRENT)
    c0 = ctx.sweep_gradhess(); lam = 1e-3
    if call:
        before = ctx.solve_stats(); four_calls(ctx, np.random.default_rng(1)); after = ctx.solve_stats()
        keys = ("lookahead_hits", "lookahead_misses", "mf_trials", "reduced_sweeps", "full_sweeps")
        assert [before[k] for k in keys] == [after[k] for k in keys], (before, after)
    c1 = ctx.lm_trial(lam); mf = ctx.solve_stats()["mf_trials"]
    out = (c0, c1, ctx.get_step().tobytes(), ctx.get_variables(_capi.VARS_NEXT).tobytes()); ctx.close()
    return out, mf


@pytest.mark.parametrize("materialise", [False, True], ids=["matrix-free", "materialised"])
def test_reads_only_on_both_trial_paths(materialise):
    """the pattern of tests/test_gpu_apply.py::test_reads_only_on_both_trial_paths: bytes cannot be compared across runs on these two paths"""
    p = chain_problem()
    (a, mfa), (c, mfc) = (_trial_run(p, call, materialise) for call in (False, True))
    assert mfa == mfc == (0 if materialise else 1), "the trial did not take the path the case was written for"
    print(f"SCHUR trial behind the calls, materialise={materialise}: costs {a[:2]} / {c[:2]}")
    assert np.allclose(c[:2], a[:2], rtol=1e-9, atol=0.0)
    assert np.allclose(np.frombuffer(c[2]), np.frombuffer(a[2]), rtol=1e-9, atol=1e-12) and np.allclose(np.frombuffer(c[3]), np.frombuffer(a[3]), rtol=1e-9, atol=1e-12)


# ---- 10. optimize ---------------------------------------------------------------------------------------------------------------------------------------
def test_optimize_with_reduced_pcg_steps():
    make = lambda: synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3), 1e-3, 1e-3)      # (the problem of tests/test_gpu_pcg.py: noise-free)
    with N.Solver(make()) as s:
        res = s.optimize(N.NLLSOptions(maxiters=50)); control = res.bestcost
        print(f"SCHUR PCG optimize, the control: cost {res.startcost:.3e} -> {res.bestcost:.3e} in {res.niterations} iterations")
        assert control <= 1e-15 * res.startcost
    with N.Solver(make()) as s:
        res = s.optimize(N.NLLSOptions(maxiters=50, linearsolver=N.PCG(rtol=1e-6, schur=True))); last = s.ls.ctx.last_pcg_schur
        print(f"SCHUR PCG optimize: cost {res.startcost:.3e} -> {res.bestcost:.3e} in {res.niterations} iterations, {res.linearsolvers} linear solves, last of {last['iterations']} iterations")
        assert res.bestcost <= 1e-15 * res.startcost and res.linearsolvers > 0 and last["iterations"] > 0 and s.ls.ctx.solve_stats()["pcg_iterations"] == 0
        op = s.schur_operator(0.5); nred, nelim, is_elim, index = s.ls.schur_info()
        assert op.shape == (nred, nred) and np.array_equal(op.index, index) and len(op.diag_blocks()) == int((~is_elim).sum())
        g = np.asarray(s.ls.ctx.get_grad()) + 1.0; yr = np.linalg.solve(np.array([op.matvec(e) for e in np.eye(nred)]).T, op.reduce(g))
        assert rel(s.hessvec(op.expand(g, yr), 0.5), g) <= 1e-8
    for it in (N.newton, N.dogleg):
        res = N.optimize(make(), N.NLLSOptions(maxiters=30, iterator=it, linearsolver=N.PCG(rtol=1e-8, schur=True)))
        print(f"SCHUR PCG optimize {it.name}: cost {res.startcost:.3e} -> {res.bestcost:.3e} in {res.niterations} iterations")
        assert res.bestcost < 1e-6 * res.startcost and res.linearsolvers > 0
    with pytest.raises(_capi.NllsError) as e:                               # no eliminated set: refused, no silent fall-back to the full system
        N.optimize(dense_curve_rosenbrock(), N.NLLSOptions(maxiters=5, linearsolver=N.PCG(schur=True)))
    assert e.value.code == _capi.ERR_UNSUPPORTED
    with N.Solver(dense_curve_rosenbrock()) as s:
        with pytest.raises(_capi.NllsError):
            s.schur_operator(0.1)


# ---- 11. a user kind ------------------------------------------------------------------------------------------------------------------------------------
def test_user_kind_in_a_process_of_its_own():
    userlib = os.path.join(ROOT, "nllssolver.jl_amd", "csrc", "libnlls_amd_userdemo.so")
    env = dict(os.environ, NLLS_AMD_LIB=userlib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "schur_userkind_worker.py")], capture_output=True, text=True, env=env, timeout=600)
    print(out.stdout[-1500:])
    assert out.returncode == 0 and "user kind schur ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
