"""nlls_hess_apply / nlls_jac_apply / nlls_jact_apply / nlls_hess_block_diag: the linearisation applied to vectors without A.data (include/nlls_amd.h).

Tolerances:
  H v against the sweep's A (A v + lambda v formed on the host): 1e-11 of the largest entry, the RTOL tests/test_gpu_linearize.py holds the reassembly of A to -- both
         sides are the same products summed in different orders;
  J v: every entry within 16 * 2^-53 * sum_j |J_mj| |v_j| of the host's product with nlls_eval_jacobians' J (a dot product of at most 12 terms);
  J' u, the identities, nlls_quadform, the diagonal blocks: 1e-11 of the largest entry; a diagonal block against its transpose: 1e-14;
  the composed CG against damp(lambda); solve(): 1e-7 of the largest entry of the step, what check_problem holds x to against the oracle.
The bit rules are exact: identical calls, vector k of a call of eight against the call on v_k, a chunked call against the unchunked one."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import synthetic, _capi
from tests.helpers import blockindices, curve_family_problem, mixed_sizes_problem, scalar_graph_problem, hub_edges
from tests.test_gpu_blockeval import adaptive_mean_problem, chain_problem
from tests.test_gpu_linearize import affine_two_groups, device_system, upload, rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-11
U = 2.0 ** -53


def dense_curve_rosenbrock():
    """the dense problem of tests/test_gpu_linearize.py::test_blocks_reassemble_the_sweep"""
    dense = curve_family_problem(1, 60, own=(), seed=4)
    first = dense.addvariables(np.random.default_rng(8).uniform(-1.0, 2.0, (3, 2)))
    dense.addcosts(K.RES_ROSENBROCK_2D, (first + np.arange(3))[:, None], np.array([[1.0, 10.0], [0.7, 8.0], [1.2, 12.0]]), N.GemanMcclureKernel(2.0))
    return dense


def scale_mix():
    from tests.test_oracle_pins import scale_mix_problem
    return scale_mix_problem(8, n=64, noise=1e-3, shared=3, robust=N.HuberKernel(0.05))


PROBLEMS = {"affine two groups": affine_two_groups,
            "so3 adaptive": lambda: (synthetic.create_so3_ba_problem(4, 30, 0.5, seed=6, adaptive=True), None),
            "dense curve + rosenbrock": lambda: (dense_curve_rosenbrock(), None),
            "mixed linear3 + cost3": lambda: (with_cost3(mixed_sizes_problem("linear3")), None),
            "scale mix": lambda: (scale_mix(), None)}


def with_cost3(p):
    """mixed_sizes_problem("linear3") with a NLLS_COST_LINEAR3 group beside its groups: the non-squared cost y'w on every fifth point"""
    ncam, npts = 12, 150; pts = np.arange(1, npts, 5)
    p.addcosts(K.COST_LINEAR3, (ncam + pts + 1)[:, None], 0.01 * np.random.default_rng(9).standard_normal((pts.size, 3)))
    assert any(g.res_kind == K.COST_LINEAR3 for g in p.costs.values()) and any(g.res_kind == K.RES_LINEAR3 for g in p.costs.values())
    return p


def block_sizes(ctx):
    bo = np.asarray(ctx.bsm_index()[3], np.int64) - 1
    return bo, np.diff(np.concatenate((bo, [ctx.info.ndof])))


# ---- 1. H v against the sweep ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, _capi.FLAG_MATERIALIZE], ids=["default", "materialize"])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_hess_apply_against_the_sweep(name, flags):
    p, unfixed = PROBLEMS[name]()
    ctx = upload(p, unfixed, flags); ctx.sweep_gradhess(); A, _ = device_system(ctx); ndof = ctx.info.ndof
    V = np.random.default_rng(17).standard_normal((3, ndof))
    for lam in (0.0, 1e-3 * np.max(np.abs(np.diag(A)))):
        ref = V @ A + lam * V                                     # (A symmetric: row k is A v_k + lam v_k)
        Y = ctx.hess_apply(V, lam); st = ctx.solve_stats()
        assert Y.shape == (3, ndof) and st["apply_short_rows"] + st["apply_wave_rows"] == ctx.info.nblocks and st["apply_chunks"] == 1
        err = max(rel(Y[k], ref[k]) for k in range(3))
        print(f"APPLY H v {name} flags {flags} lambda {lam:.3e}: ndof {ndof} error {err:.3e} (of {RTOL:.0e}) rows {st['apply_short_rows']} + {st['apply_wave_rows']}")
        assert err < RTOL, (name, lam)
        y0 = ctx.hess_apply(V[0], lam)
        assert y0.shape == (ndof,) and y0.tobytes() == Y[0].tobytes()
    ctx.close()


# ---- 2. J v and J' u ---------------------------------------------------------------------------------------------------------------------------------
def host_jacobian(p, ctx, unfixed, gi):
    """the group's J as a dense (ncost * M, ndof) array from nlls_eval_jacobians: the columns of fixed slots dropped, no column for the kernel variable"""
    g = list(p.costs.values())[gi]; vi, _ = g.arrays(); J = ctx.eval_jacobians(gi, want="J")["J"]; n, M, NJ = J.shape
    slots = K.RES_TABLE[g.res_kind][4]; first = 1 if g.res_kind in K.ADAPTIVE_KINDS else 0
    bi = blockindices(p, unfixed).astype(np.int64); bo, _ = block_sizes(ctx)
    Jd = np.zeros((n * M, ctx.info.ndof)); j0 = 0
    for s in range(first, len(slots)):
        dof = K.var_dof(*slots[s]); bs = bi[vi[:, s] - 1]; free = np.nonzero(bs > 0)[0]
        for q in range(dof):
            for m in range(M):
                Jd[free * M + m, bo[bs[free] - 1] + q] += J[free, m, j0 + q]
        j0 += dof
    assert j0 == NJ
    return Jd


@pytest.mark.parametrize("name", ["affine two groups", "so3 adaptive", "scale mix"])
def test_jac_and_jact_against_eval_jacobians(name):
    p, unfixed = PROBLEMS[name]()
    ctx = upload(p, unfixed); ndof = ctx.info.ndof; rng = np.random.default_rng(23)
    for gi in range(len(p.costs)):
        Jd = host_jacobian(p, ctx, unfixed, gi); rows = Jd.shape[0]
        V = rng.standard_normal((2, ndof)); Uu = rng.standard_normal((2, rows))
        got = ctx.jac_apply(gi, V); st = ctx.solve_stats()
        assert got.shape == (2, rows) and (st["apply_short_rows"], st["apply_wave_rows"], st["apply_chunks"], st["apply_scratch"]) == (0, 0, 1, 0)
        bound = 16 * U * (np.abs(V) @ np.abs(Jd).T); diff = np.abs(got - V @ Jd.T)
        worst = np.max(diff / np.maximum(bound, 1e-300))
        print(f"APPLY J v {name}[{gi}]: {rows} rows, largest error / bound {worst:.3f} (of 1)")
        assert np.all(diff <= bound), (name, gi)
        back = ctx.jact_apply(gi, Uu); ref = Uu @ Jd
        err = max(rel(back[k], ref[k]) for k in range(2))
        print(f"APPLY J' u {name}[{gi}]: error {err:.3e} (of {RTOL:.0e})")
        assert back.shape == (2, ndof) and err < RTOL, (name, gi)
        assert ctx.jac_apply(gi, V[1]).tobytes() == got[1].tobytes() and ctx.jact_apply(gi, Uu[1]).tobytes() == back[1].tobytes()
    ctx.close()


def test_identities_of_one_unrobustified_group():
    """J' r is the gradient and J' J v the Gauss-Newton product: without a robust kernel that is b and H v"""
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3, robust=None), 1e-3, 1e-3)
    unfixed = np.ones(p.nvariables, bool); unfixed[[0, 1]] = False; unfixed[10:40] = False
    ctx = upload(p, unfixed); ctx.sweep_gradhess()
    r = ctx.eval_jacobians(0, want="r")["r"].ravel(); b = ctx.get_grad()
    e1 = rel(ctx.jact_apply(0, r), b)
    v = np.random.default_rng(5).standard_normal(ctx.info.ndof)
    e2 = rel(ctx.hess_apply(v, 0.0), ctx.jact_apply(0, ctx.jac_apply(0, v)))
    print(f"APPLY identities: J' r against b {e1:.3e}, H v against J' (J v) {e2:.3e} (of {RTOL:.0e})")
    assert e1 < RTOL and e2 < RTOL
    ctx.close()


# ---- 3. nlls_quadform agrees --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("materialise", [False, True], ids=["matrix-free", "materialised"])
def test_quadform_agrees(materialise):
    p = chain_problem(); ctx = upload(p)
    if materialise:
        ctx.set_option(_capi.OPT_MATERIALIZE, 1)
    ctx.copy_variables(_capi.VARS_NEXT, _capi.VARS_CURRENT); ctx.sweep_gradhess()
    v = 1e-3 * np.random.default_rng(3).standard_normal(ctx.info.ndof); lam = 1e-3 * ctx.max_abs_diag()
    y = ctx.hess_apply(v, lam)                                     # (before the damping: the product takes lambda as an argument)
    ctx.set_step(v); ctx.damp(lam); xHx, gx = ctx.quadform(); g = ctx.get_grad()
    e1 = abs(v @ y - xHx) / abs(xHx); e2 = abs(g @ v - gx) / max(abs(gx), 1e-300)
    print(f"APPLY quadform materialise={materialise}: v'(H + lambda I)v {e1:.3e}, g'v {e2:.3e} (of {RTOL:.0e}); xHx {xHx:.6e}")
    assert e1 < RTOL and e2 < RTOL
    ctx.damp(-lam); c1 = ctx.lm_trial(lam)
    assert np.isfinite(c1) and ctx.solve_stats()["mf_trials"] == (0 if materialise else 1), "the trial did not take the path the case was written for"
    ctx.close()


# ---- 4. the diagonal blocks -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wave_min", [None, 8], ids=["default rows", "wave rows from 8"])
@pytest.mark.parametrize("name", ["affine two groups", "so3 adaptive", "mixed linear3 + cost3"])
def test_hess_block_diag(name, wave_min):
    p, unfixed = PROBLEMS[name]()
    ctx = upload(p, unfixed)
    if wave_min is not None:
        ctx.set_option(_capi.OPT_APPLY_WAVE_MIN, wave_min)
    ctx.sweep_gradhess(); A, _ = device_system(ctx); bo, bs = block_sizes(ctx)
    for lam in (0.0, 1e-3 * np.max(np.abs(np.diag(A)))):
        D = ctx.hess_block_diag(lam); st = ctx.solve_stats()
        assert len(D) == bs.size and (wave_min is None or st["apply_wave_rows"] > 0)
        err = sym = 0.0
        for b, d in enumerate(D):
            ref = A[bo[b]:bo[b] + bs[b], bo[b]:bo[b] + bs[b]] + lam * np.eye(bs[b])
            assert d.shape == ref.shape
            err = max(err, np.max(np.abs(d - ref)) / np.max(np.abs(ref))); sym = max(sym, np.max(np.abs(d - d.T)) / np.max(np.abs(d)))
        print(f"APPLY diagonal blocks {name} lambda {lam:.3e} wave_min {wave_min}: {bs.size} blocks, error {err:.3e} (of {RTOL:.0e}) asymmetry {sym:.3e} (of 1e-14)")
        assert err < RTOL and sym <= 1e-14, (name, lam)
    ctx.close()


# ---- 5. the bit rules -----------------------------------------------------------------------------------------------------------------------------------
def test_bit_rules():
    p, unfixed = affine_two_groups(); ctx = upload(p, unfixed); ndof = ctx.info.ndof; rng = np.random.default_rng(31)
    V = rng.standard_normal((8, ndof)); lam = 0.37
    rows1 = ctx._groups[1][0] * 2; U8 = rng.standard_normal((8, rows1))
    calls = {"hess": lambda a=V: ctx.hess_apply(a, lam), "jac": lambda a=V: ctx.jac_apply(1, a), "jact": lambda a=U8: ctx.jact_apply(1, a)}
    full = {k: f() for k, f in calls.items()}; diag = np.concatenate([d.ravel() for d in ctx.hess_block_diag(lam)])
    assert ctx.solve_stats()["apply_chunks"] == 1
    for k, f in calls.items():
        assert f().tobytes() == full[k].tobytes(), f"two identical {k} calls differ"
        src = U8 if k == "jact" else V
        for j in range(8):
            assert f(src[j]).tobytes() == full[k][j].tobytes(), f"{k}: vector {j} of eight differs from the call on it alone"
    assert np.concatenate([d.ravel() for d in ctx.hess_block_diag(lam)]).tobytes() == diag.tobytes()
    ctx.hess_apply(V[:1], lam); one = ctx.solve_stats()["apply_scratch"]                        # doubles of one vector's records
    ctx.set_option(_capi.OPT_APPLY_SCRATCH, 3 * 8 * one + 8)                                    # room for the records of three vectors: 8 vectors in chunks of 3, 3, 2
    chunked = ctx.hess_apply(V, lam); st = ctx.solve_stats()
    assert st["apply_chunks"] == 3 and st["apply_scratch"] == 3 * one, st
    assert chunked.tobytes() == full["hess"].tobytes(), "a chunked call differs from the unchunked one"
    ctx.set_option(_capi.OPT_APPLY_SCRATCH, 1)                                                  # less than one vector's records: one vector at a time
    chunked = ctx.hess_apply(V, lam); st = ctx.solve_stats()
    assert st["apply_chunks"] == 8 and chunked.tobytes() == full["hess"].tobytes()
    tchunk = ctx.jact_apply(1, U8)
    assert ctx.solve_stats()["apply_chunks"] == 8 and tchunk.tobytes() == full["jact"].tobytes()
    ctx.close()


# ---- 6. gather shapes -----------------------------------------------------------------------------------------------------------------------------------
def hub_problem(n, pendants):
    """scalar_graph_problem(hub_edges(n, pendants)) with two more variables of exactly one incident block each, in two groups of exactly one block"""
    edges, nv = hub_edges(n, pendants)
    p = scalar_graph_problem(edges, nv, seed=n + pendants, robust=N.GemanMcclureKernel(0.7))
    a = p.addvariable(0.8); b = p.addvariable(1.3)
    p.addcosts(K.RES_ROSENBROCK_A, [[a]], [[1.1]], N.HuberKernel(0.9))
    p.addcosts(K.RES_ROSENBROCK_A, [[b]], [[0.7]], N.GemanMcclureKernel(0.8))
    return p, nv - 1                                                 # (the hub is the last variable of the graph)


def incidences(p, unfixed):
    cnt = np.zeros(p.nvariables, np.int64)
    for g in p.costs.values():
        np.add.at(cnt, g.arrays()[0].ravel() - 1, 1)
    return cnt[np.ones(p.nvariables, bool) if unfixed is None else unfixed]


W = 64                                                               # NLLS_OPT_APPLY_WAVE_MIN at its default
# (n, pendants, incidences of the hub = n + pendants edges + its unary block, blocks of the edge group)
HUBS = [(61, 1, W - 1, 123), (61, 2, W, 125), (61, 3, W + 1, 127), (191, 5, 3 * 64 + 5, 391), (61, 4, 66, 2 * 64 + 1)]


@pytest.mark.parametrize("n,pendants,degree,nedges", HUBS, ids=[f"hub degree {d}" for _, _, d, _ in HUBS])
def test_gather_shapes(n, pendants, degree, nedges):
    p, hub = hub_problem(n, pendants); groups = list(p.costs.values())
    assert len(groups) == 4 and [len(g) for g in groups] == [nedges, n + pendants + 1, 1, 1]
    rng = np.random.default_rng(degree)
    only_hub = np.zeros(p.nvariables, bool); only_hub[hub] = True
    only_end = np.zeros(p.nvariables, bool); only_end[0] = True
    for tag, unfixed in (("all free", None), ("all but the hub fixed", only_hub), ("all but a chain end fixed", only_end)):
        inc = incidences(p, unfixed)
        if unfixed is None:
            assert inc[hub] == degree and np.sum(inc == 1) == 2 and inc.max() == degree
        ctx = upload(p, unfixed); ctx.sweep_gradhess(); A, _ = device_system(ctx); ndof = ctx.info.ndof
        assert ndof == inc.size
        V = rng.standard_normal((2, ndof)); lam = 0.01 * np.max(np.abs(np.diag(A)))
        Y = ctx.hess_apply(V, lam); st = ctx.solve_stats()
        err = rel(Y, V @ A + lam * V)
        print(f"APPLY gather n={n} pendants={pendants} {tag}: ndof {ndof} largest row {inc.max()} error {err:.3e} (of {RTOL:.0e}) rows {st['apply_short_rows']} + {st['apply_wave_rows']}")
        assert (st["apply_short_rows"], st["apply_wave_rows"]) == (int(np.sum(inc < W)), int(np.sum(inc >= W))), (tag, st)
        assert err < RTOL, tag
        D = ctx.hess_block_diag(lam)
        assert rel(np.array([d[0, 0] for d in D]), np.diag(A) + lam) < RTOL, tag
        Jt = ctx.jact_apply(0, ctx.jac_apply(0, V[0]))             # (one group's records alone, out of rows that hold other groups' incidences too)
        assert Jt.shape == (ndof,) and np.all(np.isfinite(Jt))
        ctx.close()


def test_rows_cut_into_segments():
    """a row of more than 4096 incidences (the adaptive kernel's variable: every block of its group) is summed by several wavefronts, a segment each, and the segments
    are added in order: 4200 blocks give the kernel's row two segments, the second partly filled; the two means' rows (2100 each) stay whole"""
    p = adaptive_mean_problem(means=(-0.4, 0.3), draws=(1700, 400)); ctx = upload(p); inc = incidences(p, None)
    assert list(inc) == [4200, 2100, 2100] and ctx.info.ndof == 5
    ctx.sweep_gradhess(); A, _ = device_system(ctx); V = np.random.default_rng(9).standard_normal((8, 5)); lam = 1e-3 * np.max(np.abs(np.diag(A)))
    Y = ctx.hess_apply(V, lam); st = ctx.solve_stats(); err = rel(Y, V @ A + lam * V)
    D = ctx.hess_block_diag(lam); ref = A[:3, :3] + lam * np.eye(3); ed = np.max(np.abs(D[0] - ref)) / np.max(np.abs(ref))
    print(f"APPLY cut rows: H v {err:.3e} kernel diagonal block {ed:.3e} (of {RTOL:.0e}) rows {st['apply_short_rows']} + {st['apply_wave_rows']}")
    assert (st["apply_short_rows"], st["apply_wave_rows"]) == (0, 3) and err < RTOL and ed < RTOL
    assert all(ctx.hess_apply(V[k], lam).tobytes() == Y[k].tobytes() for k in range(8)) and ctx.hess_apply(V, lam).tobytes() == Y.tobytes()
    u = np.random.default_rng(10).standard_normal(4200); Jt = ctx.jact_apply(0, u); J = ctx.eval_jacobians(0, want="J")["J"][:, 0, 0]
    vi = list(p.costs.values())[0].arrays()[0]; want = np.zeros(5)
    np.add.at(want, 3 + (vi[:, 1] - 2), J * u)                     # (the kernel's three rows of J' u are 0; the two means are unknowns 3 and 4)
    assert np.all(Jt[:3] == 0.0) and rel(Jt, want) < RTOL
    ctx.close()


def test_wave_min_is_an_option():
    """the threshold moves rows between the two classes; the sums are the same to rounding, each class reproducible to the bit"""
    p, unfixed = affine_two_groups(); ctx = upload(p, unfixed); inc = incidences(p, unfixed)
    v = np.random.default_rng(2).standard_normal(ctx.info.ndof)
    y64 = ctx.hess_apply(v, 0.5); st = ctx.solve_stats()
    assert (st["apply_short_rows"], st["apply_wave_rows"]) == (int(np.sum(inc < 64)), int(np.sum(inc >= 64)))
    w = int(np.unique(inc)[1])                                    # the second smallest count: the rows of the smallest count stay short, all others get a wavefront
    ctx.set_option(_capi.OPT_APPLY_WAVE_MIN, w)
    y3 = ctx.hess_apply(v, 0.5); st = ctx.solve_stats()
    assert (st["apply_short_rows"], st["apply_wave_rows"]) == (int(np.sum(inc < w)), int(np.sum(inc >= w))) and st["apply_wave_rows"] > 6 and st["apply_short_rows"] > 0
    assert rel(y3, y64) < RTOL and ctx.hess_apply(v, 0.5).tobytes() == y3.tobytes()
    ctx.set_option(_capi.OPT_APPLY_WAVE_MIN, 64)
    assert ctx.hess_apply(v, 0.5).tobytes() == y64.tobytes()
    ctx.close()


# ---- 7. read only -------------------------------------------------------------------------------------------------------------------------------------
def four_calls(ctx, p, rng):
    ndof = ctx.info.ndof
    ctx.hess_apply(rng.standard_normal((2, ndof)), 0.3, _capi.VARS_CURRENT); ctx.hess_block_diag(0.1, _capi.VARS_NEXT)
    for gi, g in enumerate(p.costs.values()):
        if K.RES_TABLE[g.res_kind][1] > 0:
            u = ctx.jac_apply(gi, rng.standard_normal(ndof), _capi.VARS_NEXT); ctx.jact_apply(gi, u, _capi.VARS_CURRENT)


def _trial_run(p, flags, call, materialise):
    ctx = upload(p, None, flags)
    if materialise:
        ctx.set_option(_capi.OPT_MATERIALIZE, 1)
    ctx.copy_variables(_capi.VARS_NEXT, _capi.VARS_CURRENT)
    c0 = ctx.sweep_gradhess(); lam = 1e-3
    if call:
        before = ctx.solve_stats(); four_calls(ctx, p, np.random.default_rng(1)); after = ctx.solve_stats()
        keys = ("lookahead_hits", "lookahead_misses", "mf_trials", "reduced_sweeps", "full_sweeps")
        assert [before[k] for k in keys] == [after[k] for k in keys], (before, after)
    c1 = ctx.lm_trial(lam); mf = ctx.solve_stats()["mf_trials"]
    out = (c0, c1, ctx.get_step().tobytes(), ctx.get_variables(_capi.VARS_NEXT).tobytes()); ctx.close()
    return out, mf


def test_reads_only_small_dense():
    """where a trial is reproducible to the bit (tests/test_gpu_linearize.py::test_reads_only_small_dense says why): the trial behind the four calls is the trial without
    them, cost and step byte for byte"""
    p = adaptive_mean_problem(means=(-0.4, 0.3), draws=(24, 6))
    (a, _), (b, _), (c, _) = (_trial_run(p, 0, call, False) for call in (False, False, True))
    assert a == b, "the trial without the calls is not reproducible"
    assert c == a


@pytest.mark.parametrize("materialise", [False, True], ids=["matrix-free", "materialised"])
def test_reads_only_on_both_trial_paths(materialise):
    """the pattern of tests/test_gpu_linearize.py::test_reads_only_on_both_trial_paths, whose docstring says why bytes cannot be compared ACROSS runs on these two paths
    (the sweeps and the assembly add with atomics: runs without any call differ in the last digits): the run with the four calls is held to what a trial is asked of
    another run, the counters around the calls exactly; the byte comparisons are test_reads_only_small_dense and test_calls_leave_the_linear_system_untouched."""
    p = chain_problem()
    (a, mfa), (c, mfc) = (_trial_run(p, _capi.FLAG_DETERMINISTIC, call, materialise) for call in (False, True))
    assert mfa == mfc == (0 if materialise else 1), "the trial did not take the path the case was written for"
    print(f"APPLY trial behind the calls, materialise={materialise}: bit-identical to the run without {c == a}; costs {a[:2]} / {c[:2]}")
    assert np.allclose(c[:2], a[:2], rtol=1e-9, atol=0.0)
    assert np.allclose(np.frombuffer(c[2]), np.frombuffer(a[2]), rtol=1e-9, atol=1e-12) and np.allclose(np.frombuffer(c[3]), np.frombuffer(a[3]), rtol=1e-9, atol=1e-12)


def test_calls_leave_the_linear_system_untouched():
    """A.data, b and the three variable sets before and behind the four calls, byte for byte in one context (a materialised upload: reading them sweeps nothing again)"""
    p, unfixed = affine_two_groups()
    ctx = upload(p, unfixed, _capi.FLAG_MATERIALIZE); ctx.copy_variables(_capi.VARS_NEXT, _capi.VARS_CURRENT); ctx.copy_variables(_capi.VARS_BEST, _capi.VARS_CURRENT)
    ctx.sweep_gradhess()
    state = lambda: [ctx.get_bsm_data().tobytes(), ctx.get_grad().tobytes()] + [ctx.get_variables(w).tobytes() for w in range(3)]
    before = state(); st0 = ctx.solve_stats()
    four_calls(ctx, p, np.random.default_rng(4))
    st1 = ctx.solve_stats()
    assert state() == before
    assert all(st0[k] == st1[k] for k in st0 if not k.startswith("apply")), (st0, st1)
    ctx.close()


# ---- 8. composition: a block-Jacobi CG of the caller's own ----------------------------------------------------------------------------------------------
def block_jacobi_cg(matvec, blocks, bo, rhs, cap, tol=1e-12):
    """preconditioned conjugate gradients on matvec(x) = rhs; the preconditioner solves with the diagonal blocks.  -> (x, iterations, converged)"""
    inv = [np.linalg.inv(d) for d in blocks]
    def prec(r):
        z = np.empty_like(r)
        for b, m in enumerate(inv):
            z[bo[b]:bo[b] + m.shape[0]] = m @ r[bo[b]:bo[b] + m.shape[0]]
        return z
    x = np.zeros_like(rhs); r = rhs.copy(); z = prec(r); d = z.copy(); rz = r @ z; stop = tol * np.linalg.norm(rhs)
    for it in range(1, cap + 1):
        q = matvec(d); alpha = rz / (d @ q); x += alpha * d; r -= alpha * q
        if np.linalg.norm(r) <= stop:
            return x, it, True
        z = prec(r); rz, old = r @ z, rz; d = z + (rz / old) * d
    return x, cap, False


def test_block_jacobi_cg_on_the_device_operator():
    p, unfixed = affine_two_groups()
    with N.Solver(p, unfixed) as s:
        op = s.operator(0.0)                                       # (puts problem.variables on the device: before the sweep)
        ctx = s.ls.ctx; ctx.sweep_gradhess(); A, b = device_system(ctx); bo, bs = block_sizes(ctx); ndof = ctx.info.ndof; cap = 4 * ndof
        lam = 1e-2 * np.max(np.abs(np.diag(A))); op.lam = lam
        host_blocks = [A[bo[k]:bo[k] + bs[k], bo[k]:bo[k] + bs[k]] + lam * np.eye(bs[k]) for k in range(bs.size)]
        xh, ith, okh = block_jacobi_cg(lambda v: A @ v + lam * v, host_blocks, bo, b, cap)
        assert okh, f"CG on the HOST matrix did not converge in {cap} iterations: lambda {lam:.3e} is too small for this problem, not a fault of the kernel"
        assert op.shape == (ndof, ndof)
        xd, itd, okd = block_jacobi_cg(op.matvec, op.diag_blocks(), bo, b, cap)
        ctx.damp(lam); xs = ctx.solve(want_x=True)               # x = -(H + lambda I)^-1 b
        err = np.max(np.abs(-xd - xs)) / np.max(np.abs(xs))
        print(f"APPLY CG: ndof {ndof} lambda {lam:.3e} iterations host {ith} device {itd} (cap {cap}); against nlls_solve {err:.3e} (of 1e-7)")
        assert okd and err <= 1e-7


# ---- 9. errors ------------------------------------------------------------------------------------------------------------------------------------------
def test_errors():
    L = _capi.lib(); ctx = _capi.Context(); P = _capi._p
    out = np.full(4096, 7.25); sentinel = out.copy(); v = np.ones(4096)
    assert L.nlls_hess_apply(ctx.h, 0, 0.0, 1, P(v), P(out)) == _capi.ERR_NOT_READY                              # no upload yet
    assert L.nlls_jac_apply(ctx.h, 0, 0, 1, P(v), P(out)) == _capi.ERR_NOT_READY
    assert L.nlls_jact_apply(ctx.h, 0, 0, 1, P(v), P(out)) == _capi.ERR_NOT_READY
    assert L.nlls_hess_block_diag(ctx.h, 0, 0.0, P(out)) == _capi.ERR_NOT_READY
    p = N.NLLSProblem(); a = p.addvariable([0.1, 0.2, 0.3]); b = p.addvariable([0.3, -0.2, 0.5])
    rng = np.random.default_rng(2)
    p.addcosts(K.RES_LINEAR3, [[a], [b], [a]], rng.standard_normal((3, 12)))
    p.addcosts(K.COST_LINEAR3, [[a]], rng.standard_normal((1, 3)))
    ctx.upload(p.var_kind, p.var_dim, blockindices(p), p.groups()); ctx.set_variables(p.variables)
    for args in ((None, P(out)), (P(v), None)):                                                                  # a null pointer
        assert L.nlls_hess_apply(ctx.h, 0, 0.0, 1, *args) == _capi.ERR_INVALID_ARG
        assert L.nlls_jac_apply(ctx.h, 0, 0, 1, *args) == _capi.ERR_INVALID_ARG
        assert L.nlls_jact_apply(ctx.h, 0, 0, 1, *args) == _capi.ERR_INVALID_ARG
    assert L.nlls_hess_block_diag(ctx.h, 0, 0.0, None) == _capi.ERR_INVALID_ARG
    for which in (-1, 3):                                                                                         # no such variable set
        assert L.nlls_hess_apply(ctx.h, which, 0.0, 1, P(v), P(out)) == _capi.ERR_INVALID_ARG
        assert L.nlls_jac_apply(ctx.h, which, 0, 1, P(v), P(out)) == _capi.ERR_INVALID_ARG
        assert L.nlls_jact_apply(ctx.h, which, 0, 1, P(v), P(out)) == _capi.ERR_INVALID_ARG
        assert L.nlls_hess_block_diag(ctx.h, which, 0.0, P(out)) == _capi.ERR_INVALID_ARG
    for bad in (-1, 2):                                                                                           # a bad group
        assert L.nlls_jac_apply(ctx.h, 0, bad, 1, P(v), P(out)) == _capi.ERR_INVALID_ARG
        assert L.nlls_jact_apply(ctx.h, 0, bad, 1, P(v), P(out)) == _capi.ERR_INVALID_ARG
    for nvec in (0, -1, _capi.APPLY_MAX_VEC + 1):
        assert L.nlls_hess_apply(ctx.h, 0, 0.0, nvec, P(v), P(out)) == _capi.ERR_INVALID_ARG
        assert L.nlls_jac_apply(ctx.h, 0, 0, nvec, P(v), P(out)) == _capi.ERR_INVALID_ARG
        assert L.nlls_jact_apply(ctx.h, 0, 0, nvec, P(v), P(out)) == _capi.ERR_INVALID_ARG
    for lam in (np.nan, np.inf, -np.inf):
        assert L.nlls_hess_apply(ctx.h, 0, lam, 1, P(v), P(out)) == _capi.ERR_INVALID_ARG
        assert L.nlls_hess_block_diag(ctx.h, 0, lam, P(out)) == _capi.ERR_INVALID_ARG
    assert L.nlls_jac_apply(ctx.h, 0, 1, 1, P(v), P(out)) == _capi.ERR_UNSUPPORTED                               # a non-squared cost kind has no residual
    assert L.nlls_jact_apply(ctx.h, 0, 1, 1, P(v), P(out)) == _capi.ERR_UNSUPPORTED
    assert out.tobytes() == sentinel.tobytes(), "a refused call wrote to an output"
    assert L.nlls_hess_apply(ctx.h, 0, 0.0, _capi.APPLY_MAX_VEC, P(v), P(out)) == _capi.OK and np.all(out[:48] != 7.25) and np.all(out[48:] == 7.25)
    with pytest.raises(_capi.NllsError):
        ctx.jac_apply(1, np.zeros(6))
    assert ctx.hess_apply(np.ones((19, 6))).shape == (19, 6)                                                     # more than eight vectors: split into calls
    ctx.close()
    # a dynamic-size group: no per-block Hessian, for the whole system; J of the other groups is still there
    ctx = _capi.Context(); out[:] = sentinel
    d = p.addvariable([1.0, 2.0, 3.0, 4.0], K.VAR_DYNAMIC)
    p.addcosts(K.COST_DYN_LINEAR, [[d]], rng.standard_normal((1, 4))); p.addcosts(K.RES_DYN_NORM, [[d]], np.zeros((1, 0)))
    ctx.upload(p.var_kind, p.var_dim, blockindices(p), p.groups()); ctx.set_variables(p.variables)
    assert L.nlls_hess_apply(ctx.h, 0, 0.0, 1, P(v), P(out)) == _capi.ERR_UNSUPPORTED
    assert L.nlls_hess_block_diag(ctx.h, 0, 0.0, P(out)) == _capi.ERR_UNSUPPORTED
    for dyn in (2, 3):
        assert L.nlls_jac_apply(ctx.h, 0, dyn, 1, P(v), P(out)) == _capi.ERR_UNSUPPORTED
        assert L.nlls_jact_apply(ctx.h, 0, dyn, 1, P(v), P(out)) == _capi.ERR_UNSUPPORTED
    assert out.tobytes() == sentinel.tobytes()
    assert L.nlls_jac_apply(ctx.h, 0, 0, 1, P(v), P(out)) == _capi.OK and np.all(out[:9] != 7.25) and np.all(out[9:] == 7.25)
    ctx.close()


def test_sharded_contexts_are_refused():
    """under nlls_set_shard(rank, nranks > 1): NLLS_ERR_UNSUPPORTED, nothing written (as tests/test_gpu_update.py::test_sharded_contexts_are_refused sets it up; a problem
    that shards -- bundle adjustment, block-sparse with an eliminated set -- keeps nranks = 2 on the context)"""
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3), 1e-3, 1e-3)
    c = _capi.Context(); P = _capi._p
    try:
        c.set_shard(0, 2); c.upload(p.var_kind, p.var_dim, blockindices(p), p.groups(), _capi.FLAG_FORCE_SPARSE); c.set_variables(p.variables)
        assert c.shard_info()["nranks"] == 2 and c.shard_info()["replicated"] == 0
        ndof = c.info.ndof; v = np.ones(ndof); (g,) = p.costs.values(); out = np.full(max(ndof, 2 * len(g)), 7.25); u = np.ones(2 * len(g))
        assert c.L.nlls_hess_apply(c.h, 0, 0.0, 1, P(v), P(out)) == _capi.ERR_UNSUPPORTED
        assert c.L.nlls_jac_apply(c.h, 0, 0, 1, P(v), P(out)) == _capi.ERR_UNSUPPORTED
        assert c.L.nlls_jact_apply(c.h, 0, 0, 1, P(u), P(out)) == _capi.ERR_UNSUPPORTED
        assert c.L.nlls_hess_block_diag(c.h, 0, 0.0, P(out)) == _capi.ERR_UNSUPPORTED
        assert np.all(out == 7.25)
    finally:
        c.close()


def test_empty_system_is_ok():
    """every variable fixed: ndof == 0, NLLS_OK and nothing written"""
    p = N.NLLSProblem(); a = p.addvariable([0.1, 0.2, 0.3])
    p.addcosts(K.RES_LINEAR3, [[a]], np.random.default_rng(2).standard_normal((1, 12)))
    ctx = upload(p, np.zeros(1, bool)); P = _capi._p; out = np.full(8, 7.25); v = np.ones(8)
    assert ctx.info.ndof == 0
    assert ctx.L.nlls_hess_apply(ctx.h, 0, 0.0, 1, P(v), P(out)) == _capi.OK and ctx.L.nlls_hess_block_diag(ctx.h, 0, 0.0, P(out)) == _capi.OK
    assert ctx.L.nlls_jac_apply(ctx.h, 0, 0, 1, P(v), P(out)) == _capi.OK and ctx.L.nlls_jact_apply(ctx.h, 0, 0, 1, P(v), P(out)) == _capi.OK
    assert np.all(out == 7.25)
    ctx.close()


# ---- 10. a user kind --------------------------------------------------------------------------------------------------------------------------------------
def test_user_kind_in_a_process_of_its_own():
    userlib = os.path.join(ROOT, "nllssolver.jl_amd", "csrc", "libnlls_amd_userdemo.so")
    env = dict(os.environ, NLLS_AMD_LIB=userlib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "apply_userkind_worker.py")], capture_output=True, text=True, env=env, timeout=600)
    print(out.stdout[-1500:])
    assert out.returncode == 0 and "user kind products ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
