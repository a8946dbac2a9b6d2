"""The matrix-free LM trial (csrc/nlls_mf.hip elimination, csrc/nlls_mfb.hip back-substitution; eligibility: build_mf in csrc/nlls_structure.cpp) across the
kernel shapes it branches on -- tile rows TR = ceil((nd+1)/16) 1..5, the right-hand-side column the last of a tile, members per batch and a partial
last batch, one cost block per member up to the 16 the gather index takes, the eliminated slot 0 or 1, one-dof blocks (no entries below the member's diagonal),
big supernodes (one workgroup) and tiny ones (one wavefront) in one launch -- on problems whose structure tests/helpers.structured_problem chooses.
Every case asserts the branch it was written for, then holds the step against an extended-precision reference: the normwise backward error with the
oracle's H and g (conditioning-free), the long-double Schur step, the materialised trial; and the trial's point, cost and statistics against the oracle.

Then call orders of the public API: a sequence of calls gives the same results whatever NLLS_OPT_MATERIALIZE is."""
import numpy as np
import pytest

from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import _capi
from oracle import oracle as O
from tests.helpers import oracle_problem, blockindices, structured_problem, check_structure, longdouble_backward_error, longdouble_schur_step, LD, bsm_coo, bsm_to_csr, _ld_sym_matvec

pytestmark = pytest.mark.gpu

U = np.finfo(np.float64).eps / 2
BA, RB = K.RES_BA_AFFINE, K.RES_ROSENBROCK_B

# (id, kind, runs [(blocks per eliminated variable, members in a row)], reduced variables, eliminated slot, trial expected matrix-free).  The matrix-free trial
# assembles through the slab + gather index, which build_schur makes for the block cyclic reduction of a narrow band (>= 128 reduced dof) and for supernodes of at
# most 16 neighbour blocks: the reduced systems here are bands of 144 (BA) and 160 (b (x^2 - y)) unknowns.
MF_CASES = (
    # BA (DP 3 / DC 6): TR 1..5 (ncb 1 -- a point seen by one camera: C_v singular without damping -- to 11); a tiny one-member and a partial batch beside a big run
    [(f"ba_ncb{n}", BA, [(n, 30), (n, 1), (n, 7)], 24, 1, True) for n in (1, 2, 3, 5, 6, 8, 10, 11)]
    # BA: members in a row around the batch sizes and the 128-member cap of a supernode (129: two supernodes)
    + [(f"ba_nmem{m}", BA, [(2, m), (3, 30)], 24, 1, True) for m in (1, 2, 7, 8, 9, 17, 63, 64, 65, 127, 128, 129)]
    # BA: big and tiny supernodes of every width in one launch
    + [("ba_mixed_a", BA, [(3, 100), (5, 1), (2, 9), (11, 64), (1, 2), (6, 129), (8, 4)], 24, 1, True),
       ("ba_mixed_b", BA, [(10, 33), (4, 3), (1, 70), (7, 17), (2, 1), (5, 128)], 24, 1, True)]
    # b (x^2 - y), DP = DC = 1 (no entries below a member's diagonal): the eliminated variable y (slot 1) or x (slot 0); ncb 15: nd + 1 = 16, the rhs column
    # the last of a tile; 16: TR 2
    + [(f"rb_ps{ps}_ncb{n}", RB, [(n, 40), (n, 3)], 160, ps, True) for ps in (1, 0) for n in (2, 15, 16)]
    # one block per member: the reduced system is diagonal (no band to reduce cyclically, no gather index) -- materialised
    # more than 16 cost blocks per member (nd + 1 = 32, 48, 64, 65, 66): the gather index takes at most 16 neighbour blocks per supernode, build_mf declines
    # and the trial is the materialised one -- which must hold the same accuracy
    + [(f"rb_ps{ps}_ncb{n}", RB, [(n, 40), (n, 3)], 160, ps, False) for ps in (1, 0) for n in (1, 31, 47, 63, 64, 65)]
)
SMALL_DAMPING = (("ba_small_lambda", BA, [(3, 40), (6, 30), (11, 9)], 24, 1, True), ("rb_small_lambda", RB, [(16, 60), (5, 20)], 160, 1, True))


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def _setup(kind, runs, nred, ps, monkeypatch, flags=0):
    monkeypatch.setenv("NLLS_SUPERNODE_PIECE", "128")           # (runs never cut into pieces: one supernode per run of up to 128 members)
    p, meta = structured_problem(kind, runs, nred, ps)
    op = oracle_problem(p); bi = blockindices(p); ols = op.linear_system(bi); c0 = ols.costgradhess()
    check_structure(ols, meta)                                  # (on the CPU first: the structure is the one intended)
    ctx = _capi.Context(); info = ctx.upload(p.var_kind, p.var_dim, bi, p.groups(), flags)
    assert info.is_sparse and info.has_schur and info.nschur_blocks == int(meta["elim_blocks"].sum()) and info.solve_mode in (1, 2), (info.solve_mode, info.nschur_blocks)
    ctx.set_variables(p.variables); ctx.set_variables(p.variables, _capi.VARS_NEXT)
    return p, meta, op, ols, c0, ctx


def _branch(ctx, st0, meta, expect_mf):
    st = ctx.solve_stats()
    assert st["mf_trials"] - st0["mf_trials"] == (1 if expect_mf else 0), "the trial did not take the path the case was written for"
    assert st["elim_supernodes"] == meta["supernodes"], (st["elim_supernodes"], meta["supernodes"])
    assert st["dropped_pivots"] == 0 and st["solve_mode"] in (1, 2), st
    assert st["status"] == 0, st


@pytest.mark.parametrize("name,kind,runs,nred,ps,expect_mf", MF_CASES, ids=[c[0] for c in MF_CASES])
def test_mf_trial_shapes_against_extended_precision(name, kind, runs, nred, ps, expect_mf, monkeypatch):
    p, meta, op, ols, c0, ctx = _setup(kind, runs, nred, ps, monkeypatch)
    try:
        ctx.sweep_gradhess()
        lam = ols.max_abs_diag() * 1e-6
        st0 = ctx.solve_stats()
        c_t = ctx.lm_trial(lam)
        _branch(ctx, st0, meta, expect_mf)
        x, v = ctx.get_step(), ctx.get_variables(_capi.VARS_NEXT); xHx, gx = ctx.quadform(); mx, nrm = ctx.step_maxabs(), ctx.step_norm()
        # two identical trials: the same bits (the matrix-free assembly has no atomics; the materialised one has)
        c_t2 = ctx.lm_trial(0.0)
        if expect_mf: assert c_t2 == c_t and np.array_equal(ctx.get_step(), x) and np.array_equal(ctx.get_variables(_capi.VARS_NEXT), v)
        else: assert np.isclose(c_t2, c_t, rtol=1e-9, atol=1e-13 * c0) and rel(ctx.get_step(), x) < 1e-9
        # the step: backward error against the oracle's H and g, the long-double Schur step, the materialised trial
        idx = ols.bsm_index()
        eta = longdouble_backward_error(ols.data, idx, ols.b, lam, x)
        assert eta <= 1e-13, f"backward error {eta:.3e}"
        x_ref, S = longdouble_schur_step(ols.data, idx, ols.b, lam, meta["elim_blocks"])
        # (the forward error a backward-stable step may have: u x cond of the reduced system.  Where S is formed by cancellation -- one block per member of b (x^2 - y):
        #  every reduced variable's curvature taken almost whole by its eliminated neighbours, a well-conditioned S of entries ~ lambda -- the whole damped system's
        #  conditioning enters instead: measured 2.6e-12 and 1.8e-11 against a cond(S) bound of 1e-12 there, with eta <= 1e-13)
        cond = np.linalg.cond(S)
        if kind == RB and all(n == 1 for n, _ in runs):
            cond = max(cond, np.linalg.cond(bsm_to_csr(idx, ols.data, len(ols.b)).toarray() + lam * np.eye(len(ols.b))))
        bound = max(1e-12, 1e2 * U * cond)
        assert rel(x, x_ref.astype(np.float64)) <= bound, (rel(x, x_ref.astype(np.float64)), bound)
        if expect_mf:
            ctx.set_option(_capi.OPT_MATERIALIZE, 1)
            st1 = ctx.solve_stats(); c_m = ctx.lm_trial(0.0)
            assert ctx.solve_stats()["mf_trials"] == st1["mf_trials"]
            assert rel(x, ctx.get_step()) < 1e-9 and np.isclose(c_m, c_t, rtol=1e-9, atol=1e-13 * c0)
            ctx.set_option(_capi.OPT_MATERIALIZE, 0)
        # the trial's point, cost and statistics against the oracle (src/iterators.jl:149-163)
        op.set_variables(p.variables, O.VARS_NEXT); op.update(ols, O.VARS_NEXT, O.VARS_CURRENT, step=x)
        assert rel(v, op.get_variables(O.VARS_NEXT)) < 1e-13
        assert np.isclose(c_t, op.cost(O.VARS_NEXT), rtol=1e-11, atol=1e-13 * c0), (c_t, op.cost(O.VARS_NEXT))
        I, J, V = bsm_coo(idx, ols.data, len(ols.b)); xl = x.astype(LD)
        xHx_ref = float(xl @ _ld_sym_matvec(I, J, V, xl, len(xl)) + LD(lam) * (xl @ xl)); gx_ref = float(ols.b.astype(LD) @ xl)
        assert np.isclose(xHx, xHx_ref, rtol=1e-11) and np.isclose(gx, gx_ref, rtol=1e-11), (xHx, xHx_ref, gx, gx_ref)
        assert mx == np.max(np.abs(x)) and np.isclose(nrm, np.linalg.norm(x), rtol=1e-12)
    finally:
        ctx.close()


@pytest.mark.parametrize("name,kind,runs,nred,ps,expect_mf", SMALL_DAMPING, ids=[c[0] for c in SMALL_DAMPING])
def test_mf_trial_small_damping_backward_error(name, kind, runs, nred, ps, expect_mf, monkeypatch):
    """lambda = 1e-10 max|diag| without the pivot floor: kappa far beyond what a tolerance on x can hold; the backward error still must be float64's."""
    p, meta, op, ols, c0, ctx = _setup(kind, runs, nred, ps, monkeypatch, flags=_capi.FLAG_NO_PIVOT_FLOOR)
    try:
        ctx.sweep_gradhess(); lam = ols.max_abs_diag() * 1e-10
        st0 = ctx.solve_stats(); ctx.lm_trial(lam)
        _branch(ctx, st0, meta, expect_mf)
        eta = longdouble_backward_error(ols.data, ols.bsm_index(), ols.b, lam, ctx.get_step())
        assert eta <= 1e-13, f"backward error {eta:.3e}"
    finally:
        ctx.close()


# ---- call orders: the same public calls on the matrix-free and on the materialised context ----------------------------------------------------------
CALL_ORDER = ("ba", BA, [(3, 60), (6, 30), (11, 9), (1, 5)], 24, 1)


def _contexts(monkeypatch, opt_before_upload=False):
    p, meta, op, ols, c0, ctx_mf = _setup(*CALL_ORDER[1:], monkeypatch)
    ctx_mat = _capi.Context()
    if opt_before_upload: ctx_mat.set_option(_capi.OPT_MATERIALIZE, 1)
    bi = blockindices(p); ctx_mat.upload(p.var_kind, p.var_dim, bi, p.groups())
    if not opt_before_upload: ctx_mat.set_option(_capi.OPT_MATERIALIZE, 1)
    ctx_mat.set_variables(p.variables); ctx_mat.set_variables(p.variables, _capi.VARS_NEXT)
    return p, op, ols, c0, ctx_mf, ctx_mat


@pytest.mark.parametrize("between", ["set_step", "sweep_cost", "set_next", "to_best"])
def test_trial_local_after_a_matrix_free_trial(between, monkeypatch):
    """lm_trial(NEXT, CURRENT), then set_step(x') / sweep_cost(NEXT) / set_variables(NEXT) / nothing, then trial_local(NEXT, CURRENT) (to_best: trial_local(BEST, CURRENT)):
    the tail of a trial of the step that is there NOW, into the set asked for -- the retraction of x' (of the trial's own step) and its cost, as the oracle's update and cost
    give them; the matrix-free context must not hand back the last trial's scalars nor leave the target unwritten."""
    p, op, ols, c0, ctx_mf, ctx_mat = _contexts(monkeypatch)
    try:
        lam = ols.max_abs_diag() * 1e-6
        rng = np.random.default_rng(3)
        to = _capi.VARS_BEST if between == "to_best" else _capi.VARS_NEXT
        out = {}
        for name, ctx in (("mf", ctx_mf), ("mat", ctx_mat)):
            ctx.set_variables(np.zeros_like(p.variables), _capi.VARS_BEST)
            ctx.sweep_gradhess(); n0 = ctx.solve_stats()["mf_trials"]          # (with the cost: A and b whole, trial_local sweeps nothing)
            ctx.lm_trial(lam)
            assert ctx.solve_stats()["mf_trials"] - n0 == (1 if name == "mf" else 0)
            x = ctx.get_step(); xp = x
            if between == "set_step":
                xp = x * (1 + 0.5 * rng.standard_normal(x.size)) if name == "mf" else out["mf"][2]
                ctx.set_step(xp)
            elif between == "sweep_cost":
                ctx.sweep_cost(_capi.VARS_NEXT)
            if between != "to_best":
                ctx.set_variables(np.zeros_like(p.variables), _capi.VARS_NEXT)      # (what the tail leaves there must be its own work)
            t = ctx.trial_local(to, _capi.VARS_CURRENT)
            out[name] = (t, ctx.get_variables(to), xp)
        for name in ("mf", "mat"):
            t, v, xp = out[name]
            op.set_variables(p.variables, O.VARS_NEXT); op.update(ols, O.VARS_NEXT, O.VARS_CURRENT, step=xp)
            assert rel(v, op.get_variables(O.VARS_NEXT)) < 1e-13, name
            assert np.isclose(t[0], op.cost(O.VARS_NEXT), rtol=1e-11, atol=1e-13 * c0), (name, t[0], op.cost(O.VARS_NEXT))
            assert t[3] == np.max(np.abs(xp)), name
        assert np.isclose(out["mf"][0][0], out["mat"][0][0], rtol=1e-9, atol=1e-13 * c0) and rel(out["mf"][1], out["mat"][1]) < 1e-11
    finally:
        ctx_mf.close(); ctx_mat.close()


def test_materialize_option_survives_an_upload(monkeypatch):
    """set_option(MATERIALIZE, 1) before the upload, and a re-upload on the same context: every trial materialised (the option is the caller's, not the upload's)."""
    p, op, ols, c0, ctx_mf, ctx_mat = _contexts(monkeypatch, opt_before_upload=True)
    try:
        lam = ols.max_abs_diag() * 1e-6
        for rep in range(2):
            if rep: ctx_mat.upload(p.var_kind, p.var_dim, blockindices(p), p.groups()); ctx_mat.set_variables(p.variables)
            ctx_mat.sweep_gradhess(); ctx_mat.lm_trial(lam)
            assert ctx_mat.solve_stats()["mf_trials"] == 0, f"upload {rep}: a matrix-free trial on a context set to materialise"
            ctx_mf.sweep_gradhess(); ctx_mf.lm_trial(lam)
            assert rel(ctx_mf.get_step(), ctx_mat.get_step()) < 1e-9
    finally:
        ctx_mf.close(); ctx_mat.close()


@pytest.mark.parametrize("want_cost", [True, False])
def test_writing_current_between_the_sweep_and_the_trial(want_cost, monkeypatch):
    """sweep_gradhess, then set_variables(new, CURRENT), then lm_trial: the linear system is the one formed at the sweep (A and b of the old point), the step is
    retracted from the NEW point -- on both paths, also when sweep_gradhess(NULL) deferred the sweep (the matrix-free path forms the linearisation on demand)."""
    p, op, ols, c0, ctx_mf, ctx_mat = _contexts(monkeypatch)
    try:
        lam = ols.max_abs_diag() * 1e-6
        new = p.variables + 1e-3 * np.random.default_rng(7).standard_normal(p.variables.size)
        out = {}
        for name, ctx in (("mf", ctx_mf), ("mat", ctx_mat)):
            ctx.sweep_gradhess(want_cost=want_cost)
            ctx.set_variables(new)
            c = ctx.lm_trial(lam)
            out[name] = (c, ctx.get_step(), ctx.get_variables(_capi.VARS_NEXT))
        assert ols.solve(lam) == 0
        op.set_variables(new, O.VARS_CURRENT); op.set_variables(new, O.VARS_NEXT); op.update(ols, O.VARS_NEXT, O.VARS_CURRENT, step=ols.x)
        for name in ("mf", "mat"):
            c, x, v = out[name]
            assert rel(x, ols.x) < 1e-7, (name, rel(x, ols.x))
            assert rel(v, op.get_variables(O.VARS_NEXT)) < 1e-9, name
            assert np.isclose(c, op.cost(O.VARS_NEXT), rtol=1e-9, atol=1e-13 * c0), (name, c, op.cost(O.VARS_NEXT))
        assert np.isclose(out["mf"][0], out["mat"][0], rtol=1e-9, atol=1e-13 * c0) and rel(out["mf"][1], out["mat"][1]) < 1e-9
    finally:
        ctx_mf.close(); ctx_mat.close()


# what nlls_lm_iterations does on the call-order problem, counted: the fixes of the call orders above add no sweep, no trial and no look-ahead miss to the loop
# (measured on the library of commit 7ed373c, before the fixes of the call orders above, with this test as it stands: six nlls_lm_iterations on CALL_ORDER's problem.
#  A later change of the look-ahead policy changes these counts on purpose: measure them again on the parent of that change)
LOOP_COUNTERS = dict(full_sweeps=1, reduced_sweeps=4, lookahead_hits=2, lookahead_misses=0, mf_trials=4, iternum=4, linearsolvers=4, gradientcomputations=3)


def test_lm_loop_counters_are_unchanged(monkeypatch):
    p, op, ols, c0, ctx_mf, ctx_mat = _contexts(monkeypatch)
    ctx_mat.close()
    try:
        ctx = ctx_mf; c = ctx.sweep_gradhess()
        opt = _capi.LmOptions(reldcost=1e-15, absdcost=1e-15, dstep=1e-15, maxfails=3, maxiters=100, stoptime_ns=0)
        st = _capi.LmState(); st.bestcost = c; st.cost = c
        ctx.lm_iterations(opt, st, 6)
        s = ctx.solve_stats()
        got = dict(full_sweeps=s["full_sweeps"], reduced_sweeps=s["reduced_sweeps"], lookahead_hits=s["lookahead_hits"], lookahead_misses=s["lookahead_misses"],
                   mf_trials=s["mf_trials"], iternum=int(st.iternum), linearsolvers=int(st.linearsolvers), gradientcomputations=int(st.gradientcomputations))
        print("lm loop counters", got)
        assert got == LOOP_COUNTERS, got
    finally:
        ctx_mf.close()
