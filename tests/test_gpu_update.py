"""nlls_set_cost_data / nlls_set_robust_params: the cost blocks' data and a group's robust parameters changed on an uploaded structure (include/nlls_amd.h;
csrc/nlls_update.hip), and N.Solver on top of them.

Every case uploads with data d0, warms the paths (cost sweep, per-block values, gradient sweep, one LM trial), updates to d1 -- an O(1) change of every updated
record -- and holds what the SAME context then computes against
  (a) the CPU oracle built with d1: cost, A.data and b to 1e-11 (RTOL of tests/test_gpu_parity.py::check_problem), and
  (b) a fresh context uploaded with d1 and driven through the same calls: the cost sweep and nlls_eval_blocks bit for bit (fixed-order sums, per-block values), the
      trial's cost and point to 1e-9 (trials are reproducible to rounding, not to the bit: notes/r08.md).
The payload lies in up to four device copies in different orders; a copy the update missed would give the d0 value.  So every case also asserts that the d1 results
differ from the d0 results by at least 1e3 x the tolerance of the comparison (1e-8 for the sweeps, 1e-6 for the trial) -- except A.data where it cannot depend on
the data (a residual linear in its measurement without a robust kernel: J'J does not see the measurement), which the case states."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import synthetic, _capi
from oracle import oracle as O
from tests.helpers import oracle_problem, blockindices, structured_problem

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL, RTOL_TRIAL = 1e-11, 1e-9
CUR, NEXT = _capi.VARS_CURRENT, _capi.VARS_NEXT
MIXED_A = [(3, 100), (5, 1), (2, 9), (11, 64), (1, 2), (6, 129), (8, 4)]        # tests/test_gpu_mf_shapes.py: ba_mixed_a


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def shifted(da, rng):
    """d1: every entry of every record moved by 0.5 .. 1.5 in either direction"""
    return da + rng.uniform(0.5, 1.5, da.shape) * rng.choice([-1.0, 1.0], da.shape)


def with_data(p, group, da):
    """the problem's description with one group's data replaced (the problem itself is left alone)"""
    gs = p.groups(); gs[group] = dict(gs[group], data=np.ascontiguousarray(da)); return gs


def upload(p, groups, bi, flags=0, variables=None):
    ctx = _capi.Context(); ctx.upload(p.var_kind, p.var_dim, bi, groups, flags)
    ctx.set_variables(p.variables if variables is None else variables)
    return ctx


def eval_groups(groups):
    return [g for g, d in enumerate(groups) if d["res_kind"] not in (K.COST_LINEAR3, K.COST_DYN_LINEAR)]


def drive(ctx, groups, lam=None, lam_scale=1e-6):
    """the calls every context of a case goes through: cost sweep, per-block values, gradient sweep (A.data, b), one LM trial"""
    out = dict(cost=ctx.sweep_cost(), ev=[ctx.eval_blocks(g) for g in eval_groups(groups)])
    out["c_gh"] = ctx.sweep_gradhess(); out["A"] = ctx.get_bsm_data(); out["b"] = ctx.get_grad()
    lam = ctx.max_abs_diag() * lam_scale if lam is None else lam
    mf0 = ctx.solve_stats()["mf_trials"]
    out["c_trial"] = ctx.lm_trial(lam); out["mf"] = ctx.solve_stats()["mf_trials"] - mf0
    out["v"] = ctx.get_variables(NEXT); out["x"] = ctx.get_step()
    return out


def oracle_of(p, groups, bi, flags, lam_scale):
    op = O.OracleProblem(p.var_kind, p.var_dim, groups); op.set_variables(p.variables)
    ols = op.linear_system(bi, flags & _capi.FLAG_FORCE_SPARSE); c = ols.costgradhess(); A = ols.data.copy()
    if not ols.info.is_sparse:          # (the device mirrors the lower triangle at the end of the sweep: check_problem)
        n = ols.info.ndof; M = A.reshape(n, n).T; M = np.tril(M) + np.tril(M, -1).T; A = M.T.ravel()
    return dict(cost=op.cost(), c_gh=c, A=A, b=ols.b.copy(), lam=ols.max_abs_diag() * lam_scale)


def same_as_fresh(u, f):
    assert u["cost"] == f["cost"], (u["cost"], f["cost"])
    for eu, ef in zip(u["ev"], f["ev"]):
        for k in ("r", "sqerr", "rho", "weight"):
            assert np.array_equal(eu[k], ef[k], equal_nan=True), k
    assert u["mf"] == f["mf"]
    print(f"TRIAL cost {u['c_trial']:.17g} / {f['c_trial']:.17g}  point {rel(u['v'], f['v']):.3e}")
    assert np.isclose(u["c_trial"], f["c_trial"], rtol=RTOL_TRIAL, atol=1e-300), (u["c_trial"], f["c_trial"])
    assert rel(u["v"], f["v"]) < RTOL_TRIAL, rel(u["v"], f["v"])


def same_as_oracle(u, o):
    print(f"ORACLE cost {abs(u['cost'] - o['cost']) / abs(o['cost']):.3e} A {rel(u['A'], o['A']):.3e} b {rel(u['b'], o['b']):.3e}")
    assert np.isclose(u["cost"], o["cost"], rtol=RTOL, atol=1e-300) and np.isclose(u["c_gh"], o["c_gh"], rtol=RTOL, atol=1e-300)
    assert rel(u["A"], o["A"]) < RTOL, "A.data mismatch"
    assert rel(u["b"], o["b"]) < RTOL, "b mismatch"


def moved(u, base, a_moves, evpos=0):
    """a stale copy of the data would have failed the comparisons above: the d0 results are at least 1e3 tolerances away (evpos: the updated group among the evaluated ones)"""
    assert abs(u["cost"] - base["cost"]) >= 1e3 * RTOL * abs(u["cost"]) and abs(u["c_gh"] - base["c_gh"]) >= 1e3 * RTOL * abs(u["c_gh"])
    assert rel(base["b"], u["b"]) >= 1e3 * RTOL
    if a_moves:
        assert rel(base["A"], u["A"]) >= 1e3 * RTOL
    eu, eb = u["ev"][evpos], base["ev"][evpos]
    assert rel(eb["r"], eu["r"]) >= 1e3 * RTOL and rel(eb["sqerr"], eu["sqerr"]) >= 1e3 * RTOL
    assert abs(u["c_trial"] - base["c_trial"]) >= 1e3 * RTOL_TRIAL * abs(u["c_trial"]) and rel(base["v"], u["v"]) >= 1e3 * RTOL_TRIAL


def run_case(p, group=0, unfixed=None, flags=0, lam_scale=1e-6, a_moves=False, expect_mf=None, seed=5):
    """d0 -> d1 for the whole of one group; returns the warmed-and-updated context's results"""
    bi = blockindices(p, unfixed); g0 = p.groups(); rng = np.random.default_rng(seed)
    d1 = shifted(g0[group]["data"], rng); g1 = with_data(p, group, d1)
    ctx = upload(p, g0, bi, flags)
    try:
        base = drive(ctx, g0, None, lam_scale)
        vc, vn = ctx.get_variables(CUR), ctx.get_variables(NEXT); mem = ctx.memory_info()
        ctx.set_cost_data(group, d1)
        assert np.array_equal(ctx.get_variables(CUR), vc) and np.array_equal(ctx.get_variables(NEXT), vn)
        assert ctx.memory_info()["working_set_bytes"] == mem["working_set_bytes"]
        ora = oracle_of(p, g1, bi, flags, lam_scale)
        ctx.set_variables(np.zeros_like(vn), NEXT)            # (whatever the trial leaves there must be its own work)
        u = drive(ctx, g1, ora["lam"])
    finally:
        ctx.close()
    fr = upload(p, g1, bi, flags)
    try:
        f = drive(fr, g1, ora["lam"])
    finally:
        fr.close()
    same_as_fresh(u, f); same_as_oracle(u, ora); moved(u, base, a_moves, eval_groups(g0).index(group))
    if expect_mf is not None:
        assert u["mf"] == expect_mf and base["mf"] == expect_mf, (u["mf"], base["mf"])
    return u


def mf_problem(monkeypatch, robust=None, noise=0.0, seed=0):
    monkeypatch.setenv("NLLS_SUPERNODE_PIECE", "128")
    p, meta = structured_problem(K.RES_BA_AFFINE, MIXED_A, 24, 1, seed=seed)
    if robust is not None or noise:
        (g,) = p.costs.values(); vi, da = g.arrays()
        q = N.NLLSProblem(); q.copy_variables_from(p)
        q.addcosts(K.RES_BA_AFFINE, vi, da + noise * np.random.default_rng(seed + 7).standard_normal(da.shape), robust)
        p = q
    return p


# ---- the matrix-free BA: mf_data, both entry lists, the cost list ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,expect_mf", [(0, 1), (_capi.FLAG_MATERIALIZE, 0)], ids=["matrix_free", "materialize"])
def test_matrix_free_ba(flags, expect_mf, monkeypatch):
    """big and tiny supernodes and a run cut at 128 members.  A.data does not move: the affine residual is linear in its measurement and there is no kernel."""
    run_case(mf_problem(monkeypatch), flags=flags, expect_mf=expect_mf)


# Values of nlls_get_memory_info for this problem (NLLS_SUPERNODE_PIECE=128, flags 0) measured on the PARENT commit (d83801e, the library built from a checkout of it):
# a context that never updates allocates what it did before.
PARENT_MEMORY_INFO = dict(working_set_bytes=1141760, arena_bytes=67960594, a_data_bytes=293400, reduced_system_bytes=85928, sharded_reduce_bytes=85928)


def test_memory_of_a_context_that_never_updates(monkeypatch):
    p = mf_problem(monkeypatch); bi = blockindices(p)
    ctx = upload(p, p.groups(), bi)
    try:
        m0 = ctx.memory_info(); print("MEMORY_INFO", m0)
        assert PARENT_MEMORY_INFO is not None and m0 == PARENT_MEMORY_INFO, (m0, PARENT_MEMORY_INFO)
        ctx.set_cost_data(0, p.groups()[0]["data"]); ctx.sweep_cost()
        assert ctx.memory_info() == m0                               # the maps and the staging lie outside the arena: hot_bytes and the rest as before
    finally:
        ctx.close()


# ---- indexed updates ---------------------------------------------------------------------------------------------------------------------------------
def _index_sets(n, rng):
    some = np.unique(np.r_[0, n - 1, rng.choice(n, int(0.37 * n), replace=False)])
    return dict(frac37=rng.permutation(some), single=np.array([n // 3]), none=np.zeros(0, np.int64), shuffled_all=rng.permutation(n))


@pytest.mark.parametrize("which", ["frac37", "single", "none", "shuffled_all"])
def test_indexed_updates(which, monkeypatch):
    p = mf_problem(monkeypatch); bi = blockindices(p); g0 = p.groups(); d0 = g0[0]["data"]; n = d0.shape[0]; rng = np.random.default_rng(21)
    idx = _index_sets(n, rng)[which]; rows = shifted(d0[idx], rng)
    d1 = d0.copy(); d1[idx] = rows; g1 = with_data(p, 0, d1)
    ctx = upload(p, g0, bi)
    try:
        base = drive(ctx, g0); ev0 = base["ev"][0]
        ctx.set_cost_data(0, rows, idx + 1)
        if which == "none":                         # nothing changes, the state included: the linearisation is still held
            assert np.isclose(ctx.lm_trial(0.0), base["c_trial"], rtol=RTOL_TRIAL)
            assert ctx.sweep_cost() == base["cost"]
            for k in ev0: assert np.array_equal(ctx.eval_blocks(0)[k], ev0[k])
            return
        ev1 = ctx.eval_blocks(0); keep = np.ones(n, bool); keep[idx] = False
        for k in ev0:
            assert np.array_equal(ev1[k][keep], ev0[k][keep]), f"{k}: an untouched block changed"
        assert np.all(ev1["sqerr"][idx] != ev0["sqerr"][idx])
        ora = oracle_of(p, g1, bi, 0, 1e-6)
        u = drive(ctx, g1, ora["lam"])
    finally:
        ctx.close()
    fr = upload(p, g1, bi)
    try:
        f = drive(fr, g1, ora["lam"])
    finally:
        fr.close()
    same_as_fresh(u, f); same_as_oracle(u, ora)
    assert u["mf"] == 1
    assert abs(u["cost"] - base["cost"]) >= 1e3 * RTOL * abs(u["cost"]) and rel(base["b"], u["b"]) >= 1e3 * RTOL


def test_bad_indices_are_refused_and_change_nothing(monkeypatch):
    p = mf_problem(monkeypatch); bi = blockindices(p); g0 = p.groups(); d0 = g0[0]["data"]; n = d0.shape[0]
    ctx = upload(p, g0, bi)
    try:
        base = drive(ctx, g0); junk = np.full((3, 2), 1e6)
        for bad in ([1, 2, 2], [0, 1, 2], [1, 2, n + 1], [-1, 2, 3]):
            with pytest.raises(_capi.NllsError) as e:
                ctx.set_cost_data(0, junk, np.array(bad))
            assert e.value.code == _capi.ERR_INVALID_ARG, bad
        L = ctx.L; big = np.zeros((n + 1, 2))
        assert L.nlls_set_cost_data(ctx.h, 0, n + 1, None, _capi._p(big)) == _capi.ERR_INVALID_ARG
        assert L.nlls_set_cost_data(ctx.h, 0, -1, None, _capi._p(big)) == _capi.ERR_INVALID_ARG
        assert L.nlls_set_cost_data(ctx.h, 0, 2, None, None) == _capi.ERR_INVALID_ARG
        for g in (-1, 1, 7):
            assert L.nlls_set_cost_data(ctx.h, g, 1, None, _capi._p(big)) == _capi.ERR_INVALID_ARG
            assert L.nlls_set_robust_params(ctx.h, g, _capi._p(np.zeros(4))) == _capi.ERR_INVALID_ARG
        assert L.nlls_set_robust_params(ctx.h, 0, None) == _capi.ERR_INVALID_ARG
        # ... and the context still gives the d0 results, the linearisation still held
        c = ctx.lm_trial(0.0)
        assert np.isclose(c, base["c_trial"], rtol=RTOL_TRIAL)
        assert ctx.sweep_cost() == base["cost"]
        ev = ctx.eval_blocks(0)
        for k in ev: assert np.array_equal(ev[k], base["ev"][0][k])
    finally:
        ctx.close()


# ---- fixed variables: blocks absent from some copies -----------------------------------------------------------------------------------------------------
def _fixed_problem():
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 60, 0.4, seed=6), 1e-3, 1e-3)      # tests/test_gpu_parity.py::test_ba_fixed_variables
    unfixed = np.ones(p.nvariables, bool); unfixed[[0, 3, 15, 16, 40]] = False
    return p, unfixed


def test_fixed_variables():
    p, unfixed = _fixed_problem()
    vi = p.groups()[0]["varind"]; allfixed = ~unfixed[vi[:, 0] - 1] & ~unfixed[vi[:, 1] - 1]
    assert allfixed.sum() >= 1 and (~unfixed[vi - 1]).any(axis=1).sum() > allfixed.sum()      # blocks in the cost-order copy alone, and blocks missing from one list
    run_case(p, unfixed=unfixed)
    # the all-fixed blocks alone: only their cost moves, and it must
    bi = blockindices(p, unfixed); g0 = p.groups(); d0 = g0[0]["data"]; idx = np.nonzero(allfixed)[0]; rng = np.random.default_rng(3)
    d1 = d0.copy(); d1[idx] = shifted(d0[idx], rng)
    ctx = upload(p, g0, bi)
    try:
        c0 = ctx.sweep_cost(); ev0 = ctx.eval_blocks(0); ctx.sweep_gradhess(); b0 = ctx.get_grad()
        ctx.set_cost_data(0, d1[idx], idx + 1)
        c1 = ctx.sweep_cost(); ev1 = ctx.eval_blocks(0); ctx.sweep_gradhess(); b1 = ctx.get_grad()
    finally:
        ctx.close()
    fr = upload(p, with_data(p, 0, d1), bi)
    try:
        assert c1 == fr.sweep_cost() and abs(c1 - c0) >= 1e3 * RTOL * c1
        assert np.isclose(c1 - c0, 0.5 * (ev1["rho"][idx].sum() - ev0["rho"][idx].sum()), rtol=1e-9)
        keep = ~allfixed
        for k in ev0: assert np.array_equal(ev1[k][keep], ev0[k][keep])
        assert rel(b1, b0) < RTOL            # no free variable sees them
    finally:
        fr.close()


# ---- the folded three-slot sweep ------------------------------------------------------------------------------------------------------------------------
def test_folded_three_slot_sweep():
    """the smallest so3_adaptive shape of check_problem (tests/test_gpu_parity.py::test_so3_ba).  A.data moves: the kernel's weights depend on the residual."""
    q = synthetic.perturb_ba_problem(synthetic.create_so3_ba_problem(8, 60, 0.5, seed=2, adaptive=True), 1e-3, 1e-3)
    run_case(q, lam_scale=1e-4, a_moves=True)


# ---- dense routes ---------------------------------------------------------------------------------------------------------------------------------------
def test_small_dense_curve_fit():
    c, _ = synthetic.create_curvefit_problem(200, seed=1)
    run_case(c, a_moves=True)            # (data = (t, y): the Jacobian depends on t)


def test_small_dense_rosenbrock():
    p = N.NLLSProblem(); p.addvariable(-0.5); p.addvariable(2.5)
    p.addcosts(K.RES_ROSENBROCK_A, [[1]], [[1.0]], N.Scaled(N.Huber2oKernel(1.6), 1.0))
    p.addcosts(K.RES_ROSENBROCK_B, [[1, 2]], [[10.0]])
    run_case(p, group=1, lam_scale=1e-3, a_moves=True)


# ---- dynamic-size kinds: the dense list in both forms, short and long records --------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,nv", [(K.RES_DYN_LINEAR, 5, 6), (K.RES_DYN_LINEARSQ, 3, 6), (K.RES_DYN_LINEARSQ, 70, 2)], ids=["linear5", "linearsq3", "linearsq70"])
@pytest.mark.parametrize("flags", [0, _capi.FLAG_FORCE_SPARSE], ids=["dense", "force_sparse"])
def test_dynamic_kinds(kind, n, nv, flags):
    """linearsq70: one record is 70 + 70 * 70 = 4970 doubles, the wavefront-per-chunk regime of the scatter; the others one lane per record.
    Under NLLS_FLAG_FORCE_SPARSE the short variables get company: blocks of at most NLLS_MAX_BLOCK_SZ unknowns are candidates for elimination, nv blocks of one size without
    a neighbour would ALL be eliminated and leave a reduced system of no unknowns.  Seven more dynamic variables of seven other lengths keep every size class below half of
    the blocks, so nothing is eliminated (as in tests/test_gpu_functional.py's all-dynamic shape) and the group under test is the block-sparse DenseList form."""
    r = np.random.default_rng(12); p = N.NLLSProblem()
    for v in range(nv):
        p.addvariable(0.3 * r.standard_normal(n), K.VAR_DYNAMIC)
    idx = np.arange(1, nv + 1)[:, None]
    if kind == K.RES_DYN_LINEAR:
        X = r.standard_normal((nv, n)); p.addcosts(kind, idx, np.concatenate([np.ones((nv, 1)), X], axis=1))
    else:
        Xs = r.standard_normal((nv, n * n)) / np.sqrt(n); p.addcosts(kind, idx, np.concatenate([r.standard_normal((nv, n)), Xs], axis=1), N.HuberKernel(0.7))
    p.addcosts(K.RES_DYN_NORM, idx, np.zeros((nv, 0)))
    if flags and n <= 32:
        for m in range(12, 19):
            v = p.addvariable(0.3 * r.standard_normal(m), K.VAR_DYNAMIC); X = r.standard_normal(m)
            p.addcosts(K.RES_DYN_LINEAR, [[v]], np.concatenate([[1.0], X / np.linalg.norm(X)])[None, :]); p.addcosts(K.RES_DYN_NORM, [[v]], np.zeros((1, 0)))
    assert p.groups()[0]["data"].shape[1] == {K.RES_DYN_LINEAR: 1 + n, K.RES_DYN_LINEARSQ: n + n * n}[kind]
    u = run_case(p, flags=flags, lam_scale=1e-4, a_moves=True)
    if not flags:
        assert u["A"].size == (n * nv) ** 2          # the dense system


# ---- robust parameters ------------------------------------------------------------------------------------------------------------------------------------
def run_robust_case(p, new_robust, flags, expect_mf, lam_scale=1e-6):
    bi = blockindices(p); g0 = p.groups()
    g1 = [dict(g0[0], robust_kind=new_robust.kind, robust_params=new_robust.params)]
    ctx = upload(p, g0, bi, flags)
    try:
        base = drive(ctx, g0, None, lam_scale); vc, vn = ctx.get_variables(CUR), ctx.get_variables(NEXT)
        ctx.set_robust_params(0, new_robust)
        assert np.array_equal(ctx.get_variables(CUR), vc) and np.array_equal(ctx.get_variables(NEXT), vn)
        assert ctx.L.nlls_lm_trial(ctx.h, 0.0, NEXT, CUR, None) == _capi.ERR_NOT_READY
        ora = oracle_of(p, g1, bi, flags, lam_scale)
        u = drive(ctx, g1, ora["lam"])
    finally:
        ctx.close()
    fr = upload(p, g1, bi, flags)
    try:
        f = drive(fr, g1, ora["lam"])
    finally:
        fr.close()
    same_as_fresh(u, f); same_as_oracle(u, ora)
    assert u["mf"] == expect_mf
    # the residuals do not move, what the kernel makes of them does
    assert abs(u["cost"] - base["cost"]) >= 1e3 * RTOL * abs(u["cost"]) and rel(base["b"], u["b"]) >= 1e3 * RTOL and rel(base["A"], u["A"]) >= 1e3 * RTOL
    assert np.array_equal(u["ev"][0]["r"], base["ev"][0]["r"]) and rel(base["ev"][0]["rho"], u["ev"][0]["rho"]) >= 1e3 * RTOL
    assert abs(u["c_trial"] - base["c_trial"]) >= 1e3 * RTOL_TRIAL * abs(u["c_trial"])


@pytest.mark.parametrize("flags,expect_mf", [(0, 1), (_capi.FLAG_MATERIALIZE, 0)], ids=["matrix_free", "materialize"])
@pytest.mark.parametrize("old,new", [(N.HuberKernel(0.05), N.HuberKernel(0.01)), (N.Scaled(N.HuberKernel(0.03), 2.0), N.Scaled(N.HuberKernel(0.03), 0.5))], ids=["huber_width", "scaled_height"])
def test_robust_parameters(old, new, flags, expect_mf, monkeypatch):
    """measurement noise of 0.05 around widths of 0.01 .. 0.05: blocks on both sides of every width"""
    run_robust_case(mf_problem(monkeypatch, robust=old, noise=0.05), new, flags, expect_mf)


def test_robust_parameters_refusals():
    q = synthetic.create_so3_ba_problem(8, 60, 0.5, seed=2, adaptive=True); bi = blockindices(q)
    ctx = upload(q, q.groups(), bi)
    try:
        c0 = ctx.sweep_gradhess()
        with pytest.raises(_capi.NllsError) as e:
            ctx.set_robust_params(0, (1.0, 0, 0, 0))                 # an adaptive group: its kernel is a variable
        assert e.value.code == _capi.ERR_INVALID_ARG
        with pytest.raises(_capi.NllsError) as e:
            ctx.set_robust_params(1, (1.0, 0, 0, 0))
        assert e.value.code == _capi.ERR_INVALID_ARG
        ctx.lm_trial(1e-3 * ctx.max_abs_diag())                      # nothing changed: the linearisation is still held
    finally:
        ctx.close()


def test_user_robust_kernel_in_a_process_of_its_own():
    lib = os.path.join(ROOT, "nllssolver.jl_amd", "csrc", "libnlls_amd_userrobust.so")
    env = dict(os.environ, NLLS_AMD_LIB=lib, NLLS_SUPERNODE_PIECE="128")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "update_userrobust_worker.py")], capture_output=True, text=True, env=env, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "update user robust ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


# ---- state -----------------------------------------------------------------------------------------------------------------------------------------------
def test_consumers_of_the_linearisation_are_refused_until_the_next_sweep(monkeypatch):
    """after either call the context is where an upload without a sweep leaves it: whatever nlls_lm_trial, nlls_solve, nlls_get_grad, nlls_damp return there"""
    p = mf_problem(monkeypatch, robust=N.HuberKernel(0.05), noise=0.05); bi = blockindices(p); g0 = p.groups()
    def consumers(c):
        L, x = c.L, np.zeros(c.info.ndof)
        return (L.nlls_lm_trial(c.h, 0.0, NEXT, CUR, None), L.nlls_solve(c.h, None), L.nlls_get_grad(c.h, _capi._p(x)), L.nlls_damp(c.h, 1.0), L.nlls_max_abs_diag(c.h, None))
    fresh = upload(p, g0, bi)
    try:
        unswept = consumers(fresh)
    finally:
        fresh.close()
    assert unswept == (_capi.ERR_NOT_READY,) * 5
    ctx = upload(p, g0, bi)
    try:
        for change in (lambda: ctx.set_cost_data(0, g0[0]["data"] + 1.0), lambda: ctx.set_robust_params(0, N.HuberKernel(0.02))):
            drive(ctx, g0); st = ctx.solve_stats()
            change()
            assert consumers(ctx) == unswept
            s2 = ctx.solve_stats()
            assert all(s2[k] == st[k] for k in ("lookahead_hits", "lookahead_misses", "mf_trials", "reduced_sweeps", "full_sweeps"))
            # the entry points that need no sweep see the new costs at once
            assert np.isfinite(ctx.sweep_cost()) and ctx.eval_blocks(0)["sqerr"].shape[0] == g0[0]["data"].shape[0]
    finally:
        ctx.close()
    # before a successful upload: NLLS_ERR_NOT_READY
    c = _capi.Context()
    try:
        assert c.L.nlls_set_cost_data(c.h, 0, 1, None, _capi._p(np.zeros(2))) == _capi.ERR_NOT_READY
        assert c.L.nlls_set_robust_params(c.h, 0, _capi._p(np.zeros(4))) == _capi.ERR_NOT_READY
        c.set_shard(0, 2)
        assert c.L.nlls_set_cost_data(c.h, 0, 1, None, _capi._p(np.zeros(2))) == _capi.ERR_NOT_READY
    finally:
        c.close()


def test_sharded_contexts_are_refused():
    """under nlls_set_shard(rank, nranks > 1): NLLS_ERR_UNSUPPORTED before anything changes (a dense system runs as a replica: the context is ready without a collective)"""
    p = N.NLLSProblem(); p.addvariable(-0.5); p.addvariable(2.5)
    p.addcosts(K.RES_ROSENBROCK_B, [[1, 2]], [[10.0]], N.HuberKernel(1.0))
    c = _capi.Context()
    try:
        c.set_shard(0, 2); c.upload(p.var_kind, p.var_dim, blockindices(p), p.groups()); c.set_variables(p.variables)
        c0 = c.sweep_cost()
        assert c.L.nlls_set_cost_data(c.h, 0, 1, None, _capi._p(np.array([3.0]))) == _capi.ERR_UNSUPPORTED
        assert c.L.nlls_set_robust_params(c.h, 0, _capi._p(np.array([0.1, 0, 0, 0]))) == _capi.ERR_UNSUPPORTED
        assert c.sweep_cost() == c0
    finally:
        c.close()


def _lm(ctx, state, n):
    opt = _capi.LmOptions(1e-15, 1e-15, 1e-15, 3, 1000, 0)
    ctx.lm_iterations(opt, state, n)


def test_update_between_lm_iterations(monkeypatch):
    """three iterations and a trial (its look-ahead sweep pending), the update, three more: a fresh d1 context started from the same variables and LM state does the same"""
    p = mf_problem(monkeypatch, robust=N.HuberKernel(0.05), noise=0.05); bi = blockindices(p); g0 = p.groups(); d1 = shifted(g0[0]["data"], np.random.default_rng(8)); g1 = with_data(p, 0, d1)
    ctx = upload(p, g0, bi)
    try:
        st = _capi.LmState(); st.bestcost = st.cost = ctx.sweep_gradhess()
        _lm(ctx, st, 3)
        assert st.iternum == 3 and st.converged == 0
        ctx.lm_trial(st.lambda_)                               # (a look-ahead sweep of the trial point may now be pending)
        s0 = ctx.solve_stats(); v = ctx.get_variables(CUR)
        ctx.set_cost_data(0, d1)
        s1 = ctx.solve_stats()
        assert (s1["lookahead_hits"], s1["lookahead_misses"]) == (s0["lookahead_hits"], s0["lookahead_misses"])      # dropped uncounted
        assert np.array_equal(ctx.get_variables(CUR), v)
        lam = st.lambda_
        a = _capi.LmState(); a.lambda_ = lam; a.bestcost = a.cost = c_start = ctx.sweep_gradhess()
        _lm(ctx, a, 3); va = ctx.get_variables(CUR)
    finally:
        ctx.close()
    fr = upload(p, g1, bi, variables=v)
    try:
        b = _capi.LmState(); b.lambda_ = lam; b.bestcost = b.cost = fr.sweep_gradhess()
        assert np.isclose(b.bestcost, c_start, rtol=RTOL)
        _lm(fr, b, 3); vb = fr.get_variables(CUR)
    finally:
        fr.close()
    print(f"LM cost {a.cost:.17g} / {b.cost:.17g} lambda {a.lambda_:.6g} / {b.lambda_:.6g} point {rel(va, vb):.3e}")
    assert (a.iternum, a.linearsolvers, a.converged) == (b.iternum, b.linearsolvers, b.converged)
    assert np.isclose(a.cost, b.cost, rtol=RTOL_TRIAL) and rel(va, vb) < RTOL_TRIAL
    assert a.bestcost < c_start


def test_optimize_singles_after_an_update():
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 60, 0.4, seed=6), 1e-2, 1e-3); bi = blockindices(p); g0 = p.groups()
    d1 = g0[0]["data"] + 0.05 * np.random.default_rng(4).standard_normal(g0[0]["data"].shape); g1 = with_data(p, 0, d1)
    pts = np.arange(11, p.nvariables + 1); lists = p.costlists(pts)
    ctx = upload(p, g0, bi)
    try:
        drive(ctx, g0); ctx.set_variables(p.variables)
        ctx.set_cost_data(0, d1)
        ita = ctx.optimize_singles(pts, *lists); va = ctx.get_variables(CUR)
    finally:
        ctx.close()
    ref = upload(p, g0, bi)
    try:
        ref.optimize_singles(pts, *lists); v0 = ref.get_variables(CUR)
    finally:
        ref.close()
    fr = upload(p, g1, bi)
    try:
        itb = fr.optimize_singles(pts, *lists); vb = fr.get_variables(CUR)
    finally:
        fr.close()
    assert np.array_equal(ita, itb) and np.array_equal(va, vb)          # one thread per point, its blocks in a fixed order
    assert rel(va, v0) >= 1e-6


# ---- N.Solver ----------------------------------------------------------------------------------------------------------------------------------------------
def test_solver_end_to_end(monkeypatch):
    """a noise-free BA solved, its measurements replaced by those of a second noise-free geometry, solved again from new variables: ONE upload, and the second
    solve is what N.optimize gives on a fresh problem with the second data (the tolerance of tests/test_gpu_functional.py::test_converged_variables_match_oracle)"""
    uploads = []
    orig = _capi.Context.upload
    monkeypatch.setattr(_capi.Context, "upload", lambda self, *a, **k: (uploads.append(1), orig(self, *a, **k))[1])
    p = synthetic.create_ba_problem(10, 50, 0.3, seed=1); truth1 = p.variables.copy()
    (g,) = p.costs.values(); vi, _ = g.arrays(); off = p.var_offsets
    rng = np.random.default_rng(9); truth2 = truth1 + 0.05 * rng.standard_normal(truth1.size)
    cam = truth2[off[vi[:, 0] - 1][:, None] + np.arange(6)]; X = truth2[off[vi[:, 1] - 1][:, None] + np.arange(3)]
    meas2 = np.stack([(cam[:, :3] * X).sum(1), (cam[:, 3:] * X).sum(1)], axis=1)
    start1 = truth1 + 1e-3 * rng.standard_normal(truth1.size); start2 = truth2 + 1e-3 * rng.standard_normal(truth1.size)
    p.variables[:] = start1
    with N.Solver(p) as s:
        assert s.cost() > 1e-6
        r1 = s.optimize()
        assert r1.bestcost < 1e-15 and s.cost() == r1.bestcost
        s.set_data(0, meas2)
        assert np.array_equal(g.arrays()[1], meas2)                         # host and device hold the same data
        p.variables[:] = start2
        assert np.array_equal(s.residuals(0), N.residuals(p, 0)) and uploads == [1, 1]        # (N.residuals uploads a context of its own)
        r2 = s.optimize()
        sq = s.squarederrors(0)
    assert len(uploads) == 2 and r2.bestcost < 1e-15 and np.max(sq) < 1e-14
    uploads.clear()
    q = synthetic.create_ba_problem(10, 50, 0.3, seed=1); (gq,) = q.costs.values(); gq.set_arrays(vi, meas2); q.variables[:] = start2
    rq = N.optimize(q)
    assert rq.bestcost < 1e-15 and np.max(np.abs(p.variables - q.variables)) < 1e-8 and abs(r2.niterations - rq.niterations) <= 2
    # an indexed set_data (0-based) and set_robust reach both sides too
    h = synthetic.create_ba_problem(10, 50, 0.3, seed=1, robust=N.HuberKernel(0.05)); (gh,) = h.costs.values()
    with N.Solver(h) as s:
        c0 = s.cost()
        s.set_data(0, [[1.0, 2.0], [3.0, 4.0]], index=[5, 0])
        assert np.array_equal(gh.arrays()[1][[5, 0]], [[1.0, 2.0], [3.0, 4.0]])
        c1 = s.cost(); assert c1 == N.cost(h) and c1 > c0
        s.set_robust(0, N.HuberKernel(0.5))
        assert gh.robust.params[0] == 0.5 and s.cost() == N.cost(h) and s.cost() > c1
        with pytest.raises(AssertionError):
            s.set_robust(0, N.Huber2oKernel(0.5))
