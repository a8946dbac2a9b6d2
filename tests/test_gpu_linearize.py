"""nlls_eval_jacobians / nlls_eval_gradhess: residual and Jacobian, cost, gradient and Hessian of single cost blocks in the caller's upload order (include/nlls_amd.h),
against the CPU oracle's oracle_block_resjac / oracle_block_costgradhess with every slot free.

Tolerances (the project's own):
  r      1e-13 * max(1, max |data of the block|), as tests/test_gpu_blockeval.py;
  J, cost, g, H   absolute error at most 1e-11 (RTOL of tests/test_gpu_parity.py) times the largest magnitude of that quantity in the block, as nlls_check_analytic
         states its differences;
  the adaptive border -- what test_closed_forms_against_dual_numbers holds the device's closed forms to against dual numbers: the kernel's three entries of g to 1e-11
         of their own largest magnitude in the block, the rows and columns of H that belong to the kernel (second derivatives) to 1e-10 of theirs;
  H against its transpose: 1e-14 of the block's largest entry.
The device and the oracle must sit on the same branch of a Huber kernel: no block of a Huber group may lie within 1e-9 (relative) of width^2 (asserted first, from the
oracle's r'r; the seeds below were checked for it on the CPU)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import synthetic, _capi
from tests.helpers import oracle_problem, blockindices, bsm_to_csr, curve_family_problem, mixed_sizes_problem, scalar_graph_problem, chain_edges
from tests.test_gpu_blockeval import adaptive_mean_problem, chain_problem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-11


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300)


def upload(p, unfixed=None, flags=0):
    ctx = _capi.Context(); ctx.upload(p.var_kind, p.var_dim, blockindices(p, unfixed), p.groups(), flags); ctx.set_variables(p.variables)
    return ctx


def is_cost_kind(kind):
    return K.RES_TABLE[kind][1] == 0


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------------------------------
def oracle_group(p, op, gi):
    """(r, J, cost, g, H) of every block of group gi by the oracle, every slot free (J, r: None for a non-squared cost kind)"""
    g = list(p.costs.values())[gi]; n = len(g); M = K.res_nres(g.res_kind)
    rs, Js, cs, gs, Hs = [], [], [], [], []
    for ci in range(n):
        if not is_cost_kind(g.res_kind):
            r, J = op.block_resjac(gi, ci, M); rs.append(r); Js.append(J)
        c, gv, H = op.block_costgradhess(gi, ci); cs.append(c); gs.append(gv); Hs.append(H)
    st = lambda a: np.stack(a) if a else None
    return st(rs), st(Js), np.array(cs), st(gs), st(Hs)


def blockmax(a):
    return np.maximum(np.max(np.abs(a.reshape(a.shape[0], -1)), axis=1), 1e-300)


def check_against_oracle(tag, p, unfixed=None, flags=0):
    op = oracle_problem(p); ctx = upload(p, unfixed, flags); L = _capi.lib()
    for gi, g in enumerate(p.costs.values()):
        n = len(g); _, da = g.arrays(); adaptive = g.res_kind in K.ADAPTIVE_KINDS
        r, J, cost, gv, H = oracle_group(p, op, gi)
        if r is not None and (g.robust.kind & 0xF) in (K.ROBUST_HUBER, K.ROBUST_HUBER2O):
            sq = (r * r).sum(1); w2 = float(g.robust.params[0]) ** 2
            assert np.min(np.abs(sq - w2)) > 1e-9 * w2, (tag, gi, "a block sits on the Huber kernel's branch point: pick another seed")
        gh = ctx.eval_gradhess(gi)
        P = L.nlls_res_gh_dim(int(g.res_kind))
        assert gh["cost"].shape == (n,) and gh["g"].shape == (n, P) and gh["H"].shape == (n, P, P), "a block is left out"
        assert gv.shape == (n, P) and H.shape == (n, P, P)
        if is_cost_kind(g.res_kind):
            assert L.nlls_eval_jacobians(ctx.h, 0, gi, n, None, None, _capi._p(np.zeros(n * P))) == _capi.ERR_UNSUPPORTED
            ej = er = 0.0
        else:
            jac = ctx.eval_jacobians(gi); M = K.res_nres(g.res_kind); NJ = L.nlls_res_jac_cols(int(g.res_kind))
            assert jac["r"].shape == (n, M) and jac["J"].shape == (n, M, NJ) and J.shape == (n, M, NJ), "a block is left out"
            scale = np.maximum(1.0, np.max(np.abs(da), axis=1)) if da.shape[1] else np.ones(n)
            er = np.max(np.abs(jac["r"] - r) / scale[:, None])
            assert jac["r"].tobytes() == ctx.eval_blocks(gi, want="r")["r"].tobytes(), "r differs from nlls_eval_blocks' r"
            ej = np.max(np.max(np.abs(jac["J"] - J).reshape(n, -1), axis=1) / blockmax(J))
        k0 = 3 if adaptive else 0
        ec = np.max(np.abs(gh["cost"] - cost) / np.maximum(np.abs(cost), 1e-300))
        eg = np.max(np.max(np.abs(gh["g"][:, k0:] - gv[:, k0:]), axis=1) / blockmax(gv))
        eh = np.max(np.max(np.abs(gh["H"][:, k0:, k0:] - H[:, k0:, k0:]).reshape(n, -1), axis=1) / blockmax(H))
        esym = np.max(np.max(np.abs(gh["H"] - gh["H"].transpose(0, 2, 1)).reshape(n, -1), axis=1) / blockmax(gh["H"]))
        print(f"LINEARIZE {tag}[{gi}]: n={n} r {er:.3e} (of 1e-13) J {ej:.3e} cost {ec:.3e} g {eg:.3e} H {eh:.3e} (of {RTOL:.0e}) H - H' {esym:.3e} (of 1e-14)")
        assert er <= 1e-13 and ej <= RTOL and ec <= RTOL and eg <= RTOL and eh <= RTOL and esym <= 1e-14, (tag, gi)
        if adaptive:
            dH, oH = gh["H"].copy(), H.copy(); dH[:, 3:, 3:] = 0.0; oH[:, 3:, 3:] = 0.0             # the kernel's rows and columns
            ek = np.max(np.max(np.abs(gh["g"][:, :3] - gv[:, :3]), axis=1) / blockmax(gv[:, :3]))
            ekk = np.max(np.max(np.abs(dH - oH).reshape(n, -1), axis=1) / blockmax(oH))
            print(f"LINEARIZE {tag}[{gi}]: border d rho / d kernel {ek:.3e} (of 1e-11) second derivatives {ekk:.3e} (of 1e-10)")
            assert ek <= 1e-11 and ekk <= 1e-10, (tag, gi)
            assert np.max(np.abs(oH)) > 0 and np.max(np.abs(gv[:, :3])) > 0
    ctx.close()


def affine_two_groups():
    """the problem of tests/test_gpu_blockeval.py::test_affine_ba_huber_two_groups_some_fixed"""
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3, robust=N.HuberKernel(0.002)), 1e-3, 1e-3)
    (g,) = p.costs.values(); vi, da = g.arrays()
    rng = np.random.default_rng(4); pick = rng.choice(vi.shape[0], 150, replace=False)
    p.addcosts(K.RES_BA_AFFINE, vi[pick], da[pick] + 0.01 * rng.standard_normal((150, 2)), N.GemanMcclureKernel(0.01))
    unfixed = np.ones(p.nvariables, bool); unfixed[[0, 1]] = False; unfixed[10:40] = False
    assert len(p.costs) == 2 and np.any(~unfixed[vi[:, 0] - 1] & ~unfixed[vi[:, 1] - 1])
    return p, unfixed


def rosenbrock_problem():
    """Rosenbrock A and B on a chain of scalars, and the 2D form on variables of their own.  B under Geman-McClure (rho'' != 0), not a Huber kernel: on Huber's linear
    branch the Hessian of a block with ONE residual is rho' J'J + 2 rho'' (J'r)(J'r)' = 0 exactly -- what either side returns there is the rounding of that
    cancellation, and a bound relative to the block's largest entry says nothing about it."""
    p = scalar_graph_problem(chain_edges(40)[0], 40, seed=5, robust=N.GemanMcclureKernel(0.7))
    rng = np.random.default_rng(6)
    first = p.addvariables(rng.uniform(-1.0, 2.0, (30, 2)))
    p.addcosts(K.RES_ROSENBROCK_2D, (first + np.arange(30))[:, None], np.stack([rng.uniform(0.5, 1.5, 30), rng.uniform(5.0, 15.0, 30)], axis=1))
    return p


def test_affine_ba_two_groups_some_fixed():
    check_against_oracle("affine+huber/gm", *affine_two_groups())


def test_ba_so3_scaled_geman_mcclure():
    check_against_oracle("ba_so3+scaled gm", synthetic.create_so3_ba_problem(8, 300, 0.3, seed=5, adaptive=False, robust=N.Scaled(N.GemanMcclureKernel(0.01), 2.5)))


def test_ba_so3_adaptive_with_its_border():
    check_against_oracle("ba_so3_adaptive", synthetic.create_so3_ba_problem(8, 300, 0.3, seed=6, adaptive=True))


def test_adaptive_mean():
    check_against_oracle("adaptive_mean", adaptive_mean_problem(means=(-0.7, 0.6)))


def test_rosenbrock_a_b_2d():
    check_against_oracle("rosenbrock", rosenbrock_problem())


def test_curve_exp4_four_slots():
    check_against_oracle("curve_exp4", curve_family_problem(6, 50, own=(0,), seed=2))


def test_linear3_and_the_huber_ba_beside_it():
    check_against_oracle("mixed linear3", mixed_sizes_problem("linear3"))


def test_cost_linear3_has_g_and_H_only():
    check_against_oracle("mixed cost3", mixed_sizes_problem("cost3"))


def test_scale_mix_with_its_bounded_scalars():
    from tests.test_oracle_pins import scale_mix_problem
    check_against_oracle("scale_mix", scale_mix_problem(8, n=64, noise=1e-3, shared=3, robust=N.HuberKernel(0.05)))


# ---- 2. the shapes the kernel branches on ------------------------------------------------------------------------------------------------------------
def raw_gradhess(ctx, gi, n, index, P):
    cost = np.zeros(n); g = np.zeros((n, P)); H = np.zeros((n, P * P))
    ix = None if index is None else np.ascontiguousarray(index, np.int64)
    ctx._chk(ctx.L.nlls_eval_gradhess(ctx.h, 0, gi, n, _capi._p(ix), _capi._p(cost), _capi._p(g), _capi._p(H)))
    return cost, g, H


def raw_jacobians(ctx, gi, n, index, M, NJ):
    r = np.zeros((n, M)); J = np.zeros((n, M * NJ))
    ix = None if index is None else np.ascontiguousarray(index, np.int64)
    ctx._chk(ctx.L.nlls_eval_jacobians(ctx.h, 0, gi, n, _capi._p(ix), _capi._p(r), _capi._p(J)))
    return r, J


def truncated(p, ncost):
    (g,) = p.costs.values(); vi, da = g.arrays(); assert vi.shape[0] >= ncost
    g.set_arrays(vi[:ncost].copy(), da[:ncost].copy())
    return p


SHAPES = [("affine", n) for n in (1, 63, 64, 65, 255, 257)] + [("so3_adaptive", n) for n in (65, 257)]


@pytest.mark.parametrize("kind,ncost", SHAPES, ids=[f"{k}-{n}" for k, n in SHAPES])
def test_selections_are_records_of_the_full_call(kind, ncost):
    """all blocks, the first n < ncost, a shuffled index, an index with repeats, the last block alone: record i is record index[i] of the full call, byte for byte.
    A wavefront takes 64 blocks and stages as many lanes' records at a time as its slab holds: the counts leave the last wavefront partly filled (1, 63, 65, 255, 257)
    and the last sub-batch of every wavefront partly filled (64 is no multiple of the sub-batch of J, 53 lanes, or of H: 12 lanes at 81 doubles, 7 at 144)."""
    if kind == "affine":
        p = truncated(synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3, robust=N.HuberKernel(0.002)), 1e-3, 1e-3), ncost)
        M, NJ, P = 2, 9, 9
    else:
        p = truncated(synthetic.create_so3_ba_problem(8, 300, 0.3, seed=6, adaptive=True), ncost)
        M, NJ, P = 2, 9, 12
    (g,) = p.costs.values(); used = np.zeros(p.nvariables, bool); used[g.arrays()[0].ravel() - 1] = True       # (variables the kept blocks do not touch stay fixed)
    ctx = upload(p, used); rng = np.random.default_rng(ncost)
    full = raw_gradhess(ctx, 0, ncost, None, P) + raw_jacobians(ctx, 0, ncost, None, M, NJ)
    st = ctx.solve_stats(); slab = st["linearize_slab"]
    batch = lambda rec: 0 if rec <= 1 or (rec | 1) > slab else min(64, slab // (rec | 1))
    assert slab == 1024 and (st["linearize_batch_J"], st["linearize_batch_g"], st["linearize_batch_H"]) == (batch(M * NJ), batch(P), batch(P * P)), st
    assert 0 < batch(P * P) < 64 and 64 % batch(P * P) != 0 and 0 < batch(M * NJ) < 64 and 64 % batch(M * NJ) != 0       # a partly filled sub-batch in every wavefront
    assert np.all(np.isfinite(np.concatenate([a.ravel() for a in full])))
    selections = [("all", ncost, np.arange(1, ncost + 1)), ("last", 1, np.array([ncost])),
                  ("shuffled", ncost, rng.permutation(ncost) + 1), ("repeats", ncost + 7, rng.integers(1, ncost + 1, ncost + 7))]
    if ncost > 1:
        selections.append(("first n", ncost - ncost // 3 - 1, None))
    for name, n, index in selections:
        got = raw_gradhess(ctx, 0, n, index, P) + raw_jacobians(ctx, 0, n, index, M, NJ)
        pick = np.arange(n) if index is None else index - 1
        for a, b in zip(got, full):
            assert a.tobytes() == np.ascontiguousarray(b[pick]).tobytes(), (kind, ncost, name)
    again = raw_gradhess(ctx, 0, ncost, None, P) + raw_jacobians(ctx, 0, ncost, None, M, NJ)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, full)), "two identical calls differ"
    only = ctx.eval_gradhess(0, want="H")                                             # (any pointer may be NULL)
    assert list(only) == ["H"] and np.ascontiguousarray(only["H"].transpose(0, 2, 1)).tobytes() == full[2].tobytes()
    ctx.close()


# ---- 3. the blocks' g and H add up to the sweep's b and A --------------------------------------------------------------------------------------------
def symmetrised(Lo):
    strict = np.tril(Lo, -1)
    return strict + strict.T + np.diag(np.diag(Lo))


def reassemble(p, ctx, unfixed):
    """every block's g and H scattered on the host into b and A (the rule of updatesymA!, src/linearsystem.jl:132-175: a diagonal block whole, an off-diagonal block
    where its larger block index is the row; fixed slots skipped), A returned symmetrised"""
    bi = blockindices(p, unfixed).astype(np.int64); bo = np.asarray(ctx.bsm_index()[3], np.int64) - 1; ndof = ctx.info.ndof
    Lo = np.zeros((ndof, ndof)); b = np.zeros(ndof)
    for gi, g in enumerate(p.costs.values()):
        vi, _ = g.arrays(); out = ctx.eval_gradhess(gi, want=("g", "H")); slots = K.RES_TABLE[g.res_kind][4]
        dofs = [K.var_dof(vk, vd) for vk, vd in slots]; loff = np.concatenate([[0], np.cumsum(dofs)])
        for s in range(len(slots)):
            bs = bi[vi[:, s] - 1]; fs = bs > 0
            pos_s = bo[np.maximum(bs, 1) - 1][:, None] + np.arange(dofs[s])[None, :]
            np.add.at(b, pos_s[fs].ravel(), out["g"][fs, loff[s]:loff[s + 1]].ravel())
            for t in range(len(slots)):
                bt = bi[vi[:, t] - 1]; m = fs & (bt > 0) & ((bs > bt) | ((s == t) & (bs == bt)))
                assert s == t or not np.any(fs & (bs == bt)), "two slots of one block on one variable"
                pos_t = bo[np.maximum(bt, 1) - 1][:, None] + np.arange(dofs[t])[None, :]
                rows = np.broadcast_to(pos_s[m][:, :, None], (int(m.sum()), dofs[s], dofs[t])); cols = np.broadcast_to(pos_t[m][:, None, :], rows.shape)
                np.add.at(Lo, (rows.ravel(), cols.ravel()), out["H"][m, loff[s]:loff[s + 1], loff[t]:loff[t + 1]].ravel())
    return symmetrised(Lo), b


def device_system(ctx):
    info = ctx.info; data = ctx.get_bsm_data(); b = ctx.get_grad()
    if info.is_sparse:
        return bsm_to_csr(ctx.bsm_index(), data, info.ndof).toarray(), b
    assert data.size == info.ndof ** 2
    return symmetrised(data.reshape(info.ndof, info.ndof).T), b


@pytest.mark.parametrize("flags", [0, _capi.FLAG_MATERIALIZE], ids=["default", "materialize"])
def test_blocks_reassemble_the_sweep(flags):
    dense = curve_family_problem(1, 60, own=(), seed=4); (gd,) = dense.costs.values(); vd, dd = gd.arrays()
    first = dense.addvariables(np.random.default_rng(8).uniform(-1.0, 2.0, (3, 2)))
    dense.addcosts(K.RES_ROSENBROCK_2D, (first + np.arange(3))[:, None], np.array([[1.0, 10.0], [0.7, 8.0], [1.2, 12.0]]), N.GemanMcclureKernel(2.0))
    p, unfixed = affine_two_groups()
    for tag, prob, unf, sparse in (("sparse affine", p, unfixed, 1), ("dense curve + rosenbrock", dense, None, 0)):
        ctx = upload(prob, unf, flags)
        assert ctx.info.is_sparse == sparse, tag
        A, b = reassemble(prob, ctx, unf)
        ctx.sweep_gradhess(); Ad, bd = device_system(ctx)
        print(f"LINEARIZE reassembly {tag} flags {flags}: ndof {ctx.info.ndof} A {rel(A, Ad):.3e} b {rel(b, bd):.3e} (of {RTOL:.0e})")
        assert rel(A, Ad) < RTOL and rel(b, bd) < RTOL, tag
        ctx.close()


# ---- 4. N.jacobian ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robust,weighted", [(None, False), (N.HuberKernel(0.002), True)], ids=["plain", "huber-weighted"])
def test_whole_problem_jacobian(robust, weighted):
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3, robust=robust), 1e-3, 1e-3)
    unfixed = np.ones(p.nvariables, bool); unfixed[[0, 1]] = False; unfixed[10:40] = False
    rows, cols, vals, r = N.jacobian(p, unfixed, weighted=weighted)
    ctx = upload(p, unfixed); ctx.sweep_gradhess(); A, b = device_system(ctx); ndof = ctx.info.ndof; ctx.close()
    (g,) = p.costs.values()
    assert r.size == 2 * len(g) and rows.max() < r.size and cols.min() >= 0 and cols.max() < ndof and rows.size == cols.size == vals.size
    J = np.zeros((r.size, ndof)); np.add.at(J, (rows, cols), vals)
    print(f"LINEARIZE jacobian weighted={weighted}: {J.shape} J'J {rel(J.T @ J, A):.3e} J'r {rel(J.T @ r, b):.3e} (of {RTOL:.0e})")
    assert rel(J.T @ J, A) < RTOL and rel(J.T @ r, b) < RTOL
    if weighted:
        w = N.Solver(p, unfixed)
        try:
            assert np.any(w.ls.eval_blocks(0, want="weight")["weight"] < 1.0), "no block on the Huber kernel's linear branch: the weights are not exercised"
        finally:
            w.close()


def test_whole_problem_jacobian_refuses_an_adaptive_group():
    with pytest.raises(ValueError):
        N.jacobian(synthetic.create_so3_ba_problem(4, 30, 0.5, seed=6, adaptive=True))


def test_public_functions_take_zero_based_blocks():
    p, unfixed = affine_two_groups()
    full = N.computeresjac(p, 1); idx = np.array([149, 0, 7, 7])
    part = N.computeresjac(p, 1, idx, unfixed)
    assert full["J"].shape == (150, 2, 9) and np.array_equal(part["J"], full["J"][idx]) and np.array_equal(part["r"], full["r"][idx])
    gh = N.computecostgradhess(p, 0, idx)
    with N.Solver(p, unfixed) as s:
        assert np.array_equal(s.gradhess(0, idx)["H"], gh["H"]) and np.array_equal(s.jacobians(1)["J"], full["J"])
        assert gh["g"].shape == (4, 9) and s.gradhess(0)["cost"].shape == (len(list(p.costs.values())[0]),)


# ---- 5. state neutrality and errors -------------------------------------------------------------------------------------------------------------------
def _trial_run(p, flags, call, materialise):
    """sweep, [both calls on every group, at both variable sets], trial: (cost of the sweep, trial cost, step, trial point), and the counters around the calls"""
    ctx = upload(p, None, flags)
    if materialise:
        ctx.set_option(_capi.OPT_MATERIALIZE, 1)
    ctx.copy_variables(_capi.VARS_NEXT, _capi.VARS_CURRENT)
    c0 = ctx.sweep_gradhess(); lam = 1e-3
    if call:
        before = ctx.solve_stats()
        for gi in range(len(p.costs)):
            ctx.eval_gradhess(gi, _capi.VARS_CURRENT); ctx.eval_gradhess(gi, _capi.VARS_NEXT, want=("g",))
            if not is_cost_kind(list(p.costs.values())[gi].res_kind):
                ctx.eval_jacobians(gi, _capi.VARS_CURRENT); ctx.eval_jacobians(gi, _capi.VARS_NEXT, index=[1], want=("J",))
        after = ctx.solve_stats()
        keys = ("lookahead_hits", "lookahead_misses", "mf_trials", "reduced_sweeps", "full_sweeps")                  # nlls_get_solve_stats [21] .. [25]
        assert [before[k] for k in keys] == [after[k] for k in keys], (before, after)
    c1 = ctx.lm_trial(lam); mf = ctx.solve_stats()["mf_trials"]
    out = (c0, c1, ctx.get_step().tobytes(), ctx.get_variables(_capi.VARS_NEXT).tobytes()); ctx.close()
    return out, mf


def test_reads_only_small_dense():
    """60 blocks of the adaptive-mean fixture: the trial is reproducible to the bit there (tests/test_gpu_blockeval.py::test_reads_only_between_sweep_and_trial says
    why), and a trial behind the two calls is the trial without them, byte for byte"""
    p = adaptive_mean_problem(means=(-0.4, 0.3), draws=(24, 6))
    (a, _), (b, _), (c, _) = (_trial_run(p, 0, call, False) for call in (False, False, True))
    assert a == b, "the trial without the calls is not reproducible"
    assert c == a


@pytest.mark.parametrize("materialise", [False, True], ids=["matrix-free", "materialised"])
def test_reads_only_on_both_trial_paths(materialise):
    """the bundle-adjustment chain: the matrix-free trial of the default upload, and the materialised one under NLLS_OPT_MATERIALIZE, with and without the two calls
    between the sweep and the trial.  A comparison of bytes ACROSS runs is not available on these paths: the sweeps and the assembly add with atomics (include/nlls_amd.h,
    NLLS_FLAG_DETERMINISTIC; tests/test_gpu_blockeval.py::_same_trial), and five identical runs WITHOUT the calls gave five different trial costs and steps on each of
    four chains (120 x 3000, 120 x 1000, 130 x 600, 150 x 400 at 4 .. 6 % visibility), on either path, with and without NLLS_FLAG_DETERMINISTIC -- differences in the last
    digits.  So the run with the calls is held to what a trial is asked of another run (1e-9, check_problem), always, and the byte comparisons are made where they can
    be: the trial of the small dense system (test_reads_only_small_dense), everything a trial reads in ONE context
    (test_calls_leave_the_linear_system_and_the_variables_untouched), and the counters [21] .. [25] around the calls (_trial_run, exactly)."""
    p = chain_problem()
    (a, mfa), (c, mfc) = (_trial_run(p, _capi.FLAG_DETERMINISTIC, call, materialise) for call in (False, True))
    assert mfa == mfc == (0 if materialise else 1), "the trial did not take the path the case was written for"
    print(f"LINEARIZE trial behind the calls, materialise={materialise}: bit-identical to the run without {c == a}; costs {a[:2]} / {c[:2]}")
    assert np.allclose(c[:2], a[:2], rtol=1e-9, atol=0.0)
    assert np.allclose(np.frombuffer(c[2]), np.frombuffer(a[2]), rtol=1e-9, atol=1e-12) and np.allclose(np.frombuffer(c[3]), np.frombuffer(a[3]), rtol=1e-9, atol=1e-12)


def test_calls_leave_the_linear_system_and_the_variables_untouched():
    """what a trial reads, before and behind the two calls, byte for byte in ONE context: A.data, b and the three variable sets of a materialised upload (there reading
    A.data and b sweeps nothing again, so the two readings are of the same memory)"""
    p, unfixed = affine_two_groups()
    ctx = upload(p, unfixed, _capi.FLAG_MATERIALIZE); ctx.copy_variables(_capi.VARS_NEXT, _capi.VARS_CURRENT); ctx.copy_variables(_capi.VARS_BEST, _capi.VARS_CURRENT)
    ctx.sweep_gradhess()
    state = lambda: [ctx.get_bsm_data().tobytes(), ctx.get_grad().tobytes()] + [ctx.get_variables(w).tobytes() for w in range(3)]
    before = state(); st0 = ctx.solve_stats()
    for gi in range(2):
        ctx.eval_jacobians(gi, _capi.VARS_NEXT); ctx.eval_gradhess(gi, _capi.VARS_CURRENT); ctx.eval_gradhess(gi, _capi.VARS_BEST, index=[5, 1, 5])
    st1 = ctx.solve_stats()
    assert state() == before
    assert all(st0[k] == st1[k] for k in st0 if not k.startswith("linearize")), (st0, st1)
    ctx.close()


def test_errors():
    L = _capi.lib(); ctx = _capi.Context(); P = _capi._p
    out = np.full(4096, 7.25); sentinel = out.copy()
    assert L.nlls_eval_jacobians(ctx.h, 0, 0, 1, None, P(out), None) == _capi.ERR_NOT_READY                      # no upload yet
    assert L.nlls_eval_gradhess(ctx.h, 0, 0, 1, None, P(out), None, None) == _capi.ERR_NOT_READY
    p = N.NLLSProblem(); a = p.addvariable([0.1, 0.2, 0.3]); b = p.addvariable([0.3, -0.2, 0.5]); d = p.addvariable([1.0, 2.0, 3.0, 4.0], K.VAR_DYNAMIC)
    rng = np.random.default_rng(2)
    p.addcosts(K.RES_LINEAR3, [[a], [b], [a]], rng.standard_normal((3, 12)))
    p.addcosts(K.COST_LINEAR3, [[a]], rng.standard_normal((1, 3)))
    p.addcosts(K.COST_DYN_LINEAR, [[d]], rng.standard_normal((1, 4)))
    p.addcosts(K.RES_DYN_NORM, [[d]], np.zeros((1, 0)))
    ctx.upload(p.var_kind, p.var_dim, blockindices(p), p.groups()); ctx.set_variables(p.variables)
    ncost = 3
    ix = lambda *v: P(np.array(v, np.int64))
    for bad in (-1, 4):                                                                                           # a bad group
        assert L.nlls_eval_jacobians(ctx.h, 0, bad, 1, None, P(out), P(out)) == _capi.ERR_INVALID_ARG
        assert L.nlls_eval_gradhess(ctx.h, 0, bad, 1, None, P(out), None, None) == _capi.ERR_INVALID_ARG
    for bad in (0, ncost + 1):                                                                                    # an index outside 1 .. ncost, behind a valid one
        assert L.nlls_eval_jacobians(ctx.h, 0, 0, 2, ix(1, bad), P(out), P(out[64:])) == _capi.ERR_INVALID_ARG
        assert L.nlls_eval_gradhess(ctx.h, 0, 0, 2, ix(1, bad), P(out), P(out[64:]), P(out[128:])) == _capi.ERR_INVALID_ARG
    assert L.nlls_eval_gradhess(ctx.h, 0, 0, -1, None, P(out), None, None) == _capi.ERR_INVALID_ARG              # n < 0
    assert L.nlls_eval_gradhess(ctx.h, 0, 0, ncost + 1, None, P(out), None, None) == _capi.ERR_INVALID_ARG       # n > ncost without an index
    assert L.nlls_eval_jacobians(ctx.h, 0, 0, ncost, None, None, None) == _capi.ERR_INVALID_ARG                  # all NULL
    assert L.nlls_eval_gradhess(ctx.h, 0, 0, ncost, None, None, None, None) == _capi.ERR_INVALID_ARG
    assert L.nlls_eval_gradhess(ctx.h, 7, 0, ncost, None, P(out), None, None) == _capi.ERR_INVALID_ARG           # no such variable set
    assert L.nlls_eval_jacobians(ctx.h, 0, 1, 1, None, P(out), P(out[64:])) == _capi.ERR_UNSUPPORTED             # a non-squared cost kind has no residual
    for dyn in (2, 3):                                                                                            # the dynamic-size kinds
        assert L.nlls_eval_jacobians(ctx.h, 0, dyn, 1, None, P(out), P(out[64:])) == _capi.ERR_UNSUPPORTED
        assert L.nlls_eval_gradhess(ctx.h, 0, dyn, 1, None, P(out), P(out[64:]), None) == _capi.ERR_UNSUPPORTED
    assert out.tobytes() == sentinel.tobytes(), "a refused call wrote to an output"
    assert L.nlls_eval_jacobians(ctx.h, 0, 0, 0, None, P(out), P(out)) == _capi.OK                                # n == 0
    assert L.nlls_eval_gradhess(ctx.h, 0, 0, 0, ix(1), P(out), None, None) == _capi.OK
    assert out.tobytes() == sentinel.tobytes()
    assert ctx.eval_gradhess(0, index=[3, 3, 1])["H"].shape == (3, 3, 3) and ctx.eval_gradhess(1)["g"].shape == (1, 3)
    assert L.nlls_eval_gradhess(ctx.h, 0, 0, ncost + 2, ix(1, 2, 3, 1, 2), P(out), None, None) == _capi.OK       # more records than blocks, through an index
    with pytest.raises(_capi.NllsError):
        ctx.eval_jacobians(1)
    ctx.close()


# ---- 6. a user kind ---------------------------------------------------------------------------------------------------------------------------------------
def test_user_kind_in_a_process_of_its_own():
    userlib = os.path.join(ROOT, "nllssolver.jl_amd", "csrc", "libnlls_amd_userdemo.so")
    env = dict(os.environ, NLLS_AMD_LIB=userlib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "linearize_userkind_worker.py")], capture_output=True, text=True, env=env, timeout=600)
    print(out.stdout[-1500:])
    assert out.returncode == 0 and "user kind linearisation ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
