"""The dynamic-size blocks on the device at the lengths their kernels branch on.

dyn_block_kernel (csrc/nlls_cost.hip) and eval_dyn_kernel (csrc/nlls_eval.hip) run ONE workgroup of TPB = 256 lanes per block and loop `for (i = threadIdx.x; i < n;
i += TPB)`; n is the variable's run-time length, 1 .. NLLS_MAX_DYN_DIM = 4096 (512 for NLLS_RES_DYN_LINEARSQ, whose residual and J'r live in rs[512] / gs[512] of LDS).
The lengths below are the smallest at which each branch is taken:

    a single lane; the first pair                                     1, 2
    one wavefront of block_sum                                        63, 64, 65
    one workgroup's lanes (the second trip of every strided loop)     255, 256, 257
    the LDS arrays and the DYN_LINEARSQ limit                         511, 512     (DYN_LINEAR at 511 / 512: ndata = 512 / 513, the update scatter's chunk edge)
    third and later trips, the largest variable                       513, 1024; 4096 where no n x n array is formed (cost and values)

Reference, companions and bound are those of tests/test_dynamic_reference.py: closed forms in long double, and for every output array q of a block
max |q_dev - q_ref| <= 8 (n + 8) u max q_abs.  Every comparison prints the share of that bound the device uses (`SHARE <case> <quantity> ...`) and every case the
kinds that ran at its length (`LENGTH ...`); the largest shares per case and quantity are printed when the module is done (`DEVICE SHARE ...`; notes/r27.md keeps them).

Cases: a  one variable under all kinds, dense system: the two sweeps, b, the lower triangle of A, max |diag|        b  nlls_eval_blocks: r, r'r, rho, weight
       c  a fixed variable between two free ones                  d  block-sparse placement (aoff): the variable's diagonal block stored in full
       e  the damped step, the retraction, the one-call trial     f  nlls_set_cost_data on long records               g  the limits the upload enforces"""
import struct

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import synthetic, _capi
from tests.helpers import oracle_problem, blockindices, longdouble_backward_error, LD
from tests.test_gpu_parity import ETA_BOUND, solver_of, rel, RTOL
from tests.test_dynamic_reference import (H_LENGTHS, VALUE_LENGTHS, KERNELS, MAGS, KIND_NAME, SQ_MAX, DYN_MAX, kinds_at, share, start, payload, add_all_kinds,
                                          one_variable_problem, problem_reference, check_regions)

pytestmark = pytest.mark.gpu

CUR, NEXT = _capi.VARS_CURRENT, _capi.VARS_NEXT
UPD_LANE_MAX, UPD_WAVE_CHUNK = 16, 512                       # csrc/nlls_update.hip: doubles a lane moves alone; doubles per wavefront
DEVICE_SHARE = {}                                            # (case, quantity) -> (largest share of the bound, where)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (case, what), (s, where) in sorted(DEVICE_SHARE.items()):
        print(f"\nDEVICE SHARE case {case} {what}: {s:.4%} of the bound ({where})", end="")
    print()


def hold(case, what, n, dev, ref, ref_abs, where):
    """assert max |dev - ref| <= 8 (n + 8) u max ref_abs; print and keep the share used"""
    s = share(dev, ref, ref_abs, n)
    print(f"SHARE {case} {what} n={n} {where}: {s:.4%}")
    if s >= DEVICE_SHARE.get((case, what), (-1.0, ""))[0]: DEVICE_SHARE[(case, what)] = (s, f"n={n} {where}")
    assert s <= 1.0, f"case {case}, {what} at n={n} ({where}): {s:.4g} x the bound 8 (n + 8) u max |.|_abs"
    return s


def names(kinds):
    return "+".join(KIND_NAME[k] for k in kinds)


def upload(p, unfixed=None, flags=0):
    bi = blockindices(p, unfixed)
    ctx = _capi.Context(); info = ctx.upload(p.var_kind, p.var_dim, bi, p.groups(), flags); ctx.set_variables(p.variables)
    return ctx, info, bi


def device_H(ctx, info):
    """A.data as an ndof x ndof array: the dense system's column-major matrix, or the stored blocks of the block-sparse one (column-major, the block row the later
    variable's) with NaN wherever nothing is stored"""
    A = ctx.get_bsm_data(); nd = info.ndof
    if not info.is_sparse: return A.reshape(nd, nd).T
    cp, rv, nz, bo = (np.asarray(a, np.int64) for a in ctx.bsm_index()); nb = len(cp) - 1
    bo0 = bo - 1; bs = np.diff(np.r_[bo0, nd]); M = np.full((nd, nd), np.nan); used = 0
    for row in range(nb):
        for e in range(cp[row] - 1, cp[row + 1] - 1):
            col = rv[e] - 1; br, bc = bs[row], bs[col]; o = nz[e] - 1
            M[bo0[row]:bo0[row] + br, bo0[col]:bo0[col] + bc] = A[o:o + br * bc].reshape(bc, br).T; used += br * bc
    assert used == A.size
    return M


def dof_offsets(p, bi):
    """the first unknown of every variable (all Euclidean or dynamic: dim unknowns each) in b, -1 for a fixed one"""
    off = np.full(p.nvariables, -1, np.int64); free = np.asarray(bi) > 0
    off[free] = np.cumsum(np.r_[0, p.var_dim[free][:-1]])
    return off


def hold_linearisation(case, ctx, info, p, bi, ref, where, variables=None):
    """what a gradient sweep leaves against the reference: the cost, b and the diagonal block of every free variable that carries dynamic-size blocks (a dense
    system: its lower triangle, the upper one its mirror; block-sparse: the full block).  Returns (b, H) of the device."""
    b = ctx.get_grad(); H = device_H(ctx, info); off = dof_offsets(p, bi)
    for v in (sorted(ref["var"]) if variables is None else variables):
        V = ref["var"][v]; n = V["n"]; o = off[v - 1]
        if o < 0: continue
        hold(case, "b", n, b[o:o + n], V["g"], V["g_abs"], f"{where} var {v}")
        Hd = H[o:o + n, o:o + n]
        if info.is_sparse:
            hold(case, "A", n, Hd, V["H"], V["H_abs"], f"{where} var {v} (full block)")
        else:
            lo = np.tril_indices(n); hold(case, "A", n, Hd[lo], V["H"][lo], V["H_abs"][lo], f"{where} var {v} (lower triangle)")
            assert np.array_equal(Hd, Hd.T), "the dense system's upper triangle is not the mirror of the lower one"
    return b, H


def same_bytes(a, b):
    return struct.pack("d", a) == struct.pack("d", b)


def step_and_trial(case, ctx, info, p, where):
    """case e: damp(1e-4 max |diag|) and solve: the long-double backward error on the device's own A and b within the bound of tests/test_gpu_parity.py::check_step;
    the retraction against current + x at one ulp (every variable Euclidean or dynamic: one rounding); lm_trial(0.0) against sweep_cost(NEXT) at 1e-9"""
    assert np.all(np.isin(p.var_kind, (K.VAR_EUCLIDEAN, K.VAR_DYNAMIC))) and info.ndof == p.variables.size
    A, b = ctx.get_bsm_data(), ctx.get_grad()
    lam = 1e-4 * ctx.max_abs_diag(); ctx.damp(lam); x = ctx.solve(want_x=True); st = ctx.solve_stats()
    assert st["dropped_pivots"] == 0
    eta = longdouble_backward_error(A, ctx.bsm_index() if info.is_sparse else None, b, lam, x); mode = solver_of(info, st)
    print(f"ETA {case} {where} {mode} ndof={info.ndof} {eta:.3e}")
    assert eta <= ETA_BOUND[mode], f"{where}: backward error {eta:.3e} of the {mode} solve above {ETA_BOUND[mode]:.0e}"
    ctx.retract(NEXT, CUR); v = ctx.get_variables(NEXT); want = p.variables + x
    assert np.all(np.abs(v - want) <= np.spacing(np.abs(want))), f"{where}: the retraction is off current + x by {np.max(np.abs(v - want) / np.spacing(np.abs(want))):.3g} ulp"
    c_next = ctx.sweep_cost(NEXT)
    ctx.set_variables(np.zeros_like(v), NEXT)                                    # (whatever the trial leaves there must be its own work)
    c_trial = ctx.lm_trial(0.0)
    assert np.isclose(c_trial, c_next, rtol=1e-9, atol=1e-300), (where, c_trial, c_next)


# ---- a. one variable under all kinds, dense system -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kname", list(KERNELS))
@pytest.mark.parametrize("n", H_LENGTHS)
def test_a_one_variable_under_all_kinds(n, kname):
    """no kernel, Huber, Geman-McClure, Scaled(Huber2o) -- on the scalar residual of DYN_LINEAR rho' + 2 rho'' r^2 of the last cancels to rounding -- at data magnitudes
    inside (0.01) and outside (2.0) the kernels' quadratic region; DYN_LINEARSQ through n = 512, the others through 1024.  The cost sweep twice: equal bytes."""
    print(f"\nLENGTH a n={n} kernel={kname} kinds={names(kinds_at(n))}")
    for mag in MAGS:
        p = one_variable_problem(n, kname, mag); ref = problem_reference(p); check_regions(ref, mag); where = f"{kname} mag={mag}"
        assert [b["kind"] for b in ref["blocks"]] == kinds_at(n)
        ctx, info, bi = upload(p)
        try:
            assert not info.is_sparse and info.ndof == n
            c1, c2 = ctx.sweep_cost(), ctx.sweep_cost()
            assert same_bytes(c1, c2), (c1, c2)
            hold("a", "sweep_cost", n, c1, ref["cost"], ref["cost_abs"], where)
            hold("a", "sweep_gradhess cost", n, ctx.sweep_gradhess(), ref["cost"], ref["cost_abs"], where)
            hold_linearisation("a", ctx, info, p, bi, ref, where)
            V = ref["var"][1]; d = np.abs(np.diag(V["H"]))
            hold("a", "max_abs_diag", n, ctx.max_abs_diag(), np.max(d), np.max(np.diag(V["H_abs"])), where)
            if n in (257, 512) and (kname, mag) in (("none", MAGS[0]), ("huber", MAGS[1])):       # case e on the dense system (rho'' = 0: H is positive definite)
                step_and_trial("e", ctx, info, p, f"dense n={n} {where}")
        finally:
            ctx.close()


# ---- b. values -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", VALUE_LENGTHS)
def test_b_values(n):
    """nlls_eval_blocks (r, r'r, rho, weight) of the three residual kinds, three blocks per group (two at n = 4096, a gigabyte of A.data less) so that r_out[k n + i]
    is written with k > 0; DYN_NORM under Huber, DYN_LINEAR under Scaled(Huber2o), DYN_LINEARSQ under Geman-McClure; the first block inside the quadratic region,
    the others outside.  And the cost sweep of the same problem, with COST_DYN_LINEAR beside them: the one sweep that runs at n = 4096."""
    nv = 3 if n < DYN_MAX else 2; mags = dict(zip(range(1, nv + 1), (MAGS[0], MAGS[1], MAGS[1])))
    kern = {K.RES_DYN_NORM: KERNELS["huber"], K.RES_DYN_LINEAR: KERNELS["scaled_huber2o"], K.RES_DYN_LINEARSQ: KERNELS["geman"], K.COST_DYN_LINEAR: None}
    rng = np.random.default_rng(n); p = N.NLLSProblem()
    for v in range(1, nv + 1): p.addvariable(start(n, mags[v], rng), K.VAR_DYNAMIC)
    for kind in kinds_at(n):
        for v in range(1, nv + 1): p.addcosts(kind, [[v]], payload(kind, p.variable(v).copy(), mags[v], rng, tag=v)[None, :], robust=kern[kind])
    groups = p.groups(); assert [g["res_kind"] for g in groups] == kinds_at(n) and all(len(g["varind"]) == nv for g in groups)
    ref = problem_reference(p, want_H=False); check_regions(ref, mags)
    print(f"\nLENGTH b n={n} blocks per group={nv} kinds={names(kinds_at(n))}")
    ctx, info, bi = upload(p)
    try:
        for gi, g in enumerate(groups):
            kind = g["res_kind"]
            if kind == K.COST_DYN_LINEAR: continue
            ev = ctx.eval_blocks(gi); blocks = [b for b in ref["blocks"] if b["group"] == gi]
            assert [b["index"] for b in blocks] == list(range(nv)) and ev["r"].shape == (nv, 1 if kind == K.RES_DYN_LINEAR else n)
            for k, b in enumerate(blocks):
                where = f"{KIND_NAME[kind]} block {k}"
                hold("b", "r", n, ev["r"][k], b["r"], b["r_abs"], where)
                hold("b", "sqerr", n, ev["sqerr"][k], b["c"], b["c_abs"], where)
                hold("b", "rho", n, ev["rho"][k], b["rho"], b["rho_abs"], where)
                hold("b", "weight", n, ev["weight"][k], b["weight"], b["weight_abs"], where)
        c1, c2 = ctx.sweep_cost(), ctx.sweep_cost()
        assert same_bytes(c1, c2), (c1, c2)
        hold("b", "sweep_cost", n, c1, ref["cost"], ref["cost_abs"], f"{nv} variables")
    finally:
        ctx.close()


# ---- c. a fixed variable -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (64, 257))
def test_c_fixed_variable(n):
    """three variables of one length under all kinds (Huber), the middle one fixed: its blocks give their cost (launch_dyn_cost(..., fixed_only), through `index`)
    and nothing to A or b; the free variables' blocks land at the offsets of the reference, 0 and n"""
    mags = {1: MAGS[0], 2: MAGS[1], 3: MAGS[1]}; rng = np.random.default_rng(100 + n); p = N.NLLSProblem()
    for v in (1, 2, 3): p.addvariable(start(n, mags[v], rng), K.VAR_DYNAMIC)
    for v in (1, 2, 3): add_all_kinds(p, v, mags[v], KERNELS["huber"], rng, tag=v)
    ref = problem_reference(p); check_regions(ref, mags)
    print(f"\nLENGTH c n={n} kinds={names(kinds_at(n))}")
    unfixed = np.array([True, False, True]); ctx, info, bi = upload(p, unfixed)
    try:
        ols = oracle_problem(p).linear_system(bi, 0)
        assert info.ndof == 2 * n and info.is_sparse == ols.info.is_sparse and info.nnz_data == ols.info.nnz_data
        if info.is_sparse:
            for g, o in zip(ctx.bsm_index(), ols.bsm_index()): assert np.array_equal(g, o)
        fixed_cost = sum(b["cost"] for b in ref["var"][2]["blocks"]); tol = 8 * (n + 8) * 2.0 ** -53 * float(ref["cost_abs"])
        assert abs(float(fixed_cost)) > 1e6 * tol, "the fixed variable's cost would hide inside the tolerance"
        hold("c", "sweep_cost", n, ctx.sweep_cost(), ref["cost"], ref["cost_abs"], "middle fixed")
        hold("c", "sweep_gradhess cost", n, ctx.sweep_gradhess(), ref["cost"], ref["cost_abs"], "middle fixed")
        assert list(dof_offsets(p, bi)) == [0, -1, n]
        b, H = hold_linearisation("c", ctx, info, p, bi, ref, "middle fixed")
        cross = H[n:, :n]
        assert np.all(np.isnan(cross)) if info.is_sparse else not np.any(cross), "something was written between the two free variables"
    finally:
        ctx.close()


# ---- d. block-sparse placement; e. on the mixed problem ---------------------------------------------------------------------------------------------------------
def test_d_block_sparse_placement():
    """NLLS_FLAG_FORCE_SPARSE over variables of 1, 64, 64, 257 and 512 unknowns (the two of 64: one group of two blocks, aoff[1] != aoff[0]), each length under its own
    kernel: no size class holds half of the blocks, so nothing is eliminated and every variable's diagonal block is stored in full -- both triangles against the
    reference, nlls_get_bsm_index against the oracle's"""
    dims = (1, 64, 64, 257, 512); kern = {1: "none", 64: "huber", 257: "geman", 512: "scaled_huber2o"}
    mags = dict(zip(range(1, 6), (MAGS[1], MAGS[0], MAGS[1], MAGS[0], MAGS[1]))); rng = np.random.default_rng(41); p = N.NLLSProblem()
    for v, n in enumerate(dims, 1): p.addvariable(start(n, mags[v], rng), K.VAR_DYNAMIC)
    for v, n in enumerate(dims, 1): add_all_kinds(p, v, mags[v], KERNELS[kern[n]], rng, tag=v)
    ref = problem_reference(p); check_regions(ref, mags)
    assert max(len(g["varind"]) for g in p.groups()) == 2
    for n in sorted(set(dims)): print(f"\nLENGTH d n={n} kernel={kern[n]} kinds={names(kinds_at(n))}", end="")
    print()
    ctx, info, bi = upload(p, flags=_capi.FLAG_FORCE_SPARSE)
    try:
        ols = oracle_problem(p).linear_system(bi, _capi.FLAG_FORCE_SPARSE)
        assert info.is_sparse == 1 and ols.info.is_sparse and info.has_schur == 0 and info.nblocks_stored == len(dims)
        assert info.ndof == sum(dims) and info.nnz_data == sum(n * n for n in dims) == ols.info.nnz_data
        for g, o in zip(ctx.bsm_index(), ols.bsm_index()): assert np.array_equal(g, o)
        hold("d", "sweep_gradhess cost", max(dims), ctx.sweep_gradhess(), ref["cost"], ref["cost_abs"], "forced sparse")
        hold_linearisation("d", ctx, info, p, bi, ref, "forced sparse")
    finally:
        ctx.close()


def test_d_e_bundle_adjustment_with_dynamic_variables():
    """a small sparse bundle adjustment (10 cameras x 50 points, Huber; points eliminated) with dynamic variables of 257 and 300 unknowns beside it: their full
    diagonal blocks sit in the reduced system next to the cameras.  The index arrays and the whole of A.data and b against the oracle (at the neighbours' 1e-11),
    the two dynamic blocks against the long-double reference at the bound; then case e."""
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 50, 0.3, seed=1, robust=N.HuberKernel(0.05), outlier_frac=0.05, outlier_sigma=0.05), 1e-3, 1e-3)
    nba = p.nvariables; rng = np.random.default_rng(43); dims = (257, 300); mags = {nba + 1: MAGS[0], nba + 2: MAGS[1]}
    for q, n in enumerate(dims): p.addvariable(start(n, mags[nba + 1 + q], rng), K.VAR_DYNAMIC)
    for q, n in enumerate(dims): add_all_kinds(p, nba + 1 + q, mags[nba + 1 + q], KERNELS["huber"], rng, tag=q)
    ref = problem_reference(p); check_regions(ref, mags)
    for n in dims: print(f"\nLENGTH d/e n={n} (beside a bundle adjustment) kinds={names(kinds_at(n))}", end="")
    print()
    ctx, info, bi = upload(p)
    try:
        ols = oracle_problem(p).linear_system(bi, 0); c_ora = ols.costgradhess()
        assert info.is_sparse == 1 and ols.info.is_sparse and info.has_schur == 1 and info.nreduced_dof == 60 + sum(dims)
        for g, o in zip(ctx.bsm_index(), ols.bsm_index()): assert np.array_equal(g, o)
        c = ctx.sweep_gradhess()
        assert np.isclose(c, c_ora, rtol=RTOL, atol=1e-300)
        assert rel(ctx.get_bsm_data(), ols.data) < RTOL and rel(ctx.get_grad(), ols.b) < RTOL
        hold_linearisation("d", ctx, info, p, bi, ref, "beside a bundle adjustment")
        step_and_trial("e", ctx, info, p, "bundle adjustment + 257 + 300")
    finally:
        ctx.close()


# ---- f. nlls_set_cost_data on long records ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n", [(K.RES_DYN_LINEAR, 15), (K.RES_DYN_LINEAR, 16), (K.RES_DYN_LINEAR, 17), (K.RES_DYN_LINEAR, 511), (K.RES_DYN_LINEAR, 512),
                                    (K.RES_DYN_LINEARSQ, 23), (K.RES_DYN_LINEARSQ, 512)], ids=["linear15", "linear16", "linear17", "linear511", "linear512", "linearsq23", "linearsq512"])
def test_f_set_cost_data(kind, n):
    """The payload of three blocks replaced on the device: all of them, then blocks 3 and 1 through an index.  DYN_LINEAR, ndata = 1 + n: 16 is the last record a lane
    moves alone, 17 / 18 the first odd / even ones a wavefront moves, 512 / 513 one and two chunks; DYN_LINEARSQ, ndata = n + n^2: 552 doubles (2 chunks) and
    262656 (513).  After each update the cost sweep and nlls_eval_blocks (the cost-order copy) and the gradient sweep (the dense list's copy) against the reference
    on the data now in place: the block the index leaves out keeps the payload of the first update.  Four more variables of other lengths keep every size class under
    half of the blocks (nothing is eliminated where the system is block-sparse)."""
    ndata = 1 + n if kind == K.RES_DYN_LINEAR else n + n * n; nch = -(-ndata // UPD_WAVE_CHUNK)
    print(f"\nLENGTH f n={n} kind={KIND_NAME[kind]} ndata={ndata} " + ("one lane per record" if ndata <= UPD_LANE_MAX else f"{nch} chunk(s) per record"))
    nv = 3; mags = {1: MAGS[1], 2: MAGS[0], 3: MAGS[1]}; rng = np.random.default_rng(600 + n); p = N.NLLSProblem(); robust = KERNELS["huber"]
    for v in range(1, nv + 1): p.addvariable(start(n, mags[v], rng), K.VAR_DYNAMIC)
    for v in range(1, nv + 1): p.addcosts(kind, [[v]], payload(kind, p.variable(v).copy(), mags[v], rng, tag=v)[None, :], robust=robust)
    p.addcosts(K.RES_DYN_NORM, np.arange(1, nv + 1)[:, None], np.zeros((nv, 0)))
    for m in (3, 5, 7, 9):
        v = p.addvariable(start(m, 1.0, rng), K.VAR_DYNAMIC)
        p.addcosts(K.RES_DYN_LINEAR, [[v]], payload(K.RES_DYN_LINEAR, p.variable(v).copy(), 1.0, rng)[None, :]); p.addcosts(K.RES_DYN_NORM, [[v]], np.zeros((1, 0)))
    g0 = p.groups(); assert g0[0]["res_kind"] == kind and g0[0]["data"].shape == (nv, ndata)
    fresh = lambda v, tag: payload(kind, p.variable(v).copy(), mags[v], rng, tag=tag)
    d1 = np.stack([fresh(v, 10 + v) for v in range(1, nv + 1)])
    index = np.array([3, 1]); d2rows = np.stack([fresh(int(v), 20 + int(v)) for v in index]); d2 = d1.copy(); d2[index - 1] = d2rows
    with_data = lambda da: [dict(g0[0], data=np.ascontiguousarray(da))] + g0[1:]
    ctx, info, bi = upload(p)
    def check(groups, where):
        ref = problem_reference(p, groups=groups); check_regions(dict(ref, blocks=[b for b in ref["blocks"] if b["var"] <= nv]), mags)
        c = ctx.sweep_cost(); hold("f", "sweep_cost", n, c, ref["cost"], ref["cost_abs"], where)
        ev = ctx.eval_blocks(0)
        for b in (b for b in ref["blocks"] if b["group"] == 0):
            hold("f", "r", n, ev["r"][b["index"]], b["r"], b["r_abs"], f"{where} block {b['index']}")
        hold("f", "sweep_gradhess cost", n, ctx.sweep_gradhess(), ref["cost"], ref["cost_abs"], where)
        b, H = hold_linearisation("f", ctx, info, p, bi, ref, where, variables=range(1, nv + 1))
        return c, b
    try:
        c0, b0 = check(g0, "as uploaded")
        ctx.set_cost_data(0, d1)
        c1, b1 = check(with_data(d1), "all replaced")
        ctx.set_cost_data(0, d2rows, index)
        c2, b2 = check(with_data(d2), "blocks 3 and 1 replaced")
        # the data moved by far more than the tolerance, so a copy the scatter missed would have failed above; and the block left out did not move
        off = dof_offsets(p, bi)
        for v in range(1, nv + 1):
            s = slice(off[v - 1], off[v - 1] + n)
            assert rel(b1[s], b0[s]) > 1e-6, v
            assert (rel(b2[s], b1[s]) > 1e-6) == (v in index), v
    finally:
        ctx.close()


# ---- g. limits ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_g_limits():
    """what nlls_upload_structure refuses, with NLLS_ERR_UNSUPPORTED and its message: a variable of 4097 unknowns, DYN_LINEARSQ at 513, two blocks of one group over
    variables of different lengths, a robust kernel on the non-squared cost; the same context then takes a valid upload and sweeps correctly"""
    def norm_problem(dims):
        p = N.NLLSProblem()
        for n in dims: p.addvariable(np.full(n, 0.5), K.VAR_DYNAMIC)
        return p
    cases = []
    p = norm_problem([DYN_MAX + 1]); p.addcosts(K.RES_DYN_NORM, [[1]], np.zeros((1, 0)))
    cases.append((p, p.groups(), "block larger than MAX_BLOCK_SZ"))
    p = norm_problem([SQ_MAX + 1]); m = SQ_MAX + 1; p.addcosts(K.RES_DYN_LINEARSQ, [[1]], np.zeros((1, m + m * m)))
    cases.append((p, p.groups(), "NLLS_RES_DYN_LINEARSQ: variable longer than 512"))
    p = norm_problem([64, 65])
    cases.append((p, [dict(res_kind=K.RES_DYN_NORM, robust_kind=K.ROBUST_NONE, robust_params=(0.0, 0.0, 0.0, 0.0), varind=np.array([[1], [2]], np.int64), data=np.zeros((2, 0)))],
                  "dynamic-size blocks of one group must share the variable length"))
    p = norm_problem([64]); p.addcosts(K.COST_DYN_LINEAR, [[1]], np.ones((1, 64))); h = KERNELS["huber"]
    cases.append((p, [dict(p.groups()[0], robust_kind=h.kind, robust_params=h.params)], "a non-squared cost takes no robust kernel"))
    ctx = _capi.Context()
    try:
        for p, groups, message in cases:
            with pytest.raises(_capi.NllsError) as e:
                ctx.upload(p.var_kind, p.var_dim, blockindices(p), groups, 0)
            assert e.value.code == _capi.ERR_UNSUPPORTED and message in str(e.value), (message, str(e.value))
        n = 257; p = one_variable_problem(n, "huber", MAGS[1]); ref = problem_reference(p); bi = blockindices(p)
        info = ctx.upload(p.var_kind, p.var_dim, bi, p.groups(), 0); ctx.set_variables(p.variables)
        hold("g", "sweep_cost", n, ctx.sweep_cost(), ref["cost"], ref["cost_abs"], "after four refusals")
        hold("g", "sweep_gradhess cost", n, ctx.sweep_gradhess(), ref["cost"], ref["cost_abs"], "after four refusals")
        hold_linearisation("g", ctx, info, p, bi, ref, "after four refusals")
    finally:
        ctx.close()
