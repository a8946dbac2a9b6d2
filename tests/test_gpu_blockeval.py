"""nlls_eval_blocks: computeresidual, r'r, robustify and rho' of every cost block, in the caller's upload order (include/nlls_amd.h), against the CPU oracle's
oracle_block_resjac / oracle_robustify / oracle_robustifydcost (adaptive kinds: oracle_robustifydkernel, whose value is robustify and whose last gradient entry is rho').

Tolerances: r to 1e-13 * max(1, max |data of the block|) -- what check_problem asks of the retraction (tests/test_gpu_parity.py), scaled by the terms that cancel in a
small residual; r'r, rho, rho' to the project's cost tolerance rtol 1e-11 against the oracle evaluated at the oracle's r, r'r with an absolute floor of
1e-13 * max(1, max |data|)^2.  The oracle's block_resjac holds fixed-size kinds only; the dynamic-size residuals are restated in numpy here: NormResidual is the variable
itself (exact), and for X'w - y / X w - y the rounding of an n-term dot product is bounded by (n + 1) u sum |X_i w_i| <= 1e-13 * max(1, sum |X_i w_i| + |y|) at n = 5."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import synthetic, _capi
from nllssolver_jl_amd.variables import contaminated_gaussian
from oracle import oracle as O
from tests.helpers import oracle_problem, blockindices

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-11


def oracle_group_values(p, op, gi, variables):
    """(r, r'r, rho, rho') of every block of group gi by the oracle, at `variables` (which `op` holds as its current set)."""
    g = list(p.costs.values())[gi]; vi, da = g.arrays(); off = p.var_offsets
    M = K.res_nres(g.res_kind); n = vi.shape[0]; L = O.lib()
    par = np.array(list(g.robust.params) + [0.0] * 4, dtype=np.float64)[:4]
    r = np.zeros((n, M)); sq = np.zeros(n); rho = np.zeros(n); w = np.zeros(n)
    for ci in range(n):
        r[ci], _ = op.block_resjac(gi, ci, M)
        sq[ci] = float(r[ci] @ r[ci])
        if g.res_kind in K.ADAPTIVE_KINDS:
            kst = np.ascontiguousarray(variables[off[vi[ci, 0] - 1]:off[vi[ci, 0] - 1] + 3])
            val = C.c_double(); dc = np.zeros(4); d2c = np.zeros(16)
            L.oracle_robustifydkernel(O._p(kst), sq[ci], C.byref(val), O._p(dc), O._p(d2c))
            rho[ci], w[ci] = val.value, dc[3]
        else:
            o3 = np.zeros(3)
            rho[ci] = L.oracle_robustify(int(g.robust.kind), O._p(par), sq[ci])
            L.oracle_robustifydcost(int(g.robust.kind), O._p(par), sq[ci], O._p(o3)); w[ci] = o3[1]
    return r, sq, rho, w


def compare(tag, dev, ref, scale):
    """dev: the dict of Context.eval_blocks; ref: (r, sq, rho, w); scale: max(1, max |data of the block|) per block"""
    r, sq, rho, w = ref
    er = np.max(np.abs(dev["r"] - r) / scale[:, None]) if r.size else 0.0
    esq = np.max((np.abs(dev["sqerr"] - sq) - 1e-13 * scale ** 2) / np.maximum(np.abs(sq), 1e-300)) if sq.size else 0.0
    erho = np.max(np.abs(dev["rho"] - rho) / np.maximum(np.abs(rho), 1e-300)) if rho.size else 0.0
    ew = np.max(np.abs(dev["weight"] - w) / np.maximum(np.abs(w), 1e-300)) if w.size else 0.0
    print(f"BLOCKEVAL {tag}: n={sq.size} r {er:.3e} (of 1e-13) sqerr {esq:.3e} rho {erho:.3e} weight {ew:.3e} (of {RTOL:.0e})")
    assert er <= 1e-13, (tag, "r", er)
    assert esq <= RTOL, (tag, "sqerr", esq)
    assert erho <= RTOL, (tag, "rho", erho)
    assert ew <= RTOL, (tag, "weight", ew)


def check_against_oracle(tag, p, unfixed=None, flags=0):
    bi = blockindices(p, unfixed); op = oracle_problem(p)
    ctx = _capi.Context(); ctx.upload(p.var_kind, p.var_dim, bi, p.groups(), flags); ctx.set_variables(p.variables)
    rhos = []
    for gi, g in enumerate(p.costs.values()):
        _, da = g.arrays()
        scale = np.maximum(1.0, np.max(np.abs(da), axis=1)) if da.shape[1] else np.ones(da.shape[0])
        dev = ctx.eval_blocks(gi)
        assert dev["r"].shape == (len(g), K.res_nres(g.res_kind))
        compare(f"{tag}[{gi}]", dev, oracle_group_values(p, op, gi, p.variables), scale)
        again = ctx.eval_blocks(gi)
        assert all(dev[k].tobytes() == again[k].tobytes() for k in dev), "two calls differ"
        only = ctx.eval_blocks(gi, want="sqerr")                                # (any pointer may be NULL)
        assert list(only) == ["sqerr"] and only["sqerr"].tobytes() == dev["sqerr"].tobytes()
        rhos.append(dev["rho"])
    total = 0.5 * math.fsum(np.concatenate(rhos).tolist()); sweep = ctx.sweep_cost()
    print(f"BLOCKEVAL {tag}: 0.5 sum rho {total!r} sweep {sweep!r}")
    assert np.isclose(total, sweep, rtol=RTOL, atol=0.0), (total, sweep)
    assert np.isclose(sweep, op.cost(), rtol=RTOL)
    ctx.close()


def adaptive_mean_problem(kernel=(0.5, 5.0, 0.6), means=(0.0, 0.0), extra=None, draws=(800, 200)):
    """the data of test/adaptivecost.jl:29-38 as tests/test_gpu_functional.py::test_adaptivecost draws it (draws: inliers, outliers; two blocks per draw)"""
    rng = np.random.default_rng(1)
    pts = np.concatenate([rng.standard_normal(draws[0]), rng.standard_normal(draws[1]) * 10.0])
    p = N.NLLSProblem()
    p.addvariable(contaminated_gaussian(*kernel), K.VAR_CONTAMINATED_GAUSSIAN)
    p.addvariable(means[0]); p.addvariable(means[1])
    vi = np.empty((2 * pts.size, 2), np.int64); da = np.empty((2 * pts.size, 1))
    vi[:, 0] = 1; vi[0::2, 1] = 2; vi[1::2, 1] = 3; da[0::2, 0] = pts - 1; da[1::2, 0] = pts + 1
    if extra is not None:
        da[0, 0] = extra
    p.addcosts(K.RES_ADAPTIVE_MEAN, vi, da)
    return p


def test_affine_ba_huber_two_groups_some_fixed():
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3, robust=N.HuberKernel(0.002)), 1e-3, 1e-3)
    (g,) = p.costs.values(); vi, da = g.arrays()
    rng = np.random.default_rng(4); pick = rng.choice(vi.shape[0], 150, replace=False)
    p.addcosts(K.RES_BA_AFFINE, vi[pick], da[pick] + 0.01 * rng.standard_normal((150, 2)), N.GemanMcclureKernel(0.01))
    unfixed = np.ones(p.nvariables, bool); unfixed[[0, 1]] = False; unfixed[10:40] = False      # two cameras and thirty points: some blocks have no free variable
    assert len(p.costs) == 2 and np.any(~unfixed[vi[:, 0] - 1] & ~unfixed[vi[:, 1] - 1])
    check_against_oracle("affine+huber", p, unfixed)


def test_ba_so3_scaled_geman_mcclure():
    p = synthetic.create_so3_ba_problem(8, 300, 0.3, seed=5, adaptive=False, robust=N.Scaled(N.GemanMcclureKernel(0.01), 2.5))
    check_against_oracle("ba_so3+scaled gm", p)


def test_ba_so3_adaptive():
    check_against_oracle("ba_so3_adaptive", synthetic.create_so3_ba_problem(8, 300, 0.3, seed=6, adaptive=True))


def test_adaptive_mean():
    check_against_oracle("adaptive_mean", adaptive_mean_problem(means=(-0.7, 0.6)))


def test_scale_mix():
    from tests.test_oracle_pins import scale_mix_problem
    check_against_oracle("scale_mix", scale_mix_problem(8, n=64, noise=1e-3, shared=3, robust=N.HuberKernel(0.05)))


def test_dynamic_kinds():
    """NormResidual (nres = n), LinearResidual X'w - y (nres 1), LinearResidualDynamic X w - y (nres n): against numpy and the oracle's kernels and cost"""
    rng = np.random.default_rng(9); n = 5; nv = 7
    p = N.NLLSProblem(); W = rng.standard_normal((nv, n))
    for k in range(nv):
        p.addvariable(W[k], K.VAR_DYNAMIC)
    rob = N.HuberKernel(1.5)
    X = rng.standard_normal((nv, n)); y = rng.standard_normal(nv); Xs = rng.standard_normal((nv, n, n)); ys = rng.standard_normal((nv, n))
    idx = np.arange(1, nv + 1, dtype=np.int64)[:, None]
    p.addcosts(K.RES_DYN_NORM, idx, np.zeros((nv, 0)), rob)
    p.addcosts(K.RES_DYN_LINEAR, idx, np.concatenate([y[:, None], X], axis=1), rob)
    p.addcosts(K.RES_DYN_LINEARSQ, idx, np.concatenate([ys, Xs.transpose(0, 2, 1).reshape(nv, n * n)], axis=1), N.GemanMcclureKernel(2.0))
    ref_r = [W.copy(), ((X * W).sum(1) - y)[:, None], np.einsum("kij,kj->ki", Xs, W) - ys]
    scale = [np.ones(nv), np.maximum(1.0, np.abs(X * W).sum(1) + np.abs(y)), np.maximum(1.0, np.abs(np.einsum("kij,kj->kij", Xs, W)).sum(2).max(1) + np.abs(ys).max(1))]
    ctx = _capi.Context(); ctx.upload(p.var_kind, p.var_dim, blockindices(p), p.groups()); ctx.set_variables(p.variables)
    L = O.lib(); rhos = []
    for gi, g in enumerate(p.costs.values()):
        dev = ctx.eval_blocks(gi)
        assert dev["r"].shape == ref_r[gi].shape
        if gi == 0:
            assert np.array_equal(dev["r"], W), "NormResidual is the variable itself"
        par = np.array(list(g.robust.params) + [0.0] * 4)[:4]; sq = (ref_r[gi] ** 2).sum(1)
        rho = np.array([L.oracle_robustify(int(g.robust.kind), O._p(par), float(s)) for s in sq]); w = np.zeros(nv)
        for k, s in enumerate(sq):
            o3 = np.zeros(3); L.oracle_robustifydcost(int(g.robust.kind), O._p(par), float(s), O._p(o3)); w[k] = o3[1]
        compare(f"dyn[{gi}]", dev, (ref_r[gi], sq, rho, w), scale[gi])
        rhos.append(dev["rho"])
    total = 0.5 * math.fsum(np.concatenate(rhos).tolist())
    assert np.isclose(total, ctx.sweep_cost(), rtol=RTOL) and np.isclose(total, oracle_problem(p).cost(), rtol=RTOL)
    ctx.close()


def chain_problem():
    return synthetic.perturb_ba_problem(synthetic.create_ba_problem(120, 3000, 0.06, seed=2, robust=N.HuberKernel(0.002)), 1e-3, 1e-3)


def test_output_order_is_upload_order():
    """the sweeps of a matrix-free Schur problem stream the blocks in elimination order; the outputs follow the caller's order: permute the blocks, they permute too"""
    p = chain_problem(); (g,) = p.costs.values(); vi, da = g.arrays()
    perm = np.random.default_rng(12).permutation(vi.shape[0])
    q = chain_problem(); (gq,) = q.costs.values(); gq.set_arrays(vi[perm].copy(), da[perm].copy())
    outs = []
    for prob in (p, q):
        ctx = _capi.Context(); ctx.upload(prob.var_kind, prob.var_dim, blockindices(prob), prob.groups()); ctx.set_variables(prob.variables)
        ctx.sweep_gradhess(); ctx.lm_trial(1e-3)
        assert ctx.solve_stats()["mf_trials"] == 1, "the chain should take the matrix-free trial"
        outs.append(ctx.eval_blocks(0)); ctx.close()
    for k in ("r", "sqerr", "rho", "weight"):
        assert np.array_equal(outs[1][k], outs[0][k][perm]), k


def _trial_run(p, flags, call, materialise=False):
    """sweep, trial, accept, sweep (the look-ahead sweep of the accepted trial is in A and b), [the calls under test], trial"""
    ctx = _capi.Context(); ctx.upload(p.var_kind, p.var_dim, blockindices(p), p.groups(), flags); ctx.set_variables(p.variables)
    if materialise:
        ctx.set_option(_capi.OPT_MATERIALIZE, 1)
    ctx.copy_variables(_capi.VARS_NEXT, _capi.VARS_CURRENT)
    c0 = ctx.sweep_gradhess(); lam = 1e-6 * ctx.max_abs_diag()
    c1 = ctx.lm_trial(lam); ctx.swap_variables(_capi.VARS_CURRENT, _capi.VARS_NEXT); ctx.sweep_gradhess(want_cost=False)
    if call:
        for gi in range(len(p.costs)):
            ctx.eval_blocks(gi, _capi.VARS_CURRENT); ctx.eval_blocks(gi, _capi.VARS_NEXT, want=("sqerr",))
    c2 = ctx.lm_trial(lam)
    out = (c0, c1, c2, ctx.get_step().tobytes(), ctx.get_variables(_capi.VARS_NEXT).tobytes()); ctx.close()
    return out


def _same_trial(tag, a, b, c):
    """a, b: two runs without the call, c: the run with it.  The library's trials are reproducible to rounding, not always to the bit (LDS and HBM atomic adds in the
    sweeps and the assembly: include/nlls_amd.h, NLLS_FLAG_DETERMINISTIC; two runs without the call were seen to differ in the trial cost's last digits): bit-equality
    says nothing there, and the run with the call must lie as close to them as a trial is asked to (check_problem: 1e-9).  The exact comparison is
    test_reads_only_between_sweep_and_trial."""
    print(f"BLOCKEVAL reads-only {tag}: runs without the call bit-identical {a == b}; trial costs {a[:3]} / {c[:3]}")
    if c != a:
        assert np.allclose(c[:3], a[:3], rtol=1e-9) and np.allclose(np.frombuffer(c[4]), np.frombuffer(a[4]), rtol=1e-9, atol=1e-12)


def test_reads_only_between_sweep_and_trial():
    """a call between a sweep and nlls_lm_trial leaves the trial's cost and step bit-identical to a run without it.  On 60 blocks of the adaptive-mean fixture: the small
    dense system's sweep sums a workgroup's blocks with LDS atomic adds, whose order is fixed only while one wavefront holds them all -- there the trial is reproducible
    to the bit and the comparison is exact, unconditionally."""
    p = adaptive_mean_problem(means=(-0.4, 0.3), draws=(24, 6))
    a, b, c = (_trial_run(p, 0, call) for call in (False, False, True))
    assert a == b, "the trial without the call is not reproducible"
    assert c == a


def test_reads_only_on_the_full_fixture():
    """... and on all 2000 blocks (several wavefronts per workgroup: see _same_trial)"""
    p = adaptive_mean_problem(means=(-0.4, 0.3))
    _same_trial("small dense", *(_trial_run(p, 0, call) for call in (False, False, True)))


@pytest.mark.parametrize("materialise", [False, True])
def test_reads_only_on_a_schur_problem(materialise):
    """the same on the bundle-adjustment chain: the matrix-free trial, and the materialised one"""
    p = chain_problem()
    _same_trial(f"chain, materialise {materialise}", *(_trial_run(p, _capi.FLAG_DETERMINISTIC, call, materialise) for call in (False, False, True)))


def test_errors():
    L = _capi.lib()
    ctx = _capi.Context()
    out = np.zeros(8)
    assert L.nlls_eval_blocks(ctx.h, 0, 0, None, _capi._p(out), None, None) == _capi.ERR_NOT_READY          # no upload yet
    st = np.zeros(3)
    assert L.nlls_adaptive_em(ctx.h, 0, 1, 1, _capi._p(st), None) == _capi.ERR_NOT_READY
    p = N.NLLSProblem(); p.addvariable([0.1, 0.2, 0.3]); p.addvariable([1.0, 2.0, 3.0, 4.0], K.VAR_DYNAMIC)
    rng = np.random.default_rng(2)
    p.addcosts(K.RES_LINEAR3, [[1]], rng.standard_normal((1, 12)))
    p.addcosts(K.COST_LINEAR3, [[1]], rng.standard_normal((1, 3)))
    p.addcosts(K.COST_DYN_LINEAR, [[2]], rng.standard_normal((1, 4)))
    ctx.upload(p.var_kind, p.var_dim, blockindices(p), p.groups()); ctx.set_variables(p.variables)
    assert ctx.eval_blocks(0)["r"].shape == (1, 3)
    for bad, code in ((1, _capi.ERR_UNSUPPORTED), (2, _capi.ERR_UNSUPPORTED), (3, _capi.ERR_INVALID_ARG), (-1, _capi.ERR_INVALID_ARG)):
        assert L.nlls_eval_blocks(ctx.h, 0, bad, None, _capi._p(out), None, None) == code, bad
    assert L.nlls_eval_blocks(ctx.h, 0, 0, None, None, None, None) == _capi.ERR_INVALID_ARG                  # all NULL
    assert L.nlls_eval_blocks(ctx.h, 7, 0, None, _capi._p(out), None, None) == _capi.ERR_INVALID_ARG
    assert L.nlls_adaptive_em(ctx.h, 0, 1, 1, _capi._p(st), None) == _capi.ERR_INVALID_ARG                   # not a ContaminatedGaussian variable
    with pytest.raises(_capi.NllsError):
        ctx.eval_blocks(1)
    ctx.close()


def test_public_functions():
    p = adaptive_mean_problem(means=(-0.7, 0.6)); (g,) = p.costs.values(); vi, da = g.arrays()
    r = N.residuals(p, 0); sq = N.squarederrors(p, 0)
    assert np.array_equal(r[:, 0], p.variables[1 + vi[:, 1]] - da[:, 0]) and np.array_equal(sq, r[:, 0] ** 2)
    assert len(N.residuals(p)) == 1 and np.array_equal(N.squarederrors(p)[0], sq)


def test_user_kind_in_a_process_of_its_own():
    userlib = os.path.join(ROOT, "nllssolver.jl_amd", "csrc", "libnlls_amd_userdemo.so")
    env = dict(os.environ, NLLS_AMD_LIB=userlib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "blockeval_userkind_worker.py")], capture_output=True, text=True, env=env, timeout=600)
    print(out.stdout[-1500:])
    assert out.returncode == 0 and "user kind block values ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
