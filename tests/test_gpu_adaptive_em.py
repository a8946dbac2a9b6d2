"""nlls_adaptive_em: optimize(kernel::ContaminatedGaussian, squarederrors, maxiters) of src/robustadaptive.jl:48-73 on the device, against its host mirror
variables.contaminated_gaussian_em (pinned by tests/test_host_logic.py) fed with the device's own squared errors (nlls_eval_blocks).

Pass counts are compared only where the host mirror's convergence ratios norm(old - new) / (1e-6 max(norm old, norm new)) stay 10 % clear of 1: a different
summation order cannot move the count then.  Fixture A (the data of test/adaptivecost.jl, kernel (0.5, 5.0, 0.6)): means (0, 0) -- 10 passes at maxiters = 10, 26 at 50,
last ratios 2.16, 1.17, 0.63; means (-1, 1) -- 22 passes, last ratios 1.26, 0.645.  The storage is held to the project's cost tolerance, rtol 1e-11: EM is a contraction
near its fixed point, so the summation error of a pass does not grow over the passes."""
import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import synthetic, _capi
from nllssolver_jl_amd.variables import contaminated_gaussian, contaminated_gaussian_em, contaminated_gaussian_params
from tests.helpers import blockindices
from tests.test_gpu_blockeval import adaptive_mean_problem

pytestmark = pytest.mark.gpu
CUR, NXT, BST = _capi.VARS_CURRENT, _capi.VARS_NEXT, _capi.VARS_BEST
RTOL = 1e-11


def host_em_ratios(storage, err, maxiters):
    """the host mirror, pass by pass: (storage after the last pass, passes made, the convergence ratio of every pass)"""
    k = np.array(storage, dtype=np.float64); old = contaminated_gaussian_params(k); ratios = []
    for it in range(maxiters):
        k1 = contaminated_gaussian_em(k, err, 1)
        # the unordered new parameters of this pass: what isapprox compares (the constructor's swap only reorders the two sigmas)
        is1, is2, w = k; wr = ((1 - w) * is2) / (is1 * w); h = -0.5 * (is2 * is2 - is1 * is1)
        with np.errstate(over="ignore"):
            lat = 1.0 / (1.0 + wr * np.exp(h * err))
        s1 = float((lat * err).sum()); tw = float(lat.sum())
        new = np.array([np.sqrt(s1 / tw), np.sqrt((float(err.sum()) - s1) / (err.size - tw)), tw / err.size])
        ratios.append(float(np.linalg.norm(old - new) / (1e-6 * max(np.linalg.norm(old), np.linalg.norm(new)))))
        k = k1; old = new
        if ratios[-1] <= 1.0:
            break
    return k, len(ratios), ratios


def clear_of_threshold(ratios):
    return all(abs(r - 1.0) > 0.1 for r in ratios)


def context(p, unfixed=None, flags=0):
    ctx = _capi.Context(); ctx.upload(p.var_kind, p.var_dim, blockindices(p, unfixed), p.groups(), flags)
    ctx.set_variables(p.variables, CUR); ctx.copy_variables(NXT, CUR); ctx.copy_variables(BST, CUR)
    return ctx


@pytest.mark.parametrize("means,expect", [((0.0, 0.0), {0: 0, 1: 1, 10: 10, 50: 26}), ((-1.0, 1.0), {50: 22})])
def test_fixture_a_against_host_mirror(means, expect):
    p = adaptive_mean_problem(means=means)
    for maxiters, passes in expect.items():
        ctx = context(p)
        err = ctx.eval_blocks(0, NXT, want="sqerr")["sqerr"]
        ref = contaminated_gaussian_em(p.variables[:3], err, maxiters)
        _, n_host, ratios = host_em_ratios(p.variables[:3], err, maxiters)
        st, n_dev = ctx.adaptive_em(1, NXT, maxiters)
        print(f"EM fixture A means {means} maxiters {maxiters}: passes host {n_host} device {n_dev}, last ratios {[f'{r:.3g}' for r in ratios[-3:]]}, "
              f"storage err {np.max(np.abs(st - ref) / np.abs(ref)):.3e}")
        assert n_host == passes and clear_of_threshold(ratios), (n_host, ratios[-3:])
        assert n_dev == n_host
        assert np.allclose(st, ref, rtol=RTOL, atol=0.0), (st, ref)
        # the set written is the set named; every other double, and the other two sets, untouched
        v = ctx.get_variables(NXT)
        assert np.array_equal(v[:3], st) and np.array_equal(v[3:], p.variables[3:])
        if maxiters == 0:
            assert np.array_equal(st, p.variables[:3])
        assert np.array_equal(ctx.get_variables(CUR), p.variables) and np.array_equal(ctx.get_variables(BST), p.variables)
        ctx.close()


def test_constructor_ordering():
    """a kernel stored unordered (1/sigma1 < 1/sigma2): the first pass uses it as stored, the result is stored narrowest Gaussian first"""
    p = adaptive_mean_problem()
    ctx = context(p)
    start = p.variables.copy(); start[:3] = (1.0 / 5.0, 1.0 / 0.5, 0.4)
    ctx.set_variables(start, CUR)
    err = ctx.eval_blocks(0, CUR, want="sqerr")["sqerr"]
    ref = contaminated_gaussian_em(start[:3], err, 1)
    st, n = ctx.adaptive_em(1, CUR, 1)
    new = contaminated_gaussian_params(st)
    print(f"EM ordering: storage {st} (sigma {new})")
    assert n == 1 and st[0] >= st[1] and np.allclose(st, ref, rtol=RTOL, atol=0.0)
    # ... and the swap did happen: the pass from the unordered kernel leaves sigma1 > sigma2 before the constructor
    is1, is2, w = start[:3]; lat = 1.0 / (1.0 + ((1 - w) * is2) / (is1 * w) * np.exp(-0.5 * (is2 * is2 - is1 * is1) * err))
    s1 = np.sqrt((lat * err).sum() / lat.sum()); s2 = np.sqrt((err.sum() - (lat * err).sum()) / (err.size - lat.sum()))
    assert s1 > s2
    assert np.array_equal(ctx.get_variables(CUR)[:3], st)
    ctx.close()


def test_one_pass_does_not_raise_the_cost():
    """one-dimensional residuals: the M-step is the exact maximiser, so cost(VARS_NEXT) does not rise (1e-11 relative for the sums' rounding)"""
    ctx = context(adaptive_mean_problem())
    before = ctx.sweep_cost(NXT)
    ctx.adaptive_em(1, NXT, 1)
    after = ctx.sweep_cost(NXT)
    print(f"EM monotone: {before!r} -> {after!r}")
    assert after <= before + 1e-11 * abs(before)
    ctx.close()


def test_bit_reproducible():
    p = adaptive_mean_problem(means=(-0.3, 0.2)); out = []
    for _ in range(2):
        ctx = context(p); st, n = ctx.adaptive_em(1, NXT, 10); out.append((st.tobytes(), n)); ctx.close()
    assert out[0] == out[1]
    ctx = context(p); a = ctx.adaptive_em(1, NXT, 10); ctx.copy_variables(NXT, CUR); b = ctx.adaptive_em(1, NXT, 10); ctx.close()      # (the same context, its scratch reused)
    assert a[0].tobytes() == b[0].tobytes() == out[0][0] and a[1] == b[1]


def test_far_outlier():
    """exp() overflows to Inf for the far outlier: its weight is exactly 0, the parameters stay finite and equal to the host mirror's"""
    p = adaptive_mean_problem(extra=1e6)
    ctx = context(p)
    err = ctx.eval_blocks(0, NXT, want="sqerr")["sqerr"]
    assert err.max() > 1e11
    ref = contaminated_gaussian_em(p.variables[:3], err, 10)
    _, n_host, ratios = host_em_ratios(p.variables[:3], err, 10)
    st, n = ctx.adaptive_em(1, NXT, 10)
    print(f"EM far outlier: storage {st} host {ref} passes {n}/{n_host} last ratios {[f'{r:.3g}' for r in ratios[-3:]]}")
    assert np.all(np.isfinite(st)) and np.allclose(st, ref, rtol=RTOL, atol=0.0)
    if clear_of_threshold(ratios):
        assert n == n_host
    ctx.close()


def _transition_run(p, unfixed, flags, em, given=None):
    """sweep, trial, accept, sweep, trial (its look-ahead sweep is now pending), then CURRENT rewritten -- by EM or by nlls_set_variables --, then the trial under test"""
    ctx = context(p, unfixed, flags)
    ctx.sweep_gradhess(); lam = 1e-4 * ctx.max_abs_diag()
    c1 = ctx.lm_trial(lam); ctx.swap_variables(CUR, NXT); ctx.sweep_gradhess(want_cost=False)
    c2 = ctx.lm_trial(lam)
    if em:
        st, n = ctx.adaptive_em(1, CUR, 3); assert n == 3
    else:
        ctx.set_variables(given, CUR)
    written = ctx.get_variables(CUR)
    c3 = ctx.lm_trial(lam)
    out = (c1, c2, c3, ctx.get_step().tobytes(), ctx.get_variables(NXT).tobytes(), written.tobytes()); ctx.close()
    return written, out


def _same_transition(tag, p, unfixed, flags):
    """The library's trials on these sizes are reproducible to rounding, not to the bit (atomic adds in the sweeps and the assembly; two runs of the nlls_set_variables
    route were seen to differ in the step's last bits, and to agree by luck): the variables written must be identical, the trial behind them as close as a trial is
    asked to be (check_problem: 1e-9).  The exact comparison is test_state_transition_like_set_variables."""
    written, a = _transition_run(p, unfixed, flags, True)
    assert not np.array_equal(written[:3], p.variables[:3])
    _, b = _transition_run(p, unfixed, flags, False, written)
    _, b2 = _transition_run(p, unfixed, flags, False, written)
    print(f"EM transition {tag}: set_variables route bit-identical between two runs {b == b2}; trial costs {a[:3]} / {b[:3]}")
    assert a[5] == b[5]
    if a != b:
        assert np.allclose(a[:3], b[:3], rtol=1e-9) and np.allclose(np.frombuffer(a[4]), np.frombuffer(b[4]), rtol=1e-9, atol=1e-12)


def test_state_transition_like_set_variables():
    """sweep, trial (look-ahead sweep enqueued), EM into CURRENT, trial: the last trial equals the one of a fresh context that was given the same variables by
    nlls_set_variables at the same point -- cost, step and trial point, exactly.  On 60 blocks of the adaptive-mean fixture, where one wavefront holds every block and the
    small dense system's trial is reproducible to the bit (its sweep sums a workgroup's blocks with LDS atomic adds)."""
    p = adaptive_mean_problem(means=(-0.4, 0.3), draws=(24, 6)); unfixed = np.array([False, True, True])
    written, a = _transition_run(p, unfixed, 0, True)
    assert not np.array_equal(written[:3], p.variables[:3])
    _, b = _transition_run(p, unfixed, 0, False, written)
    _, b2 = _transition_run(p, unfixed, 0, False, written)
    assert b == b2, "the nlls_set_variables route is not reproducible"
    assert a == b


def test_state_transition_on_the_full_fixture():
    """... and on all 2000 blocks (several wavefronts per workgroup: see _same_transition)"""
    _same_transition("small dense", adaptive_mean_problem(means=(-0.4, 0.3)), np.array([False, True, True]), 0)


def test_state_transition_on_a_schur_problem():
    """the same on the config-5 shape (pinhole blocks, Schur elimination)"""
    p = synthetic.create_so3_ba_problem(20, 2000, 0.2, adaptive=True); unfixed = np.ones(p.nvariables, bool); unfixed[0] = False
    _same_transition("Schur", p, unfixed, _capi.FLAG_DETERMINISTIC)


def test_reference_test_second_half():
    """test/adaptivecost.jl:47-59 through N.emcallback(): Newton on the two means, the kernel fixed for the optimiser and re-estimated by EM in the callback"""
    p = adaptive_mean_problem()
    res = N.optimize(p, N.NLLSOptions(iterator=N.newton), np.array([False, True, True]), N.emcallback())
    par = contaminated_gaussian_params(p.variables[:3])
    print(f"EM reference test: params {par} means {p.variables[3:]} iterations {res.niterations} costcomputations {res.costcomputations}")
    assert np.allclose(par, [1.0, 10.0, 0.8], rtol=0.1), par                                                   # :57
    assert np.isclose(p.variables[3], -1.0, rtol=0.1) and np.isclose(p.variables[4], 1.0, rtol=0.1)             # :58-59
    # the hand-written callback of tests/test_gpu_functional.py::test_adaptivecost (residual re-derived in numpy, EM on the host) ends in the same state
    q = adaptive_mean_problem(); (g,) = q.costs.values(); vi, da = g.arrays()
    def hostcallback(cost, problem, data, *unused):
        vn = problem.varnext
        vn[:3] = contaminated_gaussian_em(vn[:3], (vn[1 + vi[:, 1]] - da[:, 0]) ** 2)
        data.linsystem.ctx.set_variables(vn, NXT)
        newcost = data.linsystem.cost(NXT); data.costcomputations += 1
        return newcost, 0
    res2 = N.optimize(q, N.NLLSOptions(iterator=N.newton), np.array([False, True, True]), hostcallback)
    assert res.niterations == res2.niterations and res.costcomputations == res2.costcomputations
    assert np.allclose(p.variables, q.variables, rtol=1e-9, atol=0.0), (p.variables, q.variables)
    assert np.isclose(res.bestcost, res2.bestcost, rtol=1e-9)


def test_config5_shape_reduced():
    """BASELINE config 5, reduced: pinhole blocks over SO(3) poses under the adaptive kernel, Levenberg-Marquardt with the kernel variable fixed and N.emcallback().
    Every callback's EM is held against the host mirror on the device's squared errors of that moment."""
    p = synthetic.create_so3_ba_problem(20, 2000, 0.2, adaptive=True)
    unfixed = np.ones(p.nvariables, bool); unfixed[0] = False
    inner = N.emcallback(); log = []
    def cb(cost, problem, data, *rest):
        ctx = data.linsystem.ctx
        k0 = ctx.get_variables(NXT)[:3]
        err = ctx.eval_blocks(0, NXT, want="sqerr")["sqerr"]
        ref = contaminated_gaussian_em(k0, err, 10); _, n_host, ratios = host_em_ratios(k0, err, 10)
        ls = data.linsystem; seen = []; orig = ls.adaptive_em
        ls.adaptive_em = lambda *a, **k: seen.append(orig(*a, **k)) or seen[-1]          # (the passes the callback's own call made)
        try:
            out = inner(cost, problem, data, *rest)
        finally:
            del ls.adaptive_em
        st = ctx.get_variables(NXT)[:3]
        assert len(seen) == 1 and np.array_equal(seen[0][0], st) and np.array_equal(problem.varnext[:3], st)
        clear = clear_of_threshold(ratios)
        assert not clear or seen[0][1] == n_host, (seen[0][1], n_host, ratios[-3:])
        log.append((np.max(np.abs(st - ref) / np.abs(ref)), clear, n_host, ratios[-1], out[0]))
        return out
    start = N.cost(p)
    res = N.optimize(p, N.NLLSOptions(maxiters=12), unfixed, cb)
    for i, (e, clear, n_host, last, c) in enumerate(log):
        print(f"EM config5 callback {i}: storage err {e:.3e} host passes {n_host} last ratio {last:.3g} clear {clear} cost {c!r}")
    assert len(log) >= 2 and all(e <= RTOL for e, *_ in log)
    assert sum(not clear for _, clear, *_ in log) * 5 <= len(log), "more than one call in five within 10 % of the threshold"
    print(f"EM config5: cost {start!r} -> {res.bestcost!r} in {res.niterations} iterations")
    assert res.bestcost < start
