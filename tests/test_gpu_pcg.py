"""nlls_solve_pcg: block-Jacobi conjugate gradients on the device's matrix-free operator, in the place of nlls_solve (include/nlls_amd.h).

Every test first runs the host mirror `pcg_mirror` on the device's own A and b (device_system) and asserts the input condition it relies on -- convergence inside the
cap of 4 ndof iterations, or the breakdown -- so that a bad input blames the input and not the kernel.

Tolerances:
  x against damp(lambda); solve(): 1e-7 of the largest entry of the step, what tests/test_gpu_apply.py's composed CG and check_problem hold x to;
  true residual ||(A + lambda I)(-x) - b|| <= 2 rtol ||b|| at rtol 1e-8: the drift between the recurrence's residual and the true one is rounding (1e-11 .. 9e-11 of
         ||b|| on the host), the factor 2 only keeps the bound from being an equality;
  a truncated iterate against the mirror's (run through the device's own products), the grid caps against the default, the step's statistics against the host's:
         1e-11 of the largest entry -- the same sums in another order;
  the trial behind a call: 1e-9, the pattern of tests/test_gpu_apply.py::test_reads_only_on_both_trial_paths.
The bit rules are exact: two calls, and calls that differ in the round length only."""
import os
import subprocess
import sys

import numpy as np
import pytest

import nllssolver_jl_amd as N
from nllssolver_jl_amd import kinds as K
from nllssolver_jl_amd import synthetic, _capi
from tests.helpers import blockindices, scalar_graph_problem, hub_edges
from tests.test_gpu_blockeval import chain_problem
from tests.test_gpu_linearize import affine_two_groups, device_system, upload, rel
from tests.test_gpu_apply import PROBLEMS, block_sizes, dense_curve_rosenbrock

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE, JACOBI = _capi.PCG_PRECOND_NONE, _capi.PCG_PRECOND_BLOCK_JACOBI


def pcg_mirror(matvec, blocks, bo, rhs, cap, rtol):
    """tests/test_gpu_apply.py::block_jacobi_cg with the library's statuses: preconditioned conjugate gradients on matvec(y) = rhs from 0; blocks None: no preconditioner.
    -> (y, iterations, status, iterates): status 0 ||r|| <= rtol ||rhs||, 1 the cap, 2 d'q not > 0 or a scalar not finite (iterations: the one that broke down),
    3 a diagonal block without a Cholesky factor (0 iterations)"""
    inv = None
    if blocks is not None:
        try:
            for d in blocks:
                np.linalg.cholesky(d)
        except np.linalg.LinAlgError:
            return np.zeros_like(rhs), 0, 3, []
        inv = [np.linalg.inv(d) for d in blocks]
    def prec(r):
        if inv is None:
            return r.copy()
        z = np.empty_like(r)
        for b, m in enumerate(inv):
            z[bo[b]:bo[b] + m.shape[0]] = m @ r[bo[b]:bo[b] + m.shape[0]]
        return z
    y = np.zeros_like(rhs); r = rhs.copy(); z = prec(r); d = z.copy(); rz = r @ z; stop = rtol * np.linalg.norm(rhs); its = []
    if np.linalg.norm(r) <= stop:
        return y, 0, 0, its
    for it in range(1, cap + 1):
        q = matvec(d); dq = d @ q
        with np.errstate(all="ignore"):
            alpha = rz / dq
        if not (dq > 0) or not np.isfinite(alpha):
            return y, it, 2, its
        y = y + alpha * d; r = r - alpha * q; its.append(y.copy())
        if np.linalg.norm(r) <= stop:
            return y, it, 0, its
        z = prec(r); rz, old = r @ z, rz; d = z + (rz / old) * d
    return y, cap, 1, its


def host_blocks(A, lam, bo, bs):
    return [A[bo[k]:bo[k] + bs[k], bo[k]:bo[k] + bs[k]] + lam * np.eye(bs[k]) for k in range(bs.size)]


def pd_lambda(A, first=1e-2):
    """first * max|diag A| -- or, where the host Cholesky of A + lambda I fails there, the smallest of 1e-1, 1, 10 for which it holds"""
    top = np.max(np.abs(np.diag(A)))
    for s in (first, 1e-1, 1.0, 10.0):
        if s < first:
            continue
        try:
            np.linalg.cholesky(A + s * top * np.eye(A.shape[0])); return s * top
        except np.linalg.LinAlgError:
            pass
    raise AssertionError("A + 10 max|diag| I has no Cholesky factor: the input is not what the test was written for")


def swept(p, unfixed=None, flags=0):
    ctx = upload(p, unfixed, flags); ctx.copy_variables(_capi.VARS_NEXT, _capi.VARS_CURRENT); ctx.copy_variables(_capi.VARS_BEST, _capi.VARS_CURRENT)
    ctx.sweep_gradhess(); A, b = device_system(ctx); bo, bs = block_sizes(ctx)
    return ctx, A, b, bo, bs


_AFFINE = {}


def affine(flags=0):
    """affine_two_groups swept, with lambda = 1e-2 max|diag| set and the host mirror's converged run: (ctx, A, b, bo, bs, lam, k).  The HOST side is computed once."""
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed, flags)
    if "k" not in _AFFINE:
        lam = 1e-2 * np.max(np.abs(np.diag(A)))
        _, k, status, _ = pcg_mirror(lambda v: A @ v + lam * v, host_blocks(A, lam, bo, bs), bo, b, 4 * b.size, 1e-10)
        assert status == 0, f"the host mirror did not converge in {4 * b.size} iterations: the input is at fault"
        _AFFINE.update(lam=lam, k=k)
    ctx.damp(_AFFINE["lam"])
    return ctx, A, b, bo, bs, _AFFINE["lam"], _AFFINE["k"]


# ---- 1. against nlls_solve ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, _capi.FLAG_MATERIALIZE], ids=["default", "materialize"])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_against_the_direct_solve(name, flags):
    p, unfixed = PROBLEMS[name]()
    ctx, A, b, bo, bs = swept(p, unfixed, flags); ndof = ctx.info.ndof; cap = 4 * ndof
    lam = pd_lambda(A); Al = A + lam * np.eye(ndof)
    _, kh, sh, _ = pcg_mirror(lambda v: Al @ v, host_blocks(A, lam, bo, bs), bo, b, cap, 1e-10)
    assert sh == 0, f"{name}: the host mirror on the device's A did not converge in {cap} iterations (status {sh}): the input is at fault"
    _, kd, sd, _ = pcg_mirror(lambda v: ctx.hess_apply(v, lam), ctx.hess_block_diag(lam), bo, b, cap, 1e-10)
    assert sd == 0
    ctx.damp(lam); xs = ctx.solve(want_x=True)
    x, st = ctx.solve_pcg(JACOBI, None, 1e-10, want_x=True)
    assert st["status"] == 0 and st["iterations"] >= 1 and x.tobytes() == ctx.get_step().tobytes()
    err = np.max(np.abs(x - xs)) / np.max(np.abs(xs))
    x8, st8 = ctx.solve_pcg(JACOBI, None, 1e-8, want_x=True)
    res = np.linalg.norm(Al @ (-x8) - b) / np.linalg.norm(b)
    print(f"PCG {name} flags {flags}: ndof {ndof} lambda {lam:.3e} iterations device {st['iterations']} mirror {kd} host {kh}; against nlls_solve {err:.3e} (of 1e-7); "
          f"true residual at rtol 1e-8 {res:.3e} (of 2e-8) recurrence {st8['rnorm'] / st8['bnorm']:.3e}; rounds {st['rounds']} launches {st['launches']}")
    assert err <= 1e-7, name
    assert st8["status"] == 0 and res <= 2e-8, name
    assert abs(st["iterations"] - kd) <= 1, (name, st, kd)
    assert abs(st["bnorm"] - np.linalg.norm(b)) <= 1e-11 * np.linalg.norm(b) and st["rnorm"] <= 1e-10 * st["bnorm"]
    ss = ctx.solve_stats()
    assert (ss["pcg_iterations"], ss["pcg_status"], ss["pcg_rounds"]) == (st8["iterations"], 0, st8["rounds"])
    ctx.close()


# ---- 2. truncation ------------------------------------------------------------------------------------------------------------------------------------
def test_truncation():
    ctx, A, b, bo, bs, lam, k = affine(); Al = A + lam * np.eye(b.size)
    _, _, _, its = pcg_mirror(lambda v: ctx.hess_apply(v, lam), ctx.hess_block_diag(lam), bo, b, 3, 1e-10)
    assert len(its) == 3 and k > 4
    model = []
    for m in (1, 2, 3):
        x, st = ctx.solve_pcg(JACOBI, m, 1e-10, want_x=True)
        assert (st["status"], st["iterations"]) == (1, m) and x.tobytes() == ctx.get_step().tobytes()
        e = rel(-x, its[m - 1]); model.append(0.5 * x @ (Al @ x) + b @ x)      # (the model of the DAMPED system, the one the iteration minimises over its Krylov space)
        print(f"PCG truncated at {m}: against the mirror's iterate {e:.3e} (of 1e-11), model {model[-1]:.9e}")
        assert e <= 1e-11
    assert model[0] < 0 and model[1] < model[0] and model[2] < model[1], model
    _, stk = ctx.solve_pcg(JACOBI, None, 1e-10); kd = stk["iterations"]
    assert stk["status"] == 0 and abs(kd - k) <= 1
    _, st = ctx.solve_pcg(JACOBI, kd, 1e-10); assert (st["status"], st["iterations"]) == (0, kd)
    _, st = ctx.solve_pcg(JACOBI, kd - 1, 1e-10); assert (st["status"], st["iterations"]) == (1, kd - 1)
    ctx.close()


# ---- 3. the bit rules ---------------------------------------------------------------------------------------------------------------------------------
def test_bit_rules():
    ctx, A, b, bo, bs, lam, k = affine()
    x0, s0 = ctx.solve_pcg(JACOBI, None, 1e-10, want_x=True); x1, s1 = ctx.solve_pcg(JACOBI, None, 1e-10, want_x=True)
    assert s0["status"] == 0 and x0.tobytes() == x1.tobytes() and s0 == s1, "two calls on the same sweep differ"
    kd = s0["iterations"]
    for rnd in (1, 3, 1000):
        ctx.set_option(_capi.OPT_PCG_ROUND, rnd)
        x, st = ctx.solve_pcg(JACOBI, None, 1e-10, want_x=True)
        print(f"PCG round {rnd}: iterations {st['iterations']} synchronisations {st['rounds']} launches {st['launches']}")
        assert x.tobytes() == x0.tobytes() and st["iterations"] == kd and st["status"] == 0, rnd
        assert st["rounds"] == -(-kd // rnd) + 1, (rnd, st)               # one per round up to the one that holds iteration kd, one for the step
        x, st = ctx.solve_pcg(JACOBI, 5, 1e-10, want_x=True)              # the last round is cut to what maxiters leaves
        assert (st["status"], st["iterations"], st["rounds"]) == (1, 5, -(-5 // rnd) + 1), (rnd, st)
    with pytest.raises(_capi.NllsError):
        ctx.set_option(_capi.OPT_PCG_ROUND, 0)
    ctx.set_option(_capi.OPT_PCG_ROUND, 1)
    _, kn, sn, _ = pcg_mirror(lambda v: A @ v + lam * v, None, bo, b, 4 * b.size, 1e-10)
    assert sn == 0
    xn, st = ctx.solve_pcg(NONE, None, 1e-10, want_x=True)
    print(f"PCG no preconditioner: iterations {st['iterations']} (host {kn}, block Jacobi {kd}); against block Jacobi {rel(xn, x0):.3e}")
    assert st["status"] == 0 and abs(st["iterations"] - kn) <= 1 and rel(xn, x0) <= 1e-7
    assert ctx.solve_pcg("none", None, 1e-10, want_x=True)[0].tobytes() == xn.tobytes()
    ctx.close()


# ---- 4. grid loops and ragged sizes -------------------------------------------------------------------------------------------------------------------
def test_grid_caps():
    ctx, A, b, bo, bs, lam, k = affine()
    x0, s0 = ctx.solve_pcg(JACOBI, None, 1e-10, want_x=True)
    assert b.size == 558 and s0["status"] == 0                            # three workgroups of 256 by default: the caps 1 and 2 stride, 3 is the default grid
    for g in (1, 2, 3):
        ctx.set_option(_capi.OPT_PCG_GRID_MAX, g)
        x, st = ctx.solve_pcg(JACOBI, None, 1e-10, want_x=True); e = rel(x, x0)
        print(f"PCG grid cap {g}: iterations {st['iterations']} (default {s0['iterations']}) against the default grid {e:.3e} (of 1e-11)")
        assert st["status"] == 0 and e <= 1e-11, g
        assert ctx.solve_pcg(JACOBI, None, 1e-10, want_x=True)[0].tobytes() == x.tobytes()
        xn, sn = ctx.solve_pcg(NONE, 6, 1e-10, want_x=True); ctx.set_option(_capi.OPT_PCG_GRID_MAX, 1024)
        assert rel(xn, ctx.solve_pcg(NONE, 6, 1e-10, want_x=True)[0]) <= 1e-11
    assert ctx.solve_pcg(JACOBI, None, 1e-10, want_x=True)[0].tobytes() == x0.tobytes()
    ctx.close()


def rosenbrock_two():
    p = N.NLLSProblem(); p.addvariable(-0.5); p.addvariable(2.5)
    p.addcosts(K.RES_ROSENBROCK_A, [[1]], [[1.0]]); p.addcosts(K.RES_ROSENBROCK_B, [[1, 2]], [[10.0]])
    return p


def hub65():
    edges, nv = hub_edges(65)
    return scalar_graph_problem(edges, nv, seed=65, robust=N.GemanMcclureKernel(0.7))


@pytest.mark.parametrize("name,make", [("dense curve + rosenbrock", dense_curve_rosenbrock), ("two-variable rosenbrock", rosenbrock_two), ("hub of 65", hub65)])
def test_ragged_sizes(name, make):
    ctx, A, b, bo, bs = swept(make()); ndof = ctx.info.ndof; lam = pd_lambda(A); Al = A + lam * np.eye(ndof)
    _, kh, sh, _ = pcg_mirror(lambda v: Al @ v, host_blocks(A, lam, bo, bs), bo, b, 4 * ndof, 1e-10)
    assert sh == 0, f"{name}: the host mirror did not converge: the input is at fault"
    ctx.damp(lam); xs = ctx.solve(want_x=True)
    for pc in (JACOBI, NONE):
        x, st = ctx.solve_pcg(pc, None, 1e-10, want_x=True); err = np.max(np.abs(x - xs)) / np.max(np.abs(xs))
        print(f"PCG {name} precond {pc}: ndof {ndof} blocks of {sorted(set(bs.tolist()))} iterations {st['iterations']} (host, block Jacobi: {kh}); against nlls_solve {err:.3e} (of 1e-7)")
        assert st["status"] == 0 and err <= 1e-7, (name, pc)
    ctx.close()


# ---- 5. breakdown -------------------------------------------------------------------------------------------------------------------------------------
def system_state(ctx):
    return [ctx.get_bsm_data().tobytes(), ctx.get_grad().tobytes()] + [ctx.get_variables(w).tobytes() for w in range(3)]


def refused_not_spd(ctx, pc, status, iterations):
    ndof = ctx.info.ndof; sentinel = np.linspace(-1.0, 2.0, ndof); ctx.set_step(sentinel); before = system_state(ctx)
    out = np.full(ndof, 7.25); st = np.full(8, -1.0)
    rc = ctx.L.nlls_solve_pcg(ctx.h, pc, 4 * ndof, 1e-10, _capi._p(out), _capi._p(st))
    assert rc == _capi.ERR_NOT_SPD and (int(st[1]), int(st[0])) == (status, iterations), (rc, st)
    assert np.all(out == 7.25) and ctx.get_step().tobytes() == sentinel.tobytes() and system_state(ctx) == before
    ss = ctx.solve_stats(); assert (ss["pcg_status"], ss["pcg_iterations"]) == (status, iterations)
    with pytest.raises(_capi.NllsError) as e:
        ctx.solve_pcg(pc, None, 1e-10)
    assert e.value.code == _capi.ERR_NOT_SPD and ctx.last_pcg["status"] == status


@pytest.mark.parametrize("ncam,npts", [(3, 5), (8, 20)])
def test_breakdown_on_an_indefinite_system(ncam, npts):
    """the systems of tests/test_gpu_parity.py::test_indefinite_dense_system at lambda 0"""
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(ncam, npts, 1.0, seed=2, robust=N.GemanMcclureKernel(0.01), outlier_frac=0.3, outlier_sigma=0.2), 1e-2, 1e-2)
    ctx, A, b, bo, bs = swept(p); ndof = ctx.info.ndof
    assert ndof == 6 * ncam + 3 * npts and not ctx.info.is_sparse
    assert pcg_mirror(lambda v: A @ v, host_blocks(A, 0.0, bo, bs), bo, b, 4 * ndof, 1e-10)[1:3] == (0, 3), "a diagonal block should be indefinite: the input is at fault"
    assert pcg_mirror(lambda v: A @ v, None, bo, b, 4 * ndof, 1e-10)[1:3] == (1, 2) and b @ A @ b <= 0, "b'Hb should be <= 0: the input is at fault"
    refused_not_spd(ctx, JACOBI, 3, 0)
    refused_not_spd(ctx, NONE, 2, 1)
    ctx.close()


def test_breakdown_of_the_preconditioner_at_lambda_zero():
    p, unfixed = affine_two_groups(); ctx, A, b, bo, bs = swept(p, unfixed, _capi.FLAG_MATERIALIZE)
    assert pcg_mirror(lambda v: A @ v, host_blocks(A, 0.0, bo, bs), bo, b, 4 * b.size, 1e-10)[2] == 3, "a diagonal block should be indefinite at lambda 0: the input is at fault"
    refused_not_spd(ctx, JACOBI, 3, 0)
    ctx.close()


# ---- 6. state -----------------------------------------------------------------------------------------------------------------------------------------
def test_state_after_a_solve():
    ctx, A, b, bo, bs, lam, k = affine(_capi.FLAG_MATERIALIZE); Al = A + lam * np.eye(b.size)
    ctx.solve(); before = system_state(ctx); st0 = ctx.solve_stats()
    x, st = ctx.solve_pcg(JACOBI, None, 1e-10, want_x=True)
    assert st["status"] == 0 and system_state(ctx) == before
    st1 = ctx.solve_stats()
    assert all(st0[key] == st1[key] for key in st0 if not key.startswith(("pcg", "apply"))), (st0, st1)
    xHx, gx = ctx.quadform()                                               # (with the damping the context holds: lambda unchanged by the call)
    e = (abs(ctx.step_maxabs() - np.max(np.abs(x))) / np.max(np.abs(x)), abs(ctx.step_norm() - np.linalg.norm(x)) / np.linalg.norm(x),
         abs(xHx - x @ Al @ x) / abs(x @ Al @ x), abs(gx - b @ x) / abs(b @ x))
    print(f"PCG state: max|x| {e[0]:.3e} |x| {e[1]:.3e} x'(H + lambda I)x {e[2]:.3e} g'x {e[3]:.3e} (of 1e-11)")
    assert max(e) <= 1e-11
    ctx.retract(_capi.VARS_NEXT, _capi.VARS_CURRENT); got = ctx.get_variables(_capi.VARS_NEXT).tobytes()
    ctx.copy_variables(_capi.VARS_NEXT, _capi.VARS_CURRENT); ctx.set_step(x); ctx.retract(_capi.VARS_NEXT, _capi.VARS_CURRENT)
    assert got == ctx.get_variables(_capi.VARS_NEXT).tobytes() and got != ctx.get_variables(_capi.VARS_CURRENT).tobytes()
    ctx.close()


def _trial_run(p, call, materialise):
    ctx = upload(p, None, _capi.FLAG_DETERMINISTIC)
    if materialise:
        ctx.set_option(_capi.OPT_MATERIALIZE, 1)
    ctx.copy_variables(_capi.VARS_NEXT, _capi.VARS_CURRENT)
    c0 = ctx.sweep_gradhess(); lam = 1e-3
    if call:
        big = 1e-2 * ctx.max_abs_diag(); ctx.damp(big)
        _, st = ctx.solve_pcg(JACOBI, 4, 1e-10); assert (st["status"], st["iterations"]) == (1, 4)
        ctx.damp(-big)                                                     # (big - big: the damping is 0 again, exactly)
    c1 = ctx.lm_trial(lam); mf = ctx.solve_stats()["mf_trials"]
    out = (c0, c1, ctx.get_step().tobytes(), ctx.get_variables(_capi.VARS_NEXT).tobytes()); ctx.close()
    return out, mf


@pytest.mark.parametrize("materialise", [False, True], ids=["matrix-free", "materialised"])
def test_a_trial_behind_a_solve_runs_as_before(materialise):
    """the pattern of tests/test_gpu_apply.py::test_reads_only_on_both_trial_paths: bytes cannot be compared across runs on these two paths"""
    p = chain_problem()
    (a, mfa), (c, mfc) = (_trial_run(p, call, materialise) for call in (False, True))
    assert mfa == mfc == (0 if materialise else 1), "the trial did not take the path the case was written for"
    print(f"PCG trial behind a solve, materialise={materialise}: costs {a[:2]} / {c[:2]}")
    assert np.allclose(c[:2], a[:2], rtol=1e-9, atol=0.0)
    assert np.allclose(np.frombuffer(c[2]), np.frombuffer(a[2]), rtol=1e-9, atol=1e-12) and np.allclose(np.frombuffer(c[3]), np.frombuffer(a[3]), rtol=1e-9, atol=1e-12)


# ---- 7. optimize --------------------------------------------------------------------------------------------------------------------------------------
def test_optimize_with_pcg_steps():
    make = lambda: synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3), 1e-3, 1e-3)      # (noise-free: the optimum's cost is rounding)
    with N.Solver(make()) as s:
        res = s.optimize(N.NLLSOptions(maxiters=50, linearsolver=N.PCG(rtol=1e-6))); ss = s.ls.ctx.solve_stats()
        print(f"PCG optimize: cost {res.startcost:.3e} -> {res.bestcost:.3e} in {res.niterations} iterations, {res.linearsolvers} linear solves, last of {ss['pcg_iterations']} iterations")
        assert res.bestcost <= 1e-15 * res.startcost and res.linearsolvers > 0 and ss["pcg_iterations"] > 0
    with N.Solver(make()) as s:
        x, st = s.solve_pcg(1.0, rtol=1e-10); g = s.ls.b                   # (Solver.solve_pcg on the kept context: H = J'J here, so H + I is positive definite)
        assert st["status"] == 0 and x.shape == (s.ls.info.ndof,) and rel(s.hessvec(-x, 1.0), g) <= 1e-8 and s.ls.ctx.solve_stats()["pcg_iterations"] == st["iterations"]
    with N.Solver(make()) as s:
        res = s.optimize(N.NLLSOptions(maxiters=50)); ss = s.ls.ctx.solve_stats()
        print(f"PCG optimize, the control: cost {res.startcost:.3e} -> {res.bestcost:.3e} in {res.niterations} iterations")
        assert res.bestcost <= 1e-15 * res.startcost and ss["pcg_iterations"] == 0
    for it in (N.newton, N.dogleg):
        res = N.optimize(make(), N.NLLSOptions(maxiters=30, iterator=it, linearsolver=N.PCG(rtol=1e-8)))
        print(f"PCG optimize {it.name}: cost {res.startcost:.3e} -> {res.bestcost:.3e} in {res.niterations} iterations")
        assert res.bestcost < 1e-6 * res.startcost and res.linearsolvers > 0


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    L = _capi.lib(); ctx = _capi.Context(); P = _capi._p
    out = np.full(64, 7.25); st = np.full(8, 7.25)
    call = lambda pc=JACOBI, mi=10, rtol=1e-8: L.nlls_solve_pcg(ctx.h, pc, mi, rtol, P(out), P(st))
    assert call() == _capi.ERR_NOT_READY                                                                          # no upload yet
    p = N.NLLSProblem(); a = p.addvariable([0.1, 0.2, 0.3]); b = p.addvariable([0.3, -0.2, 0.5]); rng = np.random.default_rng(2)
    p.addcosts(K.RES_LINEAR3, [[a], [b], [a], [b]], rng.standard_normal((4, 12)))
    ctx.upload(p.var_kind, p.var_dim, blockindices(p), p.groups()); ctx.set_variables(p.variables)
    assert call() == _capi.ERR_NOT_READY                                                                          # no sweep yet
    ctx.sweep_gradhess()
    for pc in (-1, 2):
        assert call(pc=pc) == _capi.ERR_INVALID_ARG
    for mi in (0, -3):
        assert call(mi=mi) == _capi.ERR_INVALID_ARG
    for rtol in (np.nan, np.inf, -1e-3):
        assert call(rtol=rtol) == _capi.ERR_INVALID_ARG
    assert L.nlls_solve_pcg(None, JACOBI, 10, 1e-8, P(out), P(st)) == _capi.ERR_INVALID_ARG
    assert np.all(out == 7.25) and np.all(st == 7.25), "a refused call wrote to an output"
    assert L.nlls_solve_pcg(ctx.h, JACOBI, 100, 1e-12, None, None) == _capi.OK                                     # both outputs may be NULL
    assert call(mi=100, rtol=1e-12) == _capi.OK and int(st[1]) == 0 and np.all(out[:6] != 7.25) and np.all(out[6:] == 7.25) and st[6] == st[7] == 0
    A, g = device_system(ctx); assert rel(out[:6], -np.linalg.solve(A, g)) <= 1e-9
    ctx.close()
    # a dynamic-size group: no per-block Hessian
    ctx = _capi.Context(); out[:] = 7.25; st[:] = 7.25
    d = p.addvariable([1.0, 2.0, 3.0, 4.0], K.VAR_DYNAMIC)
    p.addcosts(K.COST_DYN_LINEAR, [[d]], rng.standard_normal((1, 4))); p.addcosts(K.RES_DYN_NORM, [[d]], np.zeros((1, 0)))
    ctx.upload(p.var_kind, p.var_dim, blockindices(p), p.groups()); ctx.set_variables(p.variables); ctx.sweep_gradhess()
    assert call() == _capi.ERR_UNSUPPORTED and np.all(out == 7.25) and np.all(st == 7.25)
    ctx.close()
    # every variable fixed: ndof == 0
    q = N.NLLSProblem(); a = q.addvariable([0.1, 0.2, 0.3]); q.addcosts(K.RES_LINEAR3, [[a]], rng.standard_normal((1, 12)))
    ctx = upload(q, np.zeros(1, bool)); ctx.sweep_gradhess()
    assert ctx.info.ndof == 0 and call() == _capi.OK and np.all(out == 7.25) and np.all(st == 0.0)
    ctx.close()


def test_sharded_contexts_are_refused():
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3), 1e-3, 1e-3)
    c = _capi.Context()
    try:
        c.set_shard(0, 2); c.upload(p.var_kind, p.var_dim, blockindices(p), p.groups(), _capi.FLAG_FORCE_SPARSE); c.set_variables(p.variables)
        assert c.shard_info()["nranks"] == 2 and c.shard_info()["replicated"] == 0
        c.sweep_gradhess_local()
        out = np.full(c.info.ndof, 7.25)
        assert c.L.nlls_solve_pcg(c.h, JACOBI, 10, 1e-8, _capi._p(out), None) == _capi.ERR_UNSUPPORTED and np.all(out == 7.25)
    finally:
        c.close()


def test_user_kind_in_a_process_of_its_own():
    userlib = os.path.join(ROOT, "nllssolver.jl_amd", "csrc", "libnlls_amd_userdemo.so")
    env = dict(os.environ, NLLS_AMD_LIB=userlib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pcg_userkind_worker.py")], capture_output=True, text=True, env=env, timeout=600)
    print(out.stdout[-1500:])
    assert out.returncode == 0 and "user kind pcg ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
