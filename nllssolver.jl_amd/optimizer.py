"""optimize! and its result/option structs: a behavioural mirror of src/optimize.jl:5-17,78-180 and
src/structs.jl:5-107 on the host, driving the device-resident linear system."""
import enum
import math
import time

import numpy as np

from . import iterators as It
from ._capi import VARS_BEST, VARS_CURRENT, VARS_NEXT
from .callbacks import nullcallback
from .linearsystem import makesymmvls


class NLLSIterator(enum.IntEnum):                   # src/structs.jl:5
    newton = 0
    levenbergmarquardt = 1
    dogleg = 2
    gradientdescent = 3
    steihaug = 4                                    # (not in the reference: Steihaug-Toint conjugate gradients inside a trust region, nlls_solve_pcg_tr)


newton, levenbergmarquardt, dogleg, gradientdescent, steihaug = NLLSIterator


class NLLSOptions:                                   # src/structs.jl:22-35
    def __init__(self, maxiters=100, reldcost=1e-15, absdcost=1e-15, dstep=1e-15, maxfails=3, maxtime=30.0,
                 iterator=levenbergmarquardt, callback=None, iteratordata=None, linearsolver=None):
        self.reldcost, self.absdcost, self.dstep = reldcost, absdcost, dstep
        self.maxfails, self.maxiters = maxfails, maxiters
        self.maxtime = int(round(maxtime * 1e9))     # nanoseconds
        self.iterator, self.callback, self.iteratordata = NLLSIterator(iterator), callback, iteratordata
        # None: the direct solve of the linear system.  An iterators.PCG: conjugate gradients on the device's matrix-free operator (nlls_solve_pcg) in its place --
        # Levenberg-Marquardt then runs its unfused trial (damp, solve, update, cost) in the Python loop
        assert linearsolver is None or isinstance(linearsolver, It.PCG)
        self.linearsolver = linearsolver


class NLLSResult:                                    # src/structs.jl:37-79
    def __init__(self, d):
        self.startcost, self.bestcost = d.startcost, d.bestcost
        self.timetotal, self.timeinit = d.timetotal * 1e-9, d.timeinit * 1e-9
        self.timecost, self.timegradient, self.timesolver = d.timecost * 1e-9, d.timegradient * 1e-9, d.timesolver * 1e-9
        self.termination, self.niterations = d.converged, d.iternum
        self.costcomputations, self.gradientcomputations, self.linearsolvers = d.costcomputations, d.gradientcomputations, d.linearsolvers
        self.singulartrials = d.singulartrials      # LM trials rejected because the damped factorisation met an exactly zero pivot (the reference would throw)

    def __str__(self):
        other = self.timetotal - self.timecost - self.timegradient - self.timesolver - self.timeinit
        tt = max(self.timetotal, 1e-300)
        s = ("NLLSsolver optimization took %f seconds and %d iterations to reduce the cost from %e to %e (a %.2f%% reduction), using:\n"
             "   %d cost computations in %f seconds (%.2f%% of total time),\n"
             "   %d gradient computations in %f seconds (%.2f%% of total time),\n"
             "   %d linear solver computations in %f seconds (%.2f%% of total time),\n"
             "   %f seconds for initialization (%.2f%% of total time), and\n"
             "   %f seconds for other stuff (%.2f%% of total time).\n") % (
            self.timetotal, self.niterations, self.startcost, self.bestcost, 100 * (1 - self.bestcost / self.startcost) if self.startcost else 0.0,
            self.costcomputations, self.timecost, 100 * self.timecost / tt, self.gradientcomputations, self.timegradient, 100 * self.timegradient / tt,
            self.linearsolvers, self.timesolver, 100 * self.timesolver / tt, self.timeinit, 100 * self.timeinit / tt, other, 100 * other / tt)
        reasons = ["Cost is infinite.", "Cost is NaN.", "Relative decrease in cost below threshold.", "Absolute decrease in cost below threshold.",
                   "Step contains an infinite value.", "Step contains a NaN.", "Step size below threshold.",
                   "Too many consecutive iterations increasing the cost.", "Maximum number of outer iterations reached.",
                   "Maximum allowed computation time exceeded."]
        if self.termination:
            s += "Reason(s) for termination:\n"
            for bit, r in enumerate(reasons):
                if self.termination & (1 << bit):
                    s += "   " + r + "\n"
            if self.termination >> 16:
                s += "   Terminated by user-defined callback, with flags: " + bin(self.termination >> 16)[2:] + "\n"
        return s


class NLLSInternal:                                  # src/structs.jl:81-104
    def __init__(self, linsystem, starttime):
        self.startcost = self.bestcost = 0.0
        self.starttime = starttime
        self.timetotal = self.timeinit = self.timecost = self.timegradient = self.timesolver = 0
        self.iternum = self.costcomputations = self.gradientcomputations = self.linearsolvers = self.converged = 0
        self.singulartrials = 0
        self.linsystem = linsystem


_ITER = {
    newton: (It.NewtonData, It.iterate_newton),
    levenbergmarquardt: (It.LevMarData, It.iterate_levmar),
    dogleg: (It.DoglegData, It.iterate_dogleg),
    gradientdescent: (It.GradientDescentData, It.iterate_gradientdescent),
    steihaug: (It.SteihaugData, It.iterate_steihaug),
}


def convertunfixed(unfixed, problem):                # src/optimize.jl:19-22
    n = problem.nvariables
    if unfixed is None:
        return np.ones(n, bool)
    if isinstance(unfixed, (int, np.integer)) and not isinstance(unfixed, (bool, np.bool_)):
        m = np.zeros(n, bool); m[int(unfixed) - 1] = True   # 1-based single variable index
        return m
    if isinstance(unfixed, tuple) and len(unfixed) == 2 and not isinstance(unfixed[0], (bool, np.bool_)):
        kind, dim = unfixed                          # "variable type": (kind, dim)
        return (problem.var_kind == kind) & (problem.var_dim == dim)
    return np.asarray(unfixed, dtype=bool)


class OuterLoop:
    """State of optimizeinternal! (src/optimize.jl:109-180), split so that bench.py can time exactly K outer
    iterations: start() = :111-121, iteration() = one pass of the while-loop body :124-171."""

    def __init__(self, problem, options, data, iteratedata, iterate, callback, native=None):
        self.problem, self.options, self.data = problem, options, data
        self.iteratedata, self.iterate, self.callback = iteratedata, iterate, callback
        self.fails = 0
        self.have_best = False
        self.cost = math.nan
        # native: Levenberg-Marquardt without a per-iteration callback on one GPU runs in the library's own host loop
        # (nlls_lm_iterations, csrc/nlls_lm.cpp: the same statements as iteration() + iterate_levmar below, without the interpreter
        # between two trials).  native=False keeps the Python loop (the tests hold the two against each other).
        ls = data.linsystem
        can = (iterate is It.iterate_levmar and callback is nullcallback and hasattr(ls, "ctx")
               and (not getattr(ls, "sharded", False) or getattr(ls, "native_collectives", False))     # (sharded: the collectives are inside the library)
               and hasattr(ls.ctx, "lm_iterations") and getattr(options, "linearsolver", None) is None)
        self.native = can if native is None else (bool(native) and can)
        self._state = None

    def start(self):
        data, ls = self.data, self.data.linsystem
        data.startcost = -math.inf                       # preoptimization, src/iterators.jl:7
        self.fails = 0
        data.iternum = 0
        self.stoptime = data.starttime + self.options.maxtime
        data.timeinit += time.perf_counter_ns() - data.starttime
        cost = It._timed(data, "timegradient", ls.costgradhess)      # :118
        data.gradientcomputations += 1
        data.bestcost = cost
        data.startcost = max(cost, data.startcost)
        self.cost = cost

    def iterations(self, n):
        """n outer iterations (or fewer, if one of them terminates); returns the termination flags of the last one."""
        if not self.native:
            conv = 0
            for _ in range(n):
                conv = self.iteration()
                if conv:
                    break
            return conv
        from . import _capi
        data, ls, o = self.data, self.data.linsystem, self.options
        big = 2 ** 62
        clamp = lambda v: int(max(-big, min(big, v)))
        opt = _capi.LmOptions(float(o.reldcost), float(o.absdcost), float(o.dstep), clamp(o.maxfails), clamp(o.maxiters), clamp(self.stoptime))
        if self._state is None:
            self._state = _capi.LmState()
        st = self._state
        st.lambda_, st.bestcost, st.cost = float(self.iteratedata.lambda_), float(data.bestcost), float(self.cost)
        st.iternum, st.fails, st.have_best = int(data.iternum), int(self.fails), int(self.have_best)
        st.linearsolvers, st.costcomputations, st.gradientcomputations, st.singulartrials = data.linearsolvers, data.costcomputations, data.gradientcomputations, data.singulartrials
        st.timesolver_ns = st.timegradient_ns = st.timecost_ns = 0
        ls._x = None
        try:
            ls.ctx.lm_iterations(opt, st, n)
        finally:
            self.iteratedata.lambda_ = st.lambda_
            data.bestcost, self.cost, data.iternum, self.fails, self.have_best = st.bestcost, st.cost, st.iternum, st.fails, bool(st.have_best)
            data.linearsolvers, data.costcomputations, data.gradientcomputations, data.singulartrials = st.linearsolvers, st.costcomputations, st.gradientcomputations, st.singulartrials
            data.timesolver += st.timesolver_ns; data.timegradient += st.timegradient_ns; data.timecost += st.timecost_ns      # (device times where the trials' launches time themselves: nlls_get_time_buckets)
            data.converged = st.converged
        return int(st.converged)

    def iteration(self, regrad=True):
        """One outer iteration; returns the termination flags (0 = keep going).  With regrad the linear
        problem for the next iteration is built unless terminating (:167-170)."""
        if self.native and regrad:
            return self.iterations(1)
        data, ls, options = self.data, self.data.linsystem, self.options
        data.iternum += 1
        cost = float(self.iterate(self.iteratedata, data, self.problem, options))   # :126
        if self.callback is not nullcallback:
            # a user callback sees the trial point where the reference puts it -- problem.varnext (src/optimize.jl:128) -- and what it writes there counts: the
            # reference's EM callback rewrites the kernel variable in varnext (test/adaptivecost.jl:15-25, src/robustadaptive.jl:48-73) and updatefromnext! then
            # makes it the current point.  So: the next variables up before the callback, and down again after it when they changed.
            self.problem.varnext = ls.variables(VARS_NEXT)
            before = self.problem.varnext.copy()
        cost, terminate = self.callback(cost, self.problem, data, self.iteratedata)   # :128
        if self.callback is not nullcallback and not np.array_equal(before, self.problem.varnext, equal_nan=True):
            ls.ctx.set_variables(np.ascontiguousarray(self.problem.varnext, np.float64), VARS_NEXT)
        dcost = data.bestcost - cost
        if dcost >= 0:
            data.bestcost = cost
            self.fails = 0
        else:
            dcost = cost
            self.fails += 1
            if self.fails == 1:                          # :137-144 store the current best variables
                if self.have_best:
                    ls.swap(VARS_CURRENT, VARS_BEST)
                else:
                    ls.copy(VARS_BEST, VARS_CURRENT); self.have_best = True
        ls.swap(VARS_CURRENT, VARS_NEXT)                 # updatefromnext!  :207-209
        maxstep = ls.step_maxabs()                       # :149
        converged = 0
        converged |= int(math.isinf(cost)) << 0
        converged |= int(math.isnan(cost)) << 1
        converged |= int(dcost < data.bestcost * options.reldcost) << 2
        converged |= int(dcost < options.absdcost) << 3
        converged |= int(math.isinf(maxstep)) << 4
        converged |= int(math.isnan(maxstep)) << 5
        converged |= int(maxstep < options.dstep) << 6
        converged |= int(self.fails > options.maxfails) << 7
        converged |= int(data.iternum >= options.maxiters) << 8
        late = time.perf_counter_ns() > self.stoptime
        if getattr(ls, "sharded", False) and hasattr(ls, "agree_max"):
            late = ls.agree_max(float(late)) > 0          # every rank has its own clock: all leave in the same iteration (one all-reduce of a flag)
        converged |= int(late) << 9
        converged |= int(terminate) << 16
        data.converged = converged
        self.cost = cost
        if converged == 0 and regrad:
            It._timed(data, "timegradient", lambda: ls.costgradhess(want_cost=False))   # :167-170 (the value is discarded there too)
            data.gradientcomputations += 1
        return converged

    def finish(self):
        data, ls = self.data, self.data.linsystem
        if not (data.bestcost >= self.cost):
            ls.swap(VARS_CURRENT, VARS_BEST)             # updatefrombest!  :173-176
        data.timetotal += time.perf_counter_ns() - data.starttime
        return data


def optimizeinternal(problem, options, data, iteratedata, iterate, callback, native=None):   # src/optimize.jl:109-180
    loop = OuterLoop(problem, options, data, iteratedata, iterate, callback, native)
    loop.start()
    while loop.iterations(1 << 30 if loop.native else 1) == 0:
        pass
    return loop.finish()


def optimize(problem, options=None, unfixed=None, callback=nullcallback, flags=0, device=0, stream=None, native=None):
    """optimize!(problem, options, unfixed, callback) -> NLLSResult   src/optimize.jl:5-17,57.
    Variables are optimised in place: problem.variables holds the best values on return."""
    options = options or NLLSOptions()
    starttime = time.perf_counter_ns()
    assert problem.nvariables > 0
    unfixed = convertunfixed(unfixed, problem)
    ls = makesymmvls(problem, unfixed, flags, device, stream)       # :16
    data = NLLSInternal(ls, starttime)
    mk, iterate = _ITER[options.iterator]
    try:
        optimizeinternal(problem, options, data, mk(), iterate, callback or nullcallback, native)
        problem.variables[:] = ls.variables(VARS_CURRENT)
    finally:
        ls.close()
    return NLLSResult(data)


class Solver:
    """One problem's structure kept on the device across solves: the linear system of makesymmvls (src/optimize.jl:16) built ONCE, then optimize / cost / residuals
    any number of times, with the cost blocks' data and the robust kernels' parameters changed in place in between -- the reference's mutable costs and repeated
    optimize! (src/optimize.jl:5-17): graduated non-convexity, re-measurement, outer EM / IRLS loops.  N.optimize, N.cost, ... build and drop a linear system per call.
    A context manager; `unfixed`, `flags`, `device`, `stream` as N.optimize takes them.  What cannot change without a new Solver: which variables a block depends on,
    which are fixed, the kinds, the number of blocks."""

    def __init__(self, problem, unfixed=None, flags=0, device=0, stream=None):
        assert problem.nvariables > 0
        self.problem = problem
        self.ls = makesymmvls(problem, convertunfixed(unfixed, problem), flags, device, stream)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.ls is not None:
            self.ls.close(); self.ls = None

    def _start(self):
        """problem.variables -> the device's current set, varnext = deepcopy(variables) (what a fresh linear system starts with)"""
        self.ls._x = None
        self.ls.ctx.set_variables(self.problem.variables, VARS_CURRENT)
        self.ls.copy(VARS_NEXT, VARS_CURRENT)

    def _group(self, group):
        return list(self.problem.costs.values())[group]

    def optimize(self, options=None, callback=nullcallback, native=None):
        """optimize!(problem, options, unfixed, callback) -> NLLSResult on the kept linear system: starts from problem.variables, leaves the best values there."""
        options = options or NLLSOptions()
        starttime = time.perf_counter_ns()
        self._start()
        data = NLLSInternal(self.ls, starttime)
        mk, iterate = _ITER[options.iterator]
        optimizeinternal(self.problem, options, data, mk(), iterate, callback or nullcallback, native)
        self.problem.variables[:] = self.ls.variables(VARS_CURRENT)
        return NLLSResult(data)

    def cost(self):
        """cost(problem)   src/cost.jl:9"""
        self._start()
        return self.ls.cost(VARS_CURRENT)

    def _blockvalues(self, group, what):
        self._start()
        if group is not None:
            return self.ls.eval_blocks(int(group), VARS_CURRENT, what)[what]
        return [self.ls.eval_blocks(g, VARS_CURRENT, what)[what] for g in range(len(self.problem.costs))]

    def residuals(self, group=None):
        """as N.residuals"""
        return self._blockvalues(group, "r")

    def squarederrors(self, group=None):
        """as N.squarederrors"""
        return self._blockvalues(group, "sqerr")

    def jacobians(self, group, index=None):
        """as N.computeresjac, on the kept linear system"""
        self._start()
        return self.ls.eval_jacobians(int(group), VARS_CURRENT, _one_based(index))

    def gradhess(self, group, index=None):
        """as N.computecostgradhess, on the kept linear system"""
        self._start()
        return self.ls.eval_gradhess(int(group), VARS_CURRENT, _one_based(index))

    def hessvec(self, v, lam=0.0):
        """as N.hessvec, on the kept linear system"""
        self._start()
        return self.ls.hess_apply(v, lam, VARS_CURRENT)

    def jacvec(self, group, v):
        """as N.jacvec, on the kept linear system"""
        self._start()
        return self.ls.jac_apply(int(group), v, VARS_CURRENT)

    def jactvec(self, group, u):
        """as N.jactvec, on the kept linear system"""
        self._start()
        return self.ls.jact_apply(int(group), u, VARS_CURRENT)

    def hessblockdiag(self, lam=0.0):
        """the diagonal blocks of H + lam I at problem.variables: one (dof, dof) array per unfixed variable, in the order of the gradient"""
        self._start()
        return self.ls.hess_block_diag(lam, VARS_CURRENT)

    def solve_pcg(self, lam=0.0, precond="blockjacobi", maxiters=None, rtol=1e-8):
        """The step x = -(H + lam I)^-1 g at problem.variables by conjugate gradients on the device (nlls_solve_pcg): linearises, damps by lam, solves.
        -> (x, stats) as MultiVariateLSgpu.solve_pcg; a breakdown raises NllsError (ERR_NOT_SPD)."""
        self._start()
        self.ls.costgradhess(want_cost=False); self.ls.uniformscaling(lam)
        return self.ls.solve_pcg(precond, maxiters, rtol, want_x=True)

    def solve_rhs(self, B, lam=0.0, precond="blockjacobi", maxiters=None, rtol=1e-8):
        """(H + lam I) x_k = b_k at problem.variables for right-hand sides of the caller's -- B (ndof,) or (nrhs, ndof), in the order of the gradient -- by conjugate
        gradients on the device, eight columns at a time (nlls_solve_pcg_rhs).  No linearisation is needed and none is changed.  -> (X, stats) as
        Context.solve_pcg_rhs; a breakdown raises NllsError (ERR_NOT_SPD)."""
        self._start()
        return self.ls.solve_pcg_rhs(B, lam, VARS_CURRENT, precond, maxiters, rtol)

    def covariance(self, variables, lam=0.0, precond="blockjacobi", maxiters=None, rtol=1e-10, strict=True):
        """The joint marginal covariance block of `variables` (the indices addvariable returned: 1-based, unfixed, distinct, any order) at problem.variables: the rows
        and columns of (H + lam I)^-1 that belong to them, in the listed order, in the tangent space of their update() (nlls_marginal_cov).  It is the inverse of H:
        scaling by a noise level is the caller's.  A problem whose gauge is free has a singular H: fix variables, or pass a lam.  strict: a column that ended on
        maxiters raises ValueError -- a covariance from an unconverged solve is silently wrong; strict=False returns it, stats["status"] tells.  -> (cov, stats)"""
        self._start()
        cov, st = self.ls.marginal_cov(np.asarray(variables, np.int64).ravel(), lam, VARS_CURRENT, precond, maxiters, rtol)
        if strict and np.any(np.asarray(st["status"]) != 0):
            bad = np.flatnonzero(np.asarray(st["status"]) != 0)
            raise ValueError(f"covariance: {bad.size} of {len(st['status'])} columns did not converge to rtol {rtol} within maxiters (first: column {int(bad[0])}, "
                             f"||r|| / ||b|| = {float(st['rnorm'][bad[0]]) / max(float(st['bnorm'][bad[0]]), 1e-300):.3e}): raise maxiters, pass a lam, or strict=False")
        return cov, st

    def operator(self, lam=0.0):
        """H + lam I at problem.variables (as they are NOW) as a linear operator: .shape, .matvec(v), .diag_blocks() -- what a Krylov method of the caller's needs"""
        self._start()
        return HessianOperator(self.ls, lam)

    def schur_operator(self, lam=0.0):
        """S(lam) = B + lam I - E (C + lam I)^-1 E' of the upload's eliminated set at problem.variables (as they are NOW) as a linear operator on the reduced
        unknowns: .shape, .index, .matvec(v), .reduce(b), .expand(b, yr), .diag_blocks().  A problem without an eliminated set raises NllsError (ERR_UNSUPPORTED)."""
        self._start()
        return SchurOperator(self.ls, lam)

    def set_data(self, group, data, index=None):
        """New data (measurements) for blocks of cost group `group` (0-based, the order of problem.costs): `data` (n x ndata) for the blocks `index` (0-BASED here, as
        `group` is; distinct) or, index=None, for the first n.  Written to the device (nlls_set_cost_data) and to the problem's CostGroup: the two never disagree."""
        g = self._group(group); vi, da = g.arrays()
        data = np.ascontiguousarray(data, np.float64).reshape(-1, da.shape[1])
        idx = None if index is None else np.asarray(index, np.int64).ravel()
        assert data.shape[0] == (idx.size if idx is not None else data.shape[0]) and data.shape[0] <= da.shape[0]
        self.ls.set_cost_data(int(group), data, None if idx is None else idx + 1)       # (refuses an index out of range or listed twice before anything changes)
        new = da.copy()
        if idx is None:
            new[:data.shape[0]] = data
        else:
            new[idx] = data
        g.set_arrays(vi, new)

    def set_robust(self, group, params_or_kernel):
        """New parameters for the robust kernel of cost group `group`: a kernel of the group's own kind (HuberKernel(w1), Scaled(HuberKernel(w1), h1), ...) or its
        robust_params.  Written to the device (nlls_set_robust_params) and to the problem's CostGroup.  The kind itself cannot change."""
        from . import kinds as K
        g = self._group(group)
        if isinstance(params_or_kernel, K.Robustifier):
            assert params_or_kernel.kind == g.robust.kind, "set_robust: the robust kind is fixed at upload"
            new = params_or_kernel
        else:
            new = K.Robustifier(g.robust.kind, tuple(np.asarray(params_or_kernel, np.float64).ravel()[:4]))
        self.ls.set_robust_params(int(group), new.params)
        g.robust = new


class HessianOperator:
    """v -> (H + lam I) v of a linear system's CURRENT variables, evaluated on the device with every product (nlls_hess_apply): no matrix is held.  The members a
    scipy LinearOperator has, without scipy: shape, dtype, matvec (1-D or (nvec, ndof)), and diag_blocks() for a block-Jacobi preconditioner."""

    def __init__(self, ls, lam=0.0):
        self.ls = ls; self.lam = float(lam); n = int(ls.info.ndof)
        self.shape = (n, n); self.dtype = np.dtype(np.float64)

    def matvec(self, v):
        return self.ls.hess_apply(v, self.lam, VARS_CURRENT)

    __call__ = matvec

    def diag_blocks(self):
        return self.ls.hess_block_diag(self.lam, VARS_CURRENT)

    def solve(self, B, precond="blockjacobi", maxiters=None, rtol=1e-8):
        """(H + lam I)^-1 B by conjugate gradients on the device (nlls_solve_pcg_rhs): B (ndof,) or (nrhs, ndof) -> (X, stats)"""
        return self.ls.solve_pcg_rhs(B, self.lam, VARS_CURRENT, precond, maxiters, rtol)


class SchurOperator:
    """v -> S(lam) v on the reduced unknowns of a linear system's CURRENT variables, evaluated on the device with every product (nlls_schur_apply): neither H nor S is
    held.  index: the positions of the reduced unknowns in the gradient; reduce / expand carry a right-hand side to the reduced system and a reduced solution back, so
    that expand(b, S^-1 reduce(b)) solves (H + lam I) y = b; diag_blocks(): the diagonal blocks of B + lam I -- B's blocks, NOT S's: what "blockjacobi" inverts;
    schur_diag_blocks(): the diagonal blocks of S(lam) itself (nlls_schur_block_diag), what "schurjacobi" inverts -- the preconditioner for a Krylov method of the caller's."""

    def __init__(self, ls, lam=0.0):
        self.ls = ls; self.lam = float(lam)
        nred, nelim, self.is_elim, self.index = ls.schur_info()
        if nelim == 0:
            ls.schur_apply(np.zeros(nred), self.lam, VARS_CURRENT)      # (the library's refusal, with its text)
        self.shape = (nred, nred); self.dtype = np.dtype(np.float64)

    def matvec(self, v):
        return self.ls.schur_apply(v, self.lam, VARS_CURRENT)

    __call__ = matvec

    def reduce(self, b):
        return self.ls.schur_reduce(b, self.lam, VARS_CURRENT)

    def expand(self, b, yr):
        return self.ls.schur_expand(b, yr, self.lam, VARS_CURRENT)

    def diag_blocks(self):
        blocks = self.ls.hess_block_diag(self.lam, VARS_CURRENT)
        return [blk for blk, e in zip(blocks, self.is_elim) if not e]

    def schur_diag_blocks(self):
        return self.ls.schur_block_diag(self.lam, VARS_CURRENT)


SINGLES_MAX_DOF = 12          # NLLS_SINGLES_MAX_DOF (include/nlls_amd.h)
last_singles_stats = dict(singles_wave=0, singles_thread=0)


def optimizesingles(problem, options=None, indices=None, kind=None, dim=None, device=0):
    """optimizesingles!(problem, options, indices | type)   src/optimize.jl:60-76,183-205: every listed variable is
    optimised on its own (all others fixed) against the cost blocks that depend on it.  `indices` 1-based, or select by
    variable kind (and dimension), like the reference's `type` argument.  Any of the four iterators.  On the device a variable of more than 6
    degrees of freedom, or of at least 64 cost blocks (a camera), is relaxed by one wavefront whose lanes deal its blocks, every other one (a
    point) by one thread (nlls_optimize_singles).  Listed variables that share a cost block are relaxed one after the other, as the reference
    does: in launches of independent sets (NLLSProblem.singles_levels).  Returns the iterations each variable took, in the order of `indices`.
    `last_singles_stats` (this module) keeps how many variables the last device call relaxed per wavefront and per thread."""
    options = options or NLLSOptions()
    if indices is None:
        sel = problem.var_kind == kind
        if dim is not None:
            sel &= problem.var_dim == dim
        indices = np.nonzero(sel)[0] + 1
    indices = np.asarray(indices, dtype=np.int64)
    # "sorted in order of variable size" (src/optimize.jl:67; sortperm is stable): the processing order
    from . import kinds as K
    vkind, vdim = problem.var_kind, problem.var_dim            # (properties that build an array per access: taken once)
    dof = np.array([K.var_dof(vkind[i - 1], vdim[i - 1]) for i in indices], dtype=np.int64) if indices.size else np.zeros(0, np.int64)
    order = np.argsort(dof, kind="stable")
    ordered = indices[order]
    iters = np.zeros(indices.size, np.int64)
    # What the per-variable kernels take: at most 12 degrees of freedom (NLLS_SINGLES_MAX_DOF), fixed-size blocks, not the adaptive kernel's variable.  Anything else -- a
    # DynamicVector of run-time length, the kernel variable -- is relaxed the way the reference relaxes EVERY listed variable (src/optimize.jl:183-205): the
    # sub-problem of the cost blocks that depend on it, only that variable free, through the ordinary device path (a univariate dense system).  The listed
    # order is kept: runs of kernel-sized variables go in launches of independent sets, a wide variable in between is a sub-problem of its own.
    gl = list(problem.costs.values())
    adaptive_first = [gi for gi, g in enumerate(gl) if g.res_kind in K.ADAPTIVE_KINDS]
    # (the kernel variables of the adaptive groups, gathered ONCE: a scan of every adaptive group per listed variable was O(listed x blocks) -- 37 s of host time on ba_so3_500x50k)
    kernelvars = np.unique(np.concatenate([gl[gi].arrays()[0][:, 0] for gi in adaptive_first])) if adaptive_first else np.zeros(0, np.int64)
    if ordered.size:
        is_wide = (dof[order] > SINGLES_MAX_DOF) | (vkind[ordered - 1] == K.VAR_DYNAMIC) | np.isin(ordered, kernelvars)
    else:
        is_wide = np.zeros(0, bool)
    ls = makesymmvls(problem, np.ones(problem.nvariables, bool), 0, device)
    try:
        q = 0
        while q < ordered.size:
            if is_wide[q]:
                v = int(ordered[q])
                cptr, cgroup, cindex, _ = problem.costlists(np.array([v]), check=False)
                from .problem import NLLSProblem
                sub = NLLSProblem(); sub.copy_variables_from(problem, ls.variables(VARS_CURRENT))
                for gi in sorted(set(cgroup.tolist())):
                    vi, da = gl[gi].arrays(); sel = cindex[cgroup == gi]
                    sub.addcosts(gl[gi].res_kind, vi[sel], da[sel], gl[gi].robust)
                unfixed = np.zeros(problem.nvariables, bool); unfixed[v - 1] = True
                res = optimize(sub, options, unfixed, device=device)
                ls.ctx.set_variables(sub.variables, VARS_CURRENT)
                iters[order[q]] = res.niterations
                q += 1
                continue
            r = q
            while r < ordered.size and not is_wide[r]:
                r += 1
            run = ordered[q:r]; level = problem.singles_levels(run)
            for lv in range(int(level.max()) + 1 if level.size else 0):
                pick = np.nonzero(level == lv)[0]
                cptr, cgroup, cindex, cslot = problem.costlists(run[pick])
                it = ls.ctx.optimize_singles(run[pick], cptr, cgroup, cindex, cslot, options.maxiters, options.maxfails,
                                             options.reldcost, options.absdcost, options.dstep, iterator=int(options.iterator))
                iters[order[q + pick]] = it
                st = ls.ctx.solve_stats(); last_singles_stats.update(singles_wave=st["singles_wave"], singles_thread=st["singles_thread"])
            q = r
        problem.variables[:] = ls.variables(VARS_CURRENT)
    finally:
        ls.close()
    return iters


def cost(problem, device=0):
    """cost(problem)   src/cost.jl:9"""
    ls = makesymmvls(problem, np.ones(problem.nvariables, bool), 0, device)
    try:
        return ls.cost(VARS_CURRENT)
    finally:
        ls.close()


def _blockvalues(problem, group, what, device):
    ls = makesymmvls(problem, np.ones(problem.nvariables, bool), 0, device)
    try:
        if group is not None:
            return ls.eval_blocks(int(group), VARS_CURRENT, what)[what]
        return [ls.eval_blocks(g, VARS_CURRENT, what)[what] for g in range(len(problem.costs))]
    finally:
        ls.close()


def residuals(problem, group=None, device=0):
    """computeresidual of every cost block at problem.variables (src/NLLSsolver.jl:16): an (ncost x nres) array for cost group `group` (0-based, in the order of
    problem.costs; rows in the order the blocks were added), or with group=None the list of them over all groups."""
    return _blockvalues(problem, group, "r", device)


def squarederrors(problem, group=None, device=0):
    """r'r of every cost block at problem.variables -- cost(residual, vars) before the robust kernel, src/residual.jl:52; shaped like residuals()."""
    return _blockvalues(problem, group, "sqerr", device)


def _one_based(index):
    """a 0-BASED selection of blocks (None: all) as the library takes it"""
    return None if index is None else np.asarray(index, np.int64).ravel() + 1


def computeresjac(problem, group=0, index=None, unfixed=None, device=0):
    """computeresjac of blocks of cost group `group` at problem.variables (src/NLLSsolver.jl:16, src/autodiff.jl:78-93): {"r": (n, M), "J": (n, M, NJ)} for the blocks
    `index` (0-BASED, in the order the blocks were added; any order, repeats allowed; None: all).  Every variable of a block is treated as free, whatever `unfixed`
    says (it only shapes the linear system that is built for the call): the columns are the tangent entries of the block's non-kernel variables, in slot order."""
    ls = makesymmvls(problem, convertunfixed(unfixed, problem), 0, device)
    try:
        return ls.eval_jacobians(int(group), VARS_CURRENT, _one_based(index))
    finally:
        ls.close()


def computecostgradhess(problem, group=0, index=None, unfixed=None, device=0):
    """computecostgradhess of blocks of cost group `group` at problem.variables (src/residual.jl:57-111, src/autodiff.jl:144-159): {"cost": (n,), "g": (n, P),
    "H": (n, P, P)}, robustified, every variable of a block free; adaptive kinds carry the kernel's three entries first.  `index`, `unfixed` as computeresjac."""
    ls = makesymmvls(problem, convertunfixed(unfixed, problem), 0, device)
    try:
        return ls.eval_gradhess(int(group), VARS_CURRENT, _one_based(index))
    finally:
        ls.close()


def hessvec(problem, v, lam=0.0, unfixed=None, device=0):
    """(H + lam I) v at problem.variables, H the Hessian the linear system of `unfixed` would hold (robustified, second-order term, adaptive border included), formed
    block by block on the device and never stored (nlls_hess_apply; src/linearsystem.jl:180-190, src/utils.jl:71-106).  v (ndof,) or (nvec, ndof), in the order of
    the gradient.  A linear system is built and dropped per call: N.Solver keeps one."""
    ls = makesymmvls(problem, convertunfixed(unfixed, problem), 0, device)
    try:
        return ls.hess_apply(v, lam, VARS_CURRENT)
    finally:
        ls.close()


def marginalcovariance(problem, variables, lam=0.0, unfixed=None, device=0, precond="blockjacobi", maxiters=None, rtol=1e-10, strict=True):
    """The joint marginal covariance block of `variables` at problem.variables: the rows and columns of (H + lam I)^-1 of the linear system of `unfixed` that belong
    to them, as Solver.covariance returns it (nlls_marginal_cov; the reference has no covariance routine).  -> (cov, stats).  A linear system is built and dropped
    per call: N.Solver keeps one."""
    with Solver(problem, unfixed, 0, device) as s:
        return s.covariance(variables, lam, precond, maxiters, rtol, strict)


def jacvec(problem, group, v, unfixed=None, device=0):
    """J v per block of cost group `group` (0-based) at problem.variables: (ncost * M,), block i at [i * M, (i + 1) * M); J as N.computeresjac gives it, the columns
    of fixed variables dropped (nlls_jac_apply)."""
    ls = makesymmvls(problem, convertunfixed(unfixed, problem), 0, device)
    try:
        return ls.jac_apply(int(group), v, VARS_CURRENT)
    finally:
        ls.close()


def jactvec(problem, group, u, unfixed=None, device=0):
    """J' u of cost group `group`'s blocks at problem.variables: (ndof,) in the order of the gradient (nlls_jact_apply); with u the residuals of an unrobustified
    group, the group's share of the gradient."""
    ls = makesymmvls(problem, convertunfixed(unfixed, problem), 0, device)
    try:
        return ls.jact_apply(int(group), u, VARS_CURRENT)
    finally:
        ls.close()


def jacobian(problem, unfixed=None, weighted=False, device=0):
    """The Jacobian of the whole problem at problem.variables as COO triplets (rows, cols, vals, r): rows are residual rows in group order, then the order the blocks
    were added, then m; cols are 0-based positions in the gradient b of the linear system (boffsets of nlls_get_bsm_index); the columns of fixed variables are dropped.
    r is the stacked residual: J'J is the Gauss-Newton Hessian and J'r the gradient of an unrobustified problem.  weighted=True: each block's rows of J and r times
    sqrt(rho') of its robust kernel (the IRLS weight of nlls_eval_blocks), so that the two products are the first-order robustified ones.  The values come from the
    device (nlls_eval_jacobians); the indices are assembled here.  Adaptive, non-squared and dynamic-size groups have no such Jacobian: ValueError."""
    from . import kinds as K
    gl = list(problem.costs.values())
    for gi, g in enumerate(gl):
        if g.res_kind in K.ADAPTIVE_KINDS or g.res_kind in (K.COST_LINEAR3, K.COST_DYN_LINEAR, K.RES_DYN_LINEAR, K.RES_DYN_NORM, K.RES_DYN_LINEARSQ):
            raise ValueError(f"jacobian: cost group {gi} is of an adaptive, non-squared or dynamic-size kind")
    ls = makesymmvls(problem, convertunfixed(unfixed, problem), 0, device)
    try:
        bo = np.asarray(ls.ctx.bsm_index()[3], np.int64) - 1; bi = np.asarray(ls.blockindices, np.int64)
        vkind, vdim = problem.var_kind, problem.var_dim
        rows, cols, vals, rs = [], [], [], []; row0 = 0
        for gi, g in enumerate(gl):
            vi, _ = g.arrays(); n = vi.shape[0]
            if n == 0:
                continue
            out = ls.eval_jacobians(gi, VARS_CURRENT); J, r = out["J"], out["r"]; M = r.shape[1]
            if weighted:
                w = np.sqrt(ls.eval_blocks(gi, VARS_CURRENT, ("weight",))["weight"]); J = J * w[:, None, None]; r = r * w[:, None]
            rr = row0 + M * np.arange(n)[:, None] + np.arange(M)[None, :]                   # (n, M) row of every residual entry
            j0 = 0
            for s in range(vi.shape[1]):
                v = vi[:, s] - 1; dof = K.var_dof(int(vkind[v[0]]), int(vdim[v[0]])); free = bi[v] > 0
                if np.any(free):
                    cc = bo[bi[v[free]] - 1][:, None] + np.arange(dof)[None, :]             # (nfree, dof) column of every tangent entry
                    rows.append(np.broadcast_to(rr[free][:, :, None], (cc.shape[0], M, dof)).ravel())
                    cols.append(np.broadcast_to(cc[:, None, :], (cc.shape[0], M, dof)).ravel())
                    vals.append(J[free][:, :, j0:j0 + dof].ravel())
                j0 += dof
            rs.append(r.ravel()); row0 += n * M
        cat = lambda a, t: np.concatenate(a).astype(t) if a else np.zeros(0, t)
        return cat(rows, np.int64), cat(cols, np.int64), cat(vals, np.float64), cat(rs, np.float64)
    finally:
        ls.close()
