"""Host-side iterators: Newton, Levenberg-Marquardt, dogleg, gradient descent -- a line-for-line
behavioural mirror of src/iterators.jl; they stay on the host (BASELINE north_star) and drive the
device through the generic functions of MultiVariateLSgpu."""
import math
import sys
import time

import numpy as np

from ._capi import VARS_CURRENT, VARS_NEXT, NllsError, ERR_NOT_SPD

FLOATMIN = sys.float_info.min


def _timed(data, field, fn):
    t0 = time.perf_counter_ns()
    out = fn()
    setattr(data, field, getattr(data, field) + time.perf_counter_ns() - t0)
    return out


class PCG:
    """NLLSOptions(linearsolver=PCG(...)): the iterators' linear solves by conjugate gradients on the device's matrix-free operator (nlls_solve_pcg) where they
    factor by default -- no reduced system, and with `maxiters` small a truncated-Newton step.  precond: "blockjacobi" (the diagonal blocks of H + lambda I) or "none";
    maxiters None: 4 ndof.  schur=True: the same on the reduced system of the upload's eliminated set (nlls_solve_pcg_schur; "blockjacobi" is then the diagonal blocks of
    B + lambda I, rtol bounds the reduced residual; precond "schurjacobi" -- with schur=True only, ValueError otherwise -- is the diagonal blocks of S itself, Ceres'
    SCHUR_JACOBI); a problem without an eliminated set raises NllsError (ERR_UNSUPPORTED), it does not fall back.  A breakdown (the system is not positive definite) is what a bad pivot is to the direct solve: Levenberg-Marquardt damps more."""

    def __init__(self, rtol=1e-8, maxiters=None, precond="blockjacobi", schur=False):
        assert precond in ("blockjacobi", "none", "schurjacobi") and rtol >= 0 and (maxiters is None or maxiters >= 1)
        if precond == "schurjacobi" and not schur:
            raise ValueError('PCG(precond="schurjacobi") preconditions the reduced system: it needs schur=True')
        self.rtol, self.maxiters, self.precond, self.schur = float(rtol), maxiters, precond, bool(schur)


def _solve(ls, options):
    """solve!(linsystem): the direct solve, or options.linearsolver's"""
    pcg = getattr(options, "linearsolver", None)
    if pcg is None:
        return ls.solve()
    if getattr(pcg, "schur", False):
        return ls.solve_pcg_schur(pcg.precond, pcg.maxiters, pcg.rtol)
    return ls.solve_pcg(pcg.precond, pcg.maxiters, pcg.rtol)


class NewtonData:                                   # src/iterators.jl:11-13
    def reset(self):
        return self

    def printable(self):
        return None


def iterate_newton(nd, data, problem, options):     # src/iterators.jl:15-27
    ls = data.linsystem
    _timed(data, "timesolver", lambda: _solve(ls, options))
    data.linearsolvers += 1
    ls.update(VARS_NEXT, VARS_CURRENT)
    cost_ = _timed(data, "timecost", lambda: ls.cost(VARS_NEXT))
    data.costcomputations += 1
    return cost_


class LevMarData:                                   # src/iterators.jl:120-129
    def __init__(self):
        self.lambda_ = 0.0

    def reset(self):
        self.lambda_ = 0.0

    def printable(self):
        return 1.0 / self.lambda_ if self.lambda_ else math.inf


def iterate_levmar(lmd, data, problem, options):    # src/iterators.jl:139-172
    assert lmd.lambda_ >= 0.0
    ls = data.linsystem
    if lmd.lambda_ == 0:
        lmd.lambda_ = ls.initlambda()               # :142-144
    lastlambda = 0.0
    mu = 2.0
    while True:
        # A trial whose damped factorisation meets an exactly ZERO pivot (a singular direction at a tiny lambda): the reference's
        # LDLFactorizations would throw here; this path counts it as a rejected trial -- more damping, solve again -- and records it in
        # data.singulartrials (NLLSResult.singulartrials), in both branches.  No cost was computed for such a trial.
        singular = None
        if hasattr(ls, "lm_trial") and getattr(options, "linearsolver", None) is None:   # :149-157 in one library call (same kernels, one synchronisation)
            try:
                cost_ = _timed(data, "timesolver", lambda: ls.lm_trial(lmd.lambda_ - lastlambda))
                data.costcomputations += 1
            except NllsError as e:
                if e.code != ERR_NOT_SPD:
                    raise
                singular = e
            lastlambda = lmd.lambda_
            data.linearsolvers += 1
        else:
            ls.uniformscaling(lmd.lambda_ - lastlambda)  # :149
            lastlambda = lmd.lambda_
            try:
                _timed(data, "timesolver", lambda: _solve(ls, options))     # :152 (options.linearsolver: conjugate gradients)
            except NllsError as e:
                if e.code != ERR_NOT_SPD:
                    raise
                singular = e
            data.linearsolvers += 1
            if not singular:
                ls.update(VARS_NEXT, VARS_CURRENT)       # :155
                cost_ = _timed(data, "timecost", lambda: ls.cost(VARS_NEXT))   # :157
                data.costcomputations += 1
        if singular and (not math.isfinite(lmd.lambda_) or not np.all(np.isfinite(ls.b))):
            # ... unless the linear system ITSELF holds NaN / Inf (a non-finite residual): no damping cures that.  The reference's factorisation
            # does not throw on it -- its step and the trial cost come out NaN, '!(cost_ > bestcost)' accepts them and the outer loop reports
            # "cost is NaN" + "NaN in the step" (src/optimize.jl:147-152).  Same here: a NaN step, retracted, its cost swept.
            ls.x = np.full(len(ls.b), np.nan)
            ls.update(VARS_NEXT, VARS_CURRENT)
            cost_ = _timed(data, "timecost", lambda: ls.cost(VARS_NEXT))
            data.costcomputations += 1
            singular = None
        if singular:
            if not math.isfinite(lmd.lambda_ * mu):      # nothing left to damp with
                raise singular
            data.singulartrials += 1
            lmd.lambda_ *= mu
            mu *= 2.0
            continue
        if not (cost_ > data.bestcost) or ls.step_maxabs() < options.dstep:   # :160
            ls.uniformscaling(-lastlambda)           # :162
            xHx, gx = ls.quadform()
            stepquality = (cost_ - data.bestcost) / (0.5 * xHx + gx)          # :163
            lmd.lambda_ *= (1 - (2 * stepquality - 1) ** 3) if stepquality < 0.983 else 0.1   # :164
            return cost_
        lmd.lambda_ *= mu                            # :169-170
        mu *= 2.0


class DoglegData:                                   # src/iterators.jl:30-45
    def __init__(self):
        self.trustradius = 0.0
        self.cauchy = None

    def reset(self):
        self.trustradius = 0.0

    def printable(self):
        return self.trustradius


def iterate_dogleg(dd, data, problem, options):     # src/iterators.jl:47-115
    ls = data.linsystem
    t0 = time.perf_counter_ns()
    gradient = ls.b
    gnorm2 = float(gradient @ gradient)
    a = gnorm2 / (ls.grad_quadform() + FLOATMIN)
    dd.cauchy = -a * gradient
    alpha2 = a * a * gnorm2
    alpha = math.sqrt(alpha2)
    if dd.trustradius == 0:
        dd.trustradius = alpha
    beta = 0.0
    x = None
    if alpha < dd.trustradius:
        _solve(ls, options)
        x = np.array(ls.x)
        beta = float(np.linalg.norm(x))
        data.linearsolvers += 1
    data.timesolver += time.perf_counter_ns() - t0
    cost_ = data.bestcost
    while True:
        if not (alpha < dd.trustradius):
            x = (dd.trustradius / alpha) * dd.cauchy
            linear_approx = dd.trustradius * (2 * alpha - dd.trustradius) / (2 * a)
        elif beta <= dd.trustradius:
            linear_approx = cost_
        else:
            x = x - dd.cauchy
            sq_leg = float(x @ x)
            c = float(dd.cauchy @ x)
            trsq = dd.trustradius * dd.trustradius - alpha2
            step = math.sqrt(c * c + sq_leg * trsq)
            step = (-c + step) / sq_leg if c <= 0 else trsq / (c + step)
            x = x * step + dd.cauchy
            linear_approx = 0.5 * (a * (1 - step) ** 2 * gnorm2) + step * (2 - step) * cost_
        ls.x = x
        ls.update(VARS_NEXT, VARS_CURRENT)
        cost_ = _timed(data, "timecost", lambda: ls.cost(VARS_NEXT))
        data.costcomputations += 1
        mu = (data.bestcost - cost_) / linear_approx
        if mu > 0.375:
            dd.trustradius = max(dd.trustradius, 3 * float(np.linalg.norm(x)))
        elif mu < 0.125:
            dd.trustradius *= 0.5
        if not (cost_ > data.bestcost) or float(np.max(np.abs(x))) < options.dstep:
            return cost_


class SteihaugData:                                 # (not in the reference; the state of DoglegData, src/iterators.jl:30-45)
    def __init__(self, trustradius=0.0):
        self.trustradius = float(trustradius)
        self.statuses = []                          # how every trial's conjugate gradients ended (0, 1 inside the region; 4, 5 on its boundary)

    def reset(self):
        self.trustradius = 0.0
        self.statuses = []

    def printable(self):
        return self.trustradius


def _cauchy_mnorm(ls, precond):
    """the M-norm of the Cauchy step, (b'z / z'Hz) sqrt(b'z) with z = M^-1 b -- sqrt(b'z) where z'Hz <= 0: the first radius of iterate_steihaug"""
    b = np.asarray(ls.b, np.float64); z = b.copy()
    if precond == "blockjacobi":
        o = 0
        for blk in ls.hess_block_diag(0.0):
            d = blk.shape[0]; z[o:o + d] = np.linalg.solve(blk, b[o:o + d]); o += d
    bz = float(b @ z); zhz = float(z @ ls.hess_apply(z))
    radius = (bz / zhz) * math.sqrt(bz) if zhz > 0 and bz > 0 else math.sqrt(max(bz, 0.0))
    return radius if radius > 0 and math.isfinite(radius) else 1.0       # (b == 0: any ball holds the zero step)


def iterate_steihaug(sd, data, problem, options):
    """A trust-region iteration whose every trial is ONE call: Steihaug-Toint conjugate gradients on the device (nlls_solve_pcg_tr) in the place of dogleg's Cauchy point
    plus Gauss-Newton solve (src/iterators.jl:47-115), with dogleg's radius rule (:101-106) in the norm of the preconditioner.  rtol, maxiters and precond come from
    options.linearsolver (None: PCG(rtol=1e-2)); a preconditioner block without a factor (status 3) raises, as everywhere: there is no fall-back."""
    ls = data.linsystem
    pcg = getattr(options, "linearsolver", None) or PCG(rtol=1e-2)
    if getattr(pcg, "schur", False):
        raise ValueError("iterate_steihaug: PCG(schur=True) has no trust region -- a ball in the norm of the reduced system is not a ball of the step")
    if sd.trustradius == 0:
        sd.trustradius = _timed(data, "timesolver", lambda: _cauchy_mnorm(ls, pcg.precond))
    while True:
        _, st = _timed(data, "timesolver", lambda: ls.solve_pcg_tr(sd.trustradius, pcg.precond, pcg.maxiters, pcg.rtol))
        data.linearsolvers += 1
        sd.statuses.append(st["status"])
        ls.update(VARS_NEXT, VARS_CURRENT)
        cost_ = _timed(data, "timecost", lambda: ls.cost(VARS_NEXT))
        data.costcomputations += 1
        mu = (data.bestcost - cost_) / (st["model"] + FLOATMIN)
        if mu > 0.375:
            sd.trustradius = max(sd.trustradius, 3 * st["mnorm"])
        elif mu < 0.125:
            sd.trustradius *= 0.5
        if not (cost_ > data.bestcost) or ls.step_maxabs() < options.dstep:
            return cost_


class GradientDescentData:                          # src/iterators.jl:177-185
    def __init__(self):
        self.stepsize = 1.0

    def reset(self):
        self.stepsize = 1.0

    def printable(self):
        return self.stepsize


def iterate_gradientdescent(gd, data, problem, options):   # src/iterators.jl:187-208
    ls = data.linsystem
    gradient = ls.b
    x = -gradient * gd.stepsize
    ls.x = x
    ls.update(VARS_NEXT, VARS_CURRENT)
    costc = _timed(data, "timecost", lambda: ls.cost(VARS_NEXT))
    data.costcomputations += 1
    while costc > data.bestcost:
        coststep = float(x @ gradient)
        costdiff = data.bestcost + coststep - costc
        gd.stepsize *= 0.5 * coststep / costdiff
        x = -gradient * gd.stepsize
        ls.x = x
        ls.update(VARS_NEXT, VARS_CURRENT)
        costc = _timed(data, "timecost", lambda: ls.cost(VARS_NEXT))
        data.costcomputations += 1
    gd.stepsize *= 2
    return costc
