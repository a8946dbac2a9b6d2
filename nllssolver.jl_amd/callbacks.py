"""Per-iteration callbacks, mirroring src/callbacks.jl (host-side observability)."""
import time

import numpy as np


def nullcallback(cost, *unused):
    """src/callbacks.jl:20"""
    return cost, 0


def printoutcallback(cost, problem, data, iteratedata=None):
    """src/callbacks.jl:39-60"""
    prev = data.bestcost
    tr = getattr(iteratedata, "printable", lambda: None)() if iteratedata is not None else None
    if data.iternum == 1:
        prev = data.startcost
        print("iter      cost      cost_change    |step|" + ("    tr_radius" if tr is not None else ""))
        print("% 4d % 8e  % 4.3e   % 3.2e" % (0, prev, 0, 0) + ("   % 2.1e" % tr if tr is not None else ""))
    print("% 4d % 8e  % 4.3e   % 3.2e" % (data.iternum, cost, prev - cost, data.linsystem.step_norm())
          + ("   % 2.1e" % tr if tr is not None else ""))
    return cost, 0


class CostTrajectory:
    """src/callbacks.jl:85-107"""

    def __init__(self):
        self.costs, self.times_ns, self.trajectory = [], [], []

    def empty(self):
        self.costs.clear(); self.times_ns.clear(); self.trajectory.clear()
        return self


def storecostscallback(store):
    """src/callbacks.jl:63-66,100-133: store is a list (costs only) or a CostTrajectory."""
    if isinstance(store, CostTrajectory):
        def cb(cost, problem, data, *unused):
            store.costs.append(cost)
            store.times_ns.append(time.perf_counter_ns() - data.starttime)
            store.trajectory.append(np.array(data.linsystem.x))
            return cost, 0
        return cb

    def cb(cost, *unused):
        store.append(cost)
        return cost, 0
    return cb


def emcallback(kernel_var=1, maxiters=10):
    """The EM callback of test/adaptivecost.jl:15-25 for the adaptive ContaminatedGaussian kernel: between two iterations the kernel variable `kernel_var` (1-based) of
    problem.varnext is re-estimated by Expectation-Maximization on the squared errors of its blocks (optimize(kernel, squarederrors, maxiters),
    src/robustadaptive.jl:48-73), and the cost of what that leaves is returned.  Everything runs on the device (nlls_adaptive_em, nlls_sweep_cost): the residuals never
    come to the host, so it serves any adaptive residual kind.  Use it with the kernel variable fixed for the optimiser, as the reference's test does."""
    from ._capi import VARS_NEXT

    def cb(cost, problem, data, *unused):
        ls = data.linsystem
        storage, _ = ls.adaptive_em(kernel_var, VARS_NEXT, maxiters)
        o = int(problem.var_offsets[kernel_var - 1])
        if problem.varnext is not None:
            problem.varnext[o:o + 3] = storage        # (the outer loop mirrors problem.varnext around the callback: what it uploads again is what the device holds)
        newcost = ls.cost(VARS_NEXT)
        data.costcomputations += 1
        return newcost, 0
    return cb
