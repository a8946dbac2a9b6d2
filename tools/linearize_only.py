#!/usr/bin/env python3
"""What the per-block linearisation launch costs: nlls_eval_gradhess with H only, nlls_eval_jacobians with J only, and both calls with every output, on a bench.py
workload built as bench.py builds it.  The launch alone, by an event pair around it (NLLS_OPT_PHASE_EVENTS, nlls_get_phase_times [10], [11]): the median of --repeats
timed calls behind one untimed call, the bytes of records the launch wrote, and that rate against the 6.29 TB/s copy rate bench.py measures its launches against.
The call's own host wall clock (the records' way home included) is printed beside it.  One JSON line.

  --workload   ba_100x10k (default) | ba_1kx100k"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nllssolver_jl_amd as N
from nllssolver_jl_amd import synthetic, _capi

HBM_COPY_TBS = 6.29
ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="ba_100x10k", choices=("ba_100x10k", "ba_1kx100k"))
ap.add_argument("--repeats", type=int, default=5); ap.add_argument("--group", type=int, default=0)
a = ap.parse_args()
ncam, npts, prop = {"ba_100x10k": (100, 10000, 0.1), "ba_1kx100k": (1000, 100000, 0.01)}[a.workload]
p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(ncam, npts, prop, seed=1, robust=N.HuberKernel(0.01), outlier_frac=0.05, outlier_sigma=0.05), 1e-3, 1e-3)
ctx = _capi.Context(0)
ctx.upload(p.var_kind, p.var_dim, np.arange(1, p.nvariables + 1, dtype=np.uint64), p.groups()); ctx.set_variables(p.variables)
ctx.set_option(_capi.OPT_PHASE_EVENTS, 1)
n = ctx._groups[a.group][0]
out = {"workload": a.workload, "nblocks": int(n), "repeats": a.repeats}


def measure(calls):
    """calls: the launches of one variant; (median microseconds summed over them, bytes written, median host milliseconds)"""
    us, ms, nbytes = [], [], 0
    for _ in range(a.repeats + 1):
        t_us, t0, nbytes = 0.0, time.perf_counter(), 0
        for fn in calls:
            fn(); pt = ctx.phase_times(); t_us += pt["linearize_us"]; nbytes += pt["linearize_bytes"]
        us.append(t_us); ms.append(1e3 * (time.perf_counter() - t0))
    return float(np.median(us[1:])), int(nbytes), float(np.median(ms[1:]))


variants = (("H_only", [lambda: ctx.eval_gradhess(a.group, want="H")]), ("J_only", [lambda: ctx.eval_jacobians(a.group, want="J")]),
            ("all_outputs", [lambda: ctx.eval_jacobians(a.group), lambda: ctx.eval_gradhess(a.group)]))
for name, calls in variants:
    us, nbytes, ms = measure(calls)
    out[name] = {"launch_us": us, "bytes_written": nbytes, "TBps": nbytes / (us * 1e-6) / 1e12, "frac_of_copy_rate": nbytes / (us * 1e-6) / 1e12 / HBM_COPY_TBS, "call_ms": ms}
st = ctx.solve_stats()
out["slab_doubles"] = st["linearize_slab"]; out["batch_J_g_H"] = [st["linearize_batch_J"], st["linearize_batch_g"], st["linearize_batch_H"]]
ctx.close()
print(json.dumps(out))
