#!/usr/bin/env python3
"""What a re-solve on an uploaded structure costs against a re-upload: nlls_upload_structure, nlls_set_cost_data (the whole group, and a random 1 % by index),
nlls_set_robust_params, the scatter launch alone (an event pair around it, NLLS_OPT_PHASE_EVENTS), and the first nlls_sweep_gradhess + nlls_lm_trial behind each --
on a bench.py workload, built as bench.py builds it.  Host wall clock, the median of --repeats timed calls behind one untimed call.  One JSON line.

  --workload   ba_100x10k | ba_1kx100k (default) | ba_so3_500x50k
  --group      the cost group whose data is replaced (default 0)"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nllssolver_jl_amd as N
from nllssolver_jl_amd import synthetic, _capi

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="ba_1kx100k", choices=("ba_100x10k", "ba_1kx100k", "ba_so3_500x50k"))
ap.add_argument("--repeats", type=int, default=7); ap.add_argument("--group", type=int, default=0); ap.add_argument("--flags", type=int, default=0)
a = ap.parse_args()
if a.workload == "ba_so3_500x50k":
    p = synthetic.perturb_ba_problem(synthetic.create_so3_ba_problem(500, 50000, 0.02, seed=1, adaptive=True), 1e-3, 1e-3)
else:
    ncam, npts, prop = {"ba_100x10k": (100, 10000, 0.1), "ba_1kx100k": (1000, 100000, 0.01)}[a.workload]
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(ncam, npts, prop, seed=1, robust=N.HuberKernel(0.01), outlier_frac=0.05, outlier_sigma=0.05), 1e-3, 1e-3)
groups = p.groups(); bi = np.arange(1, p.nvariables + 1, dtype=np.uint64)
d0 = groups[a.group]["data"]; n, ndata = d0.shape; rng = np.random.default_rng(1)
d1 = d0 + 1e-3 * rng.standard_normal(d0.shape)
idx = np.sort(rng.choice(n, max(n // 100, 1), replace=False)).astype(np.int64) + 1; rows = np.ascontiguousarray(d1[idx - 1])
adaptive = groups[a.group]["res_kind"] in N.kinds.ADAPTIVE_KINDS
params = np.array(list(groups[a.group]["robust_params"]) + [0.0] * 4)[:4]


def timed(fn):
    t0 = time.perf_counter(); r = fn(); return 1e3 * (time.perf_counter() - t0), r


def median_of(fn, after=None):
    """(median ms of fn, median ms of the first sweep + trial behind it) over the timed repeats"""
    ms, ms_after = [], []
    for _ in range(a.repeats + 1):
        ms.append(timed(fn)[0])
        if after: ms_after.append(timed(after)[0])
    return float(np.median(ms[1:])), (float(np.median(ms_after[1:])) if after else None)


ctx = _capi.Context(0)
def upload():
    ctx.upload(p.var_kind, p.var_dim, bi, groups, a.flags); ctx.set_variables(p.variables)
def sweep_and_trial():
    ctx.sweep_gradhess(want_cost=False); return ctx.lm_trial(lam)
upload(); ctx.sweep_gradhess(); lam = 1e-6 * ctx.max_abs_diag()
out = {"workload": a.workload, "nblocks": int(n), "ndata": int(ndata), "repeats": a.repeats}
out["upload_ms"], out["upload_then_sweep_trial_ms"] = median_of(upload, sweep_and_trial)
ctx.set_option(_capi.OPT_PHASE_EVENTS, 1)
flip = [0]
def whole():
    flip[0] ^= 1; ctx.set_cost_data(a.group, d1 if flip[0] else d0)
def some():
    ctx.set_cost_data(a.group, rows, idx)
scat = {}
for name, fn in (("set_whole", whole), ("set_1pct", some)):
    out[name + "_ms"], out[name + "_then_sweep_trial_ms"] = median_of(fn, sweep_and_trial)
    us = []
    for _ in range(a.repeats + 1):
        fn(); pt = ctx.phase_times(); us.append(pt["update_scatter_us"])
    scat[name] = float(np.median(us[1:])); copies = pt["update_copies"]
st = ctx.solve_stats(); mem = ctx.memory_info()
if not adaptive:
    out["set_robust_ms"], out["set_robust_then_sweep_trial_ms"] = median_of(lambda: ctx.set_robust_params(a.group, params), sweep_and_trial)
out["scatter_whole_us"], out["scatter_1pct_us"] = scat["set_whole"], scat["set_1pct"]
# bytes a scatter moves: every record read once (the copies' lanes find it in the cache) and written once per copy, plus one map word per record and copy
# (the cost-order copy has no map: block k sits at k)
bytes_of = lambda m: m * ndata * 8 * (1 + copies) + 4 * m * (copies - 1)
out["copies"] = copies; out["scatter_whole_bytes"] = bytes_of(n); out["scatter_1pct_bytes"] = bytes_of(idx.size)
out["scatter_whole_TBps"] = bytes_of(n) / (scat["set_whole"] * 1e-6) / 1e12; out["scatter_1pct_TBps"] = bytes_of(idx.size) / (scat["set_1pct"] * 1e-6) / 1e12
out["mf_trials"] = st["mf_trials"]; out["working_set_bytes"] = mem["working_set_bytes"]
out["speedup_whole_vs_reupload"] = (out["upload_ms"] + out["upload_then_sweep_trial_ms"]) / (out["set_whole_ms"] + out["set_whole_then_sweep_trial_ms"])
ctx.close()
print(json.dumps(out))
