#!/usr/bin/env python3
"""optimizesingles! of all points of a BA workload (cameras fixed), or of all cameras (points fixed): a target for rocprofv3 / quick timing.

  --select points|cameras   which half is relaxed (the other half is fixed at its true value, the relaxed one starts perturbed)
  --wave-min n              NLLS_SINGLES_WAVE_MIN for this run: cost blocks from which a variable gets a wavefront instead of a thread
  --repeats r               timed calls, each from the same start, behind one untimed call; call_ms is their median
  --dump file               the final variables (float64, raw) -- to compare two builds bit for bit"""
import argparse, os, sys, time, json
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser(); ap.add_argument("--ncam", type=int, default=1000); ap.add_argument("--npts", type=int, default=100000); ap.add_argument("--prop", type=float, default=0.01)
ap.add_argument("--select", choices=("points", "cameras"), default="points"); ap.add_argument("--wave-min", type=int, default=None)
ap.add_argument("--repeats", type=int, default=1); ap.add_argument("--dump", default=None)
a = ap.parse_args()
if a.wave_min is not None:
    os.environ["NLLS_SINGLES_WAVE_MIN"] = str(a.wave_min)      # (read when the context is created)
import nllssolver_jl_amd as N
from nllssolver_jl_amd import synthetic, kinds as K, _capi
p = synthetic.create_ba_problem(a.ncam, a.npts, a.prop, seed=1, robust=N.HuberKernel(0.01), outlier_frac=0.05, outlier_sigma=0.05)
p = synthetic.perturb_ba_problem(p, 3e-3, 0.0) if a.select == "points" else synthetic.perturb_ba_problem(p, 0.0, 2e-3)
ispt = (p.var_kind == K.VAR_EUCLIDEAN) & (p.var_dim == 3)
sel = np.nonzero(ispt if a.select == "points" else ~ispt)[0] + 1
cptr, cgroup, cindex, cslot = p.costlists(sel)
ctx = _capi.Context(0)
ctx.upload(p.var_kind, p.var_dim, np.arange(1, p.nvariables + 1, dtype=np.uint64), p.groups(), 0)
ctx.set_variables(p.variables); c0 = ctx.sweep_cost()
ms = []
for r in range(a.repeats + (1 if a.repeats > 1 else 0)):       # (more than one repeat: the first call is the warm-up)
    ctx.set_variables(p.variables)
    t0 = time.perf_counter(); iters = ctx.optimize_singles(sel, cptr, cgroup, cindex, cslot); t1 = time.perf_counter()
    ms.append(1e3 * (t1 - t0))
if a.repeats > 1:
    ms = ms[1:]
c1 = ctx.sweep_cost(); st = ctx.solve_stats()
if a.dump:
    np.ascontiguousarray(ctx.get_variables(), np.float64).tofile(a.dump)
print(json.dumps({"select": a.select, "nvariables": int(sel.size), "nblocks": int(cptr[-1]), "call_ms": float(np.median(ms)), "call_ms_min": min(ms), "call_ms_max": max(ms),
                  "wave": st.get("singles_wave"), "thread": st.get("singles_thread"),
                  "iters_mean": float(iters.mean()), "iters_max": int(iters.max()), "cost_before": c0, "cost_after": c1}))
