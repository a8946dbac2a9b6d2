"""Repeated damped solves of BASELINE config 4 (for rocprofv3 runs of the solve kernels alone)."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nllssolver_jl_amd as N
from nllssolver_jl_amd import synthetic, _capi

ap = argparse.ArgumentParser(); ap.add_argument("--reps", type=int, default=10); ap.add_argument("--flags", type=int, default=0)
ap.add_argument("--dump-x", default=None, metavar="FILE", help="x of one damped solve as raw float64 (to compare two builds with cmp)")
ap.add_argument("--ncam", type=int, default=1000); ap.add_argument("--npts", type=int, default=100000); ap.add_argument("--prop", type=float, default=0.01)
a = ap.parse_args()
p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(a.ncam, a.npts, a.prop, seed=1, robust=N.HuberKernel(0.01), outlier_frac=0.05, outlier_sigma=0.05), 1e-3, 1e-3)
ctx = _capi.Context(0)
bi = np.arange(1, p.nvariables + 1, dtype=np.uint64)
info = ctx.upload(p.var_kind, p.var_dim, bi, p.groups(), a.flags)
ctx.set_variables(p.variables); ctx.sweep_gradhess(); ctx.damp(1e-4 * ctx.max_abs_diag())
for _ in range(3): ctx.solve()
ms = ctx.time_solve(a.reps)
if a.dump_x: np.ascontiguousarray(ctx.solve(want_x=True), dtype=np.float64).tofile(a.dump_x)
print(json.dumps({"solve_ms": ms, "solve_mode": info.solve_mode, "reduced_dof": info.nreduced_dof}))
ctx.close()
