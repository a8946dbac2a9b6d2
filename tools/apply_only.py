#!/usr/bin/env python3
"""What a matrix-free product with the linearisation costs: nlls_hess_apply of --nvec vectors on a bench.py workload built as bench.py builds it.  The launches alone
(block launch + gather per chunk of vectors), by the event pair around them (NLLS_OPT_PHASE_EVENTS, nlls_get_phase_times [12], [13]): the median of --repeats (at least
7) timed calls behind one untimed call, beside the bytes the launches read and wrote (algorithmic: every array once) and the rate that implies against the 8 TB/s peak.
Beside it the yardstick: the accumulate launch of the same context on the same workload (nlls_time_sweep_accumulate), measured in the same run.  One JSON line.

  --workload   ba_100x10k | ba_1kx100k (default) | ba_so3_500x50k
  --cg         a block-Jacobi conjugate-gradient solve of the damped system (H + lambda I) y = b through Solver.operator: iterations, the final relative residual and
               the distance to nlls_solve's step"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nllssolver_jl_amd as N
from nllssolver_jl_amd import synthetic, _capi

HBM_PEAK_TBS = 8.0
ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="ba_1kx100k", choices=("ba_100x10k", "ba_1kx100k", "ba_so3_500x50k"))
ap.add_argument("--nvec", type=int, default=1); ap.add_argument("--repeats", type=int, default=7); ap.add_argument("--cg", action="store_true")
ap.add_argument("--cg-lambda", type=float, default=1e-3, help="lambda of --cg as a fraction of max |diag H|"); ap.add_argument("--cg-maxiter", type=int, default=2000)
a = ap.parse_args()
a.repeats = max(a.repeats, 7); assert 1 <= a.nvec <= _capi.APPLY_MAX_VEC
if a.workload == "ba_so3_500x50k":
    p = synthetic.perturb_ba_problem(synthetic.create_so3_ba_problem(500, 50000, 0.02, seed=1, adaptive=True), 1e-3, 1e-3)
else:
    ncam, npts, prop = {"ba_100x10k": (100, 10000, 0.1), "ba_1kx100k": (1000, 100000, 0.01)}[a.workload]
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(ncam, npts, prop, seed=1, robust=N.HuberKernel(0.01), outlier_frac=0.05, outlier_sigma=0.05), 1e-3, 1e-3)

with N.Solver(p) as s:
    op = s.operator(0.0); ctx = s.ls.ctx; ndof = int(ctx.info.ndof); L = ctx.L
    ctx.set_option(_capi.OPT_PHASE_EVENTS, 1)
    groups = p.groups(); ninc = rec = payload = 0
    for g in groups:
        n, nd = np.asarray(g["varind"]).reshape(len(g["data"]), -1).shape
        rec += n * L.nlls_res_gh_dim(int(g["res_kind"])); ninc += n * nd; payload += n * (8 * np.asarray(g["data"]).shape[1] + 8 * nd)   # data + storage offset + dof offset per slot
    V = np.random.default_rng(1).standard_normal((a.nvec, ndof))
    us, ms = [], []
    for _ in range(a.repeats + 1):
        t0 = time.perf_counter(); ctx.hess_apply(V, 0.0); ms.append(1e3 * (time.perf_counter() - t0)); pt = ctx.phase_times(); us.append(pt["apply_us"])
    st = ctx.solve_stats(); launch_us = float(np.median(us[1:])); written = int(pt["apply_bytes"])
    # block launch: the blocks' payload and offsets, the variables, v; gather launch: the records again, one offset per incidence, v
    read = int(payload + 8 * ctx.info.var_storage + a.nvec * 8 * (rec + 2 * ndof) + 4 * ninc + 8 * int(ctx.info.nblocks))
    acc_ms = ctx.time_sweep_accumulate(20)
    out = {"workload": a.workload, "ndof": ndof, "blocks": int(ctx.info.ncost), "nvec": a.nvec, "repeats": a.repeats,
           "apply_launches_us": launch_us, "apply_launches_us_all": [round(u, 2) for u in us[1:]], "bytes_read": read, "bytes_written": written,
           "TBps": (read + written) / (launch_us * 1e-6) / 1e12, "frac_of_8TBps_peak": (read + written) / (launch_us * 1e-6) / 1e12 / HBM_PEAK_TBS,
           "us_per_vector": launch_us / a.nvec, "call_ms": float(np.median(ms[1:])),
           "short_rows": st["apply_short_rows"], "wave_rows": st["apply_wave_rows"], "chunks": st["apply_chunks"], "scratch_doubles": st["apply_scratch"],
           "accumulate_launch_us": 1e3 * acc_ms, "apply_over_accumulate": launch_us / (1e3 * acc_ms)}
    if a.cg:
        ctx.sweep_gradhess(); b = ctx.get_grad(); lam = a.cg_lambda * ctx.max_abs_diag(); op.lam = lam
        bs = ctx.block_sizes(); bo = np.concatenate(([0], np.cumsum(bs)))[:-1]; D = op.diag_blocks()
        inv = {int(d): (np.nonzero(bs == d)[0], np.linalg.inv(np.stack([D[k] for k in np.nonzero(bs == d)[0]]))) for d in np.unique(bs)}
        def prec(r):
            z = np.empty_like(r)
            for d, (idx, m) in inv.items():
                pos = bo[idx][:, None] + np.arange(d)[None, :]; z[pos] = np.einsum("nij,nj->ni", m, r[pos])
            return z
        x = np.zeros(ndof); r = b.copy(); z = prec(r); d = z.copy(); rz = r @ z; nb = np.linalg.norm(b); it = 0; t0 = time.perf_counter()
        while it < a.cg_maxiter and np.linalg.norm(r) > 1e-10 * nb:
            q = op.matvec(d); alpha = rz / (d @ q); x += alpha * d; r -= alpha * q; z = prec(r); rz, old = r @ z, rz; d = z + (rz / old) * d; it += 1
        wall = time.perf_counter() - t0
        ctx.damp(lam); xs = ctx.solve(want_x=True)
        out["cg"] = {"lambda": lam, "iterations": it, "relative_residual": float(np.linalg.norm(r) / nb), "true_relative_residual": float(np.linalg.norm(op.matvec(x) - b) / nb),
                     "distance_to_nlls_solve": float(np.max(np.abs(-x - xs)) / np.max(np.abs(xs))), "seconds": wall}
print(json.dumps(out))
