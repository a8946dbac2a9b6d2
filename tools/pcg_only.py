#!/usr/bin/env python3
"""What nlls_solve_pcg costs: the damped system (H + lambda I) y = b of a bench.py workload, built as bench.py builds it, solved by conjugate gradients on the device.
The median wall time of --repeats (at least 7) calls behind one untimed call, the iterations, the time per iteration, the time of the call's launches alone (the event
pair of NLLS_OPT_PHASE_EVENTS, nlls_get_phase_times [14]) -- and beside it, measured in the same run on the same context: the host-composed block-Jacobi CG through
Solver.operator at the same tolerance (tools/apply_only.py --cg; --no-host-cg skips it), the launches of one nlls_hess_apply at nvec 1, and nlls_solve.  One JSON line.

  --workload   ba_100x10k | ba_1kx100k (default) | ba_so3_500x50k | ba_20x2k (with --no-schur: 6120 unknowns whose direct path is the dense LDL') |
               ba_10x200_fixed (558 unknowns in two cost groups, 32 variables fixed: the problem the tests solve)
  --lam        lambda as a fraction of max |diag H| (default 1e-3)      --rtol (default 1e-10)      --precond blockjacobi | none
  --round      NLLS_OPT_PCG_ROUND; a comma list measures each value (the table of notes/r18.md)
  --rhs K      nlls_solve_pcg_rhs instead: the first K unit columns (K = 6: those of the first unfixed camera) in ONE call, against K single-column calls and against K
               host-composed solves, same context, same run: wall time, product vectors, synchronisations
  --cov N      nlls_marginal_cov instead: the joint covariance block of the first N unfixed cameras, against the same columns through --rhs's one call
  --schur      nlls_solve_pcg_schur beside nlls_solve_pcg and nlls_solve, same context, same run: iterations, median wall time, synchronisations and launches of each, each
               one's distance to nlls_solve's step (the two iterations stop on different residuals -- the reduced system's and the full one's -- so compare them at the
               distance reached: --schur-rtols 1e-8,1e-12 adds runs of both at other tolerances), and the event pair around one nlls_schur_apply beside one
               nlls_hess_apply.  The workload graph_leaves_2kx100k (a general graph: 2000 chained hubs, 100000 leaves on three hubs each, scalar unknowns) is for this mode.
               Here --precond also takes schurjacobi (the diagonal blocks of S itself; nlls_solve_pcg beside it then runs under blockjacobi), and a comma list of the
               three: then ONLY the table of the preconditioners is measured -- per preconditioner its set-up time (the median wall time of the call truncated at ONE
               iteration: set-up, reduce, one product, expand -- the set-up is all that differs between the preconditioners), and per tolerance (--rtol and
               --schur-rtols) the iterations, the total time and the distance to nlls_solve's step
  --tr F       nlls_solve_pcg_tr beside nlls_solve_pcg, same context, same run: first with radius +inf (the same iteration: its time per iteration against
               nlls_solve_pcg's), then at F times the M-norm of that converged step (a comma list measures each fraction): iterations, status, median wall time,
               synchronisations and launches of each"""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import nllssolver_jl_amd as N
from nllssolver_jl_amd import synthetic, _capi

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="ba_1kx100k", choices=("ba_100x10k", "ba_1kx100k", "ba_so3_500x50k", "ba_20x2k", "ba_10x200_fixed", "graph_leaves_2kx100k"))
ap.add_argument("--lam", type=float, default=1e-3); ap.add_argument("--rtol", type=float, default=1e-10); ap.add_argument("--precond", default="blockjacobi", metavar="NAME[,NAME..]",
                help="blockjacobi | none; with --schur also schurjacobi, and a comma list of the three (then only the table of the preconditioners is measured)")
ap.add_argument("--round", default=""); ap.add_argument("--repeats", type=int, default=7); ap.add_argument("--maxiters", type=int, default=0)
ap.add_argument("--rhs", type=int, default=0); ap.add_argument("--cov", type=int, default=0)
ap.add_argument("--schur", action="store_true"); ap.add_argument("--schur-rtols", default=""); ap.add_argument("--tr", default="")
ap.add_argument("--no-schur", action="store_true"); ap.add_argument("--no-host-cg", action="store_true"); ap.add_argument("--host-cg-maxiter", type=int, default=2000)
a = ap.parse_args()
a.repeats = max(a.repeats, 7); unfixed = None
preconds = a.precond.split(",")
if not all(pc in ("blockjacobi", "none") or (a.schur and pc == "schurjacobi") for pc in preconds) or (len(preconds) > 1 and not a.schur):
    ap.error("--precond %s: the names are blockjacobi and none; schurjacobi (the diagonal blocks of S) and a comma list need --schur, the reduced system" % a.precond)
a.precond = preconds[0]; full_precond = "blockjacobi" if a.precond == "schurjacobi" else a.precond      # (the full system has no Schur-Jacobi)
if a.workload == "ba_10x200_fixed":
    from nllssolver_jl_amd import kinds as K
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(10, 200, 0.3, seed=3, robust=N.HuberKernel(0.002)), 1e-3, 1e-3)
    (g,) = p.costs.values(); vi, da = g.arrays(); rng = np.random.default_rng(4); pick = rng.choice(vi.shape[0], 150, replace=False)
    p.addcosts(K.RES_BA_AFFINE, vi[pick], da[pick] + 0.01 * rng.standard_normal((150, 2)), N.GemanMcclureKernel(0.01))
    unfixed = np.ones(p.nvariables, bool); unfixed[[0, 1]] = False; unfixed[10:40] = False
elif a.workload == "graph_leaves_2kx100k":
    from tests.helpers import scalar_graph_problem, shared_leaves_edges
    e, n = shared_leaves_edges(2000, 100000); p = scalar_graph_problem(e, n, seed=5)      # (no robust kernel: H = J'J is positive semi-definite, any lambda > 0 will do)
elif a.workload == "ba_so3_500x50k":
    p = synthetic.perturb_ba_problem(synthetic.create_so3_ba_problem(500, 50000, 0.02, seed=1, adaptive=True), 1e-3, 1e-3)
else:
    ncam, npts, prop = {"ba_100x10k": (100, 10000, 0.1), "ba_1kx100k": (1000, 100000, 0.01), "ba_20x2k": (20, 2000, 0.3)}[a.workload]
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(ncam, npts, prop, seed=1, robust=N.HuberKernel(0.01), outlier_frac=0.05, outlier_sigma=0.05), 1e-3, 1e-3)

with N.Solver(p, unfixed, flags=_capi.FLAG_NO_SCHUR if a.no_schur else 0) as s:
    op = s.operator(0.0); ctx = s.ls.ctx; ndof = int(ctx.info.ndof)
    ctx.sweep_gradhess(); lam = a.lam * ctx.max_abs_diag(); ctx.damp(lam); maxiters = a.maxiters or None
    out = {"workload": a.workload, "no_schur": a.no_schur, "ndof": ndof, "blocks": int(ctx.info.ncost), "solve_mode": int(ctx.info.solve_mode), "lambda": lam, "rtol": a.rtol,
           "precond": a.precond, "repeats": a.repeats}

    def measure():
        ms, dev = [], []
        for _ in range(a.repeats + 1):                # (the wall time without the event pairs: each is two marker packets on the queue per product)
            t0 = time.perf_counter(); _, st = ctx.solve_pcg(a.precond, maxiters, a.rtol); ms.append(1e3 * (time.perf_counter() - t0))
        ctx.set_option(_capi.OPT_PHASE_EVENTS, 1)
        for _ in range(a.repeats + 1):
            ctx.solve_pcg(a.precond, maxiters, a.rtol); dev.append(ctx.phase_times()["pcg_us"])
        ctx.set_option(_capi.OPT_PHASE_EVENTS, 0)
        wall = float(np.median(ms[1:]))
        return {"iterations": st["iterations"], "status": st["status"], "rounds": st["rounds"], "launches": st["launches"], "relative_residual": st["rnorm"] / max(st["bnorm"], 1e-300),
                "wall_ms": wall, "wall_ms_all": [round(m, 3) for m in ms[1:]], "launches_ms": 1e-3 * float(np.median(dev[1:])), "us_per_iteration": 1e3 * wall / max(st["iterations"], 1)}

    def host_cg_solver():
        """the composition of tools/apply_only.py --cg: one synchronous product per iteration, the vector work in numpy -> solve(b) = (x, iterations)"""
        op.lam = lam
        bs = ctx.block_sizes(); bo = np.concatenate(([0], np.cumsum(bs)))[:-1]; D = op.diag_blocks()
        inv = {int(d): (np.nonzero(bs == d)[0], np.linalg.inv(np.stack([D[k] for k in np.nonzero(bs == d)[0]]))) for d in np.unique(bs)}
        def prec(r):
            z = np.empty_like(r)
            for d, (idx, m) in inv.items():
                pos = bo[idx][:, None] + np.arange(d)[None, :]; z[pos] = np.einsum("nij,nj->ni", m, r[pos])
            return z
        def solve(b):
            x = np.zeros(ndof); r = b.copy(); z = prec(r); d = z.copy(); rz = r @ z; nb = np.linalg.norm(b); it = 0
            while it < a.host_cg_maxiter and np.linalg.norm(r) > a.rtol * nb:
                q = op.matvec(d); alpha = rz / (d @ q); x += alpha * d; r -= alpha * q; z = prec(r); rz, old = r @ z, rz; d = z + (rz / old) * d; it += 1
            return x, it
        return solve

    def median_ms(f):
        ms = []
        for _ in range(a.repeats + 1):
            t0 = time.perf_counter(); res = f(); ms.append(1e3 * (time.perf_counter() - t0))
        return float(np.median(ms[1:])), [round(m, 3) for m in ms[1:]], res

    def call_stats(st):
        return {"iterations": st["iterations"].tolist(), "status": st["status"].tolist(), "synchronisations": st["synchronisations"], "launches": st["launches"],
                "product_vectors": st["product_vectors"], "batches": st["batches"]}

    if a.schur:
        nred, nelim, _, _ = ctx.schur_info(); out["schur"] = {"nred": nred, "eliminated_blocks": nelim}
        xs = ctx.solve(want_x=True)
        def timed(call):
            ms = []
            for _ in range(a.repeats + 1):
                t0 = time.perf_counter(); x, st = call(); ms.append(1e3 * (time.perf_counter() - t0))
            return {"iterations": st["iterations"], "status": st["status"], "synchronisations": st["rounds"], "launches": st["launches"],
                    "relative_residual": st["rnorm"] / max(st["bnorm"], 1e-300), "wall_ms": float(np.median(ms[1:])), "wall_ms_all": [round(m, 3) for m in ms[1:]],
                    "distance_to_nlls_solve": float(np.max(np.abs(x - xs)) / np.max(np.abs(xs)))}
        rtols = [a.rtol] + [float(v) for v in a.schur_rtols.split(",") if v]
        if len(preconds) > 1:
            out["precond"] = preconds; table = out["schur"]["preconditioners"] = {}
            for pc in preconds:
                one = timed(lambda: ctx.solve_pcg_schur(pc, 1, a.rtol, want_x=True))
                table[pc] = {"setup_ms": one["wall_ms"], "setup_ms_all": one["wall_ms_all"], "setup_launches": one["launches"]}
                for rt in rtols:
                    t = timed(lambda: ctx.solve_pcg_schur(pc, maxiters, rt, want_x=True))
                    table[pc][f"rtol_{rt:g}"] = {k: t[k] for k in ("iterations", "status", "wall_ms", "wall_ms_all", "launches", "relative_residual", "distance_to_nlls_solve")}
                    print(f"# {pc:12s} rtol {rt:g}: set-up {one['wall_ms']:.3f} ms, {t['iterations']} iterations, total {t['wall_ms']:.3f} ms", file=sys.stderr)
            print(json.dumps(out)); sys.exit(0)
        for rt in rtols:
            out["schur"][f"rtol_{rt:g}"] = {"nlls_solve_pcg": timed(lambda: ctx.solve_pcg(full_precond, maxiters, rt, want_x=True)),
                                            "nlls_solve_pcg_schur": timed(lambda: ctx.solve_pcg_schur(a.precond, maxiters, rt, want_x=True))}
        one = timed(lambda: ctx.solve_pcg_schur(a.precond, 1, a.rtol, want_x=True))
        out["schur"]["setup_ms"] = one["wall_ms"]; out["schur"]["setup_launches"] = one["launches"]
        ts = []
        for _ in range(a.repeats + 1):
            t0 = time.perf_counter(); ctx.solve(); ts.append(1e3 * (time.perf_counter() - t0))
        out["nlls_solve_ms"] = float(np.median(ts[1:]))
        rng = np.random.default_rng(1); v = rng.standard_normal(ndof); vr = rng.standard_normal(nred); ctx.set_option(_capi.OPT_PHASE_EVENTS, 1)
        for key, call in (("hess_apply_launches_us", lambda: ctx.hess_apply(v, lam)), ("schur_apply_launches_us", lambda: ctx.schur_apply(vr, lam))):
            us = []
            for _ in range(a.repeats + 1):
                call(); us.append(ctx.phase_times()["apply_us"])
            out[key] = float(np.median(us[1:]))
        ctx.set_option(_capi.OPT_PHASE_EVENTS, 0)
        out["schur_apply_over_hess_apply"] = out["schur_apply_launches_us"] / out["hess_apply_launches_us"]
    elif a.tr:
        def timed(call):
            ms = []
            for _ in range(a.repeats + 1):
                t0 = time.perf_counter(); _, st = call(); ms.append(1e3 * (time.perf_counter() - t0))
            wall = float(np.median(ms[1:]))
            return dict({k: st[k] for k in ("iterations", "status", "launches", "mnorm", "model") if k in st}, synchronisations=st["rounds"], wall_ms=wall,
                        wall_ms_all=[round(m, 3) for m in ms[1:]], us_per_iteration=1e3 * wall / max(st["iterations"], 1))
        out["tr"] = {"nlls_solve_pcg": timed(lambda: ctx.solve_pcg(a.precond, maxiters, a.rtol)),
                     "nlls_solve_pcg_tr_inf": timed(lambda: ctx.solve_pcg_tr(np.inf, a.precond, maxiters, a.rtol))}
        full = out["tr"]["nlls_solve_pcg_tr_inf"]["mnorm"]
        for fr in (float(v) for v in a.tr.split(",") if v):
            out["tr"][f"nlls_solve_pcg_tr_{fr:g}"] = dict(timed(lambda: ctx.solve_pcg_tr(fr * full, a.precond, maxiters, a.rtol)), radius=fr * full)
        out["tr"]["tr_inf_over_pcg_per_iteration"] = out["tr"]["nlls_solve_pcg_tr_inf"]["us_per_iteration"] / out["tr"]["nlls_solve_pcg"]["us_per_iteration"]
    elif a.rhs:
        B = np.zeros((a.rhs, ndof)); B[np.arange(a.rhs), np.arange(a.rhs)] = 1.0
        one, one_all, (X, st) = median_ms(lambda: ctx.solve_pcg_rhs(B, lam, _capi.VARS_CURRENT, a.precond, maxiters, a.rtol))
        def singles():
            sts = [ctx.solve_pcg_rhs(B[k], lam, _capi.VARS_CURRENT, a.precond, maxiters, a.rtol) for k in range(a.rhs)]
            return np.stack([x for x, _ in sts]), [t for _, t in sts]
        sep, sep_all, (Xs, sts) = median_ms(singles)
        out["rhs"] = {"columns": a.rhs, "one_call": dict(call_stats(st), wall_ms=one, wall_ms_all=one_all),
                      "single_column_calls": {"wall_ms": sep, "wall_ms_all": sep_all, "synchronisations": sum(t["synchronisations"] for t in sts), "launches": sum(t["launches"] for t in sts),
                                              "product_vectors": sum(t["product_vectors"] for t in sts)},
                      "same_bytes": bool(X.tobytes() == Xs.tobytes()), "one_call_over_single_column_calls": one / sep}
        if not a.no_host_cg and a.precond == "blockjacobi":
            solve = host_cg_solver(); walls = []
            for _ in range(3):
                t0 = time.perf_counter(); hs = [solve(B[k]) for k in range(a.rhs)]; walls.append(time.perf_counter() - t0)
            out["rhs"]["host_cg"] = {"iterations": [it for _, it in hs], "seconds": float(np.median(walls)), "seconds_all": [round(w, 5) for w in walls],
                                     "distance": float(max(np.max(np.abs(hs[k][0] - X[k])) / np.max(np.abs(X[k])) for k in range(a.rhs)))}
            out["rhs"]["one_call_over_host_cg"] = 1e-3 * one / out["rhs"]["host_cg"]["seconds"]
    elif a.cov:
        cams = (np.flatnonzero(np.asarray(s.ls.blockindices) > 0)[:a.cov] + 1).astype(np.int64)          # (the cameras are the first variables of these workloads)
        wall, wall_all, (cov, st) = median_ms(lambda: ctx.marginal_cov(cams, lam, _capi.VARS_CURRENT, a.precond, maxiters, a.rtol))
        m = cov.shape[0]; E = np.zeros((m, ndof)); E[np.arange(m), np.arange(m)] = 1.0
        rhs, rhs_all, (X, sx) = median_ms(lambda: ctx.solve_pcg_rhs(E, lam, _capi.VARS_CURRENT, a.precond, maxiters, a.rtol))
        out["cov"] = dict(call_stats(st), variables=cams.tolist(), m=m, wall_ms=wall, wall_ms_all=wall_all, asymmetry=float(np.max(np.abs(cov - cov.T)) / np.max(np.abs(cov))),
                          min_diagonal=float(np.min(np.diag(cov))), same_columns_through_rhs_ms=rhs, same_bytes=bool(cov.tobytes() == np.ascontiguousarray(X[:, :m].T).tobytes()))
    elif a.round:
        out["rounds"] = {}
        for r in (int(v) for v in a.round.split(",")):
            ctx.set_option(_capi.OPT_PCG_ROUND, r); out["rounds"][str(r)] = measure()
    else:
        out["pcg"] = measure()
        xp = ctx.solve_pcg(a.precond, maxiters, a.rtol, want_x=True)[0]
        ts = []
        for _ in range(a.repeats + 1):
            t0 = time.perf_counter(); xs = ctx.solve(want_x=True); ts.append(1e3 * (time.perf_counter() - t0))
        out["nlls_solve_ms"] = float(np.median(ts[1:])); out["distance_to_nlls_solve"] = float(np.max(np.abs(xp - xs)) / np.max(np.abs(xs)))
        v = np.random.default_rng(1).standard_normal(ndof); us = []; ctx.set_option(_capi.OPT_PHASE_EVENTS, 1)
        for _ in range(a.repeats + 1):
            ctx.hess_apply(v, lam); us.append(ctx.phase_times()["apply_us"])
        ctx.set_option(_capi.OPT_PHASE_EVENTS, 0)
        out["hess_apply_launches_us"] = float(np.median(us[1:]))
        if not a.no_host_cg and a.precond == "blockjacobi":
            b = ctx.get_grad(); solve = host_cg_solver(); walls = []
            for _ in range(3):
                t0 = time.perf_counter(); x, it = solve(b); walls.append(time.perf_counter() - t0)
            out["host_cg"] = {"iterations": it, "seconds": float(np.median(walls)), "seconds_all": [round(w, 5) for w in walls], "distance_to_nlls_solve": float(np.max(np.abs(-x - xs)) / np.max(np.abs(xs)))}
            out["pcg_over_host_cg"] = 1e-3 * out["pcg"]["wall_ms"] / out["host_cg"]["seconds"]
print(json.dumps(out))
