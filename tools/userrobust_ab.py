#!/usr/bin/env python3
"""A/B of a user robust kernel against the built-in it restates: Huber2o(w) as NLLS_ROBUST_HUBER2O in the default library against its twin NLLS_ROBUST_USER0 of
tests/user_kinds/robust_kernels.hpp (robustifydcost by autodiff through nlls::Jet2) in libnlls_amd_userrobust.so, on bench.py's ba_1kx100k problem.
Each side runs in a child process of its own (the library is chosen by NLLS_AMD_LIB before it is loaded), under `timeout`.  Per side: the gradient sweep
(device time, nlls_time_sweep_gradhess) and the LM trial (wall time of nlls_lm_trial from the same point, one synchronisation each), medians over rounds.

  python tools/userrobust_ab.py [--rounds 5] [--trials 20]          (run __graft_entry__.build() first)"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nllssolver.jl_amd", "csrc")
W = 0.01


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import nllssolver_jl_amd as N
    from nllssolver_jl_amd import synthetic, _capi
    rob = N.Huber2oKernel(W) if args.side == "builtin" else N.UserRobust(N.kinds.ROBUST_USER0, W)
    p = synthetic.perturb_ba_problem(synthetic.create_ba_problem(1000, 100_000, 0.01, seed=1, robust=rob, outlier_frac=0.05, outlier_sigma=0.05), 1e-3, 1e-3)
    ctx = _capi.Context(0)
    ctx.upload(p.var_kind, p.var_dim, np.arange(1, p.nvariables + 1, dtype=np.uint64), p.groups(), 0)
    ctx.set_variables(p.variables); cost = ctx.sweep_gradhess()
    lam = 1e-4 * ctx.max_abs_diag(); n0 = ctx.solve_stats()["mf_trials"]
    trial_cost = ctx.lm_trial(lam)
    for _ in range(3): ctx.lm_trial(0.0)                                    # warm-up (the damping stays)
    sweeps, trials = [], []
    for _ in range(args.rounds):
        sweeps.append(ctx.time_sweep_gradhess(10))
        t0 = time.perf_counter()
        for _ in range(args.trials): ctx.lm_trial(0.0)
        trials.append((time.perf_counter() - t0) * 1e3 / args.trials)
    mf = ctx.solve_stats()["mf_trials"] - n0
    ctx.close()
    print(json.dumps({"side": args.side, "lib": os.path.basename(os.environ.get("NLLS_AMD_LIB", "libnlls_amd.so")), "cost": cost, "trial_cost": trial_cost,
                      "mf_trials": mf, "sweep_ms": float(np.median(sweeps)), "trial_ms": float(np.median(trials)), "sweep_all": sweeps, "trial_all": trials}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trials", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=600)
    ap.add_argument("--side", choices=("builtin", "user"))
    args = ap.parse_args()
    if args.side:
        return child(args)
    res = {}
    for side, lib in (("builtin", "libnlls_amd.so"), ("user", "libnlls_amd_userrobust.so")):
        env = dict(os.environ, NLLS_AMD_LIB=os.path.join(CSRC, lib))
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--side", side, "--rounds", str(args.rounds), "--trials", str(args.trials)]
        out = subprocess.run(cmd, capture_output=True, text=True, env=env)
        if out.returncode != 0:
            sys.stderr.write(out.stdout[-3000:] + out.stderr[-3000:])
            raise SystemExit(f"{side}: exit status {out.returncode}")
        res[side] = json.loads(out.stdout.strip().splitlines()[-1])
    b, u = res["builtin"], res["user"]
    print(json.dumps({"workload": "ba_1kx100k", "kernel": f"Huber2o({W})", "same_cost": abs(u["cost"] - b["cost"]) <= 1e-13 * abs(b["cost"]),
                      "sweep_ms": {"builtin": b["sweep_ms"], "user0": u["sweep_ms"], "ratio": u["sweep_ms"] / b["sweep_ms"]},
                      "trial_ms": {"builtin": b["trial_ms"], "user0": u["trial_ms"], "ratio": u["trial_ms"] / b["trial_ms"]},
                      "mf_trials": {"builtin": b["mf_trials"], "user0": u["mf_trials"]}, "raw": res}))


if __name__ == "__main__":
    main()
