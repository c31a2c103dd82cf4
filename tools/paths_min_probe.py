"""What does the minimiser of a posterior function draw cost?  ``PosteriorPaths.minimize`` (``bgp_paths_minimize``: one workgroup
per (start, path) carries the whole bounded quasi-Newton search) against what the package offered before it:
scipy's L-BFGS-B with ``jac=True`` over ``paths(x)`` / ``paths.gradient(x)``, one start after another, every iterate two device
calls.  Config E shape (n = 974 training points, d = 8), F = 1024 features, 128 paths x 8 starts in the unit box; both sides start
from the same points: each path's 8 lowest of 2 000 uniform candidates.

Every step is a child process of its own (it fits the same surrogate from the same seed and draws the same paths) under its own time
limit; after a step that fails or runs out of time nothing more is started and the steps not run are labelled so.  Per measurement:
the median wall time of --reps runs after a warm-up (the scipy loop warms up on the first path's starts only), the device
synchronised on both sides.  No ratio is expected in advance.  Writes one JSON document to stdout and --out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_PATHS, N_STARTS, N_CANDIDATES, N_FEATURES, GTOL, MAX_ITER = 128, 8, 2000, 1024, 1e-5, 200

# step -> (time limit in seconds, what it measures)
STEPS = {
    "device": (300, "PosteriorPaths.minimize from given starts (one launch), and with its own candidate screen"),
    "scipy": (900, "scipy L-BFGS-B (jac=True) over paths(x) / paths.gradient(x), one start after another, the same starts"),
}


def fitted(bask, n0=974, d=8):
    rng = np.random.RandomState(0)
    opt = bask.Optimizer(dimensions=[(0.0, 1.0)] * d, n_points=500, n_initial_points=n0, init_strategy="r2", acq_func="ei",
                         random_state=0)
    X = rng.uniform(size=(n0, d)).tolist()
    opt.tell(X, [float(np.sin(3 * np.sum(x)) + 0.1 * rng.randn()) for x in X], n_samples=1, gp_samples=100, gp_burnin=10)
    return opt.gp


def timed(fn, reps, sync, warm=None):
    (warm or fn)()  # (warm-up: code objects, allocations)
    ts = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ts)), "ms_min_max": [float(min(ts)), float(max(ts))]}


def run_step(step, reps):
    import bayes_skopt_amd as bask

    assert bask._lib.device_count() >= 1, "needs an MI355X"
    gp = fitted(bask)
    sync = lambda: bask._lib.device_synchronize(gp.device)  # noqa: E731
    d = int(gp._X_train_.shape[1])
    out = {"shape": {"n": int(gp._X_train_.shape[0]), "d": d, "paths": N_PATHS, "starts": N_STARTS, "features": N_FEATURES}}
    with gp.sample_paths(n_paths=N_PATHS, n_features=N_FEATURES, random_state=2) as paths:
        cand = np.random.RandomState(5).uniform(size=(N_CANDIDATES, d))
        f = paths(cand)  # (m, P)
        X0 = np.stack([cand[np.argsort(f[:, p], kind="stable")[:N_STARTS]] for p in range(N_PATHS)])
        if step == "device":
            res = paths.minimize(X0=X0, gtol=GTOL, max_iter=MAX_ITER)
            out["from_given_starts"] = timed(lambda: paths.minimize(X0=X0, gtol=GTOL, max_iter=MAX_ITER), reps, sync)
            out["with_candidate_screen"] = timed(
                lambda: paths.minimize(n_candidates=N_CANDIDATES, n_starts=N_STARTS, random_state=5, gtol=GTOL, max_iter=MAX_ITER),
                reps, sync)
            ev, st = res["evals"], res["status"]
            out["evals_total"] = int(ev.sum())
            out["evals_per_start_mean_max"] = [float(ev.mean()), int(ev.max())]
            out["iters_max"] = int(res["iters"].max())
            out["status_counts"] = np.bincount(st.ravel(), minlength=3).tolist()
            out["converged_share"] = float(np.mean(st == 0))
            out["us_per_evaluation_of_the_longest_start"] = 1e3 * out["from_given_starts"]["ms_median"] / float(ev.max())
            out["best_fun"] = res["fun"].tolist()
        elif step == "scipy":
            from scipy.optimize import minimize

            stats = {}

            def fun(x, p):
                return float(paths(x[None, :])[0, p]), np.array(paths.gradient(x[None, :])[0, p])

            def loop(n_paths):
                evals, best, conv = [], [], 0
                for p in range(n_paths):
                    vals = []
                    for s in range(N_STARTS):
                        r = minimize(fun, X0[p, s].copy(), args=(p,), jac=True, method="L-BFGS-B", bounds=[(0.0, 1.0)] * d)
                        evals.append(r.nfev)
                        vals.append(r.fun)
                        g = np.where(((r.x <= 0.0) & (r.jac > 0.0)) | ((r.x >= 1.0) & (r.jac < 0.0)), 0.0, r.jac)
                        conv += float(np.abs(g).max()) <= GTOL
                    best.append(min(vals))
                stats.update(evals=evals, best=best, conv=conv)

            out["loop"] = timed(lambda: loop(N_PATHS), reps, sync, warm=lambda: loop(1))
            ev = np.array(stats["evals"])
            out["evals_total"] = int(ev.sum())
            out["evals_per_start_mean_max"] = [float(ev.mean()), int(ev.max())]
            out["converged_share"] = stats["conv"] / float(len(ev))
            out["us_per_evaluation"] = 1e3 * out["loop"]["ms_median"] / float(ev.sum())
            out["best_fun"] = stats["best"]
        else:
            raise SystemExit("unknown step %r" % step)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its JSON")
    ap.add_argument("--skip", action="append", default=[], help="a step not to run (labelled 'not measured')")
    args = ap.parse_args()
    reps = max(3, args.reps)
    if args.step:
        print("PATHS_MIN_PROBE_JSON " + json.dumps(run_step(args.step, reps)))
        return 0
    doc = {"reps": reps, "steps": {}}
    stopped = None
    for step, (limit, what) in STEPS.items():
        entry = {"what": what, "time_limit_s": limit}
        doc["steps"][step] = entry
        if stopped or step in args.skip:
            entry["status"] = "not measured" + (": an earlier step (%s) failed or ran out of time" % stopped if stopped else
                                                ": skipped on the command line")
            continue
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(reps)], cwd=ROOT,
                                 capture_output=True, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            entry["status"] = "not measured: ran out of its time limit"
            stopped = step
            continue
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("PATHS_MIN_PROBE_JSON ")]
        if res.returncode != 0 or not lines:
            entry["status"] = "not measured: exit code %d" % res.returncode
            entry["stderr_tail"] = res.stderr[-800:]
            stopped = step
            continue
        entry["status"] = "measured"
        entry.update(json.loads(lines[-1][len("PATHS_MIN_PROBE_JSON "):]))
    dev, host = doc["steps"].get("device", {}), doc["steps"].get("scipy", {})
    if dev.get("status") == host.get("status") == "measured":
        a, b = np.array(dev.pop("best_fun")), np.array(host.pop("best_fun"))
        doc["best_value_per_path_device_minus_scipy"] = {"min": float((a - b).min()), "median": float(np.median(a - b)),
                                                         "max": float((a - b).max())}
        doc["ratio_scipy_over_device"] = host["loop"]["ms_median"] / dev["from_given_starts"]["ms_median"]
    else:
        dev.pop("best_fun", None), host.pop("best_fun", None)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
