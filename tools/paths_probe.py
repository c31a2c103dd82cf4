"""What do Thompson-type function draws cost over thousands of candidates?  ``mvn="cholesky"`` (a joint normal over the query
set: an m x m predictive covariance and its factor per draw) against ``mvn="pathwise"`` (``BayesGPR.sample_paths``: Matheron's rule
on random Fourier features, O(F + n) per query point) at config E shape (n = 974 training points, d = 8):

* ``sample_y(sample_mean=True, n_samples=10)`` over 10 000 candidates -- PVRS's Thompson points -- in both modes;
* ``_sample_hyper_rows`` with 128 draws -- ThompsonSampling -- at 2 000 candidates in both modes, at 10 000 candidates pathwise
  with F in {256, 1024, 4096}, and at 10 000 candidates with ``cholesky`` (128 covariances of 10 000^2, in chunks; the last step).

Every step is a child process of its own (it fits the same surrogate from the same seed) under its own time limit; after a step
that fails or runs out of time nothing more is started and the steps not run are labelled so.  Per measurement: the median wall
time of --reps runs after a warm-up, the device synchronised on both sides.  ``cholesky`` is what the package did before the
pathwise mode existed: the baseline.  Writes one JSON document to stdout and --out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# step -> (time limit in seconds, what it measures)
STEPS = {
    "thompson_points_10000": (240, "sample_y(sample_mean=True, n_samples=10), 10 000 candidates: cholesky, pathwise"),
    "hyper_rows_2000": (240, "_sample_hyper_rows, 128 draws, 2 000 candidates: cholesky, pathwise"),
    "hyper_rows_10000_pathwise": (240, "_sample_hyper_rows, 128 draws, 10 000 candidates, pathwise at F = 256, 1024, 4096"),
    "hyper_rows_10000_cholesky": (420, "_sample_hyper_rows, 128 draws, 10 000 candidates, cholesky"),
}


def fitted(bask, n0=974, d=8):
    rng = np.random.RandomState(0)
    opt = bask.Optimizer(dimensions=[(0.0, 1.0)] * d, n_points=500, n_initial_points=n0, init_strategy="r2", acq_func="ei",
                         random_state=0)
    X = rng.uniform(size=(n0, d)).tolist()
    opt.tell(X, [float(np.sin(3 * np.sum(x)) + 0.1 * rng.randn()) for x in X], n_samples=1, gp_samples=100, gp_burnin=10)
    return opt.gp


def timed(fn, reps, sync):
    fn()  # (warm-up: code objects, allocations)
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
    rng = np.random.RandomState(1)
    out = {"shape": {"n": int(gp._X_train_.shape[0]), "d": int(gp._X_train_.shape[1])}}

    def hyper(mode, X, F=1024):
        gp.mvn = mode
        if mode != "pathwise":
            return gp._sample_hyper_rows(128, X, np.random.RandomState(2))
        with gp.sample_paths(n_paths=128, n_features=F, random_state=np.random.RandomState(2)) as paths:
            return paths(X)

    if step == "thompson_points_10000":
        X = rng.uniform(size=(10000, 8))
        for mode in ("cholesky", "pathwise"):
            out[mode] = timed(lambda: gp.sample_y(X, sample_mean=True, n_samples=10, random_state=3, mvn=mode), reps, sync)
    elif step == "hyper_rows_2000":
        X = rng.uniform(size=(2000, 8))
        for mode in ("cholesky", "pathwise"):
            out[mode] = timed(lambda: hyper(mode, X), reps, sync)
    elif step == "hyper_rows_10000_pathwise":
        X = rng.uniform(size=(10000, 8))
        for F in (256, 1024, 4096):
            out["pathwise_F%d" % F] = timed(lambda: hyper("pathwise", X, F), reps, sync)
            # the device part alone: paths already begun, one evaluation of the 128 x 10 000 values
            with gp.sample_paths(n_paths=128, n_features=F, random_state=2) as paths:
                out["pathwise_F%d_eval_only" % F] = timed(lambda: paths(X), reps, sync)
    elif step == "hyper_rows_10000_cholesky":
        X = rng.uniform(size=(10000, 8))
        out["cholesky"] = timed(lambda: hyper("cholesky", X), reps, sync)
    else:
        raise SystemExit("unknown step %r" % step)
    gp.mvn = "auto"
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
        print("PATHS_PROBE_JSON " + json.dumps(run_step(args.step, reps)))
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
        lines = [ln for ln in res.stdout.splitlines() if ln.startswith("PATHS_PROBE_JSON ")]
        if res.returncode != 0 or not lines:
            entry["status"] = "not measured: exit code %d" % res.returncode
            entry["stderr_tail"] = res.stderr[-800:]
            stopped = step
            continue
        entry["status"] = "measured"
        entry.update(json.loads(lines[-1][len("PATHS_PROBE_JSON "):]))
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 1 if stopped else 0


if __name__ == "__main__":
    sys.exit(main())
