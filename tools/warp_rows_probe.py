"""What does averaging over hyper-posterior rows cost under input warping?  ``BayesGPR._predict_hyper_samples`` at config E shape
(n = 974 training points, d = 8, Matern-5/2 product form, 10 000 candidates) for B = 8 and B = 128 chain rows whose warp parameters
are drawn uniform(-0.7, 0.7):

* (a) ``_predict_hyper_samples`` as the tree has it: since the per-row-warped build and predict, ONE batched build + ONE batched
      predict; before them, the row-by-row loop (one context-level warp, one single-matrix build, one single-item predict per row).
      The script calls nothing else of the estimator, so it runs on either side of that change: run on the parent commit, this figure
      is the baseline (b) of the DESIGN table;
* (loop) the same call behind ``BayesGPR._warp_rows_path = "loop"`` where the tree has that switch, and the largest |difference| of
      its means and standard deviations to (a) (expected 0);
* (c) the un-warped ``hyper_predict`` of the same rows' kernel parameters at the same shape: the floor -- (a) - (c) is the cost of the
      B (n + m) d Beta CDFs and the per-row query traffic.

Median wall time of --reps runs after a warm-up, the device synchronised on both sides of every run.  Writes one JSON document to
stdout (and --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fitted(bask, n=974, d=8):
    """A fitted warped estimator at the shape (a short chain: the timed rows are made below, not drawn from it)."""
    rng = np.random.RandomState(0)
    X = rng.uniform(size=(n, d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.randn(n)
    gp = bask.BayesGPR(kernel=bask.construct_default_kernel(list(range(d))), random_state=0, warp_inputs=True, normalize_y=True)
    gp.fit(X, y, n_desired_samples=60, n_burnin=2, n_walkers_per_thread=60, progress=False)  # (>= 2 (d + 2 + 2d) walkers)
    return gp


def timed(fn, reps, sync):
    fn()  # (warm-up: code objects, allocations)
    ts, out = [], None
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [float(min(ts)), float(max(ts))], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--candidates", type=int, default=10000)
    ap.add_argument("--rows", type=int, nargs="+", default=[8, 128])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bayes_skopt_amd as bask

    assert bask._lib.device_count() >= 1, "needs an MI355X"
    reps = max(3, args.reps)
    gp = fitted(bask)
    n, d = gp._X_train_.shape
    n_theta = len(gp.kernel_.theta)
    sync = lambda: bask._lib.device_synchronize(gp.device)  # noqa: E731
    Xq = np.random.RandomState(1).uniform(size=(args.candidates, d))
    has_switch = hasattr(bask.BayesGPR, "_warp_rows_path")
    out = {"shape": {"n": int(n), "d": int(d), "candidates": args.candidates, "kernel": "matern52 product"}, "reps": reps,
           "batched_path_in_tree": has_switch, "rows": {}}
    for B in args.rows:
        rng = np.random.RandomState(100 + B)
        rows = np.hstack([np.asarray(gp.theta)[None, :n_theta] + 0.1 * rng.randn(B, n_theta), rng.uniform(-0.7, 0.7, size=(B, 2 * d))])
        a_ms, a_span, a_out = timed(lambda: gp._predict_hyper_samples(rows, Xq, noise_zero=True), reps, sync)
        rec = {"a_predict_hyper_samples": {"ms_median": a_ms, "ms_min_max": a_span, "ms_per_row": a_ms / B}}
        if has_switch:
            gp._warp_rows_path = "loop"
            try:
                l_ms, l_span, l_out = timed(lambda: gp._predict_hyper_samples(rows, Xq, noise_zero=True), reps, sync)
            finally:
                del gp._warp_rows_path
            rec["loop_switch"] = {"ms_median": l_ms, "ms_min_max": l_span, "ms_per_row": l_ms / B,
                                  "max_abs_difference_to_a": max(float(np.abs(x - y).max()) for x, y in zip(a_out, l_out))}
            rec["loop_over_a"] = l_ms / a_ms
        c_ms, c_span, _ = timed(lambda: gp._post.hyper_predict(gp, rows[:, :n_theta], Xq, True), reps, sync)
        rec["c_unwarped_hyper_predict"] = {"ms_median": c_ms, "ms_min_max": c_span, "ms_per_row": c_ms / B}
        rec["a_over_c"] = a_ms / c_ms
        out["rows"][str(B)] = rec
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
