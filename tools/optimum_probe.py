"""Where is the optimum right now?  The search behind ``expected_minimum`` / ``probability_of_optimality`` /
``expected_optimality_gap`` at config E shape (n = 974 training points, d = 8, 101 starts), for the surrogate mean (kappa = 0) and
the upper bound mean + 1.96 std:

* host   ``utils.expected_minimum`` (kappa = 0) / the same scipy L-BFGS-B loop over ``predict(return_std=True)``: one start after
         the other, every iterate one device predict of d + 1 rows (a finite-difference stencil);
* device ``utils.expected_optimum``: one launch of ``bgp_minimize_starts``, one workgroup per start, analytic gradients.

Per kappa: the median wall time of --reps runs after a warm-up (device synchronised on both sides of every run), the objective
evaluations per start and microseconds per evaluation (host: wall / evaluations -- they are sequential; device: wall / the longest
start's evaluations -- the starts run side by side -- and wall / all evaluations), and the two best values.  Then
``Optimizer.expected_optimality_gap`` with ``minimizer="scipy"`` and ``"device"``.  Writes one JSON document to stdout (and --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fitted(bask, n0=974, d=8):
    rng = np.random.RandomState(0)
    opt = bask.Optimizer(dimensions=[(0.0, 1.0)] * d, n_points=500, n_initial_points=n0, init_strategy="r2", acq_func="ei",
                         random_state=0)
    X = rng.uniform(size=(n0, d)).tolist()
    opt.tell(X, [float(np.sin(3 * np.sum(x)) + 0.1 * rng.randn()) for x in X], n_samples=1, gp_samples=100, gp_burnin=10)
    return opt


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
    ap.add_argument("--starts", type=int, default=101)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bayes_skopt_amd as bask
    from bayes_skopt_amd import utils as U

    assert bask._lib.device_count() >= 1, "needs an MI355X"
    reps = max(3, args.reps)
    opt = fitted(bask)
    gp, res = opt.gp, opt._result()
    sync = lambda: bask._lib.device_synchronize(gp.device)  # noqa: E731
    calls = {"n": 0}
    predict = gp.predict

    def counting_predict(*a, **k):
        calls["n"] += 1
        return predict(*a, **k)

    out = {"shape": {"n": int(gp._X_train_.shape[0]), "d": int(gp._X_train_.shape[1]), "starts": args.starts}, "reps": reps}
    for kappa in (0.0, 1.96):
        host = (lambda: U.expected_minimum(res, n_random_starts=args.starts - 1, random_state=args.seed)) if kappa == 0.0 else \
               (lambda: U._host_optimum(res, kappa, args.starts - 1, args.seed))
        gp.predict = counting_predict
        try:
            h_ms, h_span, h_out = timed(host, reps, sync)
            h_evals = calls["n"] // (reps + 1)
        finally:
            del gp.predict
            calls["n"] = 0
        d_ms, d_span, d_out = timed(lambda: U.expected_optimum(res, kappa=kappa, n_random_starts=args.starts - 1,
                                                               random_state=args.seed), reps, sync)
        info = d_out[2]
        ev = info["evals"]
        out["kappa_%g" % kappa] = {
            "host": {"ms_median": h_ms, "ms_min_max": h_span, "evals": h_evals, "evals_per_start": h_evals / args.starts,
                     "us_per_eval": 1e3 * h_ms / h_evals, "best": h_out[1]},
            "device": {"ms_median": d_ms, "ms_min_max": d_span, "evals": int(ev.sum()), "evals_per_start": float(ev.mean()),
                       "evals_longest_start": int(ev.max()), "us_per_eval_longest_start": 1e3 * d_ms / int(ev.max()),
                       "us_per_eval_all_starts": 1e3 * d_ms / int(ev.sum()), "best": d_out[1],
                       "status_counts": np.bincount(info["status"], minlength=3).tolist(), "iters_max": int(info["iters"].max())},
            "host_over_device": h_ms / d_ms,
        }
    gap = {}
    for minimizer in ("scipy", "device"):
        try:
            ms, span, val = timed(lambda: opt.expected_optimality_gap(random_state=args.seed, minimizer=minimizer), reps, sync)
            gap[minimizer] = {"ms_median": ms, "ms_min_max": span, "value": val}
        except ValueError as e:  # (the routine's own "upper threshold" failure)
            gap[minimizer] = {"error": str(e)}
    if all("ms_median" in g for g in gap.values()):
        gap["scipy_over_device"] = gap["scipy"]["ms_median"] / gap["device"]["ms_median"]
    out["expected_optimality_gap"] = gap
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
