"""Cost of one more point of a batch proposal (Optimizer.ask(n_points > 1)) at config E shape:
n = 974 training points, d = 8, 10 000 candidates; EI averaged over 128 hyper-posterior draws, and PVRS on the median GP.

Every ask(q) reports the wall time of each of its q - 1 steps (``_last_batch_info["step_ms"]``, host clock around a step that
ends in a device synchronisation) and, on the fast path, of bgp_fantasy_begin / _end.  Per path (fast = bgp_fantasy_*,
fallback = augmented training set with the existing device calls once per point) and q, over --reps asks after a warm-up:
the median / p10 / p90 of the step times, the median step time per step index j (does a step grow with j?), and the median
whole ask.  The fast step's share of the fp64 rate counts (3 d + 10) flops per generated kernel value (B m n per step)
against the 78.6 TFLOP/s fp64 vector peak of the MI355X (spec); the step's wall time includes its six other launches and
the copy of the m values, so the share is a lower bound.  Writes one JSON document to stdout (and to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fitted(bask, acq, n_samples, n0=974, d=8, m=10000):
    rng = np.random.RandomState(0)
    opt = bask.Optimizer(dimensions=[(0.0, 1.0)] * d, n_points=m, n_initial_points=n0, init_strategy="r2", acq_func=acq,
                         random_state=0)
    X = rng.uniform(size=(n0, d)).tolist()
    opt.tell(X, [float(np.sin(3 * np.sum(x)) + 0.1 * rng.randn()) for x in X], n_samples=n_samples, gp_samples=200,
             gp_burnin=10)
    return opt


def pct(a, q):
    return float(np.percentile(a, q)) if len(a) else None


def measure(opt, q, path, reps):
    opt._batch_path = path
    opt.ask(q)  # (warm-up: code objects, allocations)
    total, steps, by_j, begin, end = [], [], [[] for _ in range(q - 1)], [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        opt.ask(q)
        total.append((time.perf_counter() - t0) * 1e3)
        info = opt._last_batch_info
        steps += info["step_ms"]
        for j, t in enumerate(info["step_ms"]):
            by_j[j].append(t)
        if "begin_ms" in info:
            begin.append(info["begin_ms"])
            end.append(info["end_ms"])
    out = {"path": opt._last_batch_info["path"], "reps": reps, "ask_ms_median": pct(total, 50),
           "ask_ms_p10_p90": [pct(total, 10), pct(total, 90)], "step_ms_median": pct(steps, 50),
           "step_ms_p10_p90": [pct(steps, 10), pct(steps, 90)], "step_ms_median_by_j": [pct(t, 50) for t in by_j]}
    if begin:
        out["begin_ms_median"], out["end_ms_median"] = pct(begin, 50), pct(end, 50)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--qs", default="2,4,8,16")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--fallback-qmax", type=int, default=8, help="largest q timed on the (slow) fallback path of EI-128")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bayes_skopt_amd as bask

    assert bask._lib.device_count() >= 1, "needs an MI355X"
    qs = [int(v) for v in args.qs.split(",")]
    out = {"shape": {"n": 974, "d": 8, "m": 10000}, "fp64_vector_peak_tflops": 78.6}
    for tag, acq, ns in (("ei128", "ei", 128), ("pvrs", "pvrs", 0)):
        opt = fitted(bask, acq, ns)
        n, d, m = opt.gp._X_train_.shape[0], opt.gp._X_train_.shape[1], opt._last_candidates.shape[0]
        res = {"n": n, "draws": ns}
        paths = ("auto", "fallback") if tag == "ei128" else ("auto",)  # (PVRS has one path: auto IS the fallback)
        for path in paths:
            res[path] = {q: measure(opt, q, path, args.reps) for q in qs
                         if not (path == "fallback" and q > args.fallback_qmax)}
        if tag == "ei128":
            flops = (3 * d + 10) * ns * m * n
            fast, slow = res["auto"], res["fallback"]
            res["fast_step_fp64_share_lower_bound"] = {q: flops / (r["step_ms_median"] * 1e-3) / 78.6e12
                                                       for q, r in fast.items() if r["step_ms_median"]}
            res["fallback_step_over_fast_step"] = {q: slow[q]["step_ms_median"] / fast[q]["step_ms_median"]
                                                   for q in slow if fast.get(q) and fast[q]["step_ms_median"]}
        out[tag] = res
        del opt
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
