"""The hyper-posterior mixture at config E shape (n = 974 training points, d = 8, Matern-5/2 product form): 10 000 points, 128 chain
rows (the probe's fit keeps 100 rows, so 28 are walked twice), three quantiles (5 %, 50 %, 95 %) plus cdf / sf / logpdf at one value
per point.  Warm, the batched posterior build outside the timed region; per round, one after the other:

* (a) ONE device call (``bgp_predict_mixture`` through ``Context.predict_mixture``): predict and the pass behind it, 9 + Q rows of m
      numbers coming back;
* (b) ``bgp_predict_batch`` alone (``Context.predict``), the floor (a) rides on -- it downloads the 2 B m moments, which (a) does not;
* (c) numpy on the moments (b) downloaded: ordered sums, scipy's erfc, a vectorised bisection per quantile (60 halvings).

Median wall time of --reps rounds after a warm-up, the device synchronised on both sides of every run.  Reported: (a) - (b) as the cost
of the pass (negative when the download (b) pays outweighs it), (b) + (c) as what the host route costs end to end, and the solver's
largest iteration count.  Writes one JSON document to stdout (and --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.pdep_probe import fitted  # noqa: E402


def host_mixture(mean, var, y_mean, y_std, probs, t):
    """Route (c): the mixture from downloaded moments in numpy (equal weights): moments, both tails, the max-shifted log density and the
    quantiles by 60 halvings of the bracket of ``mu + z_p sd``."""
    from scipy.special import erfc, logsumexp, ndtri

    mu, sd = y_std * mean + y_mean, np.sqrt(var * (y_std * y_std))
    B = len(mu)
    m1 = mu.mean(axis=0)
    out = {"mean": m1, "within": (sd * sd).mean(axis=0), "between": ((mu - m1) ** 2).mean(axis=0)}
    z = (t[None, :] - mu) / sd
    out["cdf"] = (0.5 * erfc(-z * np.sqrt(0.5))).sum(axis=0) / B
    out["sf"] = (0.5 * erfc(z * np.sqrt(0.5))).sum(axis=0) / B
    out["logpdf"] = logsumexp(-0.5 * z * z - np.log(sd), axis=0) - np.log(B) - 0.5 * np.log(2.0 * np.pi)
    q = []
    for p in probs:
        v = mu + ndtri(p) * sd
        lo, hi = v.min(axis=0), v.max(axis=0)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            zz = (mid[None, :] - mu) / sd
            below = ((0.5 * erfc(-zz * np.sqrt(0.5))).sum(axis=0) / B < p) if p <= 0.5 else \
                ((0.5 * erfc(zz * np.sqrt(0.5))).sum(axis=0) / B > 1.0 - p)
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        q.append(hi)
    out["quantiles"] = np.array(q)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bayes_skopt_amd as bask
    from bayes_skopt_amd._posterior import noise_off

    assert bask._lib.device_count() >= 1, "needs an MI355X"
    reps = max(5, args.reps)
    opt = fitted(bask)
    gp = opt.gp
    n, d = gp._X_train_.shape
    m = args.points
    sync = lambda: bask._lib.device_synchronize(gp.device)  # noqa: E731
    Xq = opt.space.rvs_transformed(m, random_state=np.random.RandomState(1))
    y_mean, y_std = float(np.ravel(gp.y_train_mean_)[0]), float(np.ravel(gp.y_train_std_)[0])
    chain = np.asarray(gp.chain_)
    rows = chain[np.arange(args.rows) % len(chain)]  # (a chain shorter than --rows is walked again: a repeated row is built again)
    probs = (0.05, 0.5, 0.95)
    t = gp.predict(Xq) + 0.3 * np.random.RandomState(2).randn(m)
    Hk = noise_off(gp._post.build_rows(gp, rows))
    ctx = gp._ctx

    def a():
        return ctx.predict_mixture(Hk, Xq, y_mean, y_std, probs, at=t)

    def b():
        return ctx.predict(Hk, Xq)

    dev, (mean, var) = a(), b()  # (warm-up: code objects, allocations)
    host = host_mixture(mean, var, y_mean, y_std, probs, t)
    steps = ctx.mixture_stats()
    ts = {"a": [], "b": [], "c": []}
    for _ in range(reps):
        for key, fn in (("a", a), ("b", b), ("c", lambda: host_mixture(mean, var, y_mean, y_std, probs, t))):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts[key].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    out = {"shape": {"n": int(n), "d": int(d), "points": m, "rows": len(rows), "quantiles": len(probs), "at": True,
                     "moments_bytes_kept_on_the_device": 16 * len(rows) * m}, "reps": reps,
           "a_device_call_ms_median": med["a"], "a_ms_min_max": [min(ts["a"]), max(ts["a"])],
           "b_predict_alone_ms_median": med["b"], "b_ms_min_max": [min(ts["b"]), max(ts["b"])],
           "c_numpy_on_downloaded_moments_ms_median": med["c"], "c_ms_min_max": [min(ts["c"]), max(ts["c"])],
           "pass_cost_ms_a_minus_b": med["a"] - med["b"], "host_route_ms_b_plus_c": med["b"] + med["c"],
           "host_over_device": (med["b"] + med["c"]) / med["a"],
           "solver_largest_iteration_count": steps[0], "solver_largest_bracket_moves": steps[1],
           "max_abs_difference_device_host": {k: float(np.nanmax(np.abs(dev[k] - host[k]))) for k in host}}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
