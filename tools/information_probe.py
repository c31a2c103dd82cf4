"""The information about the hyper-parameters at config E shape (n = 974 training points, d = 8, Matern-5/2 product form): 10 000
points, 128 chain rows (the probe's fit keeps 100 rows, so 28 are walked twice), a 32-node Gauss-Hermite rule.
Warm, the batched posterior build outside the timed region; per round, one after the other:

* (a) ONE device call (``bgp_hyper_information`` through ``Context.hyper_information``): predict and the pass behind it, 2 m numbers
      coming back;
* (b) ``bgp_predict_batch`` alone (``Context.predict``), the floor (a) rides on -- it downloads the 2 B m moments, which (a) does not;
* (c) numpy on the moments (b) downloaded, the same rule with a (B, Q, B) temporary per point -- on the first ``--host-points`` points
      only (B Q B exponentials per point: all 10 000 take minutes), reported as measured and scaled to all points.

Median wall time of --reps rounds after a warm-up, the device synchronised on both sides of every run.  Writes one JSON document to
stdout (and --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.pdep_probe import fitted  # noqa: E402


def host_information(mean, var, y_mean, y_std, t, omega):
    """Route (c): equal weights, the rule of bgp_info.hip in numpy, one point after the other."""
    from scipy.special import logsumexp

    mu, sd = y_std * mean + y_mean, np.sqrt(var * (y_std * y_std))
    B, m = mu.shape
    lw, om = -np.log(B), omega / np.sqrt(np.pi)
    info, ent = np.empty(m), np.empty(m)
    for i in range(m):
        L = lw - np.log(sd[:, i])
        y = mu[:, i, None] + np.sqrt(2.0) * sd[:, i, None] * t[None, :]
        lse = logsumexp(L[None, None, :] - 0.5 * ((y[:, :, None] - mu[None, None, :, i]) / sd[None, None, :, i]) ** 2, axis=2)
        info[i] = (((L[:, None] - t[None, :] ** 2 - lse) - lw) * om[None, :]).sum() / B
        ent[i] = 0.5 * np.log(2.0 * np.pi) - (lse * om[None, :]).sum() / B
    return info, ent


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--nodes", type=int, default=32)
    ap.add_argument("--host-points", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bayes_skopt_amd as bask

    assert bask._lib.device_count() >= 1, "needs an MI355X"
    reps = max(3, args.reps)
    opt = fitted(bask)
    gp = opt.gp
    n, d = gp._X_train_.shape
    m, mh = args.points, min(args.host_points, args.points)
    sync = lambda: bask._lib.device_synchronize(gp.device)  # noqa: E731
    Xq = opt.space.rvs_transformed(m, random_state=np.random.RandomState(1))
    y_mean, y_std = float(np.ravel(gp.y_train_mean_)[0]), float(np.ravel(gp.y_train_std_)[0])
    chain = np.asarray(gp.chain_)
    rows = chain[np.arange(args.rows) % len(chain)]
    H = gp._post.build_rows(gp, rows)  # (every row keeps its white level: the predictive of an observation)
    ctx = gp._ctx
    t, omega = np.polynomial.hermite.hermgauss(args.nodes)

    def a():
        return ctx.hyper_information(H, Xq, y_mean, y_std, n_nodes=args.nodes)

    def b():
        return ctx.predict(H, Xq)

    def c():
        return host_information(mean[:, :mh], var[:, :mh], y_mean, y_std, t, omega)

    dev, (mean, var) = a(), b()  # (warm-up: code objects, allocations)
    host = c()
    ts = {"a": [], "b": [], "c": []}
    for _ in range(reps):
        for key, fn in (("a", a), ("b", b), ("c", c)):
            sync()
            t0 = time.perf_counter()
            fn()
            sync()
            ts[key].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    c_all = med["c"] * m / mh
    out = {"shape": {"n": int(n), "d": int(d), "points": m, "rows": len(rows), "nodes": args.nodes,
                     "exponentials": len(rows) * args.nodes * len(rows) * m}, "reps": reps,
           "a_device_call_ms_median": med["a"], "a_ms_min_max": [min(ts["a"]), max(ts["a"])],
           "b_predict_alone_ms_median": med["b"], "b_ms_min_max": [min(ts["b"]), max(ts["b"])],
           "c_numpy_ms_median_on_host_points": med["c"], "c_host_points": mh, "c_scaled_to_all_points_ms": c_all,
           "pass_cost_ms_a_minus_b": med["a"] - med["b"], "host_route_ms_b_plus_c_scaled": med["b"] + c_all,
           "host_over_device": (med["b"] + c_all) / med["a"],
           "information_min_median_max": [float(np.min(dev["information"])), float(np.median(dev["information"])),
                                          float(np.max(dev["information"]))],
           "max_abs_difference_device_host": {"information": float(np.max(np.abs(dev["information"][:mh] - host[0]))),
                                              "entropy": float(np.max(np.abs(dev["entropy"][:mh] - host[1])))}}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
