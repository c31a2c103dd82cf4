"""Case-deletion influence at config E shape (n = 974 training points, d = 8, Matern-5/2 product form): one ``bgp_influence`` call
(``Context.influence``) for B = 1 and B = 64 posteriors at m = 1 024 and 10 000 rows against (b) a plain ``bgp_predict_batch`` of the
same rows (``Context.predict``: the moments every call pays) and, at B = 1, (c) numpy ``influence.influence_values`` on an inverse,
alpha, K_* and variances downloaded before the clock starts.

Median wall time of --reps runs after a warm-up, the device synchronised on both sides of every run.  The product V = K_* K^-1 is
2 pad128(m) npad^2 flop per posterior as executed; its rate is given against the influence call's time minus the predict's, a lower
bound of the fused kernel's own rate (the difference also holds the epilogue and the strip reduction).  Writes one JSON document to
stdout (and --out, default profiles/influence_probe.json)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.pdep_probe import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=974)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "influence_probe.json"))
    args = ap.parse_args()
    from bayes_skopt_amd import _lib, influence

    assert _lib.device_count() >= 1, "needs an MI355X"
    n, d, reps, BMAX = args.n, args.d, max(3, args.reps), 64
    rng = np.random.RandomState(0)
    X = rng.uniform(size=(n, d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.randn(n)
    y = (y - y.mean()) / y.std()
    H = np.column_stack([0.1 * rng.randn(BMAX), np.log(0.25 * np.sqrt(d)) + 0.2 * rng.randn(BMAX, d), np.log(1e-2) + 0.1 * rng.randn(BMAX)])
    Hk = H.copy()
    Hk[:, -1] = -np.inf
    noise = 1e-8 + np.exp(H[:, -1])
    ctx = _lib.Context(X, y, 1e-8, max_batch=BMAX)
    sync = lambda: _lib.device_synchronize(0)  # noqa: E731
    npad = (n + 127) // 128 * 128
    out = {"shape": {"n": n, "d": d, "npad": npad}, "reps": reps}
    for m in (1024, 10000):
        Xq = rng.uniform(size=(m, d))
        flop = 2.0 * ((m + 127) // 128 * 128) * npad * npad
        for B in (1, BMAX):
            assert np.all(ctx.posterior(H[:B], want_alpha=False)["status"] == 0)
            i_ms, i_span, dev = timed(lambda: ctx.influence(Hk[:B], noise[:B], Xq, 1), reps, sync)
            p_ms, p_span, mom = timed(lambda: ctx.predict(Hk[:B], Xq), reps, sync)
            blk = {"influence_ms_median": i_ms, "influence_ms_min_max": i_span, "predict_ms_median": p_ms, "predict_ms_min_max": p_span,
                   "flop_per_posterior": flop}
            if i_ms > p_ms:
                blk["product_tflops_lower_bound"] = B * flop / ((i_ms - p_ms) * 1e-3) / 1e12
            if B == 1:
                res = ctx.posterior(H[:1], want_alpha=True, want_K_inv=True)
                t = np.sqrt(5.0) * np.sqrt(np.sum(((Xq[:, None, :] - X[None, :, :]) / np.exp(H[0, 1 : d + 1])) ** 2, axis=2))
                Ks = np.exp(H[0, 0]) * (1.0 + t + t * t / 3.0) * np.exp(-t)  # (the latent cross kernel, before the clock starts)
                h_ms, h_span, host = timed(lambda: influence.influence_values(Ks, res["K_inv"][0], res["alpha"][0], mom[1][0],
                                                                              noise[0], 1), reps, sync)
                blk.update(host_ms_median=h_ms, host_ms_min_max=h_span, host_over_device=h_ms / i_ms,
                           max_rel_difference_sum_cook=float(np.max(np.abs(dev["sum_cook"][0] - host["sum_cook"])
                                                                    / np.abs(host["sum_cook"]))))
            out["m%d_B%d" % (m, B)] = blk
    ctx.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
