"""The Hessian of the log marginal likelihood at config E shape (n = 974 training points, d = 8, Matern-5/2 product form; p = 10):
one ``bgp_lml_hess_batch`` call (``Context.lml_hess``) for B = 1 and B = 8 canonical vectors against (b) the gradient call alone
(``Context.lml_grad``: the posterior build that both share) and (c) the numpy host path ``lmlhess.lml_hess_host`` on an inverse and
an alpha downloaded before the clock starts.

Median wall time of --reps runs after a warm-up, the device synchronised on both sides of every run.  The product P = D K^-1 is
2 d npad^3 flop per matrix as executed; its rate is given against the Hessian call's time minus the gradient call's (the build is
in both), a lower bound of the GEMM's own rate.  Writes one JSON document to stdout (and --out, default
profiles/lml_hess_probe.json)."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lml_hess_probe.json"))
    args = ap.parse_args()
    from bayes_skopt_amd import _lib, lmlhess

    assert _lib.device_count() >= 1, "needs an MI355X"
    n, d, reps = args.n, args.d, max(3, args.reps)
    rng = np.random.RandomState(0)
    X = rng.uniform(size=(n, d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.randn(n)
    y = (y - y.mean()) / y.std()
    H = np.column_stack([0.1 * rng.randn(8), np.log(0.25 * np.sqrt(d)) + 0.2 * rng.randn(8, d), np.log(1e-2) + 0.1 * rng.randn(8)])
    ctx = _lib.Context(X, y, 1e-8, max_batch=8)
    sync = lambda: _lib.device_synchronize(0)  # noqa: E731
    npad = (n + 127) // 128 * 128
    flop = 2.0 * d * npad**3
    out = {"shape": {"n": n, "d": d, "npad": npad, "p": d + 2}, "reps": reps, "gemm_flop_per_matrix": flop}
    for B in (1, 8):
        h_ms, h_span, dev = timed(lambda: ctx.lml_hess(H[:B]), reps, sync)
        g_ms, g_span, _ = timed(lambda: ctx.lml_grad(H[:B]), reps, sync)
        blk = {"hess_call_ms_median": h_ms, "hess_call_ms_min_max": h_span, "grad_call_ms_median": g_ms, "grad_call_ms_min_max": g_span,
               "hess_over_grad": h_ms / g_ms}
        if h_ms > g_ms:
            blk["gemm_tflops_lower_bound"] = B * flop / ((h_ms - g_ms) * 1e-3) / 1e12
        out["B%d" % B] = blk
    res = ctx.posterior(H[:1], want_alpha=True, want_K_inv=True)
    Ki, al = res["K_inv"][0], res["alpha"][0]
    c_ms, c_span, host = timed(lambda: lmlhess.lml_hess_host(X, H[0], Ki, al, "matern52", "product"), reps, sync)
    d_ms, d_span, _ = timed(lambda: ctx.posterior(H[:1], want_alpha=True, want_K_inv=True), reps, sync)
    dev1 = ctx.lml_hess(H[:1])[2][0]
    out["host_B1"] = {"formula_ms_median": c_ms, "formula_ms_min_max": c_span, "build_and_download_ms_median": d_ms,
                      "build_and_download_ms_min_max": d_span, "formula_over_device_call": c_ms / out["B1"]["hess_call_ms_median"]}
    out["max_abs_difference_device_host_over_max_abs"] = float(np.abs(dev1 - host).max() / np.abs(host).max())
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
