"""How sharp is the optimum?  The posterior of the surrogate's Hessian at config E shape (n = 974 training points, d = 8, Matern-5/2
product form; T = 36, Tp = 48): m = 1 and m = 128 query points, the median GP (B = 1) and 64 chain rows:

* (a) ONE device call (``bgp_hess_cov`` through ``Context.hess_cov``): every output, and the mean alone (no product);
* (b) the host path on the same inputs: numpy on the downloaded inverse -- for the median GP ``hesscov.hessian_cov_host`` itself on
      an inverse downloaded before the clock starts (the same level as the device call); for the chain rows the forced host path
      of ``hessian_posterior`` on ``--host-rows`` of them, builds and downloads included, given per row.

Median wall time of --reps runs after a warm-up, the device synchronised on both sides of every run.  The product P = R K^-1 of (a)
is 2 npad^2 (m Tp padded to 128) flop per posterior as executed; its rate is given against the whole call's time (a lower bound of
the GEMM's own rate).  Writes one JSON document to stdout (and --out)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.pdep_probe import fitted, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--host-rows", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bayes_skopt_amd as bask
    from bayes_skopt_amd import _posterior, hesscov

    assert bask._lib.device_count() >= 1, "needs an MI355X"
    reps = max(3, args.reps)
    opt = fitted(bask)
    gp = opt.gp
    n, d = gp._X_train_.shape
    npad = (n + 127) // 128 * 128
    T = d * (d + 1) // 2
    Tp = (T + 15) // 16 * 16
    sync = lambda: bask._lib.device_synchronize(gp.device)  # noqa: E731
    out = {"shape": {"n": int(n), "d": int(d), "npad": npad, "T": T, "Tp": Tp}, "reps": reps}
    chain = np.asarray(gp.chain_)
    rows = chain[np.arange(args.rows) % len(chain)]  # (a chain shorter than --rows is walked again)
    rows = rows[: int(gp._ctx.max_batch)]  # (one batched build holds max_batch rows: the call alone, on what one build holds)
    hr = rows[: max(1, args.host_rows)]
    for m in (1, 128):
        Xs = opt.space.rvs_transformed(m, random_state=np.random.RandomState(1))
        flop = 2.0 * npad * npad * ((m * Tp + 127) // 128 * 128)
        blk = {"gemm_flop_per_posterior": flop}
        gp._post.make_resident(gp)
        H1 = gp._canonical(gp._kernel_theta_for_predict())
        a_ms, a_span, dev = timed(lambda: gp._ctx.hess_cov(H1, Xs, True, True, True), reps, sync)
        g_ms, g_span, _ = timed(lambda: gp._ctx.hess_cov(H1, Xs, True, False, False), reps, sync)
        blk["a_device_B1"] = {"all_outputs_ms_median": a_ms, "all_outputs_ms_min_max": a_span, "mean_only_no_gemm_ms_median": g_ms,
                              "mean_only_no_gemm_ms_min_max": g_span,
                              "gemm_tflops_lower_bound_from_whole_call": flop / (a_ms * 1e-3) / 1e12}
        # the median GP's host side is timed at the same level as the device call: the closed forms alone, on an inverse and an
        # alpha downloaded before the clock starts (seven runs: a BLAS thread pool that wakes up shows in the spread)
        Kinv, al, Xt = np.asarray(gp.K_inv_), np.ravel(gp.alpha_), gp.X_train_
        st, fm = gp._plan.stationary, gp._plan.form
        b_ms, b_span, host = timed(lambda: hesscov.hessian_cov_host(H1[0], Xt, al, Kinv, Xs, st, fm), max(reps, 7), sync)
        y_std = float(np.ravel(gp.y_train_std_)[0])
        host = (y_std * host[0], None, y_std**2 * host[2])
        _posterior.CanonicalPosterior.hessian_cov_path = "host"
        try:
            bh_ms, bh_span, _ = timed(lambda: gp.hessian_posterior(Xs, thetas=hr, return_cov=True), reps, sync)
        finally:
            _posterior.CanonicalPosterior.hessian_cov_path = "auto"
        blk["b_host_B1"] = {"ms_median": b_ms, "ms_min_max": b_span, "runs": max(reps, 7)}
        blk["b_host_rows"] = {"rows": int(len(hr)), "ms_median": bh_ms, "ms_min_max": bh_span, "ms_per_row": bh_ms / len(hr)}
        blk["max_abs_difference_device_host_B1"] = {"hess_mean": float(np.abs(y_std * dev[0][0] - host[0]).max()),
                                                    "hess_cov": float(np.abs(y_std**2 * dev[2][0] - host[2]).max())}
        blk["b_over_a_B1"] = b_ms / a_ms
        Hr = gp._post.build_rows(gp, rows)
        r_ms, r_span, _ = timed(lambda: gp._ctx.hess_cov(Hr, Xs, True, True, True), reps, sync)
        blk["a_device_rows"] = {"posteriors": int(len(rows)), "all_outputs_ms_median": r_ms, "all_outputs_ms_min_max": r_span,
                                "ms_per_row": r_ms / len(rows),
                                "gemm_tflops_lower_bound_from_whole_call": len(rows) * flop / (r_ms * 1e-3) / 1e12}
        blk["b_over_a_per_row"] = blk["b_host_rows"]["ms_per_row"] / blk["a_device_rows"]["ms_per_row"]
        out["m%d" % m] = blk
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
