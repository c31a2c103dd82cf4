"""Which directions matter?  The active-subspace sums and the gradient covariance of the surrogate at config E shape (n = 974
training points, d = 8, Matern-5/2 product form): 1024 sample points, the median GP (B = 1) and 128 chain rows (DESIGN.md section
22; the probe's fit keeps 100 rows, so 28 are walked twice):

* (a) ONE device call (``bgp_grad_cov`` through ``Context.grad_cov``): the two sums only, and every output;
* (b) the forced host path on the same inputs: numpy on the downloaded inverse (``gradcov.gradient_cov_host``; for the chain rows
      on ``--host-rows`` of them, given per row);
* (c) ``predict_gradients`` on the same points, for scale: the gradient of mean and std, not a covariance.

Median wall time of --reps runs after a warm-up, the device synchronised on both sides of every run.  The product P = R K^-1 of
(a) is 2 npad^2 (m d padded to 128) flop per posterior as executed; its rate is given against the whole call's time (a lower bound
of the GEMM's own rate) and against the 76.7 TFLOP/s this project measured for fp64 MFMA; the per-kernel split of the call comes
from a kernel trace of this script (DESIGN.md section 22 has the table).  Writes one JSON document to stdout (and --out)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.pdep_probe import fitted, timed  # noqa: E402

MFMA_PEAK = 76.7e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--host-rows", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bayes_skopt_amd as bask
    from bayes_skopt_amd import _posterior, gradcov

    assert bask._lib.device_count() >= 1, "needs an MI355X"
    reps = max(3, args.reps)
    opt = fitted(bask)
    gp = opt.gp
    n, d = gp._X_train_.shape
    npad = (n + 127) // 128 * 128
    mdpad = (args.samples * d + 127) // 128 * 128
    gemm_flop = 2.0 * npad * npad * mdpad
    sync = lambda: bask._lib.device_synchronize(gp.device)  # noqa: E731
    Xs = opt.space.rvs_transformed(args.samples, random_state=np.random.RandomState(1))
    out = {"shape": {"n": int(n), "d": int(d), "npad": npad, "samples": args.samples, "gemm_flop_per_posterior": gemm_flop},
           "reps": reps, "mfma_peak_flops": MFMA_PEAK}

    def device_block(H, label):
        B = len(H)
        s_ms, s_span, sums = timed(lambda: gp._ctx.grad_cov(H, Xs, False, False, True), reps, sync)
        f_ms, f_span, _ = timed(lambda: gp._ctx.grad_cov(H, Xs, True, True, True), reps, sync)
        g_ms, g_span, _ = timed(lambda: gp._ctx.grad_cov(H, Xs, True, False, False), reps, sync)
        out[label] = {"posteriors": B, "sums_only_ms_median": s_ms, "sums_only_ms_min_max": s_span,
                      "all_outputs_ms_median": f_ms, "all_outputs_ms_min_max": f_span,
                      "dmean_only_no_gemm_ms_median": g_ms, "dmean_only_no_gemm_ms_min_max": g_span,
                      "gemm_tflops_lower_bound_from_whole_call": B * gemm_flop / (s_ms * 1e-3) / 1e12,
                      "gemm_share_of_mfma_peak_lower_bound": B * gemm_flop / (s_ms * 1e-3) / MFMA_PEAK}
        return sums[2]

    # the median GP
    gp._post.make_resident(gp)
    H1 = gp._canonical(gp._kernel_theta_for_predict())
    dev1 = device_block(H1, "a_device_B1")
    c_ms, c_span, _ = timed(lambda: gp.predict_gradients(Xs), reps, sync)
    out["c_predict_gradients"] = {"ms_median": c_ms, "ms_min_max": c_span}
    _posterior.CanonicalPosterior.gradient_cov_path = "host"
    try:
        b_ms, b_span, host1 = timed(lambda: gp.active_subspace(Xs), reps, sync)
        out["b_host_B1"] = {"ms_median": b_ms, "ms_min_max": b_span}
        chain = np.asarray(gp.chain_)
        rows = chain[np.arange(args.rows) % len(chain)]  # (a chain shorter than --rows is walked again: a repeated row is built again)
        hr = rows[: max(1, args.host_rows)]
        bh_ms, bh_span, _ = timed(lambda: gp.active_subspace(Xs, thetas=hr), reps, sync)
        out["b_host_rows"] = {"rows": int(len(hr)), "ms_median": bh_ms, "ms_min_max": bh_span, "ms_per_row": bh_ms / len(hr)}
    finally:
        _posterior.CanonicalPosterior.gradient_cov_path = "auto"
    y2 = float(np.ravel(gp.y_train_std_)[0]) ** 2
    out["max_abs_difference_device_host_B1"] = {"C_mean": float(np.abs(y2 * dev1[0, 0] - host1[0]).max()),
                                               "C_cov": float(np.abs(y2 * dev1[0, 1] - host1[1]).max())}
    out["b_over_a_B1"] = b_ms / out["a_device_B1"]["sums_only_ms_median"]

    # the chain rows: one batched build, one call
    # (first end to end through BayesGPR.active_subspace: a batched build and a call per max_batch rows, the builds included)
    e_ms, e_span, _ = timed(lambda: gp.active_subspace(Xs, thetas=rows), reps, sync)
    out["a_rows_end_to_end"] = {"rows": int(len(rows)), "max_batch": int(gp._ctx.max_batch), "ms_median": e_ms, "ms_min_max": e_span,
                                "ms_per_row": e_ms / len(rows)}
    rows = rows[: int(gp._ctx.max_batch)]  # (one batched build holds max_batch rows: the call alone, on what one build holds)
    Hr = gp._post.build_rows(gp, rows)
    device_block(Hr, "a_device_rows")
    out["a_device_rows"]["ms_per_row"] = out["a_device_rows"]["sums_only_ms_median"] / len(rows)
    out["b_over_a_per_row"] = out["b_host_rows"]["ms_per_row"] / out["a_device_rows"]["ms_per_row"]
    res = gradcov.assemble(y2 * dev1[0, 0], y2 * dev1[0, 1], "device")
    out["median_gp"] = {"eigenvalues": res["eigenvalues"].tolist(), "explained": res["explained"].tolist(),
                        "leading_direction": res["eigenvectors"][:, 0].tolist(),
                        "trace_share_of_C_cov": float(np.trace(res["C_cov"]) / np.trace(res["C"]))}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
