"""The joint-entropy-search acquisition at config E shape (n = 974 training points, d = 8, Matern-5/2 product form): 10 000 candidates,
the median GP (B = 1) with R = 64 optimum samples and 128 chain rows with R = 8 and with R = 64 samples each (DESIGN.md section 25;
the probe's fit keeps 100 rows, so 28 are walked twice).  The optimum samples are explicit -- uniform points of the unit box with
values a little below the row's posterior mean there --, so every route sees the same inputs.  Per configuration:

* (a) ONE device call (``bgp_joint_entropy`` through ``Context.joint_entropy``), the average alone coming back;
* (b) the host path of the package on the same inputs (``JointEntropySearch.path = "host"``: ``joint_entropy_values`` on
      ``predict(return_cov=True)`` over [A_b; chunk]); for the chain rows on ``--host-rows`` of them, given per row;
* (c) ``bgp_knowledge_gradient`` with M = R reference points (posterior 0's optimum points) on the same shapes: the same stages 1-2,
      another epilogue.

Median wall time of --reps runs after a warm-up, the device synchronised on both sides of every run.  ``--kernel-stats FILE``: the
per-kernel totals of a kernel trace of ``--trace-run`` (the B = --rows, R = --trace-optima call alone, --reps times after a warm-up;
``rocprofv3 --kernel-trace --stats``, a run of its own) are merged in.  Writes one JSON document to stdout (and --out)."""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.pdep_probe import fitted, timed  # noqa: E402


def kernel_split(path, calls):
    """Per-kernel totals of a ``rocprofv3 --kernel-trace --stats`` kernel_stats CSV, grouped by the stage of the call."""
    groups = {"gemm4_kernel<2>": "hot_product_C_minus_Ks_Pt", "gemm4_kernel<0>": "optimum_rows_P", "jes_gain": "gain_epilogue",
              "rowquad4": "variance_rowquad", "kbuild_cross": "cross_builds", "rowdot_reduce": "row_reductions",
              "finish_var": "row_reductions", "acq_sum": "average"}
    tot, other = {}, 0.0
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration") or 0.0)
            key = next((g for k, g in groups.items() if k.replace("<", "ILi").replace(">", "E") in name or k in name), None)
            if key is None:
                other += ns
            else:
                tot[key] = tot.get(key, 0.0) + ns
    allns = sum(tot.values())  # (the kernels of the call; the fit in front of it runs none of them but for one small predict)
    out = {"calls_traced": calls, "kernel_ms_per_call": {k: v / calls * 1e-6 for k, v in sorted(tot.items())},
           "call_kernels_ms_per_call": allns / calls * 1e-6, "kernels_of_the_fit_ms_total": other * 1e-6}
    if tot.get("gain_epilogue"):
        out["gain_epilogue_share_of_kernel_time"] = tot["gain_epilogue"] / allns
    out["dominant_stage"] = max(tot, key=tot.get) if tot else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--candidates", type=int, default=10000)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--host-rows", type=int, default=2)
    ap.add_argument("--trace-optima", type=int, default=64)
    ap.add_argument("--trace-run", action="store_true", help="only the B = --rows, R = --trace-optima device call, --reps times after a warm-up")
    ap.add_argument("--kernel-stats", default=None, help="kernel_stats CSV of a trace of --trace-run, merged into the document")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bayes_skopt_amd as bask
    from bayes_skopt_amd._posterior import noise_off

    assert bask._lib.device_count() >= 1, "needs an MI355X"
    reps = max(3, args.reps)
    opt = fitted(bask)
    gp = opt.gp
    n, d = gp._X_train_.shape
    m = args.candidates
    sync = lambda: bask._lib.device_synchronize(gp.device)  # noqa: E731
    Xc = opt.space.rvs_transformed(m, random_state=np.random.RandomState(1))
    y_mean, y_std = float(np.ravel(gp.y_train_mean_)[0]), float(np.ravel(gp.y_train_std_)[0])
    JES = bask.acquisition.JointEntropySearch()
    chain = np.asarray(gp.chain_)
    rows = chain[np.arange(args.rows) % len(chain)]  # (a chain shorter than --rows is walked again: a repeated row is built again)
    tau = 1e-6

    def optima(B, R):
        rng = np.random.RandomState(100 + R)
        A = rng.uniform(size=(B, R, d))
        f = gp.predict(A.reshape(-1, d)).reshape(B, R) - rng.uniform(0.0, 0.5, size=(B, R))  # y units
        return A, f

    def jes_call(H, A, f):
        noise = gp._fantasy_base_alpha() + np.exp(H[:, -1])
        return gp._ctx.joint_entropy(noise_off(H), noise, Xc, A, (f - y_mean) / y_std, tau, len(H), want_rows=False)[1]

    def kg_call(H, A):
        noise = gp._fantasy_base_alpha() + np.exp(H[:, -1])
        return gp._ctx.knowledge_gradient(noise_off(H), noise, Xc, A[0], y_std, len(H), want_rows=False)[1]

    if args.trace_run:
        A, f = optima(len(rows), args.trace_optima)  # (gp.predict makes the median GP resident: before the rows are built)
        Hr = gp._post.build_rows(gp, rows)
        jes_call(Hr, A, f)
        for _ in range(reps):
            jes_call(Hr, A, f)
        sync()
        return 0

    out = {"shape": {"n": int(n), "d": int(d), "npad": (n + 127) // 128 * 128, "candidates": m}, "reps": reps, "tau": tau}

    def block(label, build, B, R, host_rows):
        A, f = optima(B, R)  # (gp.predict makes the median GP resident: before the posteriors of the call are built)
        H = build()
        a_ms, a_span, dev = timed(lambda: jes_call(H, A, f), reps, sync)
        c_ms, c_span, _ = timed(lambda: kg_call(H, A), reps, sync)
        rec = {"posteriors": B, "optimum_samples": R, "a_device_ms_median": a_ms, "a_device_ms_min_max": a_span, "a_ms_per_row": a_ms / B,
               "c_knowledge_gradient_M_eq_R_ms_median": c_ms, "c_knowledge_gradient_ms_min_max": c_span, "a_over_c": a_ms / c_ms}
        bask.acquisition.JointEntropySearch.path = "host"
        try:
            if host_rows is None:
                b_ms, b_span, host = timed(lambda: JES(Xc, gp, optimum_samples=(A, f), tau=tau), reps, sync)
                rec.update(b_host_ms_median=b_ms, b_host_ms_min_max=b_span, b_over_a=b_ms / a_ms,
                           max_abs_difference_device_host=float(np.abs(dev - host).max()), largest_value=float(dev.max()))
            else:
                hr = max(1, host_rows)
                # (the host path draws its rows itself: any hr rows cost the same)
                b_ms, b_span, _ = timed(lambda: JES(Xc, gp, optimum_samples=(A[:hr], f[:hr]), tau=tau, n_gp_samples=hr,
                                                    random_state=np.random.RandomState(0)), reps, sync)
                rec.update(b_host_rows=hr, b_host_ms_median=b_ms, b_host_ms_min_max=b_span, b_host_ms_per_row=b_ms / hr,
                           b_over_a_per_row=(b_ms / hr) / (a_ms / B))
        finally:
            bask.acquisition.JointEntropySearch.path = "auto"
        out[label] = rec

    def median():
        gp._post.make_resident(gp)
        return np.atleast_2d(gp._canonical(gp._post_theta))

    block("median_gp_R64", median, 1, 64, None)
    block("rows_R8", lambda: gp._post.build_rows(gp, rows), len(rows), 8, args.host_rows)
    block("rows_R64", lambda: gp._post.build_rows(gp, rows), len(rows), 64, args.host_rows)
    if args.kernel_stats:
        out["kernel_trace_of_rows_R%d" % args.trace_optima] = kernel_split(args.kernel_stats, reps + 1)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
