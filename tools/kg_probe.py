"""The knowledge-gradient acquisition at config E shape (n = 974 training points, d = 8, Matern-5/2 product form): 10 000 candidates,
63 reference points (the candidates of lowest mean under the median GP), the median GP (B = 1) and 128 chain rows (DESIGN.md section
23; the probe's fit keeps 100 rows, so 28 are walked twice):

* (a) ONE device call (``bgp_knowledge_gradient`` through ``Context.knowledge_gradient``), the average alone coming back -- and the
      same call with no reference point (M = 0: the cross build, the mean and the variance of the candidates, a one-line envelope),
      which is what the call costs before any of the new work;
* (b) the host path of the package on the same inputs (``KnowledgeGradient.path = "host"``: ``knowledge_gradient_values`` on
      ``predict(return_cov=True)`` over [A; chunk]) for the median GP and for ``--host-rows`` chain rows, given per row.

Median wall time of --reps runs after a warm-up, the device synchronised on both sides of every run.  The hot product C -= K_* P^T
is 2 npad pad64(m) pad64(M) flop per posterior as executed.  ``--kernel-stats FILE``: the per-kernel totals of a kernel trace of
``--trace-run`` (the B = --rows call alone, --reps times after a warm-up; ``rocprofv3 --kernel-trace --stats``, a run of its own) are
merged in -- the hot product's own rate against the 59-63 TFLOP/s the same ring reaches in ``bgp_grad_cov`` (profiles/
active_subspace_probe.json's trace) and the envelope kernel's share of the call's kernel time.  Writes one JSON
document to stdout (and --out)."""
import argparse
import csv
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.pdep_probe import fitted, timed  # noqa: E402

MFMA_PEAK = 76.7e12


def kernel_split(path, calls, flop_per_call):
    """Per-kernel totals of a ``rocprofv3 --kernel-trace --stats`` kernel_stats CSV, grouped by the stage of the call."""
    groups = {"gemm4_kernel<2>": "hot_product_C_minus_Ks_Pt", "gemm4_kernel<0>": "reference_rows_P", "kg_envelope": "envelope",
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
    if tot.get("hot_product_C_minus_Ks_Pt"):
        rate = flop_per_call * calls / (tot["hot_product_C_minus_Ks_Pt"] * 1e-9)
        out["hot_product_tflops"] = rate / 1e12
        out["hot_product_share_of_mfma_peak"] = rate / MFMA_PEAK
    if tot.get("envelope"):
        out["envelope_share_of_kernel_time"] = tot["envelope"] / allns
    out["dominant_stage"] = max(tot, key=tot.get) if tot else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--candidates", type=int, default=10000)
    ap.add_argument("--reference", type=int, default=63)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--host-rows", type=int, default=2)
    ap.add_argument("--trace-run", action="store_true", help="only the B = --rows device call, --reps times after a warm-up")
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
    npad = (n + 127) // 128 * 128
    m, M = args.candidates, args.reference
    flop = 2.0 * npad * ((m + 63) // 64 * 64) * ((M + 63) // 64 * 64)
    sync = lambda: bask._lib.device_synchronize(gp.device)  # noqa: E731
    Xc = opt.space.rvs_transformed(m, random_state=np.random.RandomState(1))
    y_std = float(np.ravel(gp.y_train_std_)[0])
    KG = bask.acquisition.KnowledgeGradient()
    A = Xc[np.argsort(gp.predict(Xc), kind="stable")[:M]]
    none = np.zeros((0, d))
    chain = np.asarray(gp.chain_)
    rows = chain[np.arange(args.rows) % len(chain)]  # (a chain shorter than --rows is walked again: a repeated row is built again)

    def call(H, ref):
        noise = gp._fantasy_base_alpha() + np.exp(H[:, -1])
        return gp._ctx.knowledge_gradient(noise_off(H), noise, Xc, ref, y_std, len(H), want_rows=False)[1]

    if args.trace_run:
        Hr = gp._post.build_rows(gp, rows)
        call(Hr, A)
        for _ in range(reps):
            call(Hr, A)
        sync()
        return 0

    out = {"shape": {"n": int(n), "d": int(d), "npad": npad, "candidates": m, "reference_points": M,
                     "hot_product_flop_per_posterior": flop}, "reps": reps, "mfma_peak_flops": MFMA_PEAK}

    def device_block(H, label):
        B = len(H)
        k_ms, k_span, vals = timed(lambda: call(H, A), reps, sync)
        z_ms, z_span, _ = timed(lambda: call(H, none), reps, sync)
        out[label] = {"posteriors": B, "ms_median": k_ms, "ms_min_max": k_span, "no_reference_points_ms_median": z_ms,
                      "no_reference_points_ms_min_max": z_span, "ms_per_row": k_ms / B,
                      "hot_product_tflops_lower_bound_from_whole_call": B * flop / (k_ms * 1e-3) / 1e12}
        return vals

    gp._post.make_resident(gp)
    dev1 = device_block(gp._canonical(gp._post_theta), "a_device_B1")
    bask.acquisition.KnowledgeGradient.path = "host"
    try:
        b_ms, b_span, host1 = timed(lambda: KG(Xc, gp, reference_points=A), reps, sync)
        out["b_host_B1"] = {"ms_median": b_ms, "ms_min_max": b_span}
        hr = max(1, args.host_rows)
        rng = np.random.RandomState(0)
        bh_ms, bh_span, _ = timed(lambda: KG(Xc, gp, reference_points=A, n_gp_samples=hr, random_state=rng), reps, sync)
        out["b_host_rows"] = {"rows": hr, "ms_median": bh_ms, "ms_min_max": bh_span, "ms_per_row": bh_ms / hr}
    finally:
        bask.acquisition.KnowledgeGradient.path = "auto"
    out["max_abs_difference_device_host_B1"] = float(np.abs(dev1 - host1).max())
    out["largest_value_B1"] = float(dev1.max())
    out["b_over_a_B1"] = b_ms / out["a_device_B1"]["ms_median"]
    Hr = gp._post.build_rows(gp, rows)
    device_block(Hr, "a_device_rows")
    out["b_over_a_per_row"] = out["b_host_rows"]["ms_per_row"] / out["a_device_rows"]["ms_per_row"]
    e_ms, e_span, _ = timed(lambda: KG(Xc, gp, reference_points=A, n_gp_samples=min(args.rows, len(chain)), random_state=0), reps, sync)
    out["a_rows_end_to_end"] = {"rows": int(min(args.rows, len(chain))), "ms_median": e_ms, "ms_min_max": e_span,
                                "what": "KnowledgeGradient.__call__: the batched posterior build and the device call"}
    if args.kernel_stats:
        out["kernel_trace_of_a_device_rows"] = kernel_split(args.kernel_stats, reps + 1, len(rows) * flop)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
