"""Which dimensions matter?  The Sobol' sensitivity indices of the surrogate at config E shape (n = 974 training points, d = 8,
Matern-5/2 product form, median GP): N = 4096 samples per matrix, the 8 singletons and the 28 pairs:

* (a) ONE device call (``bgp_sobol_indices`` through ``Context.sobol_indices``);
* (b) the same sums through ``Context.predict`` on the N (T + 2) synthesised rows, chunked, on the same context, and the numpy
      estimator: the entry points the tree had before, not the code under test;
* (c) 16 hyper-posterior rows through (a) in one call.

Median wall time of --reps runs after a warm-up, the device synchronised on both sides of every run.  (a) is also given as kernel
values per second and as a share of the fp64 vector rate, counted from the source of the inner loop for Matern-5/2 at the padded
row width 8: the 36 fp64 instructions per value of the kernel entry and the accumulation that section 16 counts (37 less the one
addition Q + t) and 8 subtractions + 8 fused multiply-adds of the distance: 52 instructions, 29 of them fused multiply-adds (81
flop); the peak is 78.6 TFLOP/s = 39.3 T instructions/s.  Writes one JSON document to stdout (and --out)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.pdep_probe import fitted, timed  # noqa: E402

INSTR_PER_VALUE, FLOP_PER_VALUE = 52, 81
PEAK_FLOPS = 78.6e12


def by_predict(ctx, Hk, A, Bm, masks, rows_per_call):
    """Route (b): the synthesised rows, ``rows_per_call`` at a time, through predict; the estimator in numpy."""
    from bayes_skopt_amd._posterior import sobol_estimator, sobol_rows

    X = np.concatenate([A, Bm] + [sobol_rows(A, Bm, m) for m in masks])
    F = np.concatenate([ctx.predict(Hk, X[r0:r0 + rows_per_call])[0] for r0 in range(0, len(X), rows_per_call)], axis=1)
    F = F.reshape(F.shape[0], len(masks) + 2, len(A))
    return sobol_estimator(F[:, 0], F[:, 1], F[:, 2:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--rows-per-call", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bayes_skopt_amd as bask
    from bayes_skopt_amd._posterior import noise_off, sobol_masks

    assert bask._lib.device_count() >= 1, "needs an MI355X"
    reps = max(3, args.reps)
    opt = fitted(bask)
    gp = opt.gp
    n, d = gp._X_train_.shape
    sync = lambda: bask._lib.device_synchronize(gp.device)  # noqa: E731
    rng = np.random.RandomState(1)
    A, Bm = opt.space.rvs_transformed(args.samples, random_state=rng), opt.space.rvs_transformed(args.samples, random_state=rng)
    masks = sobol_masks([(k,) for k in range(d)] + [(a, b) for a in range(d) for b in range(a + 1, d)], d)
    rows_synth = (len(masks) + 2) * args.samples
    values = float(rows_synth) * n
    out = {"shape": {"n": int(n), "d": int(d), "samples": args.samples, "terms": len(masks), "synthesised_rows": rows_synth,
                     "kernel_values": values}, "reps": reps}

    gp._post.make_resident(gp)
    H = gp._canonical(gp._kernel_theta_for_predict())
    a_ms, a_span, a_out = timed(lambda: gp._ctx.sobol_indices(H, A, Bm, masks), reps, sync)
    out["a_device_call"] = {"ms_median": a_ms, "ms_min_max": a_span, "kernel_values_per_s": values / (a_ms * 1e-3),
                            "frac_vector_flops": values * FLOP_PER_VALUE / (a_ms * 1e-3) / PEAK_FLOPS,
                            "frac_vector_issue": values * INSTR_PER_VALUE / (a_ms * 1e-3) / (PEAK_FLOPS / 2)}
    gp._post.make_resident(gp)
    b_ms, b_span, b_out = timed(lambda: by_predict(gp._ctx, noise_off(H), A, Bm, masks, args.rows_per_call), reps, sync)
    diff = {k: float(np.abs(np.asarray(x) - np.asarray(y)).max()) for k, x, y in zip(("f0", "V", "closed", "total"), a_out, b_out)}
    out["b_predict_route"] = {"ms_median": b_ms, "ms_min_max": b_span, "rows_per_call": args.rows_per_call,
                              "max_abs_difference_to_a": diff}
    out["b_over_a"] = b_ms / a_ms
    f0, V, closed, total = a_out
    out["indices"] = {"first": (closed[0, :d] / V[0]).tolist(), "total": (total[0, :d] / V[0]).tolist()}

    rows = np.asarray(gp.chain_)[: args.rows]
    Hr = gp._post.build_rows(gp, rows)
    c_ms, c_span, _ = timed(lambda: gp._ctx.sobol_indices(Hr, A, Bm, masks), reps, sync)
    out["c_hyper_rows"] = {"rows": int(len(rows)), "ms_median": c_ms, "ms_min_max": c_span, "ms_per_row": c_ms / len(rows),
                           "frac_vector_flops": len(rows) * values * FLOP_PER_VALUE / (c_ms * 1e-3) / PEAK_FLOPS,
                           "frac_vector_issue": len(rows) * values * INSTR_PER_VALUE / (c_ms * 1e-3) / (PEAK_FLOPS / 2)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
