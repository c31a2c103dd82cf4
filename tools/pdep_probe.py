"""What does the surrogate look like?  The data of the partial-dependence figure at config E shape (n = 974 training points, d = 8,
Matern-5/2 product form, median GP): 250 space samples, 40-point grids, all 8 curves and all 28 maps:

* (a) ONE device call (``bgp_partial_dependence`` through ``Context.partial_dependence``);
* (b) the same values through ``Context.predict`` on the synthesised rows (11.2 M of them), chunked, on the same context: the
      entry points the tree had before, not the code under test;
* (c) 16 hyper-posterior rows through (a) in one call.

Median wall time of --reps runs after a warm-up, the device synchronised on both sides of every run.  (a) is also given as kernel
values per second and as a share of the fp64 vector rate, counted from the source of the inner loop for Matern-5/2: 37 fp64
instructions per value, 21 of them fused multiply-adds (58 flop); the peak is 78.6 TFLOP/s = 39.3 T instructions/s.  Writes one
JSON document to stdout (and --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

INSTR_PER_VALUE, FLOP_PER_VALUE = 37, 58
PEAK_FLOPS = 78.6e12


def fitted(bask, n0=974, d=8):
    rng = np.random.RandomState(0)
    opt = bask.Optimizer(dimensions=[(0.0, 1.0)] * d, n_points=500, n_initial_points=n0, init_strategy="r2", acq_func="ei",
                         random_state=0)
    X = rng.uniform(size=(n0, d)).tolist()
    opt.tell(X, [float(np.sin(3 * np.sum(x)) + 0.1 * rng.randn()) for x in X], n_samples=1, gp_samples=100, gp_burnin=10)
    return opt


def timed(fn, reps, sync):
    fn()  # (warm-up: code objects, allocations)
    ts, out = [], None
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        out = fn()
        sync()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [float(min(ts)), float(max(ts))], out


def by_predict(ctx, Hk, Xs, grids, panels, rows_per_call):
    """Route (b): per panel the synthesised rows, ``rows_per_call`` at a time, the mean, the average over the samples."""
    S, d = Xs.shape
    out = []
    step = max(1, rows_per_call // S)
    for k1, k2 in panels:
        axes = [(k1, grids[k1])] + ([(k2, grids[k2])] if k2 >= 0 else [])
        shape = tuple(len(g) for _k, g in axes)
        ncell = int(np.prod(shape))
        vals = np.empty(ncell)
        for c0 in range(0, ncell, step):
            idx = np.arange(c0, min(ncell, c0 + step))
            X = np.repeat(Xs[None, :, :], len(idx), axis=0)
            for (k, g), gi in zip(axes, np.unravel_index(idx, shape)):
                X[:, :, k] = g[gi][:, None]
            vals[idx] = ctx.predict(Hk, X.reshape(-1, d))[0][0].reshape(len(idx), S).mean(axis=1)
        out.append(vals.reshape(shape))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=250)
    ap.add_argument("--points", type=int, default=40)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--rows-per-call", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bayes_skopt_amd as bask
    from bayes_skopt_amd._posterior import noise_off

    assert bask._lib.device_count() >= 1, "needs an MI355X"
    reps = max(3, args.reps)
    opt = fitted(bask)
    gp = opt.gp
    n, d = gp._X_train_.shape
    sync = lambda: bask._lib.device_synchronize(gp.device)  # noqa: E731
    Xs = opt.space.rvs_transformed(args.samples, random_state=1)
    grids = [np.linspace(0.0, 1.0, args.points)] * d
    panels = [(k, -1) for k in range(d)] + [(a, b) for a in range(d) for b in range(a + 1, d)]
    cells = sum(args.points if b < 0 else args.points**2 for _a, b in panels)
    values = float(cells) * args.samples * n
    out = {"shape": {"n": int(n), "d": int(d), "samples": args.samples, "points": args.points, "panels": len(panels), "cells": cells,
                     "kernel_values": values, "synthesised_rows": cells * args.samples}, "reps": reps}

    gp._post.make_resident(gp)
    H = gp._canonical(gp._kernel_theta_for_predict())
    a_ms, a_span, a_out = timed(lambda: gp._ctx.partial_dependence(H, Xs, grids, panels), reps, sync)
    out["a_device_call"] = {"ms_median": a_ms, "ms_min_max": a_span, "kernel_values_per_s": values / (a_ms * 1e-3),
                            "frac_vector_flops": values * FLOP_PER_VALUE / (a_ms * 1e-3) / PEAK_FLOPS,
                            "frac_vector_issue": values * INSTR_PER_VALUE / (a_ms * 1e-3) / (PEAK_FLOPS / 2)}
    gp._post.make_resident(gp)
    b_ms, b_span, b_out = timed(lambda: by_predict(gp._ctx, noise_off(H), Xs, grids, panels, args.rows_per_call), reps, sync)
    diff = max(float(np.abs(x[0] - y).max()) for x, y in zip(a_out, b_out))
    out["b_predict_route"] = {"ms_median": b_ms, "ms_min_max": b_span, "rows_per_call": args.rows_per_call,
                              "max_abs_difference_to_a": diff}
    out["b_over_a"] = b_ms / a_ms

    rows = np.asarray(gp.chain_)[: args.rows]

    Hr = gp._post.build_rows(gp, rows)
    c_ms, c_span, _ = timed(lambda: gp._ctx.partial_dependence(Hr, Xs, grids, panels), reps, sync)
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
