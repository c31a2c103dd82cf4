"""How sure is the surrogate about its own partial dependence?  The variance of the partial-dependence figure at config E shape
(tools/pdep_probe.py's: n = 974, d = 8, Matern-5/2 product form, median GP, 250 samples, 40-point grids, 8 curves + 28 maps;
DESIGN.md section 30):

* (a) ONE ``bgp_partial_dependence_var`` call, mean + variance;
* (b) the mean alone by ``bgp_partial_dependence`` on the same inputs, for scale;
* (c) the host path (``predict(return_cov=True)`` with the noise at zero on a cell's synthesised rows) on --host-cells cells,
      EXTRAPOLATED linearly to all cells and labelled so;
* (d) 16 hyper-posterior rows through (a) in one call;
* (e) (a) with the cell covariance of the 8 curves.

Median wall time of --reps runs after a warm-up, the device synchronised on both sides of every run.  ``--only-a``: (a) alone,
for a ``rocprofv3 --kernel-trace --stats -- python tools/pdep_var_probe.py --only-a`` run (per-kernel durations).  Writes one JSON
document to stdout (and --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pdep_probe import fitted, timed  # noqa: E402  (tools/ is the script's directory)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--samples", type=int, default=250)
    ap.add_argument("--points", type=int, default=40)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--host-cells", type=int, default=12)
    ap.add_argument("--only-a", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bayes_skopt_amd as bask
    from bayes_skopt_amd._posterior import latent_cov_by_predict

    assert bask._lib.device_count() >= 1, "needs an MI355X"
    reps = max(3, args.reps)
    opt = fitted(bask)
    gp = opt.gp
    n, d = gp._X_train_.shape
    sync = lambda: bask._lib.device_synchronize(gp.device)  # noqa: E731
    Xs = opt.space.rvs_transformed(args.samples, random_state=1)
    grids = [np.linspace(0.0, 1.0, args.points)] * d
    curves = [(k, -1) for k in range(d)]
    panels = curves + [(a, b) for a in range(d) for b in range(a + 1, d)]
    cells = sum(args.points if b < 0 else args.points**2 for _a, b in panels)
    npad = (n + 127) // 128 * 128
    out = {"shape": {"n": int(n), "d": int(d), "samples": args.samples, "points": args.points, "panels": len(panels), "cells": cells,
                     "kernel_values_kbar": float(cells) * args.samples * n, "product_flop": 2.0 * cells * npad * npad,
                     "prior_pair_values": len(panels) * args.samples * (args.samples + 1) // 2}, "reps": reps}
    gp._post.make_resident(gp)
    H = gp._canonical(gp._kernel_theta_for_predict())
    a_ms, a_span, a_out = timed(lambda: gp._ctx.partial_dependence_var(H, Xs, grids, panels), reps, sync)
    out["a_mean_and_var"] = {"ms_median": a_ms, "ms_min_max": a_span}
    if not args.only_a:
        b_ms, b_span, b_out = timed(lambda: gp._ctx.partial_dependence(H, Xs, grids, panels), reps, sync)
        out["b_mean_alone"] = {"ms_median": b_ms, "ms_min_max": b_span,
                               "max_abs_difference_of_the_means": max(float(np.abs(x - y).max()) for x, y in zip(a_out[0], b_out))}
        out["a_over_b"] = a_ms / b_ms
        rng = np.random.RandomState(2)
        pick = [(int(rng.randint(d)), int(rng.randint(args.points))) for _ in range(args.host_cells)]

        def host():
            v = []
            for k, g in pick:
                X = Xs.copy()
                X[:, k] = grids[k][g]
                v.append(float(latent_cov_by_predict(gp, None, X).sum()) / args.samples**2)
            return v

        c_ms, c_span, c_out = timed(host, reps, sync)
        gp._post.make_resident(gp)
        diff = max(abs(v - float(a_out[1][k][0][g])) for v, (k, g) in zip(c_out, pick))
        out["c_host_path_extrapolated"] = {"cells_measured": len(pick), "ms_median_measured": c_ms, "ms_min_max_measured": c_span,
                                           "ms_extrapolated_to_all_cells": c_ms / len(pick) * cells,
                                           "max_abs_difference_of_the_variances": diff}
        e_ms, e_span, _ = timed(lambda: gp._ctx.partial_dependence_var(H, Xs, grids, panels, want_cov=True), reps, sync)
        out["e_with_curve_cov"] = {"ms_median": e_ms, "ms_min_max": e_span, "cov_entries": len(curves) * args.points**2}
        Hr = gp._post.build_rows(gp, np.asarray(gp.chain_)[: args.rows])
        d_ms, d_span, _ = timed(lambda: gp._ctx.partial_dependence_var(Hr, Xs, grids, panels), reps, sync)
        out["d_hyper_rows"] = {"rows": int(len(Hr)), "ms_median": d_ms, "ms_min_max": d_span, "ms_per_row": d_ms / len(Hr)}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    t0 = time.perf_counter()
    rc = main()
    print("probe wall time %.1f s" % (time.perf_counter() - t0), file=sys.stderr)
    sys.exit(rc)
