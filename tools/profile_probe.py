"""Profile curves and maps of the surrogate mean at config E shape (n = 974 training points, d = 8, Matern 5/2 product form):
8 curves + 28 maps on 40-point grids, S = 4 chains -- 45 120 cells.

* (a) ONE ``bgp_profile_dependence`` call (``Context.profile_dependence``);
* (b) the per-cell loop over ``bgp_minimize_starts`` (``Context.minimize_starts`` with the cell's degenerate box, the walk of
      ``tests/test_gpu_profile.py``'s replay: all S chains of a cell in one call is NOT possible there, every chain has its own
      start) on the FIRST ``--loop-cells`` cells of the first curve and of the first map, all S chains; the figure for the whole
      call is scaled by cells and labelled so;
* (c) the scipy host path (``profile.profile_values`` on ``predict(return_mean_grad=True)``) on the first curve alone, one chain,
      scaled the same way.

Median of --reps runs after a warm-up, device synchronised on both sides of every run.  Writes one JSON document to stdout (and
--out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from optimum_probe import fitted, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=40)
    ap.add_argument("--chains", type=int, default=4)
    ap.add_argument("--loop-cells", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bayes_skopt_amd as bask
    from bayes_skopt_amd.profile import profile_values, sweep_order

    assert bask._lib.device_count() >= 1, "needs an MI355X"
    reps = max(3, args.reps)
    opt = fitted(bask)
    gp, res = opt.gp, opt._result()
    sync = lambda: bask._lib.device_synchronize(gp.device)  # noqa: E731
    d = gp._X_train_.shape[1]
    grids = [np.linspace(0.0, 1.0, args.points)] * d
    panels = [(k, -1) for k in range(d)] + [(a, b) for a in range(d) for b in range(a + 1, d)]
    order = np.argsort(np.asarray(res.func_vals), kind="stable")[:args.chains]
    X0 = np.asarray(opt.space.transform([res.x_iters[i] for i in order]), dtype=np.float64)
    H = gp._post.built_H(gp, None)
    ym, ys = gp._y_scale()
    cells = sum(args.points if b < 0 else args.points**2 for _a, b in panels)

    a_ms, a_span, a_out = timed(lambda: gp._ctx.profile_dependence(H, ym, ys, X0, 0.0, 1.0, grids, panels), reps, sync)
    nconv = sum(int(v.sum()) for v in a_out["n_converged"])

    def loop(panel, ncell):
        """The first ``ncell`` cells of the panel's first line, every chain, one minimize_starts call per (chain, cell)."""
        kf, ks = (-1, panel[0]) if panel[1] < 0 else panel
        for s in range(len(X0)):
            lo, hi, x = np.zeros(d), np.ones(d), np.clip(X0[s], 0.0, 1.0)
            if kf >= 0:
                lo[kf] = hi[kf] = x[kf] = grids[kf][0]
            for cell in sweep_order(grids[ks], x[ks])[0][:ncell]:
                lo[ks] = hi[ks] = grids[ks][cell]
                x = gp._ctx.minimize_starts(0, H, ym, ys, 0.0, x[None, :], lo, hi)["x"][0]

    nc = min(args.loop_cells, args.points)
    b_ms, b_span, _ = timed(lambda: (loop(panels[0], nc), loop(panels[d], nc)), reps, sync)
    per_cell_chain = b_ms / (2 * nc * len(X0))

    def fun(x):
        mu, g = gp.predict(x[None, :], return_mean_grad=True)
        return float(np.ravel(mu)[0]), np.asarray(g, dtype=np.float64).reshape(-1)

    c_ms, c_span, _ = timed(lambda: profile_values(fun, X0[:1], 0.0, 1.0, grids, panels[:1]), reps, sync)
    out = {"shape": {"n": int(gp._X_train_.shape[0]), "d": int(d), "points": args.points, "chains": len(X0), "panels": len(panels),
                     "cells": cells}, "reps": reps,
           "one_call": {"ms_median": a_ms, "ms_min_max": a_span, "evals": int(a_out["evals"][0]),
                        "converged_share": nconv / float(cells * len(X0)), "us_per_cell": 1e3 * a_ms / cells},
           "minimize_starts_loop": {"timed": "first %d cells of the first curve and of the first line of the first map, %d chains"
                                    % (nc, len(X0)), "ms_median": b_ms, "ms_min_max": b_span, "ms_per_chain_cell": per_cell_chain,
                                    "ms_scaled_to_all_cells": per_cell_chain * cells * len(X0), "scaled": True},
           "scipy_host": {"timed": "the first curve, one chain", "ms_median": c_ms, "ms_min_max": c_span,
                          "ms_scaled_to_all_cells": c_ms / args.points * cells * len(X0), "scaled": True}}
    out["loop_over_one_call"] = out["minimize_starts_loop"]["ms_scaled_to_all_cells"] / a_ms
    out["scipy_over_one_call"] = out["scipy_host"]["ms_scaled_to_all_cells"] / a_ms
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
