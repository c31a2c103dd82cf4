"""Does the surrogate predict the data it has not seen?  Cross-validation at config E shape (n = 974 training points, d = 8,
Matern-5/2 product form) for B = 1, 32 and 128 hyper-posterior rows and leave-one-out, 5, 8 and 10 folds, by three routes
(DESIGN.md section 20):

* (a) ONE device call on the resident inverses (``bgp_cross_validate`` through ``Context.cross_validate``); the batched build that
      makes the rows resident is timed beside it (``build_ms``): every route below pays it, or more;
* (b) the refit route, from the entry points the tree had before only: per fold a context on the remaining points, ``posterior`` of
      the rows, ``predict`` with the covariance at the held-out points.  Leave-one-out is timed on ``--loo-folds`` folds and scaled
      to all n (``extrapolated_from_folds``): 974 refits of 128 rows are not worth the device time;
* (c) numpy on the downloaded ``K_inv``: the build with ``want_K_inv=True`` (the download: B n^2 doubles) plus the host arithmetic.

Median wall time of --reps (at least 5) runs after a warm-up, the device synchronised on both sides of every run.  A split whose
folds exceed 128 points (5 folds here: 195) is refused by (a) and reported as such.  Writes one JSON document to stdout (and --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def problem(n, d, B):
    rng = np.random.RandomState(0)
    X = rng.uniform(size=(n, d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.randn(n)
    y = (y - y.mean()) / y.std()
    h = np.concatenate([[0.0], np.full(d, np.log(0.7)), [np.log(0.02)]])
    H = h[None, :] + 0.1 * rng.randn(B, d + 2)
    return X, y, np.full(n, 1e-8), H


def refit_route(lib, X, y, alpha, H, folds):
    """(b): per fold (mean (B, s), cov (B, s, s)) of the held-out observations from a context on the remaining points."""
    n = len(y)
    out = []
    for F in folds:
        rest = np.setdiff1d(np.arange(n), F)
        ctx = lib.Context(X[rest], y[rest], alpha[rest], max_batch=len(H))
        try:
            ctx.posterior(H, want_alpha=False)
            mean, _var, cov = ctx.predict(H, X[F], return_cov=True)
        finally:
            ctx.close()
        out.append((mean, cov + np.diag(alpha[F])[None]))
    return out


def numpy_route(ctx, H, y, folds):
    """(c): the identities in numpy on the downloaded inverses; returns (mean (B, n), var (B, n), fold_lpd (B, K))."""
    from scipy.linalg import cho_factor, cho_solve

    res = ctx.posterior(H, want_alpha=True, want_K_inv=True)
    A, a = res["K_inv"], res["alpha"]
    B, n = a.shape
    mean, var, lpd = np.full((B, n), np.nan), np.full((B, n), np.nan), np.empty((B, len(folds)))
    if all(len(F) == 1 for F in folds):
        idx = np.concatenate(folds)
        dA = np.einsum("bii->bi", A)[:, idx]
        mean[:, idx], var[:, idx] = y[idx][None] - a[:, idx] / dA, 1.0 / dA
        lpd[:] = -0.5 * a[:, idx] ** 2 / dA + 0.5 * np.log(dA) - 0.5 * np.log(2 * np.pi)
        return mean, var, lpd
    for b in range(B):
        for k, F in enumerate(folds):
            cf = cho_factor(A[b][np.ix_(F, F)], lower=True, check_finite=False)
            r = cho_solve(cf, a[b, F], check_finite=False)
            mean[b, F] = y[F] - r
            var[b, F] = np.diag(cho_solve(cf, np.eye(len(F)), check_finite=False))
            lpd[b, k] = -0.5 * a[b, F] @ r + np.log(np.diag(cf[0])).sum() - 0.5 * len(F) * np.log(2 * np.pi)
    return mean, var, lpd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--n", type=int, default=974)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 32, 128])
    ap.add_argument("--splits", type=int, nargs="+", default=[0, 5, 8, 10], help="folds per split; 0: leave-one-out")
    ap.add_argument("--loo-folds", type=int, default=6)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bayes_skopt_amd as bask
    from bayes_skopt_amd.crossval import MAX_FOLD, split_folds

    lib = bask._lib
    assert lib.device_count() >= 1, "needs an MI355X"
    reps = max(5, args.reps)
    n, d = args.n, args.d
    sync = lambda: lib.device_synchronize(0)  # noqa: E731
    X, y, alpha, Hall = problem(n, d, max(args.rows))
    out = {"shape": {"n": n, "d": d, "stationary": "matern52", "form": "product"}, "reps": reps, "runs": []}
    ctx = lib.Context(X, y, alpha, max_batch=max(args.rows))
    try:
        for B in args.rows:
            H = Hall[:B]
            build_ms, build_span, _ = timed(lambda: ctx.posterior(H, want_alpha=False), reps, sync)
            for K in args.splits:
                folds = split_folds(n, K or n, random_state=1)
                run = {"rows": B, "folds": len(folds), "largest_fold": max(len(F) for F in folds), "build_ms": build_ms,
                       "build_ms_min_max": build_span}
                out["runs"].append(run)
                if run["largest_fold"] > MAX_FOLD:
                    run["a_device_call"] = "refused: a fold of %d points exceeds the limit of %d" % (run["largest_fold"], MAX_FOLD)
                    continue
                ctx.posterior(H, want_alpha=False)
                a_ms, a_span, a_out = timed(lambda: ctx.cross_validate(B, folds), reps, sync)
                assert not a_out[3].any()
                run["a_device_call"] = {"ms_median": a_ms, "ms_min_max": a_span}
                sub = folds if K else folds[: args.loo_folds]
                b_ms, b_span, b_out = timed(lambda: refit_route(lib, X, y, alpha, H, sub), reps, sync)
                scale = len(folds) / len(sub)
                diff = max(float(np.abs(m - a_out[0][:, F]).max()) for (m, _c), F in zip(b_out, sub))
                run["b_refit_route"] = {"ms_median": b_ms * scale, "ms_min_max": [v * scale for v in b_span],
                                        "extrapolated_from_folds": None if K else len(sub), "max_abs_mean_difference_to_a": diff}
                c_ms, c_span, c_out = timed(lambda: numpy_route(ctx, H, y, folds), reps, sync)
                run["c_numpy_on_downloaded_inverse"] = {"ms_median": c_ms, "ms_min_max": c_span,
                                                        "downloaded_bytes": int(B) * n * n * 8,
                                                        "max_abs_lpd_difference_to_a": float(np.abs(c_out[2] - a_out[2]).max())}
                run["b_over_a"], run["c_over_a"] = run["b_refit_route"]["ms_median"] / a_ms, c_ms / a_ms
                run["b_over_a_with_build"] = run["b_refit_route"]["ms_median"] / (a_ms + build_ms)
                print("cv_probe rows %d folds %d: device %.3f ms (+ build %.1f), refit %.1f ms, numpy %.1f ms" %
                      (B, len(folds), a_ms, build_ms, run["b_refit_route"]["ms_median"], c_ms), file=sys.stderr, flush=True)
    finally:
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
