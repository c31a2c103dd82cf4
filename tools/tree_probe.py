"""Generic kernel trees through ``tree_path = "host"`` (the kernel object on the host, matrices uploaded) and ``"auto"`` (the kernel
program on the device), in one process on one device, alternating: a 256-walker LML batch
(``BayesGPR._gram_lml``) and a 128-row x 10 000-candidate predict (``GramPosterior.rows_predict``) at n = 1000, d = 8.  Wall clock around
calls that end in a device synchronise; the first call of every (tree, path, workload) is warm-up.  Writes profiles/tree_probe.json.

    python tools/tree_probe.py [--n 1000] [--walkers 256] [--rows 128] [--cand 10000] [--reps 5] [--out profiles/tree_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
from sklearn.base import clone
from sklearn.gaussian_process import kernels as sk

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bayes_skopt_amd as bask  # noqa: E402

TREES = {
    "Matern52 * RBF + White": lambda d: sk.Matern([0.5] * d, nu=2.5) * sk.RBF(1.5) + sk.WhiteKernel(0.05),
    "Constant * RationalQuadratic + White": lambda d: sk.ConstantKernel(1.0) * sk.RationalQuadratic(1.0, alpha=1.5) + sk.WhiteKernel(0.05),
}


def estimator(kernel, X, y, walkers):
    """A BayesGPR holding the training set and a context for ``walkers`` items, its posterior at the kernel's own theta (no fit)."""
    gp = bask.BayesGPR(kernel=kernel, normalize_y=False, random_state=0, max_batch=walkers)
    gp.kernel_ = clone(kernel)
    gp.X_train_, gp.y_train_ = X, y
    gp.y_train_mean_, gp.y_train_std_ = np.zeros(1), np.ones(1)
    gp._ensure_context()
    gp.theta = gp.kernel_.theta
    return gp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--walkers", type=int, default=256)
    ap.add_argument("--rows", type=int, default=128)
    ap.add_argument("--cand", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="profiles/tree_probe.json")
    a = ap.parse_args()
    rng = np.random.RandomState(0)
    X = rng.uniform(size=(a.n, a.d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.randn(a.n)
    Xc = rng.uniform(size=(a.cand, a.d))
    out = {"device": bask._lib.device_identity(0), "n": a.n, "d": a.d, "walkers": a.walkers, "rows": a.rows, "candidates": a.cand,
           "reps": a.reps, "seconds": {}}
    for name, make in TREES.items():
        gp = estimator(make(a.d), X, y, a.walkers)
        assert gp._plan.program is not None
        T = gp.kernel_.theta + 0.1 * rng.randn(a.walkers, len(gp.kernel_.theta))
        work = {"lml_batch": lambda: gp._gram_lml(T), "rows_predict": lambda: gp._post.rows_predict(gp, T[: a.rows], Xc, True)}
        for wname, call in work.items():
            times = {"host": [], "auto": []}
            for rep in range(a.reps + 1):  # (rep 0: warm-up of both paths)
                for path in ("host", "auto"):
                    gp.tree_path = path
                    t0 = time.perf_counter()
                    call()
                    if rep:
                        times[path].append(time.perf_counter() - t0)
            out["seconds"]["%s | %s" % (name, wname)] = {p: {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
                                                        for p, v in times.items()}
            print(name, wname, out["seconds"]["%s | %s" % (name, wname)], flush=True)
        gp._ctx.close()
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
