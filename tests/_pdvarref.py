"""Posterior variance of the partial dependence (``bgp_partial_dependence_var``): the cases of
tests/test_cpu_pdep_var_reference.py and tests/test_gpu_pdep_var.py on the problems of tests/_pdref.py, the long-double reference
(``hp_oracle.predict(noise_zero=True, return_cov=True)`` on the SYNTHESISED rows, a block's entries summed over S^2: no factored
distance, no kbar) and an fp64 numpy replica of the device's factored recurrences.  Errors: ``max |d var| / prior_var`` (cov on
the same scale) against ``tol("var", kappa, n)``; the mean by section 16's metric."""
import functools
import math

import numpy as np

import _pdref as R
import _precision as P


def _cases():
    rows = [  # n, d, family, form, S, ng, panels, B, Buse, twin: cells 5, 64, 65, 63, 128, 129, 127 + 5, and the r = 0 case
        (1, 1, "rbf", "product", 1, [5], [(0, -1)], 1, 1, False),
        (63, 2, "matern12", "product", 2, [8, 8], [(0, 1)], 1, 1, False),
        (64, 2, "matern32", "product", 17, [5, 13], [(0, 1)], 1, 1, False),
        (65, 9, "matern52", "product", 17, [7, 9] + [2] * 7, [(0, 1)], 1, 1, False),
        (129, 32, "rbf", "sum", 2, [8, 16] + [2] * 30, [(1, 0)], 1, 1, False),
        (20, 3, "matern12", "sum", 5, [3, 43, 5], [(0, 1)], 1, 1, False),
        (20, 3, "matern32", "sum", 5, [5, 127, 4], [(1, -1), (0, -1)], 3, 2, False),
        # a repeated curve, a pair listed as k1 > k2; sample 0 IS training point 0 and every grid holds that point's coordinate
        (40, 3, "matern52", "sum", 17, 7, [(0, -1), (2, 0), (0, -1), (1, -1)], 3, 2, True),
    ]
    return [R._case("pv%d_n%d_d%d_S%d_%s_%s" % (j, n, d, S, st, fm), n, d, st, fm, S, ng, 1700 + j, B=B, Buse=Bu, panels=pn, twin=tw)
            for j, (n, d, st, fm, S, ng, pn, B, Bu, tw) in enumerate(rows)]


CASES = _cases()
ALL = {c["id"]: c for c in CASES}
R.ALL.update(ALL)  # (``_pdref.problem`` and ``_pdref.reference`` look their cases up there)


def reference_of(X, y, alpha, h, Xs, grids, panels, stationary, form, warp=None):
    """Long double, per panel: (var shaped like the panel's block, cov (G, G) of a curve or None)."""
    from oracle import hp_oracle as HP

    S = len(Xs)
    if warp is not None:  # (per column: the training inputs, the samples and the grids once, then synthesise)
        X, Xs = HP.warp_inputs(X, warp), HP.warp_inputs(Xs, warp)
        G = HP.warp_inputs(np.array([[g[min(i, len(g) - 1)] for g in grids] for i in range(max(map(len, grids)))]), warp)
        grids = [G[: len(g), k] for k, g in enumerate(grids)]
    post = HP.lml(X, y, alpha, h, stationary, form)
    out = []
    for panel in panels:
        axes = R.panel_axes(panel, grids)
        shape, cells = R._cells(axes)
        sets = [cells] if len(axes) == 1 else [[c] for c in cells]
        blocks = []
        for cs in sets:
            rows = np.concatenate([np.asarray(R.synth_rows(Xs, axes, [c]), dtype=Xs.dtype) for c in cs])
            C = HP.predict(X, y, alpha, h, rows, stationary, form, noise_zero=True, return_cov=True, post=post)["cov"]
            blocks.append(C.reshape(len(cs), S, len(cs), S).sum(axis=(1, 3)) / (S * S))
        out.append((np.diagonal(blocks[0]).copy(), blocks[0]) if len(axes) == 1 else (np.array([b[0, 0] for b in blocks]).reshape(shape), None))
    return out


@functools.lru_cache(maxsize=None)
def reference(cid, b):
    c = ALL[cid]
    X, y, alpha, H, _kap, Xs, grids = R.problem(cid)
    return reference_of(X, y, alpha, H[b], Xs, grids, tuple(c["panels"]), c["stationary"], c["form"])


def replica64(X, y, alpha, h, Xs, grids, panels, stationary, form):
    """The device's recurrences in fp64 numpy, per panel (mean, var, cov | None)."""
    from oracle import gp_oracle as O

    (n, d), S = X.shape, len(Xs)
    K = O.gram_with_jitter(X, np.broadcast_to(alpha, (n,)), h, stationary, form)
    a, Ki = P.lml64(K, y)[1], np.linalg.inv(K)
    cst, ell = math.exp(h[0]), np.exp(np.asarray(h[1:d + 1], dtype=np.float64))
    U, u = X / ell, Xs / ell
    out = []
    for panel in panels:
        axes = R.panel_axes(panel, grids)
        shape, cells = R._cells(axes)
        rest = [k for k in range(d) if k not in [k_ for k_, _g in axes]]
        Q = sum(((u[:, k][:, None] - U[:, k][None, :]) ** 2 for k in rest), np.zeros((S, n)))
        Qss = sum(((u[:, k][:, None] - u[:, k][None, :]) ** 2 for k in rest), np.zeros((S, S)))
        T = np.array([sum((g[i] / ell[k] - U[:, k]) ** 2 for (k, g), i in zip(axes, c)) for c in cells])
        kbar = R._kernel64(Q[None, :, :] + T[:, None, :], cst, stationary, form).sum(axis=1)
        q = kbar @ Ki @ kbar.T
        prior0 = R._kernel64(Qss, cst, stationary, form).sum()
        var, cov = np.maximum((prior0 - np.diagonal(q)) / S**2, 0.0).reshape(shape), None
        if len(axes) == 1:
            gs = axes[0][1] / ell[axes[0][0]]
            Tg = (gs[:, None] - gs[None, :]) ** 2
            cov = (R._kernel64(Qss[None, None] + Tg[:, :, None, None], cst, stationary, form).sum(axis=(2, 3)) - q) / S**2
            np.fill_diagonal(cov, var)
        out.append(((kbar @ a / S).reshape(shape), var, cov))
    return out


def errs(got, ref, scale):
    """(worst var error, worst cov error) over the panels, on the prior variance's scale; ``got``: (var, cov | None) per panel."""
    ev = max(float(np.nan_to_num(np.abs(P.f(g[0]) - P.f(r[0])), nan=np.inf).max()) for g, r in zip(got, ref))
    ec = max([float(np.nan_to_num(np.abs(P.f(g[1]) - P.f(r[1])), nan=np.inf).max()) for g, r in zip(got, ref) if r[1] is not None] or [0.0])
    return ev / scale, ec / scale
