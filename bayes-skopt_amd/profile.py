"""Profile curves and maps of the surrogate mean: the best the mean can be with one or two coordinates held at a grid value and
every other coordinate re-optimised.  The device call is ``bgp_profile_dependence``
(``_lib.Context.profile_dependence``); this module holds what is not the device call: the same line / anchor / sweep order on the
host with scipy's L-BFGS-B (``profile_values``), which serves generic kernel trees, ``warp_inputs=True`` and more than 32 dimensions,
and the reduction over the chains both paths share."""
import sys

import numpy as np

_told = []


def tell_once(why):
    """One line on stderr, once per process: a profile searched on the host."""
    if not _told:
        _told.append(True)
        print("[bayes_skopt_amd] profile_dependence: searched on the host, one predict per iterate (%s)" % why, file=sys.stderr,
              flush=True)


def reduce_chains(chain_val, chain_x, chain_status):
    """(val, x, best_chain, n_converged) of per-chain results (..., S), (..., S, d), (..., S): the lowest value over the chains in
    ascending chain order -- a tie keeps the lower chain, a non-finite value never wins against a finite one."""
    v = np.where(np.isfinite(chain_val), chain_val, np.inf)
    best = np.argmin(v, axis=-1)  # (the first of equal values; chain 0 where no value is finite)
    val = np.take_along_axis(chain_val, best[..., None], axis=-1)[..., 0]
    x = np.take_along_axis(chain_x, best[..., None, None], axis=-2)[..., 0, :]
    return val, x, best.astype(np.int32), (chain_status == 0).sum(axis=-1).astype(np.int32)


def sweep_order(g, x_swept):
    """The cells of one line in the order a chain visits them, and the position at which the backward sweep restarts from the
    anchor's end point (``len(g)`` where there is none).  The anchor is the cell nearest ``x_swept``, ties and NaN to the lower
    index."""
    anchor, best = 0, abs(g[0] - x_swept)
    for j in range(1, len(g)):
        if abs(g[j] - x_swept) < best:
            anchor, best = j, abs(g[j] - x_swept)
    return list(range(anchor, len(g))) + list(range(anchor - 1, -1, -1)), len(g) - anchor


def profile_values(fun, X0, lo, hi, grids, panels, gtol=1e-5, max_iter=200):
    """The profile of ``fun(x) -> (value, gradient)`` over the box [lo, hi] on the host: per panel ``(k1, -1)`` / ``(k1, k2)`` and
    chain (row of ``X0``) the walk of ``bgp_profile_dependence`` -- start clipped into the box, panel coordinates overwritten, the
    anchor cell first, forward to the last cell, back from the anchor's end point to cell 0, every cell started from the previous
    cell's end point -- with scipy's L-BFGS-B on the free coordinates.  Returns a dict of per-panel lists: ``val`` (G1[, G2]), ``x``
    (..., d), ``best_chain``, ``n_converged``, ``chain_val`` / ``chain_status`` (..., S), ``chain_x`` (..., S, d); status 0:
    converged, 1: not."""
    from scipy.optimize import minimize

    X0 = np.atleast_2d(np.asarray(X0, dtype=np.float64))
    S, d = X0.shape
    lo = np.broadcast_to(np.asarray(lo, dtype=np.float64), (d,))
    hi = np.broadcast_to(np.asarray(hi, dtype=np.float64), (d,))
    out = {k: [] for k in ("val", "x", "best_chain", "n_converged", "chain_val", "chain_x", "chain_status")}
    for k1, k2 in panels:
        kf, ks = (-1, k1) if k2 < 0 else (k1, k2)
        gf = np.asarray(grids[kf], dtype=np.float64) if kf >= 0 else np.zeros(1)
        gs = np.asarray(grids[ks], dtype=np.float64)
        free = np.array([t for t in range(d) if t not in (kf, ks)], dtype=int)
        cv, cx = np.empty((len(gf), len(gs), S)), np.empty((len(gf), len(gs), S, d))
        cs = np.zeros((len(gf), len(gs), S), dtype=np.int32)
        for jf in range(len(gf)):
            for s in range(S):
                x = np.minimum(np.maximum(X0[s], lo), hi)
                if kf >= 0:
                    x[kf] = gf[jf]
                order, restart = sweep_order(gs, x[ks])
                for pos, cell in enumerate(order):
                    if pos == restart:
                        x = cx[jf, order[0], s].copy()
                    x[ks] = gs[cell]

                    def sub(z, x=x):
                        p = x.copy()
                        p[free] = z
                        f, g = fun(p)
                        return float(f), np.asarray(g, dtype=np.float64)[free]

                    st = 0
                    if len(free) and max_iter > 0:
                        r = minimize(sub, x[free], jac=True, method="L-BFGS-B", bounds=list(zip(lo[free], hi[free])),
                                     options={"gtol": gtol, "ftol": 0.0, "maxiter": max_iter})
                        x = x.copy()
                        x[free] = np.minimum(np.maximum(r.x, lo[free]), hi[free])
                        st = 0 if r.success else 1
                    cv[jf, cell, s], cx[jf, cell, s], cs[jf, cell, s] = fun(x)[0], x, st
        if kf < 0:
            cv, cx, cs = cv[0], cx[0], cs[0]
        val, xb, best, nc = reduce_chains(cv, cx, cs)
        for k, v in zip(out, (val, xb, best, nc, cv, cx, cs)):
            out[k].append(v)
    return out


def profile_by_predict(gp, X0, lo, hi, grids, panels, gtol, max_iter, why):
    """The host path of ``BayesGPR.profile_dependence`` for the median GP: ``profile_values`` on ``predict(return_mean_grad=True)``
    (y units), returned in normalised-target units with a leading axis of one posterior, as the device call returns them."""
    tell_once(why)

    def fun(x):
        mu, grad = gp.predict(x[None, :], return_mean_grad=True)
        return float(np.ravel(mu)[0]), np.asarray(grad, dtype=np.float64).reshape(-1)

    y_mean, y_std = gp._y_scale()
    got = profile_values(fun, X0, lo, hi, grids, panels, gtol=gtol, max_iter=max_iter)
    got["val"] = [(v - y_mean) / y_std for v in got["val"]]
    got["chain_val"] = [(v - y_mean) / y_std for v in got["chain_val"]]
    return {k: [v[None] for v in vs] for k, vs in got.items()}
