"""Per-row input warps of the predictive side (``Context.posterior(H, warps=W)`` + ``predict_warped``): ``_precision.ref_set_warp``
generalised from row 0 to every row b of a WARP_CASES problem.  Row b's reference is the long-double posterior and predict
(oracle/hp_oracle.py) on the training inputs AND the query points through W[b] (mpmath's Beta CDF); the tolerance is
``_precision.tol`` at kappa of row b's warped Gram matrix with row b's Beta-CDF sensitivity -- no constant of its own.
tests/test_cpu_warp_rows_reference.py qualifies it without a GPU, tests/test_gpu_warp_rows.py holds the device to it."""
import functools

import numpy as np

from _precision import ALL, F32, WARP_CASES, err_rel_max, f, problem, query, to32, tol, warp_params, warped_problem  # noqa: F401

QUANTITIES = ("alpha", "mean", "var")


@functools.lru_cache(maxsize=None)
def ref_row(cid, b):
    """Row b with its own warp: the long-double alpha, mean and var, and per quantity the scale its error is measured on and the
    Beta-CDF sensitivity ``sens`` (the fp64 computation's error with the warped inputs rounded to fp32, over 2^-24)."""
    from oracle import gp_oracle as O
    from oracle import hp_oracle as HP

    c = ALL[cid]
    st, fm = c["stationary"], c["form"]
    X, y, alpha, H, _ = problem(cid)
    Xw, W, kap = warped_problem(cid)
    ad = np.broadcast_to(alpha, (len(X),))
    Xqw = HP.warp_inputs(query(cid), W[b])
    post = HP.posterior(Xw[b], y, alpha, H[b], st, fm)
    pr = HP.predict(Xw[b], y, alpha, H[b], Xqw, st, fm, post=post)
    Ks = HP.gram(Xqw, H[b], st, fm, Y=Xw[b])
    scale = {"alpha": None, "mean": float(np.abs(Ks * post["alpha"][None, :]).sum(axis=1).max()),
             "var": float(HP.prior_var(H[b], c["d"], fm))}
    ref = {"alpha": post["alpha"], "mean": pr["mean"], "var": pr["var"]}
    X32, Xq32 = to32(f(Xw[b])), to32(f(Xqw))
    m32, s32 = O.predict(X32, y, ad, H[b], Xq32, st, fm)
    got32 = {"alpha": O.posterior(X32, y, ad, H[b], st, fm)[2], "mean": m32, "var": s32**2}
    sens = {q: err_rel_max(got32[q], ref[q], scale[q]) / F32 for q in ref}
    return {"ref": ref, "scale": scale, "sens": sens, "kappa": float(kap[b]), "W": W[b]}


def row_tol(cid, b, q):
    r = ref_row(cid, b)
    return tol(q, r["kappa"], ALL[cid]["n"], r["sens"][q])


def row_errs(cid, b, got):
    """{quantity: (err, tol)} of row b's ``got`` = {"alpha": .., "mean": .., "var": ..} (any subset)."""
    r = ref_row(cid, b)
    return {q: (err_rel_max(got[q], r["ref"][q], r["scale"][q]), row_tol(cid, b, q)) for q in got}


def moments64(cid, b, b_train=None, b_query=None):
    """The fp64 replica of row b (oracle/gp_oracle.py, scipy's Beta CDF): kernel parameters H[b], the training inputs through
    W[b_train] and the queries through W[b_query] (default: b, the correct computation; another row: the mistake this feature
    can make on that side)."""
    from oracle import gp_oracle as O

    c = ALL[cid]
    st, fm = c["stationary"], c["form"]
    X, y, alpha, H, _ = problem(cid)
    W = warp_params(cid)
    ad = np.broadcast_to(alpha, (len(X),))
    Xw = O.warp_inputs(X, W[b if b_train is None else b_train])
    Xqw = O.warp_inputs(query(cid), W[b if b_query is None else b_query])
    m, s = O.predict(Xw, y, ad, H[b], Xqw, st, fm)
    return {"alpha": O.posterior(Xw, y, ad, H[b], st, fm)[2], "mean": m, "var": s**2}
