"""Extended-precision references for the prediction gradients (bgp_predict_grad_batch) on the posterior
cases of tests/_precision.py, with the error metrics of its model:

* dmean   max |d| / max_{i,k} sum_j |G_ijk alpha_j|        (the absolute sum a correct fp64 summation can lose digits on)
* dvar    max |d| / (2 max_{i,k} sum_j |v_ij G_ijk|),  v = K^-1 k(X, x_i)

compared with the existing tolerance classes ``tol("mean", kappa, n)`` and ``tol("var", kappa, n)``.  G_ijk = d k(x_i, X_j) / dx_k
= cf fac(r_ij) (x_ik - X_jk) / l_k^2, cf = c (product form) or 1 (sum form), fac(r) = (dS/dr) / r -- 0 at r = 0 for Matern 1/2.
Built in long double from oracle/hp_oracle.py (``posterior``, ``_S``, ``_r2``; imported, not edited)."""
import functools

import numpy as np

import _precision as P


def _fac(r2, stationary, S, xp):
    """(dS/dr) / r from squared scaled distances; ``S``: the stationary part at ``r2``; ``xp``: the scalar type."""
    if stationary == "rbf":
        return -S
    r = np.sqrt(r2)
    if stationary == "matern12":
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(r > 0, -S / r, xp(0))
    if stationary == "matern32":
        return -xp(3) * np.exp(-np.sqrt(xp(3)) * r)
    t = np.sqrt(xp(5)) * r
    return -(xp(5) / xp(3)) * (1 + t) * np.exp(-t)


def _contract(G, alpha, V):
    """dmean, dvar and their absolute-sum scales from G (m, n, d), alpha (n,), V (m, n)."""
    dmean = np.einsum("ijk,j->ik", G, alpha)
    dvar = -2 * np.einsum("ij,ijk->ik", V, G)
    s_mean = np.abs(G * alpha[None, :, None]).sum(axis=1).max()
    s_var = 2 * np.abs(V[:, :, None] * G).sum(axis=1).max()
    return dmean, dvar, float(s_mean), float(s_var)


@functools.lru_cache(maxsize=None)
def ref_gradients(cid):
    """Long-double dmean (m, d), dvar (m, d) at ``_precision.query(cid)`` and the two scales."""
    from oracle import hp_oracle as HP

    c = P.ALL[cid]
    X, _y, _alpha, H, _ = P.problem(cid)
    post = P.ref_post(cid)
    Xq = P.query(cid)
    d = X.shape[1]
    cst, ell, _s2 = HP._unpack(H[0], d)
    r2 = HP._r2(Xq, X, ell)
    S = HP._S(r2, c["stationary"])
    fac = _fac(r2, c["stationary"], S, HP.LD)
    cf = cst if c["form"] == "product" else HP.LD(1)
    diff = (HP._ld(Xq)[:, None, :] - HP._ld(X)[None, :, :]) / (ell * ell)[None, None, :]
    G = cf * fac[:, :, None] * diff
    Ks = cst * S if c["form"] == "product" else cst + S
    V = Ks @ post["K_inv"]
    dmean, dvar, s_mean, s_var = _contract(G, post["alpha"], V)
    return {"dmean": dmean, "dvar": dvar, "scale_dmean": s_mean, "scale_dvar": s_var}


def gradients64(X, y, alpha, h, Xq, stationary, form, return_scales=False):
    """The same quantities in fp64 numpy / LAPACK (the computation the device restates); ``return_scales``: + the two scales."""
    from oracle import gp_oracle as O
    from scipy.linalg import cho_solve, cholesky

    X, Xq = np.asarray(X, dtype=np.float64), np.asarray(Xq, dtype=np.float64)
    n, d = X.shape
    K = O.gram_with_jitter(X, np.broadcast_to(alpha, (n,)), h, stationary, form)
    L = cholesky(K, lower=True, check_finite=False)
    a = cho_solve((L, True), y, check_finite=False)
    cst, ell = np.exp(h[0]), np.exp(h[1 : d + 1])
    diff = Xq[:, None, :] - X[None, :, :]
    r2 = np.sum((diff / ell) ** 2, axis=2)
    if stationary == "rbf":
        S = np.exp(-0.5 * r2)
    else:
        r = np.sqrt(r2)
        S = {"matern12": lambda: np.exp(-r), "matern32": lambda: (1 + np.sqrt(3.0) * r) * np.exp(-np.sqrt(3.0) * r),
             "matern52": lambda: (1 + np.sqrt(5.0) * r + 5.0 / 3.0 * r2) * np.exp(-np.sqrt(5.0) * r)}[stationary]()
    fac = _fac(r2, stationary, S, np.float64)
    G = (cst if form == "product" else 1.0) * fac[:, :, None] * diff / (ell * ell)
    Ks = cst * S if form == "product" else cst + S
    V = cho_solve((L, True), Ks.T, check_finite=False).T
    dmean, dvar, sm, sv = _contract(G, a, V)
    return (dmean, dvar, sm, sv) if return_scales else (dmean, dvar)


def err_dmean(got, ref):
    return P.err_rel_max(got, ref["dmean"], ref["scale_dmean"])


def err_dvar(got, ref):
    return P.err_rel_max(got, ref["dvar"], ref["scale_dvar"])
