"""Posterior distribution of the surrogate's Hessian and the curvature of the optimum.

With ``z_k = (x_k - X_jk) / l_k``, ``r^2 = sum_k z_k^2``, ``fac(r) = S'(r) / r`` as in ``CanonicalPosterior.grad_x``, ``fac2(r) =
fac'(r) / r`` (RBF: ``exp(-r^2 / 2)``; Matern 5/2: ``(25 / 3) exp(-sqrt5 r)``), ``psi = fac2(0)``, cf = c in the product form and 1 in
the sum form (the constant and white terms add nothing), ``T = d (d + 1) / 2`` and vech order (k, l), k >= l, row-major over the
lower triangle:

    h_kl(j)  = d^2 k(x, X_j) / dx_k dx_l = cf [fac delta_kl / l_k^2 + fac2 z_k z_l / (l_k l_l)]       row (k, l) of R(x), T x n
    Hbar     = R(x) alpha                                                                            Hessian of the mean
    P0       = cf psi (delta_kl delta_pq + delta_kp delta_lq + delta_kq delta_lp) / (l_k l_l l_p l_q)  prior covariance
    Cov[H_kl, H_pq] = P0 - R(x) K^-1 R(x)^T                                                          T x T, latent function

This module holds what is not the device call (``bgp_hess_cov``, ``_lib.Context.hess_cov``): the closed forms in numpy on a
downloaded ``K_inv_`` (``hessian_cov_host``: more than 16 dimensions, or forced), and the assembly of ``utils.optimum_curvature``.
Everything is in normalised-target units per unit of the transformed input squared until ``BayesGPR`` applies ``y_std``.  Matern 3/2
(``fac2 ~ 1 / r``) and Matern 1/2 have no mean-square second derivative: ValueError on both paths, never an approximation."""
import sys
import warnings

import numpy as np

HESS_DMAX = 16  # dimensions of the device call (bgp_hess.hip)
PSI = {"rbf": 1.0, "matern52": 25.0 / 3.0}  # fac2(0): the prior variance of a mixed second derivative is cf psi / (l_k l_l)^2
HOST_ROWS = 1 << 22  # entries of R (m T n) per block of the host path

_told = []


def _tell_once(why):
    """One line on stderr, once per process: the Hessian covariance computed by numpy on the downloaded inverse."""
    if not _told:
        _told.append(True)
        print("[bayes_skopt_amd] Hessian covariance: numpy on the downloaded inverse (%s)" % why, file=sys.stderr, flush=True)


def check_twice_differentiable(stationary):
    if stationary not in PSI:
        raise ValueError("the %s kernel is not twice differentiable: the Hessian of the surrogate has no posterior covariance"
                         % {"matern12": "Matern 1/2", "matern32": "Matern 3/2"}.get(stationary, stationary))


def vech_index(d):
    """(k (T,), l (T,)) of the vech order: k >= l, row-major over the lower triangle."""
    k, l = np.tril_indices(d)
    return k, l


def unvech(v, d):
    """(..., T) -> symmetric (..., d, d)."""
    k, l = vech_index(d)
    out = np.empty(v.shape[:-1] + (d, d), dtype=v.dtype)
    out[..., k, l] = v
    out[..., l, k] = v
    return out


def prior_cov(hk, d, stationary, form):
    """P0 (T, T) from one canonical vector ``hk`` (d + 2)."""
    il = 1.0 / np.exp(np.asarray(hk, dtype=np.float64)[1 : d + 1])
    cf = float(np.exp(hk[0])) if form == "product" else 1.0
    k, l = vech_index(d)
    K, L, Pq, Q = k[:, None], l[:, None], k[None, :], l[None, :]
    cnt = ((K == L) & (Pq == Q)).astype(np.float64) + ((K == Pq) & (L == Q)) + ((K == Q) & (L == Pq))
    return (cf * PSI[stationary] * cnt) * ((il[K] * il[L]) * (il[Pq] * il[Q]))  # (exactly symmetric: the products commute)


def cross_hessian(hk, Xt, Xq, stationary, form):
    """(R (m, T, n), P0 (T, T)): the second derivatives of the kernel between the query rows and the training rows with respect
    to the query, and the prior covariance of the second derivatives."""
    check_twice_differentiable(stationary)
    Xt, Xq = np.atleast_2d(np.asarray(Xt, dtype=np.float64)), np.atleast_2d(np.asarray(Xq, dtype=np.float64))
    d = Xt.shape[1]
    il = 1.0 / np.exp(np.asarray(hk, dtype=np.float64)[1 : d + 1])
    z = (Xq[:, None, :] - Xt[None, :, :]) * il
    r2 = np.sum(z * z, axis=2)
    if stationary == "rbf":
        S = np.exp(-0.5 * r2)
        fac, fac2 = -S, S
    else:
        t = np.sqrt(5.0) * np.sqrt(r2)
        e = np.exp(-t)
        fac, fac2 = -(5.0 / 3.0) * (1.0 + t) * e, (25.0 / 3.0) * e
    cf = float(np.exp(hk[0])) if form == "product" else 1.0
    w = z * il  # z_k / l_k
    k, l = vech_index(d)
    R = fac2[:, None, :] * np.swapaxes(w[:, :, k] * w[:, :, l], 1, 2)
    R = R + np.where(k == l, il[k] * il[l], 0.0)[None, :, None] * fac[:, None, :]
    return cf * R, prior_cov(hk, d, stationary, form)


def hessian_cov_host(hk, Xt, alpha, K_inv, Xq, stationary, form):
    """``(hmean (m, d, d), hvar (m, d, d), hcov (m, T, T))`` of one posterior in fp64 numpy: the closed forms above on the explicit
    inverse, block by block over the query rows.  ``hcov`` is symmetrised and its diagonal clipped at 0, and ``hvar`` is that
    diagonal, as the device call returns them."""
    Xq = np.atleast_2d(np.asarray(Xq, dtype=np.float64))
    alpha, K_inv = np.asarray(alpha, dtype=np.float64), np.asarray(K_inv, dtype=np.float64)
    n, d = np.atleast_2d(Xt).shape
    m, T = Xq.shape[0], d * (d + 1) // 2
    hmean, hvar, hcov = np.empty((m, d, d)), np.empty((m, d, d)), np.empty((m, T, T))
    step = max(1, HOST_ROWS // max(1, n * T))
    idx = np.arange(T)
    for lo in range(0, m, step):
        R, P0 = cross_hessian(hk, Xt, Xq[lo : lo + step], stationary, form)
        hmean[lo : lo + step] = unvech(R @ alpha, d)
        Q = (R @ K_inv) @ np.swapaxes(R, 1, 2)
        C = P0[None] - 0.5 * (Q + np.swapaxes(Q, 1, 2))
        C[:, idx, idx] = np.maximum(C[:, idx, idx], 0.0)
        hcov[lo : lo + step] = C
        hvar[lo : lo + step] = unvech(C[:, idx, idx], d)
    return hmean, hvar, hcov


def host_rows(gp, thetas, X, why):
    """The host path for the median GP (``thetas=None``) or a block of chain rows: ``(hmean (B, m, d, d), hvar, hcov (B, m, T, T))``."""
    _tell_once(why)
    st, fm = gp._plan.stationary, gp._plan.form
    check_twice_differentiable(st)
    Xt = gp.X_train_
    if thetas is None:
        hk = gp._canonical(gp._kernel_theta_for_predict())[0]
        out = [hessian_cov_host(hk, Xt, gp.alpha_, gp.K_inv_, X, st, fm)]
    else:
        out = []
        for t in np.atleast_2d(thetas):
            H = gp._canonical(t[None, :])
            res = gp._ctx.posterior(H, want_L=False, want_alpha=True, want_K_inv=True)
            if res["status"][0] != 0:
                raise np.linalg.LinAlgError("%d-th leading minor of the array is not positive definite" % res["status"][0])
            out.append(hessian_cov_host(H[0], Xt, res["alpha"][0], res["K_inv"][0], X, st, fm))
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def eigen_signed(Hm):
    """(eigenvalues ascending, eigenvectors as columns each signed so that its largest-magnitude component is positive) of a
    symmetric matrix -- the sign rule of ``gradcov.eigen_summary``."""
    w, V = np.linalg.eigh(0.5 * (Hm + Hm.T))
    big = np.argmax(np.abs(V), axis=0)
    return w, V * np.where(V[big, np.arange(V.shape[1])] < 0.0, -1.0, 1.0)[None, :]


def tolerances(Hm, delta):
    """(conditional, marginal) tolerances of every coordinate for a loss of ``delta``: ``sqrt(2 delta / H_kk)`` (the others held)
    and ``sqrt(2 delta (H^-1)_kk)`` (the others re-optimised); NaN where the curvature is not positive (conditional) or H is not
    positive definite (marginal)."""
    d = len(Hm)
    diag = np.diag(Hm)
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.where(diag > 0.0, np.sqrt(2.0 * delta / np.where(diag > 0.0, diag, 1.0)), np.nan)
    marg = np.full(d, np.nan)
    w = np.linalg.eigvalsh(0.5 * (Hm + Hm.T))
    if w[0] > 0.0:
        marg = np.sqrt(2.0 * delta * np.diag(np.linalg.inv(Hm)))
    return cond, marg


def draw_hessians(mean, cov, n_draws, rng):
    """(n_draws, d, d) draws ``vech H ~ N(vech mean, cov)``; the covariance is factored by an eigendecomposition with negative
    eigenvalues clipped at 0 (it may be singular)."""
    d = mean.shape[-1]
    k, l = vech_index(d)
    w, V = np.linalg.eigh(0.5 * (cov + cov.T))
    A = V * np.sqrt(np.maximum(w, 0.0))[None, :]
    v = mean[k, l][None, :] + rng.standard_normal((n_draws, len(k))) @ A.T
    return unvech(v, d)


def assemble_curvature(x, hmean, hvar, hcov, delta, n_draws, rng, path):
    """The dict of ``utils.optimum_curvature`` (without the interval) from the (d, d) / (T, T) arrays of the median GP, or (B, ...)
    stacks of chain rows in y units: the reported Hessian is the average over the rows, its variance the average within-row
    variance plus the between-row variance of the means, and the ``n_draws`` draws are dealt over the rows in turn."""
    hmean, hvar, hcov = (np.asarray(v, dtype=np.float64) for v in (hmean, hvar, hcov))
    if hmean.ndim == 2:
        hmean, hvar, hcov = hmean[None], hvar[None], hcov[None]
    B, d = hmean.shape[0], hmean.shape[-1]
    Hm = hmean.mean(axis=0)
    Hm = 0.5 * (Hm + Hm.T)
    var = hvar.mean(axis=0) + hmean.var(axis=0)
    w, V = eigen_signed(Hm)
    cond, marg = tolerances(Hm, delta)
    counts = [n_draws // B + (1 if b < n_draws % B else 0) for b in range(B)]
    draws = np.concatenate([draw_hessians(hmean[b], hcov[b], counts[b], rng) for b in range(B) if counts[b] > 0]) \
        if n_draws > 0 else np.empty((0, d, d))
    out = {"x": np.asarray(x, dtype=np.float64), "hessian": Hm, "hessian_std": np.sqrt(var), "eigenvalues": w, "eigenvectors": V,
           "tolerance_conditional": cond, "tolerance_marginal": marg, "delta": float(delta), "path": path, "n_draws": len(draws)}
    if len(draws):
        ew = np.linalg.eigvalsh(draws)
        tol = [tolerances(Hd, delta) for Hd in draws]
        out["prob_minimum"] = float(np.mean(ew[:, 0] > 0.0))
        with warnings.catch_warnings():  # (a coordinate whose tolerance is NaN in every draw has a NaN band)
            warnings.simplefilter("ignore", RuntimeWarning)
            out["band"] = {"eigenvalues": tuple(np.percentile(ew, [5.0, 95.0], axis=0)),
                           "tolerance_conditional": tuple(np.nanpercentile(np.stack([t[0] for t in tol]), [5.0, 95.0], axis=0)),
                           "tolerance_marginal": tuple(np.nanpercentile(np.stack([t[1] for t in tol]), [5.0, 95.0], axis=0))}
    else:
        out["prob_minimum"], out["band"] = float("nan"), None
    return out
