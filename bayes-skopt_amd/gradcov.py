"""Posterior distribution of the surrogate's gradient and the active subspace.

With ``G_jk(x) = d k(x, X_j) / dx_k = cf fac(r_j) (x_k - X_jk) / l_k^2`` (cf = c in the product form, 1 in the sum form; ``fac`` as
in ``CanonicalPosterior.grad_x``; the constant and white terms add nothing) and ``phi = -fac(0)`` (1 RBF, 3 Matern 3/2, 5/3 Matern
5/2):

    g(x)     = G(x)^T alpha                                   gradient of the mean
    Sigma(x) = diag(cf phi / l_k^2) - G(x)^T K^-1 G(x)        posterior covariance of grad f(x), latent function
    C_mean   = mean_s g(x_s) g(x_s)^T      C_cov = mean_s Sigma(x_s)      C = C_mean + C_cov   (the active-subspace matrix)

This module holds what is not the device call (``bgp_grad_cov``, ``_lib.Context.grad_cov``): the closed forms in numpy on a
downloaded ``K_inv_`` (``gradient_cov_host``: more than 32 dimensions, or forced), the choice between the two, and the assembly of
the result of ``utils.active_subspace``.  Everything is in normalised-target units per unit of the transformed input until
``BayesGPR`` applies ``y_std``.  Matern 1/2 has no mean-square derivative: ValueError on both paths, never an approximation."""
import sys

import numpy as np

GCOV_DMAX = 32  # dimensions of the device call (bgp_gcov.hip)
PHI = {"rbf": 1.0, "matern32": 3.0, "matern52": 5.0 / 3.0}  # -fac(0): the prior variance of a derivative is cf phi / l^2
HOST_ROWS = 1 << 22  # entries of G (m n d) per block of the host path

_told = []


def _tell_once(why):
    """One line on stderr, once per process: the gradient covariance computed by numpy on the downloaded inverse."""
    if not _told:
        _told.append(True)
        print("[bayes_skopt_amd] gradient covariance: numpy on the downloaded inverse (%s)" % why, file=sys.stderr, flush=True)


def check_differentiable(stationary):
    if stationary not in PHI:
        raise ValueError("the Matern 1/2 kernel is not differentiable: the gradient of the surrogate has no posterior covariance")


def cross_gradient(hk, Xt, Xq, stationary, form):
    """(G (m, n, d), H0 diagonal (d,)) from one canonical vector ``hk`` (d + 2): the cross derivative of the kernel between the
    query rows and the training rows, and the prior variance of every partial derivative."""
    check_differentiable(stationary)
    Xt, Xq = np.atleast_2d(np.asarray(Xt, dtype=np.float64)), np.atleast_2d(np.asarray(Xq, dtype=np.float64))
    d = Xt.shape[1]
    il = 1.0 / np.exp(np.asarray(hk, dtype=np.float64)[1 : d + 1])
    u = (Xq[:, None, :] - Xt[None, :, :]) * il
    r2 = np.sum(u * u, axis=2)
    if stationary == "rbf":
        fac = -np.exp(-0.5 * r2)
    elif stationary == "matern32":
        fac = -3.0 * np.exp(-np.sqrt(3.0) * np.sqrt(r2))
    else:
        t = np.sqrt(5.0) * np.sqrt(r2)
        fac = -(5.0 / 3.0) * (1.0 + t) * np.exp(-t)
    cf = float(np.exp(hk[0])) if form == "product" else 1.0
    return cf * fac[:, :, None] * (u * il), cf * PHI[stationary] * il * il


def gradient_cov_host(hk, Xt, alpha, K_inv, Xq, stationary, form):
    """``(dmean (m, d), cov (m, d, d))`` of one posterior in fp64 numpy: the closed forms above on the explicit inverse, block by
    block over the query rows.  ``cov`` is symmetrised and its diagonal clipped at 0, as the device call returns it."""
    Xq = np.atleast_2d(np.asarray(Xq, dtype=np.float64))
    alpha, K_inv = np.asarray(alpha, dtype=np.float64), np.asarray(K_inv, dtype=np.float64)
    n, d = np.atleast_2d(Xt).shape
    m = Xq.shape[0]
    dmean, cov = np.empty((m, d)), np.empty((m, d, d))
    step = max(1, HOST_ROWS // max(1, n * d))
    for lo in range(0, m, step):
        G, h0 = cross_gradient(hk, Xt, Xq[lo : lo + step], stationary, form)
        Gt = np.swapaxes(G, 1, 2)  # (s, k, j)
        dmean[lo : lo + step] = Gt @ alpha
        Q = (Gt @ K_inv) @ G  # G^T K^-1 G per point: two matrix products
        S = -0.5 * (Q + np.swapaxes(Q, 1, 2))
        idx = np.arange(d)
        S[:, idx, idx] = np.maximum(h0[None, :] - Q[:, idx, idx], 0.0)
        cov[lo : lo + step] = S
    return dmean, cov


def subspace_sums(dmean, cov):
    """``(C_mean, C_cov)`` over the second-to-last (points) axis of ``dmean`` (..., m, d) and ``cov`` (..., m, d, d)."""
    return np.einsum("...sk,...sl->...kl", dmean, dmean) / dmean.shape[-2], cov.mean(axis=-3)


def host_rows(gp, thetas, X, why):
    """The host path for the median GP (``thetas=None``) or a block of chain rows: ``(dmean (B, m, d), cov (B, m, d, d))``."""
    _tell_once(why)
    st, fm = gp._plan.stationary, gp._plan.form
    check_differentiable(st)
    Xt = gp.X_train_
    if thetas is None:
        hk = gp._canonical(gp._kernel_theta_for_predict())[0]
        out = [gradient_cov_host(hk, Xt, gp.alpha_, gp.K_inv_, X, st, fm)]
    else:
        out = []
        for t in np.atleast_2d(thetas):
            H = gp._canonical(t[None, :])
            res = gp._ctx.posterior(H, want_L=False, want_alpha=True, want_K_inv=True)
            if res["status"][0] != 0:
                raise np.linalg.LinAlgError("%d-th leading minor of the array is not positive definite" % res["status"][0])
            out.append(gradient_cov_host(H[0], Xt, res["alpha"][0], res["K_inv"][0], X, st, fm))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def eigen_summary(C):
    """(eigenvalues descending, eigenvectors as columns each signed so that its largest-magnitude component is positive,
    cumulative eigenvalue share) of a symmetric matrix."""
    w, V = np.linalg.eigh(0.5 * (C + C.T))
    order = np.argsort(w)[::-1]
    w, V = w[order], V[:, order]
    big = np.argmax(np.abs(V), axis=0)
    V = V * np.where(V[big, np.arange(V.shape[1])] < 0.0, -1.0, 1.0)[None, :]
    total = w.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        explained = np.cumsum(w) / total
    return w, V, explained


def assemble(C_mean, C_cov, path):
    """The dict of ``utils.active_subspace`` from (d, d) matrices of the median GP, or (B, d, d) stacks of chain rows: the
    matrices are averaged over the rows and ``"band"`` is the per-row 5 % / 95 % band of each ranked eigenvalue."""
    C_mean, C_cov = np.asarray(C_mean, dtype=np.float64), np.asarray(C_cov, dtype=np.float64)
    out = {"path": path}
    if C_mean.ndim == 3:
        per_row = np.stack([eigen_summary(a + b)[0] for a, b in zip(C_mean, C_cov)])
        out["band"] = tuple(np.percentile(per_row, [5.0, 95.0], axis=0))
        C_mean, C_cov = C_mean.mean(axis=0), C_cov.mean(axis=0)
    C = C_mean + C_cov
    w, V, explained = eigen_summary(C)
    tr = float(np.trace(C))
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.diag(C) / tr
    out.update({"C": C, "C_mean": C_mean, "C_cov": C_cov, "eigenvalues": w, "eigenvectors": V, "explained": explained,
                "diag_share": {k: float(share[k]) for k in range(len(share))}})
    return out
