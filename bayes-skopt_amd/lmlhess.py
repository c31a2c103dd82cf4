"""Hessian of the log marginal likelihood and the Laplace approximation of the hyper-posterior.

With ``alpha = K^-1 y``, ``W = alpha alpha^T - K^-1``, ``D_k = dK / dh_k`` and ``D_kl = d2K / dh_k dh_l`` over the canonical vector
``h = [log c, log l_1 .. l_d, log s2]``:

    H_kl = 1/2 tr(W D_kl) - (D_k alpha)^T K^-1 (D_l alpha) + 1/2 tr(K^-1 D_k K^-1 D_l)

Length scales, ``u_k = (x_ik - x_jk)^2 / l_k^2``, ``fr = -2 dS / dr^2``, ``fr2 = -2 dfr / dr^2``, cf = c (product form) or 1 (sum):
``D_k = cf fr u_k``, ``D_kl = cf (fr2 u_k u_l - 2 delta_kl fr u_k)``; coincident points contribute exactly 0.  Constant: ``D_0 = D_00``
is ``c S`` (product) or ``c 1 1^T`` (sum), ``D_0k = D_k`` (product) or 0 (sum); noise: ``D_n = D_nn = s2 I``; every other mixed
second derivative is 0.

This module holds what is not the device call (``bgp_lml_hess_batch``, ``_lib.Context.lml_hess``): the same formula in numpy on a
downloaded ``K^-1`` and ``alpha`` (``lml_hess_host``: more than 16 dimensions, or forced), the form for generic kernel trees
(``lml_hess_generic``: the kernel object's gradient and central differences of it), and the assembly of
``BayesGPR.hyper_laplace``."""
import sys

import numpy as np

LMLHESS_DMAX = 16  # dimensions of the device call (bgp_lmlhess.hip)

_told = []


def _tell_once(why):
    """One line on stderr, once per process: the LML Hessian computed by numpy on the downloaded inverse."""
    if not _told:
        _told.append(True)
        print("[bayes_skopt_amd] LML Hessian: numpy on the downloaded inverse (%s)" % why, file=sys.stderr, flush=True)


def stationary_facs(r2, stationary):
    """(S, fr, fr2) of the squared scaled distances ``r2``; fr and fr2 are 0 where r = 0 makes them singular."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if stationary == "rbf":
            S = np.exp(-0.5 * r2)
            return S, S, S
        r = np.sqrt(r2)
        if stationary == "matern12":
            S = np.exp(-r)
            return S, np.where(r > 0, S / r, 0.0), np.where(r > 0, S * (1.0 + r) / (r * r * r), 0.0)
        if stationary == "matern32":
            t = np.sqrt(3.0) * r
            e = np.exp(-t)
            return (1.0 + t) * e, 3.0 * e, np.where(t > 0, 9.0 * e / t, 0.0)
        if stationary == "matern52":
            t = np.sqrt(5.0) * r
            e = np.exp(-t)
            return (1.0 + t + t * t / 3.0) * e, (5.0 / 3.0) * (t + 1.0) * e, (25.0 / 3.0) * e
    raise ValueError(stationary)


def lml_hess_host(X, h, K_inv, alpha, stationary, form):
    """The (p, p) Hessian with respect to the canonical vector ``h`` from the training inputs ``X`` (n, d; as the device sees them),
    the inverse ``K_inv`` (n, n) and ``alpha`` (n,) of the posterior at ``h``."""
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    n, d = X.shape
    p = d + 2
    h = np.asarray(h, dtype=np.float64)
    cst, s2 = np.exp(h[0]), np.exp(h[d + 1])
    Xs = X / np.exp(h[1 : d + 1])
    U = (Xs[:, None, :] - Xs[None, :, :]) ** 2  # (n, n, d)
    S, fr, fr2 = stationary_facs(U.sum(axis=2), stationary)
    off = ~np.eye(n, dtype=bool)
    fr, fr2 = fr * off, fr2 * off
    np.fill_diagonal(S, 1.0)
    product = form == "product"
    cf = cst if product else 1.0
    D = np.empty((p, n, n))
    D[0] = cst * S if product else cst
    D[1 : d + 1] = np.moveaxis(cf * fr[:, :, None] * U, 2, 0)
    D[d + 1] = s2 * np.eye(n)
    W = np.outer(alpha, alpha) - K_inv
    g = 0.5 * np.einsum("ij,kij->k", W, D)
    first = np.zeros((p, p))
    Ud = np.moveaxis(U, 2, 0)
    first[1 : d + 1, 1 : d + 1] = 0.5 * np.einsum("ij,kij,lij->kl", W * (cf * fr2), Ud, Ud) - 2.0 * np.diag(g[1 : d + 1])
    first[0, 0] = g[0]
    if product:
        first[0, 1 : d + 1] = first[1 : d + 1, 0] = g[1 : d + 1]
    first[d + 1, d + 1] = g[d + 1]
    P = D @ K_inv
    T = np.einsum("kij,lji->kl", P, P)
    v = D @ alpha
    q = v @ K_inv @ v.T
    Hm = first - q + 0.5 * T
    return 0.5 * (Hm + Hm.T)


def lml_hess_generic(kernel, theta, X, K_inv, alpha, rel_step=1e-5):
    """The Hessian with respect to ``theta`` of a kernel object: ``D_k`` from ``kernel(X, eval_gradient=True)``, ``D_kl`` from
    central differences of that gradient (step ``rel_step (1 + |theta_l|)``)."""
    theta = np.asarray(theta, dtype=np.float64)
    p = len(theta)
    with np.errstate(divide="ignore"):
        D = np.moveaxis(kernel.clone_with_theta(theta)(X, eval_gradient=True)[1], 2, 0)
        W = np.outer(alpha, alpha) - K_inv
        first = np.empty((p, p))
        for l in range(p):
            e = np.zeros(p)
            e[l] = rel_step * (1.0 + abs(theta[l]))
            Dp = kernel.clone_with_theta(theta + e)(X, eval_gradient=True)[1]
            Dm = kernel.clone_with_theta(theta - e)(X, eval_gradient=True)[1]
            first[:, l] = 0.5 * np.einsum("ij,ijk->k", W, (Dp - Dm) / (2.0 * e[l]))
    P = D @ K_inv
    v = D @ alpha
    Hm = first - v @ K_inv @ v.T + 0.5 * np.einsum("kij,lji->kl", P, P)
    return 0.5 * (Hm + Hm.T)


def prior_derivatives(priors, theta, rel_step=1e-4):
    """(log prior, gradient (p,), Hessian (p, p)) at ``theta`` by central differences, step ``rel_step (1 + |theta_k|)``: a list
    holds one univariate callable per hyper-parameter (a diagonal Hessian), a single callable takes the whole vector."""
    theta = np.asarray(theta, dtype=np.float64)
    p = len(theta)
    step = rel_step * (1.0 + np.abs(theta))
    g, Hp = np.zeros(p), np.zeros((p, p))
    if callable(priors):
        f = lambda t: float(priors(t))  # noqa: E731
        f0 = f(theta)
        E = np.diag(step)
        for k in range(p):
            fp, fm = f(theta + E[k]), f(theta - E[k])
            g[k] = (fp - fm) / (2.0 * step[k])
            Hp[k, k] = (fp - 2.0 * f0 + fm) / step[k] ** 2
            for l in range(k):
                Hp[k, l] = Hp[l, k] = (f(theta + E[k] + E[l]) - f(theta + E[k] - E[l]) - f(theta - E[k] + E[l])
                                       + f(theta - E[k] - E[l])) / (4.0 * step[k] * step[l])
        return f0, g, Hp
    priors = list(priors)
    if len(priors) != p:
        raise ValueError(f"{len(priors)} priors for {p} hyper-parameters")
    f0 = 0.0
    for k, prior in enumerate(priors):
        fm, fc, fp = (float(prior(theta[k] + s)) for s in (-step[k], 0.0, step[k]))
        f0 += fc
        g[k] = (fp - fm) / (2.0 * step[k])
        Hp[k, k] = (fp - 2.0 * fc + fm) / step[k] ** 2
    return f0, g, Hp


def laplace(mode, log_post, hess, bounds=None, n_samples=0, rng=None):
    """The Gaussian approximation at ``mode`` from the Hessian ``hess`` (p, p) of the log posterior there: ``cov = (-hess)^-1``,
    ``sd``, ``corr``, ``log_evidence = log_post + p / 2 log 2 pi - 1/2 log det(-hess)`` and ``negative_definite`` (False: NaN in
    ``cov``, ``sd``, ``corr`` and ``log_evidence``, no draws).  ``n_samples`` > 0: ``samples`` (n_samples, p) drawn with ``rng`` and
    clipped to ``bounds`` (p, 2)."""
    mode = np.asarray(mode, dtype=np.float64)
    p = len(mode)
    A = -0.5 * (hess + hess.T)
    out = {"mode": mode.copy(), "hessian": -A, "cov": np.full((p, p), np.nan), "sd": np.full(p, np.nan),
           "corr": np.full((p, p), np.nan), "log_evidence": float("nan"), "negative_definite": False}
    try:
        if not np.all(np.isfinite(A)):
            raise np.linalg.LinAlgError
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        if n_samples > 0:
            out["samples"] = np.empty((0, p))
        return out
    Li = np.linalg.solve(L, np.eye(p))
    cov = Li.T @ Li
    sd = np.sqrt(np.diag(cov))
    out.update(cov=cov, sd=sd, corr=cov / np.outer(sd, sd), negative_definite=True,
               log_evidence=float(log_post + 0.5 * p * np.log(2.0 * np.pi) - np.log(np.diag(L)).sum()))
    if n_samples > 0:
        draws = mode + rng.standard_normal((int(n_samples), p)) @ Li  # (cov = Li^T Li)
        if bounds is not None:
            draws = np.clip(draws, bounds[:, 0], bounds[:, 1])
        out["samples"] = draws
    return out
