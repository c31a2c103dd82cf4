"""Extended-precision CPU reference for the fp64 GP kernels -- TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Plain numpy in ``np.longdouble`` (x87 extended: 64-bit mantissa, eps = 2^-63 ~ 1.1e-19, 2048 times finer than fp64).  It
restates, from the definitions in ``gp_oracle.py``'s docstring (canonical vector ``h = [log c, log l_1..l_d, log s2]``,
product form ``c*S(r) + s2*I``, sum form ``c + S(r) + s2*I``), the Gram build, the Cholesky factor, triangular solves, the
LML and its gradient, the posterior factors, predict, the closed-form acquisitions averaged over draws (Phi, phi from mpmath),
PVRS covs, the ``sample_y`` transform for a fixed z, warped inputs, fantasy conditioning on chosen candidates (every prefix
refactorised), and the posterior / predict of a given fp64 kernel matrix (generic kernels).
Only the tests import it; the product never does.  ``gp_oracle.py`` (fp64, scipy/LAPACK) stays the parity oracle; this
module is what both are measured against in ``tests/test_cpu_precision.py`` and ``tests/test_gpu_precision.py``.

Where no 64-bit mantissa is available (``long double`` == double on some platforms) ``require()`` raises
``PrecisionUnavailable``: the tests that need it skip with that reason instead of comparing fp64 with fp64.

Error budget
------------
* n <= LD_MAX_N (1100): everything in long double.  Inputs are fp64 numbers (exact in long double); the reference's own
  error is ~ c * n * kappa(K) * 2^-63, i.e. more than 2000x below the fp64 error of the same computation.
* n > LD_MAX_N (2048, 4096; long-double factorisation there costs minutes): ``lml_refined`` factorises in fp64 (LAPACK),
  solves, and refines alpha ONCE with the residual ``y - K a`` formed in long double from the long-double Gram matrix.
  After one step alpha's relative error is ~ (kappa * eps64)^2 + kappa * 2^-63 -- far below kappa * eps64 for kappa <= 1e7.
  The log-determinant comes from the fp64 factor: Cholesky is backward stable, L L^T = K + E with
  |E| <= (n+1) eps64 |L||L^T|, so |delta logdet| = |tr(K^-1 E)| <~ (n+1) eps64 * n in the worst case and ~ sqrt(n) eps64 *
  n in practice (the rounding errors are not aligned); on the LML's absolute-sum scale (which is >= n/2 log 2 pi) that is
  a relative error of order eps64 * sqrt(n), not kappa-dependent and below the LML floor of the tolerance model.

The ``kappa`` used by the tolerance model is the 2-norm condition number of the fp64 Gram matrix from ``eigvalsh``.
"""
import numpy as np

LD = np.longdouble
LD_MAX_N = 1100
BLOCK = 64
STATIONARY = ("rbf", "matern12", "matern32", "matern52")


class PrecisionUnavailable(RuntimeError):
    """np.longdouble has fewer than 63 mantissa bits on this platform."""


def available():
    return np.finfo(LD).nmant >= 63


_AVAILABLE = available()


def require():
    """Raise PrecisionUnavailable unless long double carries a 64-bit mantissa.  Every entry point that computes in long
    double (``gram``, the factorisation and solves, ``warp_inputs``) calls it, so no caller can compare fp64 with fp64."""
    if not _AVAILABLE:
        raise PrecisionUnavailable("np.longdouble has a %d-bit mantissa here; the extended-precision reference needs 63"
                                   % np.finfo(LD).nmant)


_LOG_2PI = None


def _log2pi():
    global _LOG_2PI
    if _LOG_2PI is None:
        _LOG_2PI = np.log(LD(2) * LD("3.14159265358979323846264338327950288"))
    return _LOG_2PI


def _unpack(h, d):
    h = np.asarray(h, dtype=np.float64)
    assert h.shape == (d + 2,)
    e = np.exp(h.astype(LD))
    return e[0], e[1 : d + 1], e[d + 1]


def _S(r2, stationary):
    """Stationary part from squared scaled distances (long double)."""
    if stationary == "rbf":
        return np.exp(LD(-0.5) * r2)
    r = np.sqrt(r2)
    if stationary == "matern12":
        return np.exp(-r)
    if stationary == "matern32":
        t = np.sqrt(LD(3)) * r
        return (1 + t) * np.exp(-t)
    if stationary == "matern52":
        t = np.sqrt(LD(5)) * r
        return (1 + t + t * t / 3) * np.exp(-t)
    raise ValueError(stationary)


def _ld(X):
    """fp64 (or long-double, e.g. warped) inputs as a 2-D long-double array."""
    X = np.atleast_2d(np.asarray(X))
    return X if X.dtype == LD else X.astype(np.float64).astype(LD)


def _r2(X, Y, ell):
    Xs = _ld(X) / ell
    Ys = _ld(Y) / ell
    out = np.zeros((Xs.shape[0], Ys.shape[0]), dtype=LD)
    for k in range(Xs.shape[1]):  # (per dimension: no (n, m, d) temporary at n = 4096)
        out += (Xs[:, k][:, None] - Ys[:, k][None, :]) ** 2
    return out


def gram(X, h, stationary="matern52", form="product", alpha_diag=None, Y=None, noise=True):
    """k(X, X) [+ s2 I][+ diag(alpha)] or k(X, Y), long double.  ``alpha_diag`` scalar or (n,); ``h[-1] = -inf`` = no noise."""
    require()
    X = _ld(X)
    d = X.shape[1]
    c, ell, s2 = _unpack(h, d)
    if Y is None:
        S = _S(_r2(X, X, ell), stationary)
        np.fill_diagonal(S, LD(1))
        K = c * S if form == "product" else c + S
        idx = np.diag_indices_from(K)
        if noise:
            K[idx] += s2
        if alpha_diag is not None:
            K[idx] += np.broadcast_to(np.asarray(alpha_diag, dtype=np.float64), (X.shape[0],)).astype(LD)
        return K
    S = _S(_r2(X, np.atleast_2d(Y), ell), stationary)
    return c * S if form == "product" else c + S


def prior_var(h, d, form="product", noise=True):
    c, _, s2 = _unpack(h, d)
    base = c if form == "product" else c + 1
    return base + (s2 if noise else 0)


# ---------------------------------------------------------------------------------------------------------------------------
# dense linear algebra in long double (blocked: numpy's long-double matmul is a plain loop, ~0.2 GFLOP/s)
# ---------------------------------------------------------------------------------------------------------------------------
def cholesky(A, block=BLOCK):
    """Lower factor of A (long double, right-looking, blocked).  Raises np.linalg.LinAlgError at a non-positive pivot."""
    require()
    L = np.array(A, dtype=LD, copy=True)
    n = L.shape[0]
    for k in range(0, n, block):
        e = min(k + block, n)
        for j in range(k, e):
            v = L[j, k:j]
            p = L[j, j] - v @ v
            if not p > 0:
                raise np.linalg.LinAlgError("not positive definite at pivot %d" % (j + 1))
            L[j, j] = np.sqrt(p)
            if j + 1 < e:
                L[j + 1 : e, j] = (L[j + 1 : e, j] - L[j + 1 : e, k:j] @ v) / L[j, j]
        if e < n:
            # panel: L21 = A21 L11^-T
            L[e:, k:e] = solve_lower(L[k:e, k:e], L[e:, k:e].T).T
            P = L[e:, k:e]
            for i in range(e, n, block):  # trailing update, lower block columns only
                ie = min(i + block, n)
                L[i:, i:ie] -= P[i - e :] @ P[i - e : ie - e].T
    return np.tril(L)


def solve_lower(L, B, block=BLOCK):
    """L^-1 B for lower-triangular L (long double, blocked forward substitution); B (n,) or (n, m)."""
    require()
    L = np.asarray(L, dtype=LD)
    vec = np.ndim(B) == 1
    X = np.array(B, dtype=LD, copy=True).reshape(L.shape[0], -1)
    n = L.shape[0]
    for k in range(0, n, block):
        e = min(k + block, n)
        if k:
            X[k:e] -= L[k:e, :k] @ X[:k]
        for r in range(k, e):
            if r > k:
                X[r] -= L[r, k:r] @ X[k:r]
            X[r] /= L[r, r]
    return X[:, 0] if vec else X


def solve_upper_t(L, B, block=BLOCK):
    """L^-T B (back substitution on the transpose of lower-triangular L)."""
    require()
    L = np.asarray(L, dtype=LD)
    vec = np.ndim(B) == 1
    X = np.array(B, dtype=LD, copy=True).reshape(L.shape[0], -1)
    n = L.shape[0]
    starts = list(range(0, n, block))
    for k in reversed(starts):
        e = min(k + block, n)
        if e < n:
            X[k:e] -= L[e:, k:e].T @ X[e:]
        for r in range(e - 1, k - 1, -1):
            if r + 1 < e:
                X[r] -= L[r + 1 : e, r] @ X[r + 1 : e]
            X[r] /= L[r, r]
    return X[:, 0] if vec else X


def cho_solve(L, B):
    return solve_upper_t(L, solve_lower(L, B))


def inverse_from_factor(L):
    """K^-1 = L^-T L^-1."""
    Li = solve_lower(L, np.eye(L.shape[0], dtype=LD))
    return Li.T @ Li


def kappa(K):
    """2-norm condition number of the (fp64) symmetric positive definite matrix K, from eigvalsh."""
    w = np.linalg.eigvalsh(np.asarray(K, dtype=np.float64))
    return float(w[-1] / w[0]) if w[0] > 0 else np.inf


# ---------------------------------------------------------------------------------------------------------------------------
# GP quantities
# ---------------------------------------------------------------------------------------------------------------------------
def _lml_terms(L, a, y):
    n = L.shape[0]
    fit = LD(-0.5) * (np.asarray(y, dtype=np.float64).astype(LD) @ a)
    logdet = np.log(np.diagonal(L)).sum()
    const = LD(n) / 2 * _log2pi()
    val = fit - logdet - const
    scale = abs(fit) + np.abs(np.log(np.diagonal(L))).sum() + const
    return val, scale


def lml(X, y, alpha_diag, h, stationary="matern52", form="product"):
    """Returns dict: lml, scale (absolute sum of its terms), L, alpha, K (all long double)."""
    n = np.atleast_2d(X).shape[0]
    if n > LD_MAX_N:
        return lml_refined(X, y, alpha_diag, h, stationary, form)
    K = gram(X, h, stationary, form, alpha_diag)
    L = cholesky(K)
    a = cho_solve(L, np.asarray(y, dtype=np.float64).astype(LD))
    val, scale = _lml_terms(L, a, y)
    return {"lml": val, "scale": scale, "L": L, "alpha": a, "K": K}


def lml_refined(X, y, alpha_diag, h, stationary="matern52", form="product"):
    """Large n: fp64 LAPACK factor and solve, one refinement step with the residual in long double (see the module's error
    budget).  Returns lml, scale, alpha (no long-double factor)."""
    from scipy.linalg import cho_solve as _cs, cholesky as _ch

    K = gram(X, h, stationary, form, alpha_diag)
    L64 = _ch(K.astype(np.float64), lower=True, check_finite=False)
    yl = np.asarray(y, dtype=np.float64).astype(LD)
    a = _cs((L64, True), np.asarray(y, dtype=np.float64), check_finite=False).astype(LD)
    r = yl - K @ a
    a = a + _cs((L64, True), r.astype(np.float64), check_finite=False).astype(LD)
    val, scale = _lml_terms(L64.astype(LD), a, y)
    return {"lml": val, "scale": scale, "L": None, "alpha": a, "K": K}


def kernel_gradient_k(X, h, k, stationary="matern52", form="product"):
    """dK/dh_k (long double, n x n) for the canonical vector."""
    X = _ld(X)
    n, d = X.shape
    c, ell, s2 = _unpack(h, d)
    if k == d + 1:
        return np.diag(np.full(n, s2, dtype=LD))
    if k == 0:
        if form == "product":
            S = _S(_r2(X, X, ell), stationary)
            np.fill_diagonal(S, LD(1))
            return c * S
        return np.full((n, n), c, dtype=LD)
    Xs = X / ell
    r2 = _r2(X, X, ell)
    D2 = (Xs[:, k - 1][:, None] - Xs[:, k - 1][None, :]) ** 2
    if stationary == "rbf":
        dS = D2 * np.exp(LD(-0.5) * r2)
    elif stationary == "matern12":
        r = np.sqrt(r2)
        with np.errstate(divide="ignore", invalid="ignore"):
            dS = np.where(r > 0, D2 * np.exp(-r) / r, LD(0))
    elif stationary == "matern32":
        t = np.sqrt(LD(3) * r2)
        dS = 3 * D2 * np.exp(-t)
    elif stationary == "matern52":
        t = np.sqrt(LD(5) * r2)
        dS = LD(5) / 3 * D2 * (t + 1) * np.exp(-t)
    else:
        raise ValueError(stationary)
    return c * dS if form == "product" else dS


def lml_and_grad(X, y, alpha_diag, h, stationary="matern52", form="product"):
    """LML, its gradient 0.5 tr(W dK/dh_k) with W = a a^T - K^-1, and per component the absolute-sum scale
    0.5 sum_ij |W_ij dK_ij/dh_k| that bounds what a correct fp64 summation can lose on it."""
    r = lml(X, y, alpha_diag, h, stationary, form)
    a = r["alpha"]
    W = np.outer(a, a) - inverse_from_factor(r["L"])
    p = len(h)
    g, s = np.empty(p, dtype=LD), np.empty(p, dtype=LD)
    for k in range(p):
        P = W * kernel_gradient_k(X, h, k, stationary, form)
        g[k] = LD(0.5) * P.sum()
        s[k] = LD(0.5) * np.abs(P).sum()
    r.update(grad=g, grad_scale=s)
    return r


def posterior(X, y, alpha_diag, h, stationary="matern52", form="product"):
    r = lml(X, y, alpha_diag, h, stationary, form)
    r["K_inv"] = inverse_from_factor(r["L"])
    return r


def predict(X, y, alpha_diag, h, Xq, stationary="matern52", form="product", noise_zero=False, return_cov=False, post=None):
    """Mean, variance (and covariance) of the posterior built with h (noise included), evaluated with the kernel of h or, with
    ``noise_zero``, of h without its white level (``noise_set_to_zero``: the factors stay).  ``post``: a ``posterior`` result
    to reuse."""
    X = _ld(X)
    d = X.shape[1]
    if post is None:
        post = lml(X, y, alpha_diag, h, stationary, form)
    Ks = gram(Xq, h, stationary, form, Y=X)  # (m, n); the white kernel adds nothing off the training set
    mean = Ks @ post["alpha"]
    V = solve_lower(post["L"], Ks.T)
    var = prior_var(h, d, form, noise=not noise_zero) - np.einsum("ij,ij->j", V, V)
    out = {"mean": mean, "var": var}
    if return_cov:
        Kss = gram(Xq, h, stationary, form, noise=not noise_zero)
        out["cov"] = Kss - V.T @ V
    return out


def pvrs_covs(X_train, alpha_vec, h, X_cand, thompson_points, stationary="matern52", form="product"):
    """Per candidate: factorise the augmented matrix (alpha only when it is a vector, 0 on the new point), trace of
    K_t K_aug^-1 K_t^T -- the quantity of ``gp_oracle.pvrs_covs``."""
    out = np.empty(len(X_cand), dtype=LD)
    for i in range(len(X_cand)):
        Xa = np.concatenate([_ld(X_train), _ld(X_cand)[i : i + 1]])
        ad = None if alpha_vec is None else np.concatenate([alpha_vec, [0.0]])
        L = cholesky(gram(Xa, h, stationary, form, ad))
        Kt = gram(thompson_points, h, stationary, form, Y=Xa)
        V = solve_lower(L, Kt.T)
        out[i] = (V * V).sum()
    return out


def sample_y_factor(X, y, alpha_diag, h, Xq, jitter, stationary="matern52", form="product", noise_zero=True):
    """(mean, chol(cov + jitter I), predict result) of the ``sample_y`` transform: what draws of one posterior at one set of
    query points share."""
    p = predict(X, y, alpha_diag, h, Xq, stationary, form, noise_zero=noise_zero, return_cov=True)
    C = p["cov"]
    C[np.diag_indices_from(C)] += LD(jitter)
    return p["mean"], cholesky(C), p


def sample_y(X, y, alpha_diag, h, Xq, z, jitter, stationary="matern52", form="product", noise_zero=True, factor=None):
    """mean + chol(cov + jitter I) z for fixed z (rows of z are draws): (n_draws, m).  ``factor``: a ``sample_y_factor``
    result of the same arguments to reuse."""
    mean, Lc, p = factor if factor is not None else sample_y_factor(X, y, alpha_diag, h, Xq, jitter, stationary, form,
                                                                     noise_zero)
    return mean[None, :] + np.asarray(z, dtype=np.float64).astype(LD) @ Lc.T, p


def posterior_gram(K, alpha_diag, y):
    """Posterior factors from a GIVEN fp64 kernel matrix (generic kernels: the host evaluates K, the device factorises
    K + diag(alpha)): the entries of K are taken as exact and everything behind them is long double."""
    require()
    K = np.asarray(K, dtype=np.float64)
    Kl = K.astype(LD)
    Kl[np.diag_indices_from(Kl)] += np.broadcast_to(np.asarray(alpha_diag, dtype=np.float64), (len(K),)).astype(LD)
    L = cholesky(Kl)
    a = cho_solve(L, np.asarray(y, dtype=np.float64).astype(LD))
    return {"K": Kl, "L": L, "alpha": a, "K_inv": inverse_from_factor(L)}


def predict_gram(post, Ks, kss, Kss=None):
    """Mean, variance (and covariance) from given fp64 ``Ks`` (m, n), ``kss`` (m,), ``Kss`` (m, m) and a ``posterior_gram``
    result."""
    Ks = np.asarray(Ks, dtype=np.float64).astype(LD)
    V = solve_lower(post["L"], Ks.T)
    out = {"mean": Ks @ post["alpha"], "var": np.asarray(kss, dtype=np.float64).astype(LD) - np.einsum("ij,ij->j", V, V)}
    if Kss is not None:
        out["cov"] = np.asarray(Kss, dtype=np.float64).astype(LD) - V.T @ V
    return out


ACQ_DPS = 40  # (the precision ``warp_inputs`` evaluates the Beta CDF at)


def _mp_to_ld(v):
    import mpmath

    return LD(mpmath.nstr(v, 30, min_fixed=-1, max_fixed=-1))


def normal_cdf_pdf(x):
    """Phi(x) and phi(x) of a long-double array from mpmath at ACQ_DPS digits, rounded to long double."""
    require()
    import mpmath

    x = np.asarray(x, dtype=LD)
    Phi, phi = np.empty(x.shape, dtype=LD), np.empty(x.shape, dtype=LD)
    with mpmath.workdps(ACQ_DPS):
        for idx in np.ndindex(x.shape):
            v = mpmath.mpf(np.format_float_scientific(x[idx], precision=24, unique=False))
            Phi[idx], phi[idx] = _mp_to_ld(mpmath.ncdf(v)), _mp_to_ld(mpmath.npdf(v))
    return Phi, phi


def acquisitions(mean, var, y_mean, y_std, kinds, params, n_samples):
    """Closed-form acquisitions averaged over the draws, from the long-double moments ``mean``, ``var`` (B, m) of ``predict``:
    per draw ``mu = y_std mean + y_mean``, ``sd = sqrt(max(var, 0)) y_std``; "EI" ``(x Phi(x) + phi(x)) sd`` with
    ``x = (y_opt - mu) / sd`` (``y_opt`` the parameter, or the draw's lowest ``mu`` when it is NaN; 0 where sd is not
    positive), "LCB" ``param sd - mu``, "MEAN" ``-mu``, "STD" ``sd``; added in draw order, each over ``n_samples``.
    Returns values (n_acq, m) and per draw ``mu``, ``sd`` (B, m), ``y_opt`` (n_acq, B; NaN for the other kinds), ``x``,
    ``Phi``, ``phi`` (n_acq, B, m; zeros for the other kinds) for the tolerance model."""
    require()
    mean, var = np.atleast_2d(np.asarray(mean, dtype=LD)), np.atleast_2d(np.asarray(var, dtype=LD))
    B, m = mean.shape
    ys, ym, ns = LD(float(y_std)), LD(float(y_mean)), LD(int(n_samples))
    mu, sd = ys * mean + ym, np.sqrt(np.maximum(var, LD(0))) * ys
    out = np.zeros((len(kinds), m), dtype=LD)
    info = {"mu": mu, "sd": sd, "y_opt": np.full((len(kinds), B), np.nan, dtype=LD),
            "x": np.zeros((len(kinds), B, m), dtype=LD), "Phi": np.zeros((len(kinds), B, m), dtype=LD),
            "phi": np.zeros((len(kinds), B, m), dtype=LD)}
    for k, (kind, par) in enumerate(zip(kinds, params)):
        for b in range(B):
            if kind == "MEAN":
                v = -mu[b]
            elif kind == "STD":
                v = sd[b]
            elif kind == "LCB":
                v = LD(float(par)) * sd[b] - mu[b]
            elif kind == "EI":
                yo = mu[b].min() if np.isnan(par) else LD(float(par))
                pos = sd[b] > 0
                x = np.zeros(m, dtype=LD)
                x[pos] = (yo - mu[b][pos]) / sd[b][pos]
                Phi, phi = normal_cdf_pdf(x)
                v = np.where(pos, (x * Phi + phi) * sd[b], LD(0))
                info["y_opt"][k, b], info["x"][k, b], info["Phi"][k, b], info["phi"][k, b] = yo, x, Phi, phi
            else:
                raise ValueError(kind)
            out[k] += v / ns
    return out, info


def fantasy(X, y, alpha_diag, h, Xc, picks, lies, base_alpha, stationary="matern52", form="product"):
    """Latent mean and variance at every candidate ``Xc`` after conditioning on ``Xc[picks[:j+1]]`` with fantasy observations,
    for each prefix j of ``picks`` -- WITHOUT the rank-1 identities of the device path: every prefix refactorises the augmented
    set ``vstack([X, Xc[picks[:j+1]]])`` (``lml`` / ``predict(noise_zero=True)``), alpha vector ``concat(alpha, base_alpha)``,
    targets ``concat(y, lies)``.  ``gram`` puts s2 on every diagonal entry, so a fantasy observation's variance is
    ``base_alpha + exp(h[-1])``.  ``lies`` (q,) normalised values, or None for the kriging believer: the lie of step j is the
    conditioned mean at ``picks[j]`` before that step (kept in long double), so the means do not move.

    Returns mean, var (q, m); mean0, var0 (m,) before any step; per prefix ``mean_scale`` = max_i sum_j |K*_ij a_j| on the
    augmented set and ``kappa`` of the augmented Gram matrix; ``prior_var`` (latent); ``lies`` as used."""
    require()
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    Xc = np.atleast_2d(np.asarray(Xc, dtype=np.float64))
    n, d = X.shape
    ad = np.broadcast_to(np.asarray(alpha_diag, dtype=np.float64), (n,))
    yl = np.asarray(y, dtype=np.float64).astype(LD)
    picks = [int(p) for p in picks]
    q, m = len(picks), Xc.shape[0]
    p0 = predict(X, y, ad, h, Xc, stationary, form, noise_zero=True)
    out = {"mean": np.empty((q, m), dtype=LD), "var": np.empty((q, m), dtype=LD), "mean0": p0["mean"], "var0": p0["var"],
           "mean_scale": np.empty(q), "kappa": np.empty(q), "prior_var": prior_var(h, d, form, noise=False),
           "lies": np.empty(q, dtype=LD)}
    before = p0["mean"]
    for j in range(q):
        out["lies"][j] = before[picks[j]] if lies is None else LD(float(lies[j]))
        Xa = np.vstack([X, Xc[picks[: j + 1]]])
        aa = np.concatenate([ad, np.full(j + 1, float(base_alpha))])
        ya = np.concatenate([yl, out["lies"][: j + 1]])
        post = lml(Xa, ya.astype(np.float64), aa, h, stationary, form)
        post["alpha"] = cho_solve(post["L"], ya)  # (the believer's lies are long-double numbers: not rounded to fp64)
        pr = predict(Xa, None, aa, h, Xc, stationary, form, noise_zero=True, post=post)
        out["mean"][j], out["var"][j] = pr["mean"], pr["var"]
        Ks = gram(Xc, h, stationary, form, Y=Xa)
        out["mean_scale"][j] = float(np.abs(Ks * post["alpha"][None, :]).sum(axis=1).max())
        out["kappa"][j] = kappa(post["K"])
        before = pr["mean"]
    return out


def warp_inputs(X, w, dps=40):
    """Column k through the regularised incomplete Beta function I_x(exp(w[k]), exp(w[d+k])) from mpmath at ``dps`` digits,
    rounded to long double."""
    require()
    import mpmath

    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    d = X.shape[1]
    w = np.asarray(w, dtype=np.float64)
    out = np.empty(X.shape, dtype=LD)
    with mpmath.workdps(dps):
        for k in range(d):
            a, b = mpmath.exp(mpmath.mpf(float(w[k]))), mpmath.exp(mpmath.mpf(float(w[d + k])))
            for i in range(X.shape[0]):
                v = mpmath.betainc(a, b, 0, mpmath.mpf(float(X[i, k])), regularized=True)
                out[i, k] = LD(mpmath.nstr(v, 30, min_fixed=-1, max_fixed=-1))
    return out
