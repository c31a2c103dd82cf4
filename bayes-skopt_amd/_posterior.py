"""The two posterior backends of ``BayesGPR``.  ``CanonicalPosterior`` (``kernels.KernelPlan``): the device builds every
matrix from the canonical vector ``H``.  ``GramPosterior`` (``kernels.GramPlan``): the host evaluates the kernel object, as
the reference does for every kernel (``sklearn/_gpr.py:582``), and the device factorises, solves, inverts and forms the
predictive products (``ctx.*_gram``).  Every method takes the estimator and reads ``gp._ctx`` at the call: a backend holds no
context.  What only the canonical form has -- the resident sampler, the device acquisitions, the fantasy fast path, the
device ``mvn`` draw, the sharded asynchronous gather -- is behind ``canonical``.  Predictions: normalised-target units."""
import sys

import numpy as np
from sklearn.base import clone

from . import gradcov, hesscov, influence, lmlhess
from .kernels import WhiteKernel, compile_tree, gradient_x, param_for_white_kernel_in_sum
from .profile import profile_by_predict

_PD_MESSAGE = (
    "The kernel, %s, is not returning a positive definite matrix. Try gradually increasing the "
    "'alpha' parameter of your GaussianProcessRegressor estimator."
)


def raise_if_not_pd(status, kernel=None):
    """LinAlgError for the first failed factorisation of a batch of ``status`` words (scikit-learn's message, naming
    ``kernel``; without it only the leading-minor line, the message PVRS raises)."""
    status = np.atleast_1d(status)
    if np.any(status != 0):
        minor = "%d-th leading minor of the array is not positive definite" % status[np.flatnonzero(status)[0]]
        raise np.linalg.LinAlgError(*((minor,) if kernel is None else (_PD_MESSAGE % kernel, minor)))


def noise_off(H):
    """A copy of canonical vectors with the white level at -inf: the predictive kernel of ``noise_set_to_zero``."""
    Hk = H.copy()
    Hk[:, -1] = -np.inf
    return Hk


_pd_told = []


def _pd_tell_once(why):
    """One line on stderr, once per process: a partial dependence computed through ``predict`` on synthesised rows."""
    if not _pd_told:
        _pd_told.append(True)
        print("[bayes_skopt_amd] partial_dependence: through predict on synthesised rows (%s)" % why, file=sys.stderr, flush=True)


PD_ROWS = 8192  # synthesised rows per predict of the fallbacks


def means_by_predict(gp, thetas, X):
    """The (B, m) latent means at ``X`` of both ``*_by_predict`` fallbacks, normalised-target units.  ``thetas=None``: the resident
    posterior with ``kernel_`` as it is (B = 1); otherwise one item per chain row -- under ``warp_inputs`` one row at a time with the
    row's own warp (``BayesGPR._warped_rows_moments``), because every draw there has its own training inputs."""
    if thetas is None:
        return gp._post.predict(gp, X, False)[0]
    if gp.warp_inputs:
        return gp._warped_rows_moments(np.atleast_2d(thetas), X, True)[0]
    return gp._post.hyper_predict(gp, np.atleast_2d(thetas), X, True)[0]


def partial_dependence_by_predict(gp, thetas, Xs, grids, panels, why):
    """The fallback of ``partial_dependence``: per panel, the sample rows with the panel's columns overwritten cell by cell, at most
    ``PD_ROWS`` rows per ``predict`` (``means_by_predict``), the mean, the average over the samples."""
    _pd_tell_once(why)
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    S = Xs.shape[0]
    out = []
    for k1, k2 in panels:
        axes = [(k1, np.asarray(grids[k1], dtype=np.float64))] + ([(k2, np.asarray(grids[k2], dtype=np.float64))] if k2 >= 0 else [])
        shape = tuple(len(g) for _k, g in axes)
        ncell = int(np.prod(shape))
        vals = None
        step = max(1, PD_ROWS // S)
        for c0 in range(0, ncell, step):
            cells = range(c0, min(ncell, c0 + step))
            X = np.repeat(Xs[None, :, :], len(cells), axis=0)
            for i, c in enumerate(cells):
                for (k, g), gi in zip(axes, np.unravel_index(c, shape)):
                    X[i, :, k] = g[gi]
            m = means_by_predict(gp, thetas, X.reshape(-1, Xs.shape[1]))
            if vals is None:
                vals = np.empty((m.shape[0], ncell))
            vals[:, c0:c0 + len(cells)] = m.reshape(m.shape[0], len(cells), S).mean(axis=2)
        out.append(vals.reshape((vals.shape[0],) + shape))
    return out


PDVAR_SMAX = 16384  # sample rows of the device call with a variance: its prior term is a pair sum (bgp_pdvar.hip)


def latent_cov_by_predict(gp, thetas, X):
    """The (B, m, m) latent covariance at ``X`` -- ``predict(return_cov=True)`` with the noise set to zero --, normalised-target
    units; the rows of ``thetas`` as in ``means_by_predict``."""
    if thetas is None:
        with gp.noise_set_to_zero():
            return gp._post.predict(gp, X, True)[2]
    thetas = np.atleast_2d(thetas)
    if gp.warp_inputs:
        with gp._row_warps() as install:
            return np.concatenate([gp._post.rows_predict(gp, install(row), X, True, return_cov=True)[2] for row in thetas])
    return gp._post.rows_predict(gp, thetas, X, True, return_cov=True)[2]


def partial_dependence_var_by_predict(gp, thetas, Xs, grids, panels, want_cov, why):
    """The fallback of ``partial_dependence`` with ``return_std`` / ``return_cov``: the means as ``partial_dependence_by_predict``
    gives them; per cell the latent covariance of its S synthesised rows, ``1^T cov 1 / S^2``; for the cells g > g' of a curve
    (``want_cov``) the cross block of the covariance of both cells' rows.  Returns (means, variances, covariances | None)."""
    means = partial_dependence_by_predict(gp, thetas, Xs, grids, panels, why)
    Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
    S = Xs.shape[0]

    def rows(axes, shape, c):
        X = Xs.copy()
        for (k, g), gi in zip(axes, np.unravel_index(c, shape)):
            X[:, k] = g[gi]
        return X

    var, cov = [], ([] if want_cov else None)
    for k1, k2 in panels:
        axes = [(k1, np.asarray(grids[k1], dtype=np.float64))] + ([(k2, np.asarray(grids[k2], dtype=np.float64))] if k2 >= 0 else [])
        shape = tuple(len(g) for _k, g in axes)
        ncell = int(np.prod(shape))
        v = np.stack([latent_cov_by_predict(gp, thetas, rows(axes, shape, c)).sum(axis=(1, 2)) for c in range(ncell)], axis=1) / S**2
        v = np.maximum(v, 0.0)
        var.append(v.reshape((v.shape[0],) + shape))
        if want_cov and k2 < 0:
            Cm = np.zeros((v.shape[0], ncell, ncell))
            for g in range(ncell):
                Cm[:, g, g] = v[:, g]
                for h in range(g):
                    both = latent_cov_by_predict(gp, thetas, np.concatenate([rows(axes, shape, g), rows(axes, shape, h)]))
                    Cm[:, g, h] = Cm[:, h, g] = both[:, :S, S:].sum(axis=(1, 2)) / S**2
            cov.append(Cm)
    return means, var, cov


_sens_told = []
SENS_DMAX = 32  # dimensions of the device call: one bit of a 32-bit mask each (bgp_sobol.hip)


def _sens_tell_once(why):
    """One line on stderr, once per process: sensitivity indices computed through ``predict`` on synthesised rows."""
    if not _sens_told:
        _sens_told.append(True)
        print("[bayes_skopt_amd] sensitivity: through predict on synthesised rows (%s)" % why, file=sys.stderr, flush=True)


def sobol_masks(terms, d):
    """The terms of a sensitivity analysis -- each a dimension or a tuple of dimensions of ``d``, the empty tuple included -- as a
    list of Python ints with bit k set for dimension k.  ValueError for an empty list and for a dimension outside [0, d)."""
    masks = []
    for term in terms:
        m = 0
        for k in np.atleast_1d(np.asarray(term, dtype=np.int64)).reshape(-1):
            if not 0 <= int(k) < d:
                raise ValueError(f"term {term!r} names dimension {int(k)} outside [0, {d})")
            m |= 1 << int(k)
        masks.append(m)
    if not masks:
        raise ValueError("sensitivity needs at least one term")
    return masks


def sobol_rows(A, Bm, mask):
    """The synthetic rows of one term: ``A`` with the columns whose bits are set in ``mask`` taken from ``Bm``."""
    pick = np.array([(mask >> k) & 1 for k in range(A.shape[1])], dtype=bool)
    return np.where(pick[None, :], Bm, A)


def sobol_estimator(fA, fB, fT):
    """The pick-freeze estimator on means ``fA``, ``fB`` (..., N) and ``fT`` (..., T, N): ``(f0 (...), V (...), closed (..., T),
    total (..., T))`` -- the identities of DESIGN.md section 21 (Saltelli et al. 2010 for the closed effect, Jansen 1999 for the
    total one), not yet divided by V."""
    fA, fB, fT = np.asarray(fA), np.asarray(fB), np.asarray(fT)
    N = fA.shape[-1]
    f0 = (fA + fB).sum(axis=-1) / (2.0 * N)
    ca, cb = fA - f0[..., None], fB - f0[..., None]
    V = (ca * ca + cb * cb).sum(axis=-1) / (2.0 * N)
    dt = fT - fA[..., None, :]
    closed = (cb[..., None, :] * dt).sum(axis=-1) / N
    total = (dt * dt).sum(axis=-1) / (2.0 * N)
    return f0, V, closed, total


def sensitivity_by_predict(gp, thetas, A, Bm, masks, why):
    """The fallback of ``sensitivity``: the means of A, Bm and every term's synthetic rows through ``predict``, at most ``PD_ROWS``
    rows per call (``means_by_predict``), then ``sobol_estimator`` in numpy.  Returns (f0 (B,), V (B,), closed (B, T), total (B, T))
    in normalised-target units."""
    _sens_tell_once(why)
    A, Bm = np.atleast_2d(np.asarray(A, dtype=np.float64)), np.atleast_2d(np.asarray(Bm, dtype=np.float64))
    N = A.shape[0]
    X = np.concatenate([A, Bm] + [sobol_rows(A, Bm, m) for m in masks])
    F = np.concatenate([means_by_predict(gp, thetas, X[r0:r0 + PD_ROWS]) for r0 in range(0, len(X), PD_ROWS)], axis=1)
    F = F.reshape(F.shape[0], len(masks) + 2, N)
    return sobol_estimator(F[:, 0], F[:, 1], F[:, 2:])


_shap_told = []
SHAP_DMAX = 16             # dimensions of the device call: all 2^d coalitions are enumerated (bgp_shapley.hip)
SHAP_PARTMAX = 1 << 26     # doubles of chunk partials per device call, B P 2^d ceil(n N / 1024) (bgp_shapley.hip)
SHAP_EXACT_ROWS = 1 << 22  # synthesised rows per point up to which the host route enumerates the coalitions


def _shap_tell_once(why):
    """One line on stderr, once per process: Shapley values computed through ``predict`` on synthesised rows."""
    if not _shap_told:
        _shap_told.append(True)
        print("[bayes_skopt_amd] shapley: through predict on synthesised rows (%s)" % why, file=sys.stderr, flush=True)


def shapley_from_values(v, d, interactions=False):
    """The Shapley values and interaction indices of a set function: ``v`` (..., 2^d) holds the value of coalition S at index S
    (bit k set: dimension k is in).  Returns ``(phi (..., d), inter (..., d, d) | None)`` -- the identities of DESIGN.md section 29,
    every difference weighted by |S|! (d - |S| - 1)! / d!, or by |S|! (d - |S| - 2)! / (d - 1)! for a pair; ``inter`` is symmetric
    with a zero diagonal."""
    from math import factorial as fac

    v = np.asarray(v)
    S = np.arange(1 << d)
    size = np.zeros(1 << d, dtype=np.int64)
    for k in range(d):
        size += (S >> k) & 1
    w1 = np.array([fac(s) * fac(d - s - 1) for s in range(d)], dtype=v.dtype) / v.dtype.type(fac(d))  # (exact integers: one rounding)
    w2 = np.array([fac(s) * fac(d - s - 2) for s in range(d - 1)] + [0], dtype=v.dtype) / v.dtype.type(fac(max(d - 1, 0)))
    phi = np.zeros(v.shape[:-1] + (d,), dtype=v.dtype)
    inter = np.zeros(v.shape[:-1] + (d, d), dtype=v.dtype) if interactions else None
    for k in range(d):
        out = S[((S >> k) & 1) == 0]
        phi[..., k] = ((v[..., out | (1 << k)] - v[..., out]) * w1[size[out]]).sum(axis=-1)
        for l in range(k + 1, d) if interactions else ():
            o2 = out[((out >> l) & 1) == 0]
            kb, lb = 1 << k, 1 << l
            inter[..., k, l] = (((v[..., o2 | kb | lb] - v[..., o2 | kb]) - (v[..., o2 | lb] - v[..., o2])) * w2[size[o2]]).sum(axis=-1)
            inter[..., l, k] = inter[..., k, l]
    return phi, inter


def coalition_picks(d):
    """Every coalition of ``d`` dimensions as a boolean (2^d, d) array: row S picks dimension k when bit k of S is set."""
    return ((np.arange(1 << d)[:, None] >> np.arange(d)[None, :]) & 1).astype(bool)


def coalition_rows(x, Z, pick):
    """The synthesised rows of the coalitions ``pick`` (m, d), coalition-major (m N, d): ``Z`` with the picked columns from ``x``."""
    return np.where(pick[:, None, :], x[None, None, :], Z[None, :, :]).reshape(-1, Z.shape[1])


def coalition_means(gp, thetas, x, Z, pick):
    """v (B, m): for every row of the boolean ``pick`` (m, d) the mean over the background rows ``Z`` (N, d) of the latent mean at
    ``Z`` with the picked columns taken from the point ``x`` -- through ``predict``, at most ``PD_ROWS`` rows per call."""
    N, d = Z.shape
    step, out = max(1, PD_ROWS // N), []
    for m0 in range(0, len(pick), step):
        rows = coalition_rows(x, Z, pick[m0:m0 + step])
        F = np.concatenate([means_by_predict(gp, thetas, rows[r0:r0 + PD_ROWS]) for r0 in range(0, len(rows), PD_ROWS)], axis=1)
        out.append(F.reshape(F.shape[0], -1, N).mean(axis=2))
    return np.concatenate(out, axis=1)


def shapley_by_predict(gp, thetas, Xp, Z, why, interactions=False, n_permutations=None, rng=None):
    """The fallback of ``shapley``: coalition rows synthesised on the host, their means through ``predict`` (``coalition_means``),
    the weights in numpy.  Up to ``SHAP_EXACT_ROWS`` rows per point (2^d N) every coalition is enumerated
    (``shapley_from_values``).  Beyond that the values are a permutation-sampling estimate: ``n_permutations`` orders of the
    dimensions drawn from the generator ``rng`` -- both must be given --, the columns switched from the background to the point one
    after the other and every step credited to its dimension; no interaction index then.  Returns ``(phi (B, P, d), base (B,),
    value (B, P), inter (B, P, d, d) | None, se (B, P, d) | None)`` in normalised-target units; ``se``: the standard error of the
    estimate, None for the enumeration."""
    _shap_tell_once(why)
    Xp, Z = np.atleast_2d(np.asarray(Xp, dtype=np.float64)), np.atleast_2d(np.asarray(Z, dtype=np.float64))
    (P, d), N = Xp.shape, Z.shape[0]
    exact = d < 40 and (N << d) <= SHAP_EXACT_ROWS
    if not exact and (n_permutations is None or int(n_permutations) < 2 or rng is None):
        raise ValueError(f"2^{d} coalitions on {N} background rows are not enumerated on the host: the permutation estimate needs "
                         "n_permutations >= 2 and a random generator")
    phi, base, value, inter, se = [], None, [], [], []
    for x in Xp:
        if exact:
            v = coalition_means(gp, thetas, x, Z, coalition_picks(d))
            ph, it = shapley_from_values(v, d, interactions)
            inter.append(it)
            first, last = v[:, 0], v[:, -1]
        else:
            R = int(n_permutations)
            orders = np.stack([rng.permutation(d) for _ in range(R)])
            pick = np.zeros((R, d + 1, d), dtype=bool)
            for r in range(R):
                for i in range(d):
                    pick[r, i + 1] = pick[r, i]
                    pick[r, i + 1, orders[r, i]] = True
            v = coalition_means(gp, thetas, x, Z, pick.reshape(-1, d)).reshape(-1, R, d + 1)
            steps = np.empty((v.shape[0], R, d))
            for r in range(R):
                steps[:, r, orders[r]] = np.diff(v[:, r], axis=1)
            ph = steps.mean(axis=1)
            se.append(steps.std(axis=1, ddof=1) / np.sqrt(R))
            first, last = v[:, 0, 0], v[:, 0, -1]
        phi.append(ph)
        value.append(last)
        base = first if base is None else base
    return (np.stack(phi, axis=1), base, np.stack(value, axis=1), np.stack(inter, axis=1) if exact and interactions else None,
            None if exact else np.stack(se, axis=1))


class PendingLml:
    """A block's LML between ``lml_begin`` and ``lml_finish``; ``submitted``: the device is already working on it."""

    def __init__(self, args, submitted=False):
        self.args, self.submitted = args, submitted


class CanonicalPosterior:
    canonical = True

    def lml(self, gp, T, eval_gradient):
        """(LML, gradient | None) of every row of the (B, p) block ``T``."""
        H = gp._canonical(T)
        if eval_gradient:
            lml, gh, _ = gp._ctx.lml_grad(H)
            return lml, gp._plan.grad_to_theta(gh, gp._X_train_.shape[1])
        return gp._ctx.lml(H), None

    lml_hess_path = "auto"  # "host": always numpy on the downloaded inverse (tests compare the two paths)

    def lml_hess(self, gp, theta):
        """(LML, gradient (p,), Hessian (p, p), status, "device" | "host") at ONE theta, derivatives with respect to theta.  Up to
        16 dimensions: ``bgp_lml_hess_batch`` (nothing stays resident).  More dimensions, or
        ``lml_hess_path = "host"``: ``lmlhess.lml_hess_host`` on the downloaded inverse, said once (the posterior at ``theta`` is
        the resident one afterwards).  The training inputs are the context's: a context-level warp is a fixed warp."""
        d = gp._X_train_.shape[1]
        H = gp._canonical(theta)
        if d <= lmlhess.LMLHESS_DMAX and self.lml_hess_path != "host":
            lml, gh, Hc, st = gp._ctx.lml_hess(H)
            path = "device"
        else:
            lmlhess._tell_once("more than 16 dimensions" if d > lmlhess.LMLHESS_DMAX else "forced")
            res = gp._ctx.posterior(H, want_alpha=True, want_K_inv=True)
            lml, st = res["lml"], res["status"]
            gh, Hc = np.zeros((1, d + 2)), np.zeros((1, d + 2, d + 2))
            if st[0] == 0:
                Hc[0] = lmlhess.lml_hess_host(gp.X_train_, H[0], res["K_inv"][0], res["alpha"][0], gp._plan.stationary, gp._plan.form)
                gh = gp._ctx.lml_grad(H)[1]
            path = "host"
        return float(lml[0]), gp._plan.grad_to_theta(gh, d)[0], gp._plan.hess_to_theta(Hc[0], d), int(st[0]), path

    def lml_begin(self, gp, T, W):
        """Put the block's LML batch on the device (``W``: per-row input warps) and return at once."""
        H = gp._canonical(T)
        if W is None:
            return PendingLml((H, None), gp._ctx.lml_submit(H))
        W = np.ascontiguousarray(W)
        return PendingLml((H, W), gp._ctx.lml_warped_submit(H, W))

    def lml_finish(self, gp, pending):
        if pending.submitted:
            return gp._ctx.lml_wait()
        H, W = pending.args
        return gp._ctx.lml(H) if W is None else gp._ctx.lml_warped(H, W)

    def posterior(self, gp, theta):
        """Build the resident posterior at ``theta``; returns alpha."""
        res = gp._ctx.posterior(gp._canonical(theta), want_L=False, want_alpha=True, want_K_inv=False)
        raise_if_not_pd(res["status"], gp.kernel_)
        return res["alpha"][0]

    def factor(self, gp, which):
        """``L`` or ``K_inv`` of the posterior at ``gp._post_theta``."""
        res = gp._ctx.posterior(gp._canonical(gp._post_theta), want_L=(which == "L"), want_alpha=False,
                                want_K_inv=(which == "K_inv"))
        return res[which][0]

    def make_resident(self, gp):
        H = gp._canonical(gp._post_theta)
        res = gp._ctx.resident_H
        if res is None or res.shape[0] < 1 or not np.array_equal(res[0], H[0]):
            gp._ctx.posterior(H, want_alpha=False)

    def build_rows(self, gp, thetas):
        """One batched posterior build for a set of chain rows (every row, repeated ones too); returns their H."""
        H = gp._canonical(np.atleast_2d(thetas))
        raise_if_not_pd(gp._ctx.posterior(H, want_alpha=False)["status"], gp.kernel_)
        return H

    def built_H(self, gp, thetas):
        """The H to evaluate with: ``thetas=None``: the median GP made resident, with the kernel parameters currently in ``kernel_``
        (B = 1); a block of chain rows: one batched build, their H."""
        if thetas is None:
            self.make_resident(gp)
            return gp._canonical(gp._kernel_theta_for_predict())
        return self.build_rows(gp, thetas)

    def forget(self):
        """A new context-level warp: nothing is mirrored here (``Context.set_warp`` drops ``resident_H`` itself)."""

    def predict(self, gp, X, return_cov):
        """(mean, var, cov | None) of the resident posterior, with the kernel parameters currently in ``kernel_``."""
        out = gp._ctx.predict(self.built_H(gp, None), X, return_cov=return_cov)
        return out if return_cov else (*out, None)

    def rows_predict(self, gp, thetas, X, noise_zero, return_cov=False):
        """One batched build over the distinct rows of ``thetas`` + one batched predict, scattered back to the rows."""
        uniq, inverse = np.unique(gp._canonical(thetas), axis=0, return_inverse=True)
        raise_if_not_pd(gp._ctx.posterior(uniq, want_alpha=False)["status"], gp.kernel_)
        out = gp._ctx.predict(noise_off(uniq) if noise_zero else uniq, X, return_cov=return_cov)
        inverse = np.asarray(inverse).ravel()
        return out[0][inverse], out[1][inverse], (out[2][inverse] if return_cov else None)

    def hyper_predict(self, gp, thetas, X, noise_zero, warps=None):
        """(mean, var) of every hyper-posterior draw: one build over all rows, one predict.  ``warps`` (B, 2d): every row with
        its own input warp -- its own training inputs and its own view of ``X`` -- still one build and one predict
        (``bgp_posterior_batch_warped`` / ``bgp_predict_batch_warped``); the context-level warp is not touched."""
        if warps is None:
            H = self.build_rows(gp, thetas)
            return gp._ctx.predict(noise_off(H) if noise_zero else H, X)
        H = gp._canonical(np.atleast_2d(thetas))
        raise_if_not_pd(gp._ctx.posterior(H, want_alpha=False, warps=warps)["status"], gp.kernel_)
        return gp._ctx.predict_warped(noise_off(H) if noise_zero else H, X)

    def grad_x(self, gp, x, Xt):
        """(d k(x, X_i) / dx as (n, d), k(x, X_i)) at one (warped) query point, in closed form from H."""
        hk = gp._canonical(gp._kernel_theta_for_predict())[0]
        d = Xt.shape[1]
        ell2 = np.exp(2.0 * hk[1 : d + 1])
        diff = x[None, :] - Xt                       # (n, d)
        r = np.sqrt(np.sum(diff * diff / ell2, axis=1))
        stat = gp._plan.stationary
        with np.errstate(divide="ignore", invalid="ignore"):
            if stat == "rbf":
                S = np.exp(-0.5 * r * r)
                fac = -S
            elif stat == "matern12":
                S = np.exp(-r)
                fac = np.where(r > 0, -S / r, 0.0)
            elif stat == "matern32":
                e = np.exp(-np.sqrt(3.0) * r)
                S = (1.0 + np.sqrt(3.0) * r) * e
                fac = -3.0 * e
            else:
                e = np.exp(-np.sqrt(5.0) * r)
                S = (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r * r) * e
                fac = -(5.0 / 3.0) * (1.0 + np.sqrt(5.0) * r) * e
        cst = np.exp(hk[0])
        product = gp._plan.form == "product"
        grad = (cst if product else 1.0) * fac[:, None] * diff / ell2  # (Constant / White terms: zero)
        return grad, (cst * S if product else cst + S)

    def device_gradients(self, gp):
        """The device gradient kernels serve this estimator (``bgp_predict_grad_batch``'s limits: d <= 32, no input warp)."""
        return not gp.warp_inputs and gp._X_train_.shape[1] <= 32

    def predict_grad(self, gp, X, want_dvar=True):
        """(mean (m,), var (m,), dmean (m, d), dvar (m, d) | None) of the resident posterior at the rows of X, with the kernel
        parameters currently in ``kernel_``."""
        mean, var, dmean, dvar = gp._ctx.predict_grad(self.built_H(gp, None), X, want_dvar=want_dvar)
        return mean[0], var[0], dmean[0], (dvar[0] if want_dvar else None)

    def minimize(self, gp, kappa, X0, lo, hi, gtol=1e-5, max_iter=200):
        """Minima of mean + kappa std (y units) of the resident posterior over the box from every start, in one launch."""
        return gp._ctx.minimize_starts(0, self.built_H(gp, None), *gp._y_scale(), kappa, X0, lo, hi, gtol=gtol, max_iter=max_iter)

    def partial_dependence(self, gp, thetas, Xs, grids, panels, return_std=False, return_cov=False):
        """(per panel a (B, G1) or (B, G1, G2) array in normalised-target units, "device" | "host").  ``thetas=None``: the resident
        median GP (B = 1); a block of chain rows: one batched build, then ONE device call over all of them
        (``bgp_partial_dependence``).  More than 32 dimensions, and chain rows under ``warp_inputs`` (every
        row has its own training inputs), go through ``predict``.  With ``return_std`` / ``return_cov`` the first item is ``(means,
        variances, covariances | None)`` of the latent function instead, from ONE ``bgp_partial_dependence_var`` call (DESIGN.md
        section 30) or, on the host, from ``predict(return_cov=True)`` on the synthesised rows."""
        wide = return_std or return_cov
        if gp._X_train_.shape[1] > 32 or (thetas is not None and gp.warp_inputs):
            why = "more than 32 dimensions" if gp._X_train_.shape[1] > 32 else "hyper-posterior rows with input warping"
            if wide:
                return partial_dependence_var_by_predict(gp, thetas, Xs, grids, panels, return_cov, why), "host"
            return partial_dependence_by_predict(gp, thetas, Xs, grids, panels, why), "host"
        if wide:
            if len(Xs) > PDVAR_SMAX:  # (the device route alone: the host path has no pair sum)
                raise ValueError(f"partial_dependence with return_std / return_cov takes at most {PDVAR_SMAX} sample rows, got {len(Xs)}")
            return gp._ctx.partial_dependence_var(self.built_H(gp, thetas), Xs, grids, panels, want_cov=return_cov), "device"
        return gp._ctx.partial_dependence(self.built_H(gp, thetas), Xs, grids, panels), "device"

    def profile_dependence(self, gp, thetas, X0, lo, hi, grids, panels, gtol=1e-5, max_iter=200, per_chain=False):
        """(dict of per-panel lists in normalised-target units with a leading posterior axis, "device" | "host"): the profile of
        the mean -- panel coordinates held, every other coordinate re-optimised in the box.  ``thetas=None``: the resident median GP
        (B = 1); a block of chain rows: one batched build, then ONE device call over all panels, chains and rows
        (``bgp_profile_dependence``).  ``warp_inputs`` and more than 32 dimensions take
        ``profile.profile_by_predict`` (the median GP alone)."""
        if not self.device_gradients(gp):
            if thetas is not None:
                raise ValueError("profile_dependence of hyper-posterior rows needs the device path (no input warping, d <= 32)")
            why = "input warping" if gp.warp_inputs else "more than 32 dimensions"
            return profile_by_predict(gp, X0, lo, hi, grids, panels, gtol, max_iter, why), "host"
        return gp._ctx.profile_dependence(self.built_H(gp, thetas), *gp._y_scale(), X0, lo, hi, grids, panels, gtol=gtol,
                                          max_iter=max_iter, per_chain=per_chain), "device"

    def sensitivity(self, gp, thetas, A, Bm, masks):
        """((f0 (B,), V (B,), closed (B, T), total (B, T)) in normalised-target units, "device" | "host").  ``thetas=None``: the
        resident median GP (B = 1); a block of chain rows: one batched build, then ONE device call over all of them
        (``bgp_sobol_indices``).  More than 32 dimensions, and chain rows under ``warp_inputs`` (every row
        has its own training inputs), go through ``predict``."""
        if gp._X_train_.shape[1] > SENS_DMAX or (thetas is not None and gp.warp_inputs):
            why = "more than 32 dimensions" if gp._X_train_.shape[1] > SENS_DMAX else "hyper-posterior rows with input warping"
            return sensitivity_by_predict(gp, thetas, A, Bm, masks, why), "host"
        return gp._ctx.sobol_indices(self.built_H(gp, thetas), A, Bm, masks), "device"

    def shapley(self, gp, thetas, Xp, Z, interactions=False, n_permutations=None, rng=None):
        """((phi (B, P, d), base (B,), value (B, P), inter (B, P, d, d) | None, se | None) in normalised-target units, "device" |
        "host").  ``thetas=None``: the resident median GP (B = 1); a block of chain rows: one batched build, then ONE device call
        over all of them (``bgp_shapley``; a call whose chunk partials would pass the entry's scratch bound
        goes point block by point block: a point's bits do not depend on what shares its call).  More than 16 dimensions, chain
        rows under ``warp_inputs`` (every row has its own training inputs), and a single point whose partials pass that bound (at
        d = 16 and n = 974: more than 1 077 background rows) go through ``predict`` (``shapley_by_predict``)."""
        n, d = gp._X_train_.shape
        B = 1 if thetas is None else len(np.atleast_2d(thetas))
        per_point = B * (1 << min(d, 62)) * -(-n * len(Z) // 1024)
        if d > SHAP_DMAX or (thetas is not None and gp.warp_inputs) or per_point > SHAP_PARTMAX:
            why = ("more than 16 dimensions" if d > SHAP_DMAX else
                   "hyper-posterior rows with input warping" if thetas is not None and gp.warp_inputs else
                   "one point's chunk partials pass the device call's scratch bound: fewer background rows or chain rows fit")
            return shapley_by_predict(gp, thetas, Xp, Z, why, interactions, n_permutations, rng), "host"
        H = self.built_H(gp, thetas)
        step = max(1, min(SHAP_PARTMAX // per_point, 65535 // len(H)))
        parts = [gp._ctx.shapley(H, Xp[lo:lo + step], Z, interactions) for lo in range(0, len(Xp), step)]
        phi, value = (np.concatenate([q[i] for q in parts], axis=1) for i in (0, 2))
        inter = np.concatenate([q[3] for q in parts], axis=1) if interactions else None
        return (phi, parts[0][1], value, inter, None), "device"

    gradient_cov_path = "auto"  # "host": always numpy on the downloaded inverse (tests compare the two paths)

    def gradient_cov(self, gp, thetas, X, want):
        """((dmean (B, m, d) | None, cov (B, m, d, d) | None, csum (B, 2, d, d) | None) in normalised-target units, "device" |
        "host"); ``want``: which of the three.  ``thetas=None``: the resident median GP (B = 1); a block of chain rows: one batched
        build and ONE device call per ``max_batch`` rows (``bgp_grad_cov``).  More than 32 dimensions, or
        ``gradient_cov_path = "host"``: ``gradcov.gradient_cov_host``, said once.  Matern 1/2: ValueError; ``warp_inputs``:
        NotImplementedError (the chain rule through the Beta pdf is not built)."""
        gradcov.check_differentiable(gp._plan.stationary)
        if gp.warp_inputs:
            raise NotImplementedError("the gradient covariance is not available with warp_inputs=True: the derivative with respect "
                                      "to the un-warped coordinates needs the chain rule through the Beta pdf")
        d = gp._X_train_.shape[1]
        if d > gradcov.GCOV_DMAX or self.gradient_cov_path == "host":
            dmean, cov = gradcov.host_rows(gp, thetas, X, "more than 32 dimensions" if d > gradcov.GCOV_DMAX else "forced")
            csum = np.stack(gradcov.subspace_sums(dmean, cov), axis=1) if want[2] else None
            return (dmean if want[0] else None, cov if want[1] else None, csum), "host"
        call = lambda H: gp._ctx.grad_cov(H, X, want_dmean=want[0], want_cov=want[1], want_csum=want[2])  # noqa: E731
        if thetas is None:
            return call(self.built_H(gp, None)), "device"
        thetas = np.atleast_2d(thetas)
        step = max(1, int(gp._ctx.max_batch))  # (the batched build holds max_batch rows: one build and one call per block)
        parts = [call(self.built_H(gp, thetas[lo : lo + step])) for lo in range(0, len(thetas), step)]
        return tuple(np.concatenate([p[i] for p in parts]) if want[i] else None for i in range(3)), "device"

    hessian_cov_path = "auto"  # "host": always numpy on the downloaded inverse (tests compare the two paths)

    def hessian_cov(self, gp, thetas, X, want_cov=False):
        """((hmean (B, m, d, d), hvar (B, m, d, d), hcov (B, m, T, T) | None) in normalised-target units, "device" | "host").
        ``thetas=None``: the resident median GP (B = 1); a block of chain rows: one batched build and ONE device call per
        ``max_batch`` rows (``bgp_hess_cov``).  More than 16 dimensions, or ``hessian_cov_path = "host"``:
        ``hesscov.hessian_cov_host``, said once; with chain rows the host path builds every row as posterior 0 of the context to
        download its inverse (as ``gradcov.host_rows`` does), so the median GP's posterior is no longer the resident one afterwards
        and the next call that needs it makes it resident again (section 28).  Matern 1/2 and 3/2: ValueError; ``warp_inputs``: NotImplementedError (the chain
        rule through the Beta pdf is not built)."""
        hesscov.check_twice_differentiable(gp._plan.stationary)
        if gp.warp_inputs:
            raise NotImplementedError("the Hessian covariance is not available with warp_inputs=True: the derivative with respect "
                                      "to the un-warped coordinates needs the chain rule through the Beta pdf")
        d = gp._X_train_.shape[1]
        if d > hesscov.HESS_DMAX or self.hessian_cov_path == "host":
            hmean, hvar, hcov = hesscov.host_rows(gp, thetas, X, "more than 16 dimensions" if d > hesscov.HESS_DMAX else "forced")
            return (hmean, hvar, hcov if want_cov else None), "host"
        call = lambda H: gp._ctx.hess_cov(H, X, want_mean=True, want_var=True, want_cov=want_cov)  # noqa: E731
        if thetas is None:
            return call(self.built_H(gp, None)), "device"
        thetas = np.atleast_2d(thetas)
        step = max(1, int(gp._ctx.max_batch))  # (the batched build holds max_batch rows: one build and one call per block)
        parts = [call(self.built_H(gp, thetas[lo : lo + step])) for lo in range(0, len(thetas), step)]
        return tuple(np.concatenate([p[i] for p in parts]) if parts[0][i] is not None else None for i in range(3)), "device"

    def cross_validate(self, gp, thetas, folds, warps=None):
        """(mean (B, n), var (B, n), fold_lpd (B, K), status (B, K)) of the held-out observations, normalised-target units
        (``bgp_cross_validate``).  ``thetas=None``: the resident median GP; a block of chain rows (``warps``
        (B, 2d): every row with its own input warp): the batched build, ``max_batch`` rows at a time, each followed by ONE device
        call over its rows."""
        if thetas is None:
            self.make_resident(gp)
            return gp._ctx.cross_validate(1, folds)
        thetas = np.atleast_2d(thetas)
        parts, step = [], max(1, int(gp._ctx.max_batch))
        for lo in range(0, len(thetas), step):
            T = thetas[lo : lo + step]
            if warps is None:
                self.build_rows(gp, T)
            else:
                res = gp._ctx.posterior(gp._canonical(T), want_alpha=False, warps=np.ascontiguousarray(warps[lo : lo + step]))
                raise_if_not_pd(res["status"], gp.kernel_)
            parts.append(gp._ctx.cross_validate(len(T), folds))
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))

    def influence(self, gp, thetas, X, n_focus):
        """(normalised (B, ...) arrays of ``bgp_influence``, "device" | "host"): the case-deletion influence of every observation at
        the rows of ``X``.  ``thetas=None``: the resident median GP; a block of chain rows: the batched
        build, ``max_batch`` rows at a time, each followed by ONE device call.  An observation's variance is the scalar alpha plus
        the row's white level, as the knowledge gradient takes it -- which is why the median GP's H is that of the posterior
        (``_post_theta``, made resident as ``built_H`` makes it) and not ``built_H``'s own answer, the kernel as ``predict`` sees
        it: under ``noise_set_to_zero`` that one has lost the white level the noise needs; the call gets ``noise_off(H)`` either
        way.  ``warp_inputs`` or more than 32 dimensions: ``influence.host_rows``, said once."""
        why = "input warping" if gp.warp_inputs else "more than 32 dimensions" if X.shape[1] > influence.INFL_DMAX else None
        if why is not None:
            return influence.host_rows(gp, thetas, X, n_focus, why), "host"
        base = gp._fantasy_base_alpha()
        call = lambda H: gp._ctx.influence(noise_off(H), base + np.exp(H[:, -1]), X, n_focus)  # noqa: E731
        if thetas is None:
            self.make_resident(gp)
            return call(gp._canonical(gp._post_theta)), "device"
        thetas = np.atleast_2d(thetas)
        step = max(1, int(gp._ctx.max_batch))
        return influence.concat([call(self.build_rows(gp, thetas[lo : lo + step])) for lo in range(0, len(thetas), step)]), "device"

    def pvrs(self, gp, X, T, has_alpha_vec):
        Hk = gp._canonical(gp._kernel_theta_for_predict())
        raise_if_not_pd(gp._ctx.pvrs_prepare(Hk, has_alpha_vec))
        return gp._ctx.pvrs(Hk, X, T)


class GramPosterior:
    canonical = False

    def __init__(self):
        self._resident = None  # theta whose posterior the device holds under the CURRENT warp (every posterior_gram overwrites it)

    def forget(self):
        """A new context-level warp: the host Gram matrices depend on it, so what the device holds is nobody's posterior now."""
        self._resident = None

    def _posterior_gram(self, gp, K, theta=None, **want):
        self._resident = None
        res = gp._ctx.posterior_gram(K, **want)
        self._resident = None if theta is None else np.array(theta, copy=True)
        return res

    def _build(self, gp, thetas, theta=None, **want):
        """The batched posterior build of the rows ``thetas``: by the kernel program on the device where the estimator has one
        (``BayesGPR._tree_program``; ``bgp_posterior_batch_tree``), else from host-evaluated matrices.  ``theta``: the row that is
        the resident posterior afterwards."""
        prog = gp._tree_program()
        if prog is None:
            return self._posterior_gram(gp, gp._gram_stack(thetas), theta, **want)
        self._resident = None
        res = gp._ctx.posterior_tree(prog, prog.params(thetas), **want)
        self._resident = None if theta is None else np.array(theta, copy=True)
        return res

    def lml(self, gp, T, eval_gradient):
        """``sklearn/_gpr.py:579-647``: ``K, K_gradient = kernel(X, eval_gradient=True)`` on the host; factorisation, alpha,
        K^-1 and the LML on the device; the contraction ``1/2 sum_ij (alpha_i alpha_j - K^-1_ij) dK_ij/dtheta_k`` of the
        host-evaluated gradient tensor with them (``:615-647``)."""
        if not eval_gradient:
            return gp._gram_lml(T), None
        vals, grads = np.empty(len(T)), np.empty(T.shape)
        for i, t in enumerate(T):
            K, Kg = gp._kernel_at(t)(gp.X_train_, eval_gradient=True)
            res = self._posterior_gram(gp, K, want_alpha=True, want_K_inv=True)
            if res["status"][0] != 0:
                vals[i], grads[i] = -np.inf, 0.0
                continue
            a, Ki = res["alpha"][0], res["K_inv"][0]
            vals[i] = res["lml"][0]
            grads[i] = 0.5 * (np.einsum("i,ijk,j->k", a, Kg, a) - np.einsum("ij,ijk->k", Ki, Kg))
        return vals, grads

    def lml_hess(self, gp, theta):
        """As ``CanonicalPosterior.lml_hess`` for a kernel object: its gradient tensor and central differences of it on the host,
        factorisation, alpha and K^-1 on the device (``lmlhess.lml_hess_generic``); always "host"."""
        lmlhess._tell_once("generic kernel tree")
        theta = np.asarray(theta, dtype=np.float64)
        vals, grads = self.lml(gp, theta[None, :], True)
        res = self._posterior_gram(gp, gp._gram_stack(theta), want_alpha=True, want_K_inv=True)
        st = int(res["status"][0])
        Hm = np.zeros((len(theta), len(theta)))
        if st == 0:
            Hm = lmlhess.lml_hess_generic(gp.kernel_, theta, gp.X_train_, res["K_inv"][0], res["alpha"][0])
        return float(vals[0]), grads[0], Hm, st, "host"

    def lml_begin(self, gp, T, W):
        return PendingLml((T, W))  # host kernel matrices: nothing to overlap the priors with

    def lml_finish(self, gp, pending):
        return gp._gram_lml(*pending.args)

    def posterior(self, gp, theta):
        res = self._build(gp, theta, theta, want_alpha=True)
        raise_if_not_pd(res["status"], gp.kernel_)
        return res["alpha"][0]

    def factor(self, gp, which):
        res = self._build(gp, gp._post_theta, gp._post_theta, want_L=(which == "L"), want_alpha=False,
                          want_K_inv=(which == "K_inv"))
        return res[which][0]

    def make_resident(self, gp):
        if self._resident is None or not np.array_equal(self._resident, gp._post_theta):
            self._build(gp, gp._post_theta, gp._post_theta, want_alpha=False)

    def predict(self, gp, X, return_cov):
        return self.rows_predict(gp, None, X, noise_zero=False, return_cov=return_cov)

    def rows_predict(self, gp, thetas, X, noise_zero, return_cov=False):
        """The kernel object on the host (training matrix, cross covariances, prior variances), the rest on the device.
        ``thetas=None``: the resident posterior with ``kernel_`` as it is.  With a kernel program (``BayesGPR._tree_program``) the
        three kernel matrices are the device's too (``bgp_predict_batch_tree``), which warps the query rows itself."""
        prog = gp._tree_program()
        if thetas is None:
            self.make_resident(gp)
            kernels = [gp.kernel_]
        else:
            thetas = np.atleast_2d(thetas)
            raise_if_not_pd(self._build(gp, thetas, want_alpha=False)["status"], gp.kernel_)
            kernels = None if prog is not None else [gp._kernel_at(t) for t in thetas]
        if prog is not None:
            if thetas is None:
                thetas = gp._kernel_theta_for_predict()
                if len(thetas) != prog.n_theta:  # (noise_set_to_zero has put a free WhiteKernel in a fixed one's place)
                    prog = compile_tree(gp.kernel_, gp._X_train_.shape[1])
            out = gp._ctx.predict_tree(prog, prog.params(thetas, noise_zero=noise_zero), X, return_cov=return_cov)
            return out[0], out[1], (out[2] if return_cov else None)
        Xw = gp.warp(X) if gp.warp_inputs else X  # BayesGPR.predict warps the query points (bask/bayesgpr.py:630-632)
        Xt = gp.X_train_
        if noise_zero:
            kernels = [_with_white_zeroed(k) for k in kernels]
        Ks = np.stack([k(Xw, Xt) for k in kernels])
        kss = np.stack([k.diag(Xw) for k in kernels])
        Kss = np.stack([k(Xw) for k in kernels]) if return_cov else None
        out = gp._ctx.predict_gram(Ks, kss, Kss)
        return out[0], out[1], (out[2] if return_cov else None)

    def hyper_predict(self, gp, thetas, X, noise_zero):
        return self.rows_predict(gp, thetas, X, noise_zero)[:2]

    def grad_x(self, gp, x, Xt):
        """``kernel_.gradient_x`` is ``kernels.gradient_x`` (skopt's method restated for scikit-learn kernel objects)."""
        return gradient_x(gp.kernel_, x, Xt), gp.kernel_(x[None, :], Xt)[0]

    def partial_dependence(self, gp, thetas, Xs, grids, panels, return_std=False, return_cov=False):
        if return_std or return_cov:
            return partial_dependence_var_by_predict(gp, thetas, Xs, grids, panels, return_cov, "generic kernel tree"), "host"
        return partial_dependence_by_predict(gp, thetas, Xs, grids, panels, "generic kernel tree"), "host"

    def profile_dependence(self, gp, thetas, X0, lo, hi, grids, panels, gtol=1e-5, max_iter=200, per_chain=False):
        if thetas is not None:
            raise ValueError("profile_dependence of hyper-posterior rows needs a canonical kernel")
        return profile_by_predict(gp, X0, lo, hi, grids, panels, gtol, max_iter, "generic kernel tree"), "host"

    def sensitivity(self, gp, thetas, A, Bm, masks):
        return sensitivity_by_predict(gp, thetas, A, Bm, masks, "generic kernel tree"), "host"

    def shapley(self, gp, thetas, Xp, Z, interactions=False, n_permutations=None, rng=None):
        return shapley_by_predict(gp, thetas, Xp, Z, "generic kernel tree", interactions, n_permutations, rng), "host"

    def gradient_cov(self, gp, thetas, X, want):
        raise NotImplementedError("the gradient covariance needs a canonical kernel: a generic kernel tree has no closed-form "
                                  "cross derivative")

    def hessian_cov(self, gp, thetas, X, want_cov=False):
        raise NotImplementedError("the Hessian covariance needs a canonical kernel: a generic kernel tree has no closed-form "
                                  "second derivative")

    def cross_validate(self, gp, thetas, folds, warps=None):
        """As ``CanonicalPosterior.cross_validate``: the device call reads the resident inverses alone, so host kernel matrices
        serve it as they are.  Chain rows: their matrices ``max_batch`` at a time (under ``warp_inputs`` the caller installs one
        row's warp after the other and passes one row)."""
        if thetas is None:
            self.make_resident(gp)
            return gp._ctx.cross_validate(1, folds)
        thetas = np.atleast_2d(thetas)
        parts, step = [], max(1, int(gp._ctx.max_batch))
        for lo in range(0, len(thetas), step):
            T = thetas[lo : lo + step]
            raise_if_not_pd(self._build(gp, T, want_alpha=False)["status"], gp.kernel_)
            parts.append(gp._ctx.cross_validate(len(T), folds))
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))

    def influence(self, gp, thetas, X, n_focus):
        return influence.host_rows(gp, thetas, X, n_focus, "generic kernel tree"), "host"

    def pvrs(self, gp, X, T, has_alpha_vec):
        """PVRS through the bordered-inverse identity of ``bgp_pvrs``,
        ``covs_i = sum_t [k_t^T K^-1 k_t + (k(x_t, x_i) - k_i^T K^-1 k_t)^2 / (kappa_i - k_i^T K^-1 k_i)]``, every term read off
        ONE device predictive covariance ``C = K_** - K_* K^-1 K_*^T`` over [Thompson points; candidates] per candidate chunk:
        ``C_ti``, ``C_ii`` and ``k_t^T K^-1 k_t = kappa_t - C_tt``.  K carries alpha only when it is a vector (reference quirk,
        ``bask/acquisition.py:332-333``).  All of its kernel matrices come from the host-evaluated ``kernel_``, under every
        ``tree_path``: it reads ``kernel_(Q)`` of the query rows as a matrix, which no device entry returns, and host and device
        matrices are not mixed in one computation."""
        k = gp.kernel_
        Xt = gp.X_train_
        res = self._posterior_gram(gp, k(Xt)[None], use_alpha=bool(has_alpha_vec), want_alpha=False)
        raise_if_not_pd(res["status"], k)
        if gp.warp_inputs:
            X, T = gp.warp(X), gp.warp(T)
        nt = T.shape[0]
        covs = np.empty(X.shape[0])
        step = max(1, 2048 - nt)
        for lo in range(0, X.shape[0], step):
            Q = np.vstack([T, X[lo : lo + step]])
            kss = k.diag(Q)
            C = gp._ctx.predict_gram(k(Q, Xt)[None], kss[None], k(Q)[None])[2][0]
            tt = kss[:nt] - np.diag(C)[:nt]
            cross = C[:nt, nt:]
            cii = np.diag(C)[nt:]
            covs[lo : lo + step] = tt.sum() + np.sum(cross * cross / cii[None, :], axis=0)
        return covs


def _with_white_zeroed(kernel):
    """A copy of ``kernel`` with its WhiteKernel (inside nested sums) at level 0: what ``noise_set_to_zero`` does to
    ``kernel_`` (``bask/bayesgpr.py:327-333``)."""
    k = clone(kernel)
    if isinstance(k, WhiteKernel):
        k.set_params(noise_level=0.0)
        return k
    present, white_param = param_for_white_kernel_in_sum(k)
    if present:
        k.set_params(**{white_param: WhiteKernel(noise_level=0.0)})
    return k
