"""The two posterior backends of ``BayesGPR``.  ``CanonicalPosterior`` (``kernels.KernelPlan``): the device builds every
matrix from the canonical vector ``H``.  ``GramPosterior`` (``kernels.GramPlan``): the host evaluates the kernel object, as
the reference does for every kernel (``sklearn/_gpr.py:582``), and the device factorises, solves, inverts and forms the
predictive products (``ctx.*_gram``).  Every method takes the estimator and reads ``gp._ctx`` at the call: a backend holds no
context.  What only the canonical form has -- the resident sampler, the device acquisitions, the fantasy fast path, the
device ``mvn`` draw, the sharded asynchronous gather -- is behind ``canonical``.  Predictions: normalised-target units."""
import sys

import numpy as np
from sklearn.base import clone

from . import gradcov
from .kernels import WhiteKernel, gradient_x, param_for_white_kernel_in_sum

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

    def partial_dependence(self, gp, thetas, Xs, grids, panels):
        """(per panel a (B, G1) or (B, G1, G2) array in normalised-target units, "device" | "host").  ``thetas=None``: the resident
        median GP (B = 1); a block of chain rows: one batched build, then ONE device call over all of them
        (``bgp_partial_dependence``).  More than 32 dimensions, and chain rows under ``warp_inputs`` (every
        row has its own training inputs), go through ``predict``."""
        if gp._X_train_.shape[1] > 32 or (thetas is not None and gp.warp_inputs):
            why = "more than 32 dimensions" if gp._X_train_.shape[1] > 32 else "hyper-posterior rows with input warping"
            return partial_dependence_by_predict(gp, thetas, Xs, grids, panels, why), "host"
        return gp._ctx.partial_dependence(self.built_H(gp, thetas), Xs, grids, panels), "device"

    def sensitivity(self, gp, thetas, A, Bm, masks):
        """((f0 (B,), V (B,), closed (B, T), total (B, T)) in normalised-target units, "device" | "host").  ``thetas=None``: the
        resident median GP (B = 1); a block of chain rows: one batched build, then ONE device call over all of them
        (``bgp_sobol_indices``).  More than 32 dimensions, and chain rows under ``warp_inputs`` (every row
        has its own training inputs), go through ``predict``."""
        if gp._X_train_.shape[1] > SENS_DMAX or (thetas is not None and gp.warp_inputs):
            why = "more than 32 dimensions" if gp._X_train_.shape[1] > SENS_DMAX else "hyper-posterior rows with input warping"
            return sensitivity_by_predict(gp, thetas, A, Bm, masks, why), "host"
        return gp._ctx.sobol_indices(self.built_H(gp, thetas), A, Bm, masks), "device"

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

    def lml_begin(self, gp, T, W):
        return PendingLml((T, W))  # host kernel matrices: nothing to overlap the priors with

    def lml_finish(self, gp, pending):
        return gp._gram_lml(*pending.args)

    def posterior(self, gp, theta):
        res = self._posterior_gram(gp, gp._gram_stack(theta), theta, want_alpha=True)
        raise_if_not_pd(res["status"], gp.kernel_)
        return res["alpha"][0]

    def factor(self, gp, which):
        res = self._posterior_gram(gp, gp._gram_stack(gp._post_theta), gp._post_theta, want_L=(which == "L"),
                                   want_alpha=False, want_K_inv=(which == "K_inv"))
        return res[which][0]

    def make_resident(self, gp):
        if self._resident is None or not np.array_equal(self._resident, gp._post_theta):
            self._posterior_gram(gp, gp._gram_stack(gp._post_theta), gp._post_theta, want_alpha=False)

    def predict(self, gp, X, return_cov):
        return self.rows_predict(gp, None, X, noise_zero=False, return_cov=return_cov)

    def rows_predict(self, gp, thetas, X, noise_zero, return_cov=False):
        """The kernel object on the host (training matrix, cross covariances, prior variances), the rest on the device.
        ``thetas=None``: the resident posterior with ``kernel_`` as it is."""
        Xw = gp.warp(X) if gp.warp_inputs else X  # BayesGPR.predict warps the query points (bask/bayesgpr.py:630-632)
        Xt = gp.X_train_
        if thetas is None:
            self.make_resident(gp)
            kernels = [gp.kernel_]
        else:
            thetas = np.atleast_2d(thetas)
            res = self._posterior_gram(gp, gp._gram_stack(thetas, Xt), want_alpha=False)
            raise_if_not_pd(res["status"], gp.kernel_)
            kernels = [gp._kernel_at(t) for t in thetas]
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

    def partial_dependence(self, gp, thetas, Xs, grids, panels):
        return partial_dependence_by_predict(gp, thetas, Xs, grids, panels, "generic kernel tree"), "host"

    def sensitivity(self, gp, thetas, A, Bm, masks):
        return sensitivity_by_predict(gp, thetas, A, Bm, masks, "generic kernel tree"), "host"

    def gradient_cov(self, gp, thetas, X, want):
        raise NotImplementedError("the gradient covariance needs a canonical kernel: a generic kernel tree has no closed-form "
                                  "cross derivative")

    def cross_validate(self, gp, thetas, folds, warps=None):
        """As ``CanonicalPosterior.cross_validate``: the device call reads the resident inverses alone, so host kernel matrices
        serve it as they are.  Chain rows: their matrices ``max_batch`` at a time (under ``warp_inputs`` the caller installs one
        row's warp after the other and passes one row)."""
        if thetas is None:
            self.make_resident(gp)
            return gp._ctx.cross_validate(1, folds)
        thetas = np.atleast_2d(thetas)
        Xt = gp.X_train_
        parts, step = [], max(1, int(gp._ctx.max_batch))
        for lo in range(0, len(thetas), step):
            T = thetas[lo : lo + step]
            raise_if_not_pd(self._posterior_gram(gp, gp._gram_stack(T, Xt), want_alpha=False)["status"], gp.kernel_)
            parts.append(gp._ctx.cross_validate(len(T), folds))
        return tuple(np.concatenate([p[i] for p in parts]) for i in range(4))

    def pvrs(self, gp, X, T, has_alpha_vec):
        """PVRS through the bordered-inverse identity of ``bgp_pvrs``,
        ``covs_i = sum_t [k_t^T K^-1 k_t + (k(x_t, x_i) - k_i^T K^-1 k_t)^2 / (kappa_i - k_i^T K^-1 k_i)]``, every term read off
        ONE device predictive covariance ``C = K_** - K_* K^-1 K_*^T`` over [Thompson points; candidates] per candidate chunk:
        ``C_ti``, ``C_ii`` and ``k_t^T K^-1 k_t = kappa_t - C_tt``.  K carries alpha only when it is a vector (reference quirk,
        ``bask/acquisition.py:332-333``); the kernel matrices come from the host-evaluated ``kernel_``."""
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
