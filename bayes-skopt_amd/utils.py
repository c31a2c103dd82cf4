"""Host helpers mirroring ``bask/utils.py``: chain summary (geometric median), default priors,
default kernel, input validation."""
import collections.abc
import math
import sys

import numpy as np

from .init import r2_sequence  # noqa: F401  (re-exported like bask/utils.py:8-9)
from .kernels import ConstantKernel, Matern
from .priors import halfnorm_logpdf_logspace, make_roundflat

__all__ = ["expected_minimum", "expected_optimum", "partial_dependence", "sensitivity_indices", "active_subspace", "cross_validate", "hdi", "geometric_median", "guess_priors", "construct_default_kernel", "validate_zeroone", "r2_sequence",
           "get_progress_bar"]


def geometric_median(X, eps=1e-5):
    """Geometric median (point minimising the summed Euclidean distance) of the rows of X.

    Weiszfeld's fixed-point iteration started at the mean, with the Vardi-Zhang correction when
    the iterate coincides with data rows, stopped when two iterates are closer than ``eps`` --
    the same algorithm and stopping rule as ``bask/utils.py:21-65``.
    """
    X = np.asarray(X, dtype=np.float64)
    n_pts = X.shape[0]
    cur = X.mean(axis=0)
    while True:
        dist = np.sqrt(np.einsum("ij,ij->i", X - cur, X - cur))
        away = dist != 0
        n_at = n_pts - int(np.count_nonzero(away))
        if n_at == n_pts:
            return cur
        w = 1.0 / dist[away]
        w_sum = w.sum()
        target = (w[:, None] / w_sum * X[away]).sum(axis=0)
        if n_at == 0:
            nxt = target
        else:
            pull = (target - cur) * w_sum
            r = np.linalg.norm(pull)
            shrink = 0.0 if r == 0 else n_at / r
            nxt = max(0.0, 1.0 - shrink) * target + min(1.0, shrink) * cur
        if np.sqrt(((cur - nxt) ** 2).sum()) < eps:
            return nxt
        cur = nxt


def _collect_priors(kernel, out):
    if hasattr(kernel, "kernel"):  # unary wrappers (Exponentiation)
        _collect_priors(kernel.kernel, out)
    elif hasattr(kernel, "k1"):  # Sum / Product
        _collect_priors(kernel.k1, out)
        _collect_priors(kernel.k2, out)
    elif hasattr(kernel, "kernels"):  # CompoundKernel
        for k in kernel.kernels:
            _collect_priors(k, out)
    else:
        name = type(kernel).__name__
        if name == "ConstantKernel":
            if kernel.constant_value_bounds == "fixed":
                return
            out.append(halfnorm_logpdf_logspace(2.0))
        elif name == "WhiteKernel":
            if kernel.noise_level_bounds == "fixed":
                return
            out.append(halfnorm_logpdf_logspace(2.0))
        elif name in ("Matern", "RBF"):
            if isinstance(kernel.length_scale, (collections.abc.Sequence, np.ndarray)):
                count = len(kernel.length_scale)
            else:
                count = 1
            roundflat = make_roundflat(lower_bound=0.1, upper_bound=0.6, lower_steepness=2.0, upper_steepness=8.0)

            def ls_prior(t, _rf=roundflat):
                t = np.asarray(t, dtype=np.float64)
                with np.errstate(over="ignore"):
                    out_ = _rf(np.exp(t)) + t
                return float(out_) if np.ndim(out_) == 0 else out_

            _lo, _hi, _plo, _phi, _ln = roundflat._bgp_roundflat
            ls_prior._bgp_device = (2, (math.log(_lo), math.log(_hi), _plo, _phi, _ln))  # include/bgp.h bgp_mcmc_run, prior_kind 2
            out.extend([ls_prior] * count)
        else:
            raise NotImplementedError(f"Unable to guess priors for this kernel: {kernel}.")


def guess_priors(kernel):
    """One log-prior callable per entry of ``kernel.theta`` (same order): half-Normal(0, 2) on the
    square root of every signal variance / noise level, round-flat(0.1, 0.6) on every length scale,
    both with the log-space change of variables (``bask/utils.py:68-124,154-179``)."""
    priors = []
    _collect_priors(kernel, priors)
    return priors


def construct_default_kernel(dimensions):
    """``ConstantKernel(1.0, (0.1, 2.0)) * Matern([0.3]*d, (0.2, 0.5), nu=2.5)``
    (``bask/utils.py:127-151``)."""
    d = len(dimensions)
    return ConstantKernel(constant_value=1.0, constant_value_bounds=(0.1, 2.0)) * Matern(
        length_scale=[0.3] * d, length_scale_bounds=(0.2, 0.5), nu=2.5
    )


def validate_zeroone(arr):
    """Raise ValueError unless every entry lies in [0, 1] (``bask/utils.py:212-228``)."""
    arr = np.asarray(arr)
    if np.any(arr < 0) or np.any(arr > 1):
        raise ValueError("Not all values of the array are between 0 and 1.")


def expected_minimum(res, n_random_starts=20, random_state=None):
    """Minimum of the surrogate's predictive mean: L-BFGS-B from the best observed point and
    ``n_random_starts`` random points of the space (restatement of ``skopt.utils.expected_minimum``, the
    routine ``bask/optimizer.py:497-503`` calls).  Returns (x in the original space, predicted value).

    skopt lets scipy difference the objective one point at a time; here every iterate and its 2-point
    difference stencil go to the device as ONE predict batch (d + 1 rows), forward differences switching
    to backward ones at the upper bound like scipy's ``approx_derivative``."""
    from scipy.optimize import minimize
    from sklearn.utils import check_random_state

    space = res.space
    if space.is_partly_categorical:
        raise ValueError("expected_minimum does not support any categorical values")
    reg = res.models[-1]
    bounds = np.asarray(space.bounds, dtype=np.float64)
    d = len(bounds)
    eps = np.sqrt(np.finfo(np.float64).eps)

    def fun_and_grad(x):
        h = eps * np.maximum(1.0, np.abs(x))
        sign = np.where(x + h > bounds[:, 1], -1.0, 1.0)
        pts = np.tile(x, (d + 1, 1))
        pts[1:, :][np.arange(d), np.arange(d)] += sign * h
        vals = np.asarray(reg.predict(space.transform(pts.tolist())), dtype=np.float64)
        return float(vals[0]), (vals[1:] - vals[0]) / (sign * h)

    rng = check_random_state(random_state)
    xs = [res.x]
    if n_random_starts > 0:
        xs.extend(space.rvs(n_random_starts, random_state=rng))
    best_x, best_fun = None, np.inf
    for x0 in xs:
        r = minimize(fun_and_grad, x0=np.asarray(x0, dtype=np.float64), jac=True, bounds=space.bounds, method="L-BFGS-B")
        if r.fun < best_fun:
            best_x, best_fun = r.x, r.fun
    return [float(v) for v in best_x], float(best_fun)


_told = set()


def _tell_once(reason):
    """One line on stderr, once per process and reason: a search that could have stayed on the device is driven from the host."""
    if reason not in _told:
        _told.add(reason)
        print("[bayes_skopt_amd] expected_optimum: this search is driven from the host, one device predict per iterate (%s)" % reason,
              file=sys.stderr, flush=True)


def _host_optimum(res, kappa, n_random_starts, random_state):
    """The scipy loop of ``expected_minimum`` on ``mean + kappa std`` (``predict(return_std=True)``), same starts."""
    from scipy.optimize import minimize
    from sklearn.utils import check_random_state

    space = res.space
    reg = res.models[-1]
    bounds = np.asarray(space.bounds, dtype=np.float64)
    d = len(bounds)
    eps = np.sqrt(np.finfo(np.float64).eps)

    def fun_and_grad(x):
        h = eps * np.maximum(1.0, np.abs(x))
        sign = np.where(x + h > bounds[:, 1], -1.0, 1.0)
        pts = np.tile(x, (d + 1, 1))
        pts[1:, :][np.arange(d), np.arange(d)] += sign * h
        mu, sd = reg.predict(space.transform(pts.tolist()), return_std=True)
        vals = np.asarray(mu, dtype=np.float64) + kappa * np.asarray(sd, dtype=np.float64)
        return float(vals[0]), (vals[1:] - vals[0]) / (sign * h)

    rng = check_random_state(random_state)
    xs = [res.x]
    if n_random_starts > 0:
        xs.extend(space.rvs(n_random_starts, random_state=rng))
    best_x, best_fun = None, np.inf
    for x0 in xs:
        r = minimize(fun_and_grad, x0=np.asarray(x0, dtype=np.float64), jac=True, bounds=space.bounds, method="L-BFGS-B")
        if r.fun < best_fun:
            best_x, best_fun = r.x, r.fun
    return [float(v) for v in best_x], float(best_fun)


def inverse_unrounded(space, xt):
    """A point of the transformed unit box in the original space, un-rounded: integer dimensions by their affine map
    (``expected_minimum`` returns un-rounded values too), every other dimension by its own inverse transform."""
    from .space import Integer

    return [float(xt[j] * (dim.high - dim.low) + dim.low) if isinstance(dim, Integer) else float(dim.inverse_transform(xt[j]))
            for j, dim in enumerate(space.dimensions)]


def expected_optimum(res, kappa=0.0, n_random_starts=20, random_state=None, gtol=1e-5, max_iter=200):
    """Minimum of ``mean + kappa std`` of the surrogate (``kappa = 0``: the predictive mean, as ``expected_minimum``; ``kappa``
    > 0: an upper confidence bound of the optimum), searched on the device: every start -- ``[res.x] + space.rvs(n_random_starts,
    random_state)``, the starts of ``expected_minimum`` -- is one workgroup of ONE launch that runs a bounded quasi-Newton iteration
    with analytic gradients in the transformed unit box (``bgp_minimize_starts``) until the projected gradient
    is below ``gtol`` (y units) or ``max_iter`` iterations.  Returns ``(x, value, info)``: ``x`` in the original space, un-rounded
    (integer dimensions by their affine map: ``expected_minimum`` returns un-rounded values too), ``info`` with per-start
    ``status`` (0 converged, 1 ``max_iter``, 2 no decrease), ``iters``, ``evals``, ``fun``, the transformed end points
    ``x_transformed`` with their normalised ``mean`` / ``var``, ``best`` and ``path``.  Warped inputs, generic kernel trees and more than 32 dimensions take the host
    loop (``expected_minimum``, or the same loop over ``predict(return_std=True)``), ``path == "host"``, and say so once."""
    from sklearn.utils import check_random_state

    space = res.space
    if space.is_partly_categorical:
        raise ValueError("expected_minimum does not support any categorical values")
    reg = res.models[-1]
    post = getattr(reg, "_post", None)
    if post is None or not post.canonical or not post.device_gradients(reg):
        _tell_once("input warping" if getattr(reg, "warp_inputs", False) else
                   "more than 32 dimensions" if getattr(post, "canonical", False) else "generic kernel tree")
        if kappa == 0.0:
            x, fun = expected_minimum(res, n_random_starts=n_random_starts, random_state=random_state)
        else:
            x, fun = _host_optimum(res, kappa, n_random_starts, random_state)
        return x, fun, {"path": "host"}
    rng = check_random_state(random_state)
    xs = [res.x]
    if n_random_starts > 0:
        xs.extend(space.rvs(n_random_starts, random_state=rng))
    out = post.minimize(reg, float(kappa), space.transform(xs), 0.0, 1.0, gtol=gtol, max_iter=max_iter)
    y_mean, y_std = float(np.ravel(reg.y_train_mean_)[0]), float(np.ravel(reg.y_train_std_)[0])
    fun = y_mean + y_std * out["mean"] + kappa * (y_std * np.sqrt(out["var"]))
    best = int(np.argmin(fun))
    x = inverse_unrounded(space, out["x"][best])
    info = {"path": "device", "status": out["status"], "iters": out["iters"], "evals": out["evals"], "fun": fun,
            "x_transformed": out["x"], "mean": out["mean"], "var": out["var"], "best": best}
    return x, float(fun[best]), info


def _pd_grid(dim, n_points):
    """(grid in the original space, the same in the transformed space) of one dimension: ``n_points`` values equally spaced in the
    TRANSFORMED space for a Real dimension (log-spaced for a log-uniform one), the distinct integers (at most ``n_points`` of them)
    for an Integer one, every category for a Categorical one."""
    from .space import Categorical, Integer

    if isinstance(dim, Categorical):
        orig = list(dim.categories)
    elif isinstance(dim, Integer):
        orig = [int(v) for v in np.unique(np.round(np.linspace(dim.low, dim.high, min(n_points, dim.high - dim.low + 1))))]
    else:
        t = np.linspace(0.0, 1.0, n_points)
        return np.asarray(dim.inverse_transform(t), dtype=np.float64), t
    return np.asarray(orig, dtype=object if isinstance(dim, Categorical) else np.int64), np.asarray(dim.transform(orig), dtype=np.float64)


def partial_dependence(res, dims=None, pairs="all", n_samples=250, n_points=40, samples=None, n_gp_samples=0, random_state=None):
    """The data of the "plot objective" figure: the partial dependence of the surrogate mean on single dimensions and on pairs,
    i.e. the mean of ``res.models[-1]`` averaged over ``n_samples`` points of the space (``space.rvs_transformed(n_samples,
    random_state)``, or the given ``samples`` in the original space) with one or two coordinates swept over a grid (``_pd_grid``:
    at most ``n_points`` values, at most 256).  ``dims``: the dimensions (default all); ``pairs``: "all" (every k1 < k2 of
    ``dims``), None, or a list of pairs.  Returns a dict: ``"dims"`` {k: (grid, values)}, ``"pairs"`` {(k1, k2): (grid1, grid2,
    values[G1, G2])}, grids in the original space and values in y units, and ``"path"``: "device" when every panel came from ONE
    device call (``bgp_partial_dependence``), "host" when they came through ``predict`` on synthesised rows.
    ``n_gp_samples > 0``: the fully Bayesian curve -- the average over that many rows drawn from ``chain_`` with
    ``random_state`` -- and under ``"band"`` {k: (5 %, 95 %)} the per-draw band of the 1-D curves; the default is the median GP,
    which ``res.models[-1]`` predicts with."""
    from sklearn.utils import check_random_state

    space = res.space
    reg = res.models[-1]
    rng = check_random_state(random_state)
    d = space.n_dims
    dims = list(range(d)) if dims is None else [int(k) for k in dims]
    if pairs == "all":
        pairs = [(a, b) for i, a in enumerate(dims) for b in dims[i + 1:]]
    pairs = [] if pairs is None else [(int(a), int(b)) for a, b in pairs]
    Xs = space.rvs_transformed(n_samples, random_state=rng) if samples is None else space.transform(samples)
    both = [_pd_grid(dim, n_points) for dim in space.dimensions]
    panels = [(k, -1) for k in dims] + pairs
    thetas = None
    if n_gp_samples > 0:
        chain = np.asarray(reg.chain_)
        thetas = chain[rng.randint(0, len(chain), size=int(n_gp_samples))]
    vals, path = reg.partial_dependence(Xs, [g[1] for g in both], panels, thetas=thetas, return_path=True)
    out = {"dims": {}, "pairs": {}, "path": path}
    if thetas is not None:
        out["band"] = {k: tuple(np.percentile(v, [5.0, 95.0], axis=0)) for k, v in zip(dims, vals)}
        vals = [v.mean(axis=0) for v in vals]
    for k, v in zip(dims, vals):
        out["dims"][k] = (both[k][0], v)
    for (a, b), v in zip(pairs, vals[len(dims):]):
        out["pairs"][(a, b)] = (both[a][0], both[b][0], v)
    return out


def sensitivity_indices(res, dims=None, pairs=None, n_samples=4096, n_gp_samples=0, random_state=None):
    """Which dimensions matter, and which interact: variance-based (Sobol') sensitivity indices of the surrogate mean of
    ``res.models[-1]`` over the space, by the pick-freeze design on two successive ``space.rvs_transformed(n_samples,
    random_state)`` draws (Integer and Categorical dimensions keep their snapped values; a dimension is one column).  ``dims``: the
    dimensions (default all); ``pairs``: None, "all" (every k1 < k2 of ``dims``) or a list of pairs -- a pair adds the term {a, b}
    (and its two dimensions, where ``dims`` leaves them out).  Returns a dict: ``"first"`` {k: S_k}, the share of the variance
    explained by dimension k alone; ``"total"`` {k: T_k}, the share of everything k takes part in -- a dimension with a small
    total index can be frozen; ``"interaction"`` {(a, b): S_ab - S_a - S_b}; ``"mean"`` and ``"variance"`` of the surrogate over
    the samples (y units); and ``"path"``: "device" when every term came from ONE device call (``bgp_sobol_indices``, DESIGN.md
    section 21), "host" when they came through ``predict`` on synthesised rows.  The indices are NaN when the variance is 0.
    ``n_gp_samples > 0``: the averages over that many rows drawn from ``chain_`` with ``random_state``, and under ``"band"``
    {"first": {k: (5 %, 95 %)}, "total": {k: (5 %, 95 %)}} the per-draw band; the default is the median GP, which
    ``res.models[-1]`` predicts with."""
    from sklearn.utils import check_random_state

    space = res.space
    reg = res.models[-1]
    rng = check_random_state(random_state)
    d = space.n_dims
    dims = list(range(d)) if dims is None else [int(k) for k in dims]
    if pairs == "all":
        pairs = [(a, b) for i, a in enumerate(dims) for b in dims[i + 1:]]
    pairs = [] if pairs is None else [(int(a), int(b)) for a, b in pairs]
    singles = dims + [k for k in dict.fromkeys(v for pr in pairs for v in pr) if k not in dims]
    A = space.rvs_transformed(n_samples, random_state=rng)
    Bm = space.rvs_transformed(n_samples, random_state=rng)
    thetas = None
    if n_gp_samples > 0:
        chain = np.asarray(reg.chain_)
        thetas = chain[rng.randint(0, len(chain), size=int(n_gp_samples))]
    mean, var, closed, total, path = reg.sensitivity(A, Bm, [(k,) for k in singles] + pairs, thetas=thetas, return_path=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        S, Tt = closed / np.asarray(var)[..., None], total / np.asarray(var)[..., None]
    at = {k: i for i, k in enumerate(singles)}
    inter = np.stack([S[..., len(singles) + i] - S[..., at[a]] - S[..., at[b]] for i, (a, b) in enumerate(pairs)], axis=-1) \
        if pairs else np.zeros(S.shape[:-1] + (0,))
    out = {"path": path}
    if thetas is not None:
        out["band"] = {"first": {k: tuple(np.percentile(S[:, at[k]], [5.0, 95.0])) for k in dims},
                       "total": {k: tuple(np.percentile(Tt[:, at[k]], [5.0, 95.0])) for k in dims}}
        mean, var, S, Tt, inter = (np.mean(v, axis=0) for v in (mean, var, S, Tt, inter))
    out["first"] = {k: float(S[at[k]]) for k in dims}
    out["total"] = {k: float(Tt[at[k]]) for k in dims}
    out["interaction"] = {pr: float(inter[i]) for i, pr in enumerate(pairs)}
    out["mean"], out["variance"] = float(mean), float(var)
    return out


def active_subspace(res, n_samples=1024, samples=None, n_gp_samples=0, random_state=None):
    """Which DIRECTIONS matter: the active-subspace matrix ``C = E_x[grad f grad f^T]`` of the surrogate ``res.models[-1]`` over
    ``n_samples`` points of the space (``space.rvs_transformed(n_samples, random_state)``, or the given ``samples`` in the original
    space), in transformed coordinates.  Under the GP, ``C = C_mean + C_cov``: the average of the mean gradient's outer product and
    of the gradient's posterior covariance (``BayesGPR.active_subspace``, ``bgp_grad_cov``) -- without the
    second term the eigenvalues are understated exactly where the space is unexplored.  Where Sobol' indices call two dimensions
    "important and interacting", the eigenvectors show an objective that moves along ``x_1 + x_2`` and is flat along ``x_1 - x_2``.
    Returns a dict: ``"C"``, ``"C_mean"``, ``"C_cov"`` (d, d; y units squared); ``"eigenvalues"`` in descending order;
    ``"eigenvectors"`` as columns, each signed so that its largest-magnitude component is positive; ``"explained"``, the cumulative
    eigenvalue share; ``"diag_share"`` {k: C_kk / trace}; ``"path"``: "device" | "host".  ``n_gp_samples > 0``: the matrices
    averaged over that many rows drawn from ``chain_`` with ``random_state``, and under ``"band"`` the per-draw (5 %, 95 %) band of
    each ranked eigenvalue; the default is the median GP, which ``res.models[-1]`` predicts with."""
    from sklearn.utils import check_random_state

    from .gradcov import assemble

    space = res.space
    reg = res.models[-1]
    rng = check_random_state(random_state)
    Xs = space.rvs_transformed(n_samples, random_state=rng) if samples is None else space.transform(samples)
    thetas = None
    if n_gp_samples > 0:
        chain = np.asarray(reg.chain_)
        thetas = chain[rng.randint(0, len(chain), size=int(n_gp_samples))]
    C_mean, C_cov, path = reg.active_subspace(Xs, thetas=thetas, return_path=True)
    return assemble(C_mean, C_cov, path)


def cross_validate(res, n_folds=None, n_samples=0, folds=None, weights="is", random_state=None):
    """Cross-validation of the surrogate ``res.models[-1]`` on its own training points ``res.x_iters`` (the indices of ``folds`` and
    of the result refer to ``Xi``): the held-out predictive of every fold from the resident inverse, without a refit
    (``BayesGPR.cross_validate``, ``bgp_cross_validate``).  ``n_folds=None`` and no ``folds``: leave-one-out.
    ``n_samples = 0``: the median GP, which ``res.models[-1]`` predicts with; ``n_samples > 0``: that many rows of ``chain_``,
    drawn -- like the fold split -- with a generator made from ``random_state``, combined with ``weights``.  Returns
    ``BayesGPR.cross_validate``'s dict (y units; ``z``, ``point_lpd``, ``elpd`` are the calibration and the score)."""
    from sklearn.utils import check_random_state

    reg = res.models[-1]
    rng = check_random_state(random_state)
    thetas = None
    if n_samples > 0:
        chain = np.asarray(reg.chain_)
        thetas = chain[rng.randint(0, len(chain), size=int(n_samples))]
    return reg.cross_validate(folds=folds, n_folds=n_folds, thetas=thetas, weights=weights, random_state=rng)


def predict_marginal(res, X, **kw):
    """The fully Bayesian prediction of the surrogate ``res.models[-1]`` at points ``X`` of the ORIGINAL space: mean, the spread split
    into its within-GP and between-hyper-parameter parts, quantiles of the hyper-posterior mixture and, with ``at``, P(f <= at),
    P(f > at) and the log predictive density (``BayesGPR.predict_marginal`` on ``res.space.transform(X)``, same keyword arguments;
    ``bgp_predict_mixture``)."""
    X = list(X)
    if X and not np.iterable(X[0]):
        X = [X]
    return res.models[-1].predict_marginal(res.space.transform(X), **kw)


def hdi(samples, hdi_prob=0.95, multimodal=False, max_modes=10, grid=512):
    """Highest density interval(s) of a 1-d sample (the quantity ``bask/optimizer.py:684`` takes from
    ``arviz.hdi``; arviz is not part of this image, so its two estimators are restated):

    * ``multimodal=False``: the narrowest interval containing ``hdi_prob`` of the sorted sample -> (2,);
    * ``multimodal=True``: density estimate on a regular grid (Gaussian KDE, Silverman bandwidth), grid cells
      taken in order of decreasing density until they hold ``hdi_prob`` of the mass, contiguous runs of
      cells reported as separate intervals -> (n_modes, 2)."""
    x = np.sort(np.asarray(samples, dtype=np.float64).ravel())
    x = x[np.isfinite(x)]
    n = len(x)
    if n == 0:
        raise ValueError("hdi needs at least one finite sample")
    if not multimodal:
        inc = min(int(np.floor(hdi_prob * n)), n - 1)
        widths = x[inc:] - x[: n - inc]
        i = int(np.argmin(widths))
        return np.array([x[i], x[i + inc]])
    lower, upper = x[0], x[-1]
    if upper <= lower:
        return np.array([[lower, upper]])
    from scipy.stats import gaussian_kde

    bins = np.linspace(lower, upper, grid)
    density = gaussian_kde(x, bw_method="silverman")(bins)
    dx = (upper - lower) / grid
    density = density * dx
    density = density / density.sum()
    order = np.argsort(-density)
    keep = np.sort(bins[order][np.cumsum(density[order]) <= hdi_prob])
    if keep.size == 0:
        return np.array([[lower, upper]])
    step = bins[1] - bins[0]
    runs = np.split(keep, np.where(np.diff(keep) >= step * 1.1)[0] + 1)
    return np.array([[r[0], r[-1]] for r in runs[:max_modes]])


def get_progress_bar(display, total):
    """``bask/utils.py:198-209``: a tqdm bar of ``total`` ticks when ``display is True``, an object with the same ``update`` /
    ``close`` / context-manager interface that does nothing otherwise (or when tqdm cannot be imported)."""
    from .sampler import _progress

    return _progress(display is True, total)
