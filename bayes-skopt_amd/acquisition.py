"""Acquisition functions and their evaluation driver (host side of SURVEY.md 8a row a9).

Mirrors ``bask/acquisition.py``: the same class hierarchy (``UncertaintyAcquisition`` /
``SampleAcquisition`` / ``FullGPAcquisition``), the same eight criteria and the
``evaluate_acquisitions`` driver.  What moved to the MI355X:

* ``evaluate_acquisitions`` builds the posteriors of ALL ``n_samples`` hyper-posterior draws in one
  batched device call and predicts mean/std at the candidates for all of them in one more
  (the reference rebuilds ``gpr.theta = chain_[i]`` + ``predict`` one draw at a time,
  ``bask/acquisition.py:112-141``);
* ``PVRS`` / ``VarianceReduction`` replace the per-candidate (n+1)x(n+1) Cholesky loop
  (``:287-300,328-338``) by the bordered-inverse identity evaluated with tile GEMMs on the device
  (``bgp_pvrs``) -- same numbers to rounding;
* the closed forms on (mu, std) (EI, TopTwoEI, LCB, mean, MES) are elementwise numpy on the host;
* ``KnowledgeGradient`` is not in the reference: the expected decrease of the minimum of the posterior mean after one more noisy
  observation, one device call for all candidates and hyper-posterior rows (``bgp_knowledge_gradient``);
* ``JointEntropySearch`` is not in the reference either: the expected drop of the entropy of an observation once the optimum's
  location AND value are known, on optimum samples found continuously on the device (``PosteriorPaths.minimize``), one device call
  for all candidates and hyper-posterior rows (``bgp_joint_entropy``).
"""
import sys
from abc import ABC, abstractmethod

import numpy as np
import scipy.stats as st
from scipy.optimize import brentq
from scipy.special import ndtr
from sklearn.utils import check_random_state

__all__ = [
    "evaluate_acquisitions",
    "ExpectedImprovement",
    "TopTwoEI",
    "Expectation",
    "LCB",
    "MaxValueSearch",
    "ThompsonSampling",
    "VarianceReduction",
    "PVRS",
    "KnowledgeGradient",
    "knowledge_gradient_values",
    "JointEntropySearch",
    "joint_entropy_values",
]


class Acquisition(ABC):
    @abstractmethod
    def __call__(self, *args, **kwargs):
        pass


class UncertaintyAcquisition(Acquisition, ABC):
    """Criteria computed from the predictive mean and standard deviation."""

    @abstractmethod
    def __call__(self, mu, std, *args, **kwargs):
        pass


class SampleAcquisition(Acquisition, ABC):
    """Criteria computed from one function realisation of the GP."""

    @abstractmethod
    def __call__(self, gp_sample, *args, **kwargs):
        pass


class FullGPAcquisition(Acquisition, ABC):
    """Criteria that need the whole (median) GP."""

    @abstractmethod
    def __call__(self, X, gp, *args, **kwargs):
        pass


# Closed forms with a device implementation (include/bgp.h BGP_ACQ_*).  Set to False to keep the means / standard
# deviations of all draws on the host and call the acquisition objects one draw at a time (tests compare both).
DEVICE_ACQUISITIONS = True
_ACQ_EI, _ACQ_MEAN, _ACQ_LCB, _ACQ_STD = 0, 1, 2, 3
_ACQ_MAX = 8


def _device_acq_spec(acq, kwargs):
    """(kind, parameter) of an acquisition the device evaluates itself, else None.  Exact types only: a subclass
    may redefine ``__call__``."""
    if type(acq) is ExpectedImprovement:
        y_opt = kwargs.get("y_opt")
        return _ACQ_EI, (np.nan if y_opt is None else float(y_opt))
    if type(acq) is Expectation:
        return _ACQ_MEAN, 0.0
    if type(acq) is LCB:
        alpha = kwargs.get("alpha", 1.96)
        return (_ACQ_STD, 0.0) if isinstance(alpha, str) and alpha == "inf" else (_ACQ_LCB, float(alpha))
    return None


def evaluate_acquisitions(X, gpr, acquisition_functions=None, n_samples=10, progress=False, random_state=None,
                          _record=None, **kwargs):
    """Evaluate a set of acquisition functions on candidate points X (m, d).

    Same arguments, RNG consumption and averaging as ``bask/acquisition.py:48-147``:
    ``FullGPAcquisition``s are called once with the median GP; ``UncertaintyAcquisition``s /
    ``SampleAcquisition``s are averaged over ``n_samples`` chain rows drawn WITHOUT replacement, with
    the noise switched off (``noise_set_to_zero``); an output that is not all finite contributes
    zeros; ``gpr.theta`` is restored at the end.
    Returns (len(acquisition_functions), m).

    ``_record`` (private, never forwarded to the acquisitions): a dict that receives what a batch proposal needs to
    condition this evaluation on fantasy points (``Optimizer.ask(n_points > 1)``) -- the chain rows drawn (``rows``),
    ``n_samples``, per PVRS position its Thompson points (``thompson``) and, per other whole-GP acquisition, the
    generator state it was handed (``replay``).  The generator is consumed as without it.
    """
    X = np.atleast_2d(np.asarray(X, dtype=np.float64))
    n_cand = len(X)
    acqs = list(acquisition_functions)
    out = np.zeros((len(acqs), n_cand))
    random_state = check_random_state(random_state)
    trace_i = random_state.choice(len(gpr.chain_), replace=False, size=n_samples)
    theta_backup = np.copy(gpr.theta)

    for i_acq, acq in enumerate(acqs):
        if isinstance(acq, FullGPAcquisition):
            if _record is not None and type(acq) is PVRS:
                vals, thompson = acq._evaluate(X, gpr, random_state=random_state, **kwargs)
                _record.setdefault("thompson", {})[i_acq] = thompson
            else:
                if _record is not None:  # (a batch replays the acquisition itself with the same generator state)
                    _record.setdefault("replay", {})[i_acq] = random_state.get_state()
                vals = acq(X, gpr, random_state=random_state, **kwargs)
            if np.all(np.isfinite(vals)):
                out[i_acq] = vals

    has_unc = any(isinstance(a, UncertaintyAcquisition) for a in acqs)
    has_smp = any(isinstance(a, SampleAcquisition) for a in acqs)
    rows = gpr.chain_[trace_i]
    if _record is not None:
        _record.update(rows=rows, n_samples=n_samples)
    on_device = {}
    if len(trace_i) > 0 and has_unc:
        specs = [(j, _device_acq_spec(a, kwargs)) for j, a in enumerate(acqs) if isinstance(a, UncertaintyAcquisition)]
        if (DEVICE_ACQUISITIONS and not getattr(gpr, "warp_inputs", False) and hasattr(gpr, "_acq_hyper_samples")
                and not getattr(gpr, "_generic", False)
                and len(specs) <= _ACQ_MAX and all(sp is not None for _, sp in specs)):
            # build, predict, acquisition closed forms and the average over the draws in one device pass: the
            # (draws x candidates) means and variances stay in HBM
            vals = gpr._acq_hyper_samples(rows, X, [sp[0] for _, sp in specs], [sp[1] for _, sp in specs], n_samples)
            on_device = {j: vals[k] for k, (j, _) in enumerate(specs)}
        else:
            # ONE batched posterior build + ONE batched predict for all hyper-posterior draws
            mus, stds = gpr._predict_hyper_samples(rows, X, noise_zero=True)
    samples = None
    if len(trace_i) > 0 and has_smp:
        # one function realisation per draw, each from a chain row chosen by sample_y itself (bask/acquisition.py:132-136
        # -> bask/bayesgpr.py:679), with that row's kernel parameters and -- with input warping -- its own warp
        samples = gpr._sample_hyper_rows(len(trace_i), X, random_state)
    for j, vals in on_device.items():
        out[j] = vals
    for pos in range(len(trace_i)):
        for j, acq in enumerate(acqs):
            if j in on_device:
                continue
            if isinstance(acq, UncertaintyAcquisition):
                tmp = acq(mus[pos], stds[pos], **kwargs)
            elif isinstance(acq, SampleAcquisition):
                tmp = acq(samples[pos], **kwargs)
            else:
                continue
            if np.all(np.isfinite(tmp)):
                out[j] += tmp / n_samples
    if not np.array_equal(gpr.theta, theta_backup):
        gpr.theta = theta_backup
    return out


def _average_uncertainty(gpr, acq, mus, stds, n_samples, kwargs):
    """One uncertainty acquisition averaged over the rows' (mu, std) as ``evaluate_acquisitions`` averages it: the
    device closed forms (bgp_acq_values) where the acquisition has one, else the host callable one row at a time; a row
    whose values are not all finite contributes zeros."""
    spec = _device_acq_spec(acq, kwargs)
    if DEVICE_ACQUISITIONS and spec is not None:
        return gpr._ctx.acq_values(mus, stds, [spec[0]], [spec[1]], n_samples)[0]
    out = np.zeros(mus.shape[1])
    for pos in range(mus.shape[0]):
        tmp = acq(mus[pos], stds[pos], **kwargs)
        if np.all(np.isfinite(tmp)):
            out += tmp / n_samples
    return out


_SQRT_2PI = np.sqrt(2.0 * np.pi)


def _ei_f(x):
    # x Phi(x) + phi(x) with scipy's own kernels (norm.cdf is special.ndtr, norm.pdf is exp(-x^2/2)/sqrt(2 pi)): the
    # same values as ``st.norm.cdf(x)`` / ``st.norm.pdf(x)`` without the per-call overhead of the distribution
    # machinery (34 ms -> a few ms per tell at 128 hyper-samples x 10 000 candidates)
    return x * ndtr(x) + np.exp(-(x**2) / 2.0) / _SQRT_2PI


class ExpectedImprovement(UncertaintyAcquisition):
    """Expected improvement over the current optimum ``y_opt`` (default: min of mu)
    (``bask/acquisition.py:154-172``)."""

    def __call__(self, mu, std, *args, y_opt=None, **kwargs):
        if y_opt is None:
            y_opt = mu.min()
        values = np.zeros_like(mu)
        ok = std > 0
        values[ok] = _ei_f((y_opt - mu[ok]) / std[ok]) * std[ok]
        return values


class TopTwoEI(ExpectedImprovement):
    """Expected improvement over the point with the highest EI (``bask/acquisition.py:175-194``)."""

    def __call__(self, mu, std, *args, y_opt=None, **kwargs):
        ei = super().__call__(mu, std, *args, y_opt=y_opt, **kwargs)
        values = np.zeros_like(mu)
        top = np.argmax(ei)
        ok = std > 0
        spread = np.sqrt(std[ok] ** 2 + std[top] ** 2)
        values[ok] = spread * _ei_f((mu[top] - mu[ok]) / spread)
        return values


class Expectation(UncertaintyAcquisition):
    """Lowest predicted mean (``bask/acquisition.py:197-201``)."""

    def __call__(self, mu, std, *args, **kwargs):
        return -mu


class LCB(UncertaintyAcquisition):
    """Lower confidence bound ``alpha * std - mu``; ``alpha="inf"`` returns std
    (``bask/acquisition.py:204-216``)."""

    def __call__(self, mu, std, *args, alpha=1.96, **kwargs):
        if alpha == "inf":
            return std
        return alpha * std - mu


class MaxValueSearch(UncertaintyAcquisition):
    """Max-value entropy search (Wang & Jegelka 2017) with a Gumbel fit of the optimum distribution
    from three quantiles found by bisection (``bask/acquisition.py:219-267``; uses the global numpy
    RNG like the reference)."""

    def __call__(self, mu, std, *args, n_min_samples=1000, **kwargs):
        mean = -mu  # the algorithm is stated for maximisation

        def prob_below(x):
            return np.exp(np.sum(st.norm.logcdf((x - mean) / std), axis=0))

        lo = np.min(mean - 3 * std)
        hi = np.max(mean + 5 * std)
        q1, med, q2 = [brentq(lambda x, v=v: prob_below(x) - v, lo, hi) for v in (0.25, 0.5, 0.75)]
        beta = (q1 - q2) / (np.log(np.log(4.0 / 3.0)) - np.log(np.log(4.0)))
        alpha = med + beta * np.log(np.log(2.0))
        max_values = -np.log(-np.log(np.random.rand(n_min_samples).astype(np.float32))) * beta + alpha
        gamma = (max_values[None, :] - mean[:, None]) / std[:, None]
        norm = st.norm()
        return np.sum(gamma * norm.pdf(gamma) / (2.0 * norm.cdf(gamma)) - norm.logcdf(gamma), axis=1) / n_min_samples


class ThompsonSampling(SampleAcquisition):
    """Optimum of one sampled function (``bask/acquisition.py:270-274``)."""

    def __call__(self, gp_sample, *args, **kwargs):
        return -gp_sample


def _device_pvrs(gp, X, thompson_points):
    """covs[i] = trace(K_trans K_aug,i^-1 K_trans^T) for every candidate i on the device.  The
    augmented kernel matrix uses kernel_ as it stands (median noise included) and adds ``alpha`` only
    when it is a vector (``bask/acquisition.py:293-294,332-333``)."""
    has_vec = bool(np.iterable(gp.alpha))
    return gp._pvrs(X, thompson_points, has_vec)


class VarianceReduction(FullGPAcquisition):
    """Global variance reduction (``bask/acquisition.py:277-300``): PVRS with every candidate as a
    reference point."""

    def __call__(self, X, gp, *args, **kwargs):
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        return _device_pvrs(gp, X, X)


class PVRS(FullGPAcquisition):
    """Predictive variance reduction search (Nguyen et al. 2017; ``bask/acquisition.py:303-339``):
    draw ``n_thompson`` functions from the median GP, take their minimisers among the candidates and
    score each candidate by how much observing it reduces the predictive variance at those points."""

    def __call__(self, X, gp, *args, n_thompson=10, random_state=None, **kwargs):
        return self._evaluate(X, gp, n_thompson=n_thompson, random_state=random_state)[0]

    def _evaluate(self, X, gp, *args, n_thompson=10, random_state=None, **kwargs):
        """(values, Thompson points): the batch proposal conditions on fantasy points with the same Thompson points."""
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        thompson_sample = gp.sample_y(X, sample_mean=True, n_samples=n_thompson, random_state=random_state)
        thompson_points = X[np.argmin(thompson_sample, axis=0)]
        return _device_pvrs(gp, X, thompson_points), thompson_points


# ---- knowledge gradient ----------------------------------------------------------------------------------
KG_DMAX, KG_MMAX = 32, 255  # limits of the device call (bgp_kg.hip)
KG_HOST_ROWS = 2048         # rows of [reference points; candidates] per predict(return_cov=True) of the host path
_kg_told = []


def _tell_once(name, why):
    """One line on stderr, once per process and acquisition: computed on the host from ``predict(return_cov=True)``."""
    told = globals()[{"knowledge_gradient": "_kg_told", "joint_entropy": "_jes_told"}[name]]
    if not told:
        told.append(True)
        print("[bayes_skopt_amd] %s: on the host from predict(return_cov=True) (%s)" % (name, why), file=sys.stderr, flush=True)


def knowledge_gradient_values(p, q):
    """``min_j p_j - E[min_j (p_j + q_j Z)]``, Z ~ N(0, 1), for line arrays ``p``, ``q`` of shape (..., L): the sorted-breakpoint
    form (Frazier, Powell & Dayanik 2009, algorithm 1, stated for the minimum).  The lines are sorted by slope (equal slopes: the
    lower intercept stays), the lower envelope is built by one pass with a stack, and with ``c_k`` the breakpoint between the
    envelope's lines k and k + 1 the value is ``sum_k |q_(k+1) - q_(k)| f(-|c_k|)``, ``f(z) = z Phi(z) + phi(z)``.  Returns (...)
    values >= 0 in the units of ``p``."""
    p, q = np.broadcast_arrays(np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64))
    shape, L = p.shape[:-1], p.shape[-1]
    a, b = -p.reshape(-1, L), -q.reshape(-1, L)  # E[max_j (a_j + b_j Z)] - max_j a_j
    N = a.shape[0]
    if N == 0 or L < 2:
        return np.zeros(shape)
    # slope ascending; among equal slopes the largest intercept first (the others never reach the envelope)
    o1 = np.argsort(-a, axis=1, kind="stable")
    o2 = np.argsort(np.take_along_axis(b, o1, axis=1), axis=1, kind="stable")
    order = np.take_along_axis(o1, o2, axis=1)
    a, b = np.take_along_axis(a, order, axis=1), np.take_along_axis(b, order, axis=1)
    skip = np.zeros((N, L), dtype=bool)
    skip[:, 1:] = b[:, 1:] == b[:, :-1]
    stack = np.zeros((N, L), dtype=np.intp)  # envelope so far: sorted line indices, bottom = the smallest slope (z -> -inf)
    cs = np.zeros((N, L))                    # cs[:, k]: where stack[:, k] takes over from stack[:, k - 1]
    cs[:, 0] = -np.inf
    top = np.zeros(N, dtype=np.intp)
    for j in range(1, L):
        idx = np.flatnonzero(~skip[:, j])
        while idx.size:  # (a row leaves when its line is pushed; every pass pops one line of each row left: <= L passes per row in all)
            t = stack[idx, top[idx]]
            with np.errstate(invalid="ignore", over="ignore"):
                z = (a[idx, t] - a[idx, j]) / (b[idx, j] - b[idx, t])
            pop = z <= cs[idx, top[idx]]
            push = idx[~pop]
            top[push] += 1
            stack[push, top[push]] = j
            cs[push, top[push]] = z[~pop]
            idx = idx[pop]
            top[idx] -= 1
    valid = np.arange(1, L)[None, :] <= top[:, None]
    db = np.take_along_axis(b, stack[:, 1:], axis=1) - np.take_along_axis(b, stack[:, :-1], axis=1)
    z = -np.abs(cs[:, 1:])
    z = np.where(np.isinf(z), -1e300, z)  # (a breakpoint that overflowed: f is 0 there, not -inf * 0)
    with np.errstate(over="ignore", under="ignore"):
        f = z * ndtr(z) + np.exp(-(z * z) / 2.0) / _SQRT_2PI
    return np.where(valid, db * f, 0.0).sum(axis=1).reshape(shape)


def _kg_white_level(gp, theta):
    """The white level of the kernel at ``theta`` (0 without one): what a row's fantasy observation carries beside alpha."""
    if gp._post.canonical:
        return float(np.exp(gp._canonical(np.atleast_2d(theta))[0, -1]))
    from .kernels import WhiteKernel, param_for_white_kernel_in_sum

    k = gp._kernel_at(theta)
    if isinstance(k, WhiteKernel):
        return float(k.noise_level)
    present, name = param_for_white_kernel_in_sum(k)
    return float(k.get_params()[name].noise_level) if present else 0.0


def _host_rows(gp, rows, X, points, noise_of, value, n_samples):
    """The row loop of the host paths: per row b (``rows=None``: the median GP) the latent joint moments of [points[b]; chunk] from
    ``predict(return_cov=True)`` (the device's predictive products, the kernel on the host where it is a generic tree), handed to
    ``value(out, b, noise, mean_p, var_p, mean_c, var_c, cov)`` -- ``out`` the chunk's slice of the row's values, ``cov`` (chunk,
    points), ``noise = noise_of(white level of the row)``.  Under ``warp_inputs`` a chain row is installed with its own warp, one
    row after the other.  Returns (m,), averaged as ``evaluate_acquisitions`` averages (a row that is not all finite contributes
    nothing)."""
    from ._posterior import noise_off

    post = gp._post
    m = X.shape[0]

    def row_values(theta_row, theta, b):
        noise = noise_of(_kg_white_level(gp, theta))
        M = points[b].shape[0]
        step = max(1, KG_HOST_ROWS - M)
        out = np.zeros(m)
        for lo in range(0, m, step):
            Q = np.vstack([points[b], X[lo : lo + step]])
            if theta_row is None and post.canonical:
                post.make_resident(gp)
                mean, var, cov = gp._ctx.predict(noise_off(gp._canonical(gp._kernel_theta_for_predict())), Q, return_cov=True)
            else:
                mean, var, cov = post.rows_predict(gp, theta_row, Q, noise_zero=True, return_cov=True)
            mean, var, cov = mean[0], var[0], cov[0]
            value(out[lo : lo + step], b, noise, mean[:M], var[:M], mean[M:], var[M:], cov[:M, M:].T)
        return out

    if rows is None:
        return row_values(None, gp._post_theta, 0)
    total = np.zeros(m)
    n_theta = len(gp.kernel_.theta)
    if gp.warp_inputs:
        with gp._row_warps() as install:
            vals = [row_values(install(r), r[:n_theta], b) for b, r in enumerate(rows)]
    else:
        vals = [row_values(r[None, :], r, b) for b, r in enumerate(rows)]
    for v in vals:
        if np.all(np.isfinite(v)):
            total += v / n_samples
    return total


def _kg_host(gp, rows, X, A, n_samples, why):
    """The host path: the lines of every candidate from the joint moments of [A; chunk] (``_host_rows``; the observation's noise
    is not floored), ``knowledge_gradient_values``; written only where ``s > 0``.  Returns (m,) in y units."""
    _tell_once("knowledge_gradient", why)
    y_std = gp._y_scale()[1]
    base = gp._fantasy_base_alpha()

    def value(out, b, noise, mean_p, var_p, mean_c, v, cov):
        ok = v + noise > 0.0
        if not ok.any():
            return
        rs = 1.0 / np.sqrt((v + noise)[ok])
        pl = np.concatenate([np.broadcast_to(mean_p, (int(ok.sum()), len(mean_p))), mean_c[ok][:, None]], axis=1)
        ql = np.concatenate([cov[ok], v[ok][:, None]], axis=1) * rs[:, None]
        out[ok] = np.maximum(knowledge_gradient_values(pl, ql), 0.0) * y_std

    return _host_rows(gp, rows, X, np.broadcast_to(A, (1 if rows is None else len(rows),) + A.shape), lambda white: base + white, value,
                      n_samples)


class KnowledgeGradient(FullGPAcquisition):
    """Knowledge gradient for minimisation under noise (Frazier, Powell & Dayanik 2009; Scott, Frazier & Powell 2011): how much one
    more noisy observation at x is expected to lower the minimum of the posterior MEAN over a reference set and x itself,
    ``KG(x) = min_j mu(a_j) - E[min_j mu_+(a_j)]`` -- the quantity ``expected_optimum`` reports at the end of a noisy run.

    ``reference_points`` (M, d), or by default the ``min(n_reference, m)`` candidates of lowest posterior mean under the median GP
    (stable argsort); every row shares them.  ``n_gp_samples = 0``: the median GP; ``n_gp_samples > 0``: the average over that many
    chain rows drawn without replacement from ``random_state``, ONE batched posterior build and ONE device call
    (``bgp_knowledge_gradient``).  The observation at x carries the noise a ``tell`` with noise 0 would give
    it (the scalar alpha + the row's white level).  Values in y units, >= 0.  Generic kernel trees, ``warp_inputs=True``, more than
    32 dimensions or more than 255 reference points: the host path (``knowledge_gradient_values`` on ``predict(return_cov=True)``),
    said once on stderr.  ``return_path``: also "device" | "host"."""

    path = "auto"  # "host": always the host path (tests compare the two)

    def __call__(self, X, gp, *args, n_reference=63, reference_points=None, n_gp_samples=0, random_state=None, return_path=False,
                 **kwargs):
        from ._posterior import noise_off

        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        m, d = X.shape
        if reference_points is None:
            mean = np.asarray(gp._post.predict(gp, X, False)[0])[0]
            A = X[np.argsort(mean, kind="stable")[: max(0, min(int(n_reference), m))]]
        else:
            A = np.asarray(reference_points, dtype=np.float64).reshape(-1, d)
        rows = None
        if n_gp_samples > 0:
            rng = check_random_state(random_state)
            rows = gp.chain_[rng.choice(len(gp.chain_), replace=False, size=int(n_gp_samples))]
        why = ("forced" if self.path == "host" else "generic kernel tree" if not gp._post.canonical else "input warping"
               if gp.warp_inputs else "more than 32 dimensions" if d > KG_DMAX else "more than 255 reference points"
               if len(A) > KG_MMAX else None)
        if why is not None:
            vals = _kg_host(gp, rows, X, A, max(int(n_gp_samples), 1), why)
            return (vals, "host") if return_path else vals
        y_std = gp._y_scale()[1]
        if rows is None:
            gp._post.make_resident(gp)
            H = gp._canonical(gp._post_theta)
        else:
            H = gp._post.build_rows(gp, rows)
        noise = gp._fantasy_base_alpha() + np.exp(H[:, -1])
        vals = gp._ctx.knowledge_gradient(noise_off(H), noise, X, A, y_std, len(H), want_rows=False)[1]
        return (vals, "device") if return_path else vals


# ---- joint entropy search --------------------------------------------------------------------------------
JES_DMAX, JES_RMAX = 32, 255  # limits of the device call (bgp_jes.hip)
JES_F_SWITCH, JES_F_DEPTH = 4.0, 40  # F: the definition below the switch point, the continued fraction (cut at this numerator) from it on
JES_NOISE_FLOOR = 1e-12
_jes_told, _jes_floor_told = [], []


def _jes_F_direct(z):
    """``1 - lam (lam - z)``, ``lam = sqrt(2 / pi) / erfcx(z / sqrt 2)``: loses ``eps z^4`` for large positive z."""
    from scipy.special import erfcx

    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        lam = np.sqrt(2.0 / np.pi) / erfcx(z * np.sqrt(0.5))
        return 1.0 - lam * (lam - z)


def _jes_F_cf(z, depth=JES_F_DEPTH):
    """``T (U - T)`` with ``T = 1 / (z + U)``, ``U = 2 / (z + 3 / (z + ... depth / z))`` (Laplace's continued fraction of the Mills
    ratio; z > 0), U bottom-up as a ratio scaled by 1 / z: ``N_k = k D_{k+1} / z``, ``D_k = D_{k+1} + N_{k+1} / z``."""
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        rz = 1.0 / z
        N, D = np.zeros_like(z), np.ones_like(z)
        for k in range(depth, 1, -1):
            N, D = (k * rz) * D, D + rz * N
        U = N / D
        T = 1.0 / (z + U)
        return T * (U - T)


def _jes_F(z):
    """The variance factor of a normal truncated below at z, ``1 - lam (lam - z)`` with ``lam = phi(z) / Phi(-z)``: the definition
    for z < 4, the continued fraction from 4 on (a function of z alone; bgp_jes.hip takes the same two forms)."""
    z = np.asarray(z, dtype=np.float64)
    big = z >= JES_F_SWITCH
    return np.where(big, _jes_F_cf(np.where(big, z, JES_F_SWITCH)), _jes_F_direct(np.where(big, 0.0, z)))


def joint_entropy_values(mu, var, mu_opt, var_opt, cov, f_opt, noise, tau):
    """The joint-entropy-search gain (nats, >= 0) of candidates with latent moments ``mu``, ``var`` (..., m) given R samples of the
    optimum with latent moments ``mu_opt``, ``var_opt`` and values ``f_opt`` (..., R) and cross-covariances ``cov`` (..., m, R):
    each sample conditions on ``f(a_r) = f_r`` (jitter ``tau``; nothing where ``var_opt + tau <= 0``), truncates ``f(x) >= f_r``
    (``v_t = clip(v_s F(z), 0, v_s)``, 0 where ``v_s <= 0``) and contributes ``1/2 [log(v + noise) - log(v_t + noise)]`` clipped at
    0; the mean over the samples.  Everything in normalised-y units; ``noise`` > 0 is the variance of an observation."""
    mu, var = np.asarray(mu, dtype=np.float64)[..., None], np.asarray(var, dtype=np.float64)[..., None]
    mo, vo, fo = (np.asarray(a, dtype=np.float64)[..., None, :] for a in (mu_opt, var_opt, f_opt))
    c = np.asarray(cov, dtype=np.float64)
    nu = np.asarray(noise, dtype=np.float64)[..., None, None]
    w = vo + tau
    on = w > 0.0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ws = np.where(on, w, 1.0)
        mr = mu + np.where(on, c * ((fo - mo) / ws), 0.0)
        vs = np.maximum(var - np.where(on, c * c / ws, 0.0), 0.0)
        pos = vs > 0.0
        z = (fo - mr) / np.sqrt(np.where(pos, vs, 1.0))
        vt = np.where(pos, np.clip(vs * _jes_F(z), 0.0, vs), 0.0)
        g = np.maximum(0.5 * (np.log(var + nu) - np.log(vt + nu)), 0.0)
    return g.mean(axis=-1)


def _jes_noise(gp, whites):
    """The variance of an observation per row, ``_fantasy_base_alpha() + white``, floored at 1e-12 (said once if the floor bites)."""
    noise = gp._fantasy_base_alpha() + np.asarray(whites, dtype=np.float64)
    if np.any(noise < JES_NOISE_FLOOR) and not _jes_floor_told:
        _jes_floor_told.append(True)
        print("[bayes_skopt_amd] joint_entropy: observation noise below %g, floored there" % JES_NOISE_FLOOR, file=sys.stderr, flush=True)
    return np.maximum(noise, JES_NOISE_FLOOR)


def _jes_host(gp, rows, X, A, f, tau, n_samples, why):
    """The host path: ``joint_entropy_values`` on the joint moments of [A_b; chunk] (``_host_rows``; the observation's noise floored
    by ``_jes_noise``).  ``A`` (B, R, d), ``f`` (B, R) in normalised-y units.  Returns (m,) in nats."""
    _tell_once("joint_entropy", why)

    def value(out, b, noise, mean_p, var_p, mean_c, var_c, cov):
        out[:] = joint_entropy_values(mean_c, var_c, mean_p, var_p, cov, f[b], noise, tau)

    return _host_rows(gp, rows, X, A, lambda white: _jes_noise(gp, [white])[0], value, n_samples)


class JointEntropySearch(FullGPAcquisition):
    """Joint entropy search for minimisation under noise (Hvarfner, Hutter & Nardi 2022; Tu, Gandy, Kantas & Shafei 2022): the
    expected drop of the entropy of an observation at x once the optimum's location and value ``(x*, f*)`` are known, moment
    matched -- each optimum sample conditions the GP on ``f(x*) = f*`` (jitter ``tau``, normalised-y units squared) and truncates
    ``f(x) >= f*`` (``joint_entropy_values``).  Values in nats, >= 0.

    ``n_gp_samples = 0``: the median GP with ``n_optima`` optimum samples; ``n_gp_samples = B > 0``: B chain rows drawn without
    replacement from ``random_state`` (first), each with ``n_optima`` samples of ITS optimum.  The samples are pathwise draws of
    exactly those rows (``n_features`` Fourier features each), minimised over the unit box on the device from the ``n_starts``
    lowest of ``n_candidates`` uniform points (``PosteriorPaths.minimize``); ``optimum_samples=(X_opt, f_opt)`` gives them instead:
    ``X_opt`` (R, d) in the transformed space and ``f_opt`` (R,) in y units, or (B, R, d) / (B, R).  ONE batched posterior build
    for the rows and ONE device call (``bgp_joint_entropy``); the observation carries the noise a ``tell``
    with noise 0 would give it (the scalar alpha + the row's white level, floored at 1e-12).  Generic kernel trees,
    ``warp_inputs=True``, more than 32 dimensions or more than 255 optimum samples: the host path (``joint_entropy_values`` on
    ``predict(return_cov=True)``), said once on stderr -- and ``ValueError`` with ``sample_paths``' own reason where the draws
    cannot run and no ``optimum_samples`` were given.  ``return_path``: also "device" | "host"."""

    path = "auto"  # "host": always the host path (tests compare the two)

    def __call__(self, X, gp, *args, n_optima=64, n_gp_samples=0, optimum_samples=None, n_features=1024, n_candidates=2000,
                 n_starts=4, tau=1e-6, random_state=None, return_path=False, **kwargs):
        from ._posterior import noise_off

        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        m, d = X.shape
        rng = check_random_state(random_state)
        rows = None
        if n_gp_samples > 0:
            rows = gp.chain_[rng.choice(len(gp.chain_), replace=False, size=int(n_gp_samples))]
        B = 1 if rows is None else len(rows)
        y_mean, y_std = gp._y_scale()
        if optimum_samples is None:
            thetas = np.asarray(gp._post_theta, dtype=np.float64)[None, :] if rows is None else rows
            with gp._sample_paths_rows(thetas, int(n_optima), n_features, rng) as paths:
                found = paths.minimize(bounds=(0.0, 1.0), n_candidates=n_candidates, n_starts=n_starts, random_state=rng)
            A, f = found["x"].reshape(B, -1, d), found["fun"].reshape(B, -1)
        else:
            A, f = (np.asarray(a, dtype=np.float64) for a in optimum_samples)
            if A.ndim == 2:
                A, f = np.broadcast_to(A[None], (B,) + A.shape), np.broadcast_to(f.reshape(1, -1), (B, f.size))
            if A.ndim != 3 or A.shape[0] != B or A.shape[2] != d or f.shape != A.shape[:2] or A.shape[1] < 1:
                raise ValueError("optimum_samples must be ((R, d), (R,)) or ((%d, R, d), (%d, R)) with R >= 1 and d = %d, got %r, %r"
                                 % (B, B, d, A.shape, f.shape))
        A, f = np.ascontiguousarray(A), (np.ascontiguousarray(f) - y_mean) / y_std
        if not np.all(np.isfinite(f)):
            raise ValueError("the optimum values are not all finite")
        tau = float(tau)
        why = ("forced" if self.path == "host" else "generic kernel tree" if not gp._post.canonical else "input warping"
               if gp.warp_inputs else "more than 32 dimensions" if d > JES_DMAX else "more than 255 optimum samples"
               if A.shape[1] > JES_RMAX else None)
        if why is not None:
            vals = _jes_host(gp, rows, X, A, f, tau, max(int(n_gp_samples), 1), why)
            return (vals, "host") if return_path else vals
        if rows is None:
            gp._post.make_resident(gp)
            H = gp._canonical(gp._post_theta)
        else:
            H = gp._post.build_rows(gp, rows)
        H = np.atleast_2d(H)
        noise = _jes_noise(gp, np.exp(H[:, -1]))
        vals = gp._ctx.joint_entropy(noise_off(H), noise, X, A, f, tau, len(H), want_rows=False)[1]
        return (vals, "device") if return_path else vals
