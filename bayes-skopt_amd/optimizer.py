"""Stepwise Bayesian optimisation: ``Optimizer.ask / tell / run`` (host mirror of
``bask/optimizer.py:35-445``).  ``tell`` is the per-iteration entry of the hot path: it
(re)fits / resumes the BayesGPR hyper-posterior MCMC on the device and evaluates the acquisition
function over ``n_points`` random candidates with the device predict / PVRS kernels.

The post-hoc diagnostics ``probability_of_optimality`` / ``expected_optimality_gap`` /
``optimum_intervals`` (``bask/optimizer.py:447-689``) run on the device ``sample_y``.
"""
import sys
import warnings

import numpy as np
from sklearn.utils import check_random_state

from . import acquisition
from .acquisition import evaluate_acquisitions
from .bayesgpr import BayesGPR
from .init import r2_sequence, sb_sequence
from .space import create_result, is_2Dlistlike, is_listlike, normalize_dimensions
from .utils import active_subspace, construct_default_kernel, cross_validate, expected_minimum, expected_optimum, hdi, inverse_unrounded, partial_dependence, predict_marginal, sensitivity_indices

__all__ = ["Optimizer"]

ACQUISITION_FUNC = {
    "ei": acquisition.ExpectedImprovement(),
    "kg": acquisition.KnowledgeGradient(),
    "jes": acquisition.JointEntropySearch(),
    "lcb": acquisition.LCB(),
    "mean": acquisition.Expectation(),
    "mes": acquisition.MaxValueSearch(),
    "pvrs": acquisition.PVRS(),
    "ts": acquisition.ThompsonSampling(),
    "ttei": acquisition.TopTwoEI(),
    "vr": acquisition.VarianceReduction(),
}

_INT32_MAX = np.iinfo(np.int32).max
BATCH_STRATEGIES = ("cl_min", "cl_mean", "cl_max", "kb")
JOINT_STRATEGIES = ("joint_ei", "thompson")  # batches picked on joint pathwise draws (PosteriorPaths.select_batch)


class Optimizer:
    """Ask/tell optimiser with the constructor arguments, public attributes (``rng, space, gp, gp_priors, Xi, yi,
    noisei, n_points, n_initial_points_, init_strategy, acq_func, acq_func_kwargs``) and defaults of
    ``bask/optimizer.py:120-175``.  The generator ``rng`` is consumed in the reference's order (initial-design seed,
    surrogate seed; per tell: candidate draw, acquisition seed), so a seeded run visits the same points."""

    _batch_path = "auto"  # "fallback": batch proposals always through the host-driven path (tests compare the two)
    _batch_moments = False  # True: _last_batch_info carries the fast path's conditioned latent moments (tests)

    def __init__(self, dimensions, n_points=500, n_initial_points=10, init_strategy="sb", gp_kernel=None,
                 gp_kwargs=None, gp_priors=None, acq_func="pvrs", acq_func_kwargs=None, random_state=None, **kwargs):
        self.rng = check_random_state(random_state)
        self.space = normalize_dimensions(dimensions)
        self.n_points = n_points
        self.acq_func = acq_func if callable(acq_func) else ACQUISITION_FUNC[acq_func]
        self.acq_func_kwargs = acq_func_kwargs if acq_func_kwargs is not None else {}
        self._plan_initial_design(n_initial_points, init_strategy)
        self.gp = self._new_surrogate(gp_kernel, gp_kwargs)
        self.gp_priors = gp_priors
        self._forget_observations()
        self._next_x = None
        self._last_candidates = None  # transformed candidates / acquisition values of the latest proposal (tests, plots)
        self._last_acq_values = None
        self._last_batch_state = None  # what the latest proposal drew (chain rows, Thompson points) for ask(n_points > 1)
        self._last_batch_info = None   # path taken / step values / device counters of the latest batch (tests, probes)

    # ---- construction helpers ------------------------------------------------------------------------------
    def _plan_initial_design(self, n_initial_points, init_strategy):
        """"r2": the whole quasi-random design up front; "sb": a private generator for the sequential Steinerberger
        points (seeded from ``rng``); anything else: uniform random points drawn on demand."""
        self.n_initial_points_ = self._n_initial_points = n_initial_points
        self.init_strategy = init_strategy
        if init_strategy == "r2":
            self._initial_points = self.space.inverse_transform(r2_sequence(n=n_initial_points, d=self.space.n_dims))
        elif init_strategy == "sb":
            self._init_rng = np.random.RandomState(self.rng.randint(2**31))

    def _new_surrogate(self, kernel, gp_kwargs):
        if kernel is None:  # the default kernel only needs the number of (transformed) dimensions
            kernel = construct_default_kernel(list(range(self.space.transformed_n_dims)))
        return BayesGPR(kernel=kernel, random_state=self.rng.randint(0, _INT32_MAX), **(gp_kwargs or {}))

    def _forget_observations(self):
        self.Xi, self.yi, self.noisei = [], [], []

    def _result(self):
        return create_result(self.Xi, self.yi, self.space, self.rng, models=[self.gp])

    # ---- ask ---------------------------------------------------------------------------------------------------
    def ask(self, n_points=1, strategy="cl_min", pending=None, n_paths=256, n_features=1024):
        """Next point to evaluate (``bask/optimizer.py:177-226``): a point of the initial design while it lasts, then
        the maximiser of the acquisition function found by the last ``tell``.

        ``n_points > 1`` returns a list of ``n_points`` distinct points (``n_points == 1``: the single point, and
        ``strategy`` is not looked at):

        * while the initial design lasts, or before any model has been fit, the next ``n_points`` points of the design --
          "r2": the following design points in the order single ask / tell rounds hand them out; "sb": the sequential
          Steinerberger extension of the points seen so far; otherwise ``space.rvs(n_points)``.  Slots the design has no
          points left for are filled with ``space.rvs`` points;
        * once a model exists, a greedy batch over the candidates of the last proposal: point 1 is ``ask()``; point
          j + 1 maximises the same acquisition on the same candidates, with the same hyper-posterior rows (PVRS: the same
          Thompson points), for the GPs conditioned on the training data plus the j chosen points with a fantasy
          observation ("lie"); points already chosen are excluded.  Hyper-parameters and the y normalisation stay fixed;
          a fantasy point has the noise a ``tell`` with noise 0 would give it (scalar alpha + the row's white level).
          ``strategy``: the lie is min / mean / max of ``yi`` ("cl_min" / "cl_mean" / "cl_max"), or each row's own
          posterior mean ("kb", kriging believer: the means stay, only the variances shrink).  PVRS / VR do not read y,
          so the strategy does not change their batches.  The averages follow ``evaluate_acquisitions``.  Any other
          whole-GP acquisition (``FullGPAcquisition``) is called itself on the conditioned median GP, with the
          generator state the proposal handed it.  ``n_points`` may not exceed the number of candidates.  This does not
          consume ``rng`` and changes nothing on the optimizer: asking twice gives the same list, and telling the first
          point alone continues exactly as after ``ask()``.  Sample acquisitions (Thompson sampling, "ts") have no
          batch form under these strategies.

        ``strategy="joint_ei" | "thompson"`` builds the batch, for every acquisition function, on ONE
        joint draw of ``n_paths`` posterior functions of ``n_features`` random features each
        (``gp.sample_paths(n_paths, sample_mean=False, ...)``: every path with its own hyper-posterior row) over the training
        inputs and the candidates of the last proposal, instead of on a lie: "joint_ei" adds, step by step, the candidate that
        raises the Monte-Carlo q-EI most, each path's incumbent being its own minimum over the training inputs (noisy EI);
        "thompson" gives step j to path j's minimiser among the candidates left.  Point 1 is ``ask()``, the other points are
        the greedy picks given it.  ``pending``: points (original space) that are being evaluated right now; with it only
        those points are taken as chosen -- a pending point that is a candidate row by its index, any other appended to the
        candidates --, no returned point is one of them, and ``n_points == 1`` still returns a single point.  The paths are
        seeded from a copy of ``rng``'s state: ``rng`` is not consumed and asking twice gives the same list.  Where
        ``sample_paths`` cannot run (input warping, generic kernel trees, more than 32 dimensions) its ``ValueError`` passes
        through.  ``pending`` with any other strategy is a ``ValueError``.
        """
        joint = strategy in JOINT_STRATEGIES
        if pending is not None and not joint:
            raise ValueError(f"pending points need a joint strategy {JOINT_STRATEGIES}, got {strategy!r}")
        if n_points > 1 and not joint and strategy not in BATCH_STRATEGIES:
            raise ValueError(f"strategy must be one of {BATCH_STRATEGIES + JOINT_STRATEGIES}, got {strategy!r}")
        if joint and (n_points > 1 or pending is not None) and self._n_initial_points <= 0 and self.gp.kernel_:
            points = self._ask_joint(n_points, strategy, pending, n_paths, n_features)
            return points if n_points > 1 else points[0]
        if n_points > 1:
            if self._n_initial_points > 0 or not self.gp.kernel_:
                return self._ask_design(n_points)
            return self._ask_batch(n_points, strategy)
        if self._n_initial_points <= 0:
            if not self.gp.kernel_:
                raise RuntimeError("Initialization is finished, but no model has been fit.")
            return self._next_x
        if self.init_strategy == "r2":
            return self._initial_points[self._n_initial_points - 1]
        if self.init_strategy != "sb":
            return self.space.rvs()[0]
        seen = len(self.Xi)
        design = sb_sequence(n=seen + 1, d=self.space.transformed_n_dims,
                             existing_points=self.space.transform(self.Xi) if seen else None,
                             random_state=self._init_rng.randint(2**31))
        return self.space.inverse_transform(np.atleast_2d(design[seen]))[0]

    def _ask_design(self, n_points):
        """The next ``n_points`` points of the initial design, topped up with ``space.rvs`` points."""
        k = min(max(self._n_initial_points, 0), n_points)
        points = []
        if k and self.init_strategy == "r2":
            points = [self._initial_points[self._n_initial_points - 1 - i] for i in range(k)]
        elif k and self.init_strategy == "sb":
            seen = len(self.Xi)
            design = sb_sequence(n=seen + k, d=self.space.transformed_n_dims,
                                 existing_points=self.space.transform(self.Xi) if seen else None,
                                 random_state=self._init_rng.randint(2**31))
            points = list(self.space.inverse_transform(np.atleast_2d(design[seen:])))
        elif k:
            points = list(self.space.rvs(n_samples=k))
        if len(points) < n_points:
            points += list(self.space.rvs(n_samples=n_points - len(points)))
        return points

    def _ask_batch(self, n_points, strategy):
        """Greedy fantasy batch over the last proposal (``BayesGPR._fantasy_batch``)."""
        if isinstance(self.acq_func, acquisition.SampleAcquisition):
            raise NotImplementedError("Batch proposals (n_points > 1) are not implemented for Thompson sampling "
                                      "or other sample acquisitions.")
        state = self._last_batch_state
        if self._last_candidates is None or state is None:
            raise RuntimeError("No proposal to extend: tell() has not fit a model and proposed a point yet.")
        cand, values = self._last_candidates, self._last_acq_values
        if n_points > len(cand):
            raise ValueError(f"n_points={n_points} exceeds the {len(cand)} candidates of a proposal (Optimizer.n_points)")
        lie = {"cl_min": np.min, "cl_mean": np.mean, "cl_max": np.max}.get(strategy)
        lie = None if lie is None else float(lie(self.yi))
        picks, step_values, path, info = self.gp._fantasy_batch(
            cand, int(np.argmax(values)), n_points, self.acq_func, state.get("rows"), state.get("n_samples", 0),
            self.acq_func_kwargs, lie, thompson=state.get("thompson", {}).get(0), replay=state.get("replay", {}).get(0),
            path=self._batch_path, want_moments=self._batch_moments)
        self._last_batch_info = dict(info, picks=picks, values=step_values, path=path)
        return [self.space.inverse_transform(cand[i].reshape((1, -1)))[0] for i in picks]

    def _ask_joint(self, n_points, strategy, pending, n_paths, n_features):
        """Batch on joint pathwise draws over the last proposal's candidates (``PosteriorPaths.select_batch``); a list."""
        if self._last_candidates is None:
            raise RuntimeError("No proposal to extend: tell() has not fit a model and proposed a point yet.")
        cand = self._last_candidates
        if pending is None:
            forced = [int(np.argmax(self._last_acq_values))]
        else:
            pend = self.space.transform([list(p) for p in pending]) if len(pending) else np.empty((0, cand.shape[1]))
            # a pending point is a candidate when it is the point ask() would return for that row, or transforms to the row itself
            known = {}
            for i, x in enumerate(self.space.inverse_transform(cand)):
                known.setdefault(tuple(x), i)
            forced, extra = [], []
            for x, row in zip(pending, np.atleast_2d(pend)):
                hit = [known[tuple(x)]] if tuple(x) in known else list(np.flatnonzero(np.all(cand == row[None, :], axis=1)))
                hit = [int(i) for i in hit if int(i) not in forced]
                if hit:
                    forced.append(hit[0])
                else:
                    forced.append(len(cand) + len(extra))
                    extra.append(row)
            if extra:
                cand = np.vstack([cand, np.asarray(extra, dtype=np.float64)])
        q = n_points - (1 if pending is None else 0)
        if q + len(forced) > len(cand):
            raise ValueError(f"n_points={n_points} exceeds the {len(cand)} candidates of a proposal (Optimizer.n_points)")
        clone = np.random.RandomState()
        clone.set_state(self.rng.get_state())
        with self.gp.sample_paths(n_paths=n_paths, sample_mean=False, n_features=n_features, random_state=clone) as paths:
            out = paths.select_batch(cand, q, kind="improvement" if strategy == "joint_ei" else "thompson",
                                     incumbent="paths", forced=forced, return_values=True)
        chosen = ([] if pending is not None else forced) + [int(i) for i in out["picks"]]
        self._last_batch_info = dict(picks=chosen, values=out["values"], incumbents=out["incumbents"], path="pathwise",
                                     forced=list(forced), candidates=cand)
        return [self.space.inverse_transform(cand[i].reshape((1, -1)))[0] for i in chosen]

    # ---- tell --------------------------------------------------------------------------------------------------
    def _record(self, x, y, noise_vector):
        """Append one observation (x a point, y a number) or a batch (x a list of points, y a list); returns how many
        were added.  Noise variances default to 0 and must match the shape of y (``bask/optimizer.py:298-329``)."""
        batch = is_listlike(y) and is_2Dlistlike(x)
        if not batch and not is_listlike(x):
            raise ValueError(f"Type of arguments `x` ({type(x)}) and `y` ({type(y)}) not compatible.")
        if batch:
            if noise_vector is None:
                noise_vector = [0.0] * len(y)
            elif not is_listlike(noise_vector) or len(noise_vector) != len(y):
                raise ValueError("Vector of noise variances needs to be of equal length as `y`.")
            xs, ys, noises = list(x), list(y), list(noise_vector)
        else:
            if is_listlike(noise_vector):
                raise ValueError("Vector of noise variances is a list, while tell only received one datapoint.")
            xs, ys, noises = [x], [y], [0.0 if noise_vector is None else noise_vector]
        self.Xi += xs
        self.yi += ys
        self.noisei += noises
        return len(ys)

    def _update_surrogate(self, from_scratch, gp_samples, gp_burnin, progress):
        """First model (or after ``replace``): MAP fit + MCMC (``BayesGPR.fit``); afterwards the walkers resume from
        their last positions on the grown data set (``BayesGPR.sample``) -- ``bask/optimizer.py:330-351``."""
        if self.gp_priors is not None and len(self.gp_priors) != self.space.transformed_n_dims + 2:
            raise ValueError("The number of priors does not match the number of dimensions + 2.")
        infer = self.gp.fit if (from_scratch or self.gp.pos_ is None) else self.gp.sample
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            infer(self.space.transform(self.Xi), self.yi, noise_vector=np.array(self.noisei), priors=self.gp_priors,
                  n_desired_samples=gp_samples, n_burnin=gp_burnin, progress=progress)

    def _propose(self, n_samples):
        """Maximise the acquisition function over ``n_points`` random candidates (uniform in the warped space when
        the surrogate warps its inputs, ``bask/optimizer.py:353-357``) on the device."""
        if self.gp.warp_inputs:
            cand = self.gp.unwarp(self.rng.uniform(size=(self.n_points, self.space.transformed_n_dims)))
        else:
            cand = self.space.rvs_transformed(n_samples=self.n_points, random_state=self.rng)
        record = {}
        values = evaluate_acquisitions(X=cand, gpr=self.gp, acquisition_functions=(self.acq_func,), n_samples=n_samples,
                                       progress=False, random_state=self.rng.randint(0, _INT32_MAX), _record=record,
                                       **self.acq_func_kwargs).ravel()
        self._last_candidates, self._last_acq_values, self._last_batch_state = cand, values, record
        return self.space.inverse_transform(cand[np.argmax(values)].reshape((1, -1)))[0]

    def tell(self, x, y, noise_vector=None, fit=True, replace=False, n_samples=0, gp_samples=100, gp_burnin=10,
             progress=False):
        """Record observation(s); once the initial design is used up (and ``fit``) update the hyper-posterior MCMC of
        the surrogate and choose the next point.  Arguments, return value (an ``OptimizeResult`` with ``x, fun,
        x_iters, func_vals, space, models``) and raised errors as ``bask/optimizer.py:228-380``."""
        if replace:
            self._forget_observations()
            self._n_initial_points = self.n_initial_points_
        self._n_initial_points -= self._record(x, y, noise_vector)
        if fit and self._n_initial_points <= 0:
            self._update_surrogate(replace, gp_samples, gp_burnin, progress)
            self._next_x = self._propose(n_samples)
        return self._result()

    def run(self, func, n_iter=1, replace=False, n_samples=5, gp_samples=100, gp_burnin=10):
        """``n_iter`` rounds of ask -> ``func`` -> tell; ``func`` returns the objective value or a (value, noise
        variance) pair; ``replace`` applies to the first round only (``bask/optimizer.py:382-445``)."""
        for it in range(n_iter):
            x = self.ask()
            outcome = func(x)
            value, noise = outcome if hasattr(outcome, "__len__") else (outcome, 0.0)
            self.tell(x, value, noise_vector=noise, replace=replace and it == 0, n_samples=n_samples,
                      gp_samples=gp_samples, gp_burnin=gp_burnin)
        return self._result()

    def expected_optimum(self, kappa=0.0, n_random_starts=100, random_state=None):
        """Where the optimum is right now: the minimiser of the surrogate mean (``kappa = 0``) or of the upper confidence bound
        ``mean + kappa std``, found on the device from the best observed point and ``n_random_starts`` random points
        (``utils.expected_optimum``).  Returns (x, value, info)."""
        return expected_optimum(self._result(), kappa=kappa, n_random_starts=n_random_starts, random_state=random_state)

    def partial_dependence(self, **kw):
        """What the surrogate looks like right now: 1-D curves and 2-D maps of its partial dependence
        (``utils.partial_dependence`` on the current result, same keyword arguments)."""
        return partial_dependence(self._result(), **kw)

    def active_subspace(self, **kw):
        """Which directions matter: the eigen-decomposition of the active-subspace matrix of the current surrogate
        (``utils.active_subspace`` on the current result, same keyword arguments)."""
        return active_subspace(self._result(), **kw)

    def sensitivity_indices(self, **kw):
        """Which dimensions matter and which interact: first-order, total and pair-interaction Sobol' indices of the current
        surrogate (``utils.sensitivity_indices`` on the current result, same keyword arguments)."""
        return sensitivity_indices(self._result(), **kw)

    def cross_validate(self, **kw):
        """Does the surrogate predict the observations it has not seen?  Held-out predictives of the training points, fold by fold,
        without a refit (``utils.cross_validate`` on the current result, same keyword arguments; the optimizer's own random state
        is not consumed)."""
        return cross_validate(self._result(), **kw)

    def predict_marginal(self, X, **kw):
        """What the surrogate predicts at points ``X`` of the original space once the kernel hyper-parameters are integrated out:
        mean, within / between spread, mixture quantiles, P(f <= at) and the log predictive density (``utils.predict_marginal`` on
        the current result, same keyword arguments; the optimizer's own random state is not consumed)."""
        return predict_marginal(self._result(), X, **kw)

    def _optimum_vs_space_draws(self, n_space_samples, n_gp_samples, n_random_starts, use_mean_gp, seed, minimizer="scipy"):
        """Function draws (device ``sample_y``) at [expected optimum, n_space_samples random points]:
        (1 + n_space_samples, n_gp_samples); row 0 belongs to the minimiser of the surrogate mean found by
        ``utils.expected_minimum`` (``bask/optimizer.py:493-512``).  ``seed`` is handed unchanged to each of the
        three consumers, as the reference does.  ``minimizer="device"``: the minimiser comes from ``utils.expected_optimum``."""
        if minimizer not in ("scipy", "device"):
            raise ValueError(f"minimizer must be 'scipy' or 'device', got {minimizer!r}")
        res = self._result()
        if minimizer == "device":
            x_opt = expected_optimum(res, n_random_starts=n_random_starts, random_state=seed)[0]
        else:
            x_opt, _ = expected_minimum(res, n_random_starts=n_random_starts, random_state=seed)
        points = [x_opt] + self.space.rvs(n_samples=n_space_samples, random_state=seed)
        return self.gp.sample_y(self.space.transform(points), sample_mean=use_mean_gp, n_samples=n_gp_samples,
                                random_state=seed)

    def probability_of_optimality(self, threshold, n_space_samples=500, n_gp_samples=200, n_random_starts=100,
                                  use_mean_gp=True, normalized_scores=True, random_state=None, minimizer="scipy"):
        """Probability that no point of the space beats the current expected optimum by more than
        ``threshold`` (a float, or a list giving a list of probabilities) -- ``bask/optimizer.py:447-525``,
        same arguments.  With ``normalized_scores`` the gaps are measured in units of each draw's standard
        deviation over the points.  ``minimizer``: "scipy" (``utils.expected_minimum``) or "device" (``utils.expected_optimum``)
        finds the expected optimum."""
        draws = self._optimum_vs_space_draws(n_space_samples, n_gp_samples, n_random_starts, use_mean_gp, random_state,
                                             minimizer=minimizer)
        gap = draws[0][None, :] - draws          # how much better every point is than the optimum, per draw
        if normalized_scores:
            gap = gap / np.std(draws, axis=0)
        worst = gap.max(axis=0)                  # the best competitor in each draw
        probs = [float(np.mean(worst - eps < 0.0)) for eps in (threshold if is_listlike(threshold) else [threshold])]
        return probs if is_listlike(threshold) and len(probs) > 1 else probs[0]

    def expected_optimality_gap(self, max_tries=3, n_probabilities=50, n_space_samples=500, n_gp_samples=200,
                                n_random_starts=100, tol=0.01, use_mean_gp=True, normalized_scores=True,
                                random_state=None, minimizer="scipy"):
        """Expected optimality gap of the current global optimum (``bask/optimizer.py:527-620``): the
        distribution function of the gap is sampled with ``probability_of_optimality`` on ``n_probabilities``
        thresholds between 0 and the smallest threshold at which the probability reaches 1 (found by a
        bounded scalar minimisation of ``(p - 1)^2 + 1e-3 t^2``, at most ``max_tries`` attempts)."""
        from scipy.optimize import minimize_scalar

        seed = check_random_state(random_state).randint(0, 2**32 - 1, dtype=np.int64)
        kw = dict(n_space_samples=n_space_samples, n_gp_samples=n_gp_samples, n_random_starts=n_random_starts,
                  use_mean_gp=use_mean_gp, normalized_scores=normalized_scores, random_state=seed, minimizer=minimizer)
        span = float(np.max(self.yi) - np.min(self.yi))
        upper = None
        for _ in range(max_tries):
            try:
                upper = minimize_scalar(
                    lambda t: (self.probability_of_optimality(threshold=t, **kw) - 1.0) ** 2 + 1e-3 * t * t,
                    bounds=(0.0, span), tol=tol).x
            except ValueError:
                continue
            break
        if upper is None:
            raise ValueError("Determining the upper threshold was not possible.")
        grid = np.linspace(0.0, upper, num=n_probabilities)
        cdf = np.asarray(self.probability_of_optimality(list(grid), **kw), dtype=np.float64)
        return float(np.sum(np.diff(cdf) * grid[1:]))

    def _optimum_samples_transformed(self, n_samples, only_mean, n_features, n_candidates, n_starts, random_state):
        """(locations (n_samples, d) in the transformed unit box, values (n_samples,) in y units) of ``optimum_samples``."""
        if self.space.is_partly_categorical:
            raise ValueError("optimum_samples does not support any categorical values")
        rng = check_random_state(random_state)
        with self.gp.sample_paths(n_paths=n_samples, sample_mean=only_mean, n_features=n_features, random_state=rng) as paths:
            out = paths.minimize(bounds=(0.0, 1.0), n_candidates=n_candidates, n_starts=n_starts, random_state=rng)
        return out["x"], out["fun"]

    def optimum_samples(self, n_samples=200, only_mean=True, n_features=1024, n_candidates=2000, n_starts=8, random_state=None):
        """Samples of the optimum: ``n_samples`` posterior function draws (``BayesGPR.sample_paths``; ``only_mean``: all of the
        median GP, otherwise one chain row each) and the continuous minimiser of every draw over the whole space, searched on
        the device from the draw's ``n_starts`` lowest of ``n_candidates`` uniform points (``PosteriorPaths.minimize``, DESIGN.md
        section 15).  ONE generator made from ``random_state`` serves ``sample_paths`` first, then the candidates.  Returns
        ``(X_opt, values)``: X_opt (n_samples, d) in the original space, un-rounded as ``expected_optimum``'s point, and the
        draws' minima (n_samples,) in y units.  ``ValueError`` where ``sample_paths`` raises it (warped inputs, generic kernel
        trees, more than 32 dimensions) and for partly categorical spaces."""
        Xt, values = self._optimum_samples_transformed(n_samples, only_mean, n_features, n_candidates, n_starts, random_state)
        return np.array([inverse_unrounded(self.space, xt) for xt in Xt]), values

    def optimum_intervals(self, hdi_prob=0.95, multimodal=True, opt_samples=200, space_samples=500, only_mean=True,
                          random_state=None, method="argmin"):
        """Highest density intervals of the optimum's location per dimension by Thompson sampling
        (``bask/optimizer.py:622-689``); ``utils.hdi`` restates the two arviz estimators.  ``method="argmin"`` (default): the
        reference's samples, the argmin row of every joint draw over ``space_samples`` random points.  ``method="pathwise"``:
        the continuous minimisers of ``opt_samples`` function draws (``optimum_samples`` with ``space_samples`` candidates per
        draw); where the pathwise draws cannot run (warped inputs, generic kernel trees, more than 32 dimensions) the call takes
        ``"argmin"`` and says so once on stderr."""
        if method not in ("argmin", "pathwise"):
            raise ValueError(f"method must be 'argmin' or 'pathwise', got {method!r}")
        if self.space.is_partly_categorical:
            raise NotImplementedError("Highest density interval not implemented for categorical parameters.")
        if method == "pathwise":
            why = self.gp._pathwise_obstacle()
            if why is None:
                X_opt, _ = self._optimum_samples_transformed(opt_samples, only_mean, 1024, space_samples,
                                                             min(8, space_samples), random_state)
                return self._intervals_of(X_opt, hdi_prob, multimodal)
            _intervals_tell_once(why)
        X = self.space.transform(self.space.rvs(n_samples=space_samples, random_state=random_state))
        optimum_samples = self.gp.sample_y(X, sample_mean=only_mean, n_samples=opt_samples, random_state=random_state)
        X_opt = X[np.argmin(optimum_samples, axis=0)]
        return self._intervals_of(X_opt, hdi_prob, multimodal)

    def _intervals_of(self, X_opt, hdi_prob, multimodal):
        intervals = []
        for i, col in enumerate(X_opt.T):
            raw_interval = hdi(col, hdi_prob=hdi_prob, multimodal=multimodal)
            intervals.append(self.space.dimensions[i].inverse_transform(raw_interval))
        return intervals


_intervals_told = []


def _intervals_tell_once(why):
    """One line on stderr, once per process: optimum_intervals(method="pathwise") asked for where the paths cannot run."""
    if not _intervals_told:
        _intervals_told.append(True)
        print("[bayes_skopt_amd] optimum_intervals(method='pathwise'): not available for %s; taking method='argmin'" % why,
              file=sys.stderr, flush=True)
