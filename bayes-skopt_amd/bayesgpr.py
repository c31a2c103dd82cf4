"""BayesGPR: fully Bayesian Gaussian-process regressor whose posterior arithmetic runs on the MI355X.

Host-side mirror of ``bask.BayesGPR`` (``bask/bayesgpr.py``): same constructor, ``fit`` / ``sample`` /
``predict`` / ``sample_y`` / ``theta`` / ``noise_set_to_zero`` surface and the same derived
quantities (walker count, step count, start ball, chain flattening, geometric median, warm start
through ``pos_``).  Everything numerical -- kernel matrices, Cholesky factorisations, solves, the
log-marginal likelihood evaluated for every MCMC proposal, predictive means / variances -- is done
by the HIP kernels behind the C-ABI (``include/bgp.h``); there is no CPU fallback.

Where the reference relies on inherited third-party code, the behaviour restated here is:
  * skopt's GaussianProcessRegressor.fit: append ``+ WhiteKernel()`` when ``noise="gaussian"``,
    MAP-fit theta, remember ``noise_``, replace the fitted WhiteKernel by ``WhiteKernel(0.0)`` in
    ``kernel_`` (so ``theta[-1] == -inf`` afterwards), keep factors that include the noise
    (SURVEY.md 2b, Appendix B.1);
  * sklearn's fit: y normalisation, L-BFGS-B on -LML from ``kernel_.theta`` within ``kernel_.bounds``
    (``sklearn/_gpr.py:296-341``) -- objective and gradient are evaluated on the device;
  * skopt's predict: ``var = diag - einsum(K*, K*, K_inv_)`` clipped at 0.
"""
import sys
import warnings
from contextlib import contextmanager, nullcontext

import numpy as np
import scipy.optimize
from sklearn.base import BaseEstimator, RegressorMixin, clone
from sklearn.utils import check_random_state

from . import _lib, distributed
from ._posterior import CanonicalPosterior, GramPosterior, noise_off, raise_if_not_pd, sobol_masks
from .crossval import check_folds, combine_rows, split_folds
from .kernels import ConstantKernel, WhiteKernel, analyse_kernel, param_for_white_kernel_in_sum
from .kernels import RBF as _RBF
from .sampler import EnsembleSampler
from .utils import geometric_median, guess_priors, validate_zeroone

__all__ = ["BayesGPR", "PosteriorPaths"]

MVN_MODES = ("auto", "reference", "cholesky", "pathwise")


class BayesGPR(RegressorMixin, BaseEstimator):
    """Gaussian process regressor of which the kernel hyper-parameters are inferred in a fully
    Bayesian framework (constructor arguments as ``bask/bayesgpr.py:148-159``).

    Extra, MI355X-specific keyword: ``device`` (HIP device ordinal, default 0),
    ``max_batch`` (matrices factorised concurrently; default = half the walkers) and ``mvn`` -- how
    ``sample_y`` turns a predictive mean / covariance into function draws:

    * ``"reference"``: mean and covariance come from the device, the draw is numpy's legacy
      ``RandomState.multivariate_normal`` (SVD) on the host, exactly what the reference does
      (``sklearn/_gpr.py:522-526`` behind ``bask/bayesgpr.py:669-718``): a seeded call returns the
      reference's own variates;
    * ``"cholesky"``: ``mean + chol(cov + jitter I) z`` entirely on the device (same distribution, other
      variates; the only practical choice for thousands of query points, where the SVD takes minutes);
    * ``"auto"`` (default): ``"reference"`` up to ``MVN_REFERENCE_MAX_POINTS`` (512) query points,
      ``"cholesky"`` beyond.  The generator is consumed identically in both modes.
    * ``"pathwise"`` (opt-in, never chosen by ``"auto"``): the draws are ``sample_paths(...)(X)`` -- Matheron's rule on random
      Fourier features, O(F + n) per query point and no m x m covariance: the mode for Thompson-type
      draws over thousands of candidates.  Same mean and covariance as ``predict``; a single path is Gaussian only in the
      limit of many features.  Where it cannot run (warped inputs, generic kernel trees, d > 32, ``noise=True``) the call
      takes what ``"auto"`` would take and says so once on stderr.

    ``resident_sampler`` (default True): ``sample`` / ``fit`` run the ensemble sampler with its walkers, proposals,
    log-priors, accept tests and chain resident on the device (``bgp_mcmc_begin_ex`` / ``_steps`` / ``_end``: no transfer
    between the first and the last half-step) whenever the kernel has a canonical device form and every prior is one of
    ``guess_priors``' two families or a frozen ``scipy.stats.norm`` (the default warp priors) -- with or without a progress
    bar, warped inputs, or an ensemble sharded over an RCCL group; the same moves as the host-driven loop, log-probabilities
    equal to ~1e-15 relative (the device's exp in the priors instead of numpy's).  A run that has to be driven from the
    host (custom priors, an odd ensemble, a generic kernel tree, a gloo group) says so once on stderr.
    """

    MVN_REFERENCE_MAX_POINTS = 512

    def __init__(
        self,
        kernel=None,
        alpha=1e-10,
        optimizer="fmin_l_bfgs_b",
        n_restarts_optimizer=0,
        normalize_y=False,
        warp_inputs=False,
        copy_X_train=True,
        random_state=None,
        noise="gaussian",
        device=0,
        max_batch=None,
        shard_ensemble=False,
        mvn="auto",
        resident_sampler=True,
    ):
        self._kernel = None if kernel is None else kernel.clone_with_theta(kernel.theta)
        self.kernel = kernel
        self.alpha = alpha
        self._alpha = alpha
        self.optimizer = optimizer
        self.n_restarts_optimizer = n_restarts_optimizer
        self.normalize_y = normalize_y
        self.warp_inputs = bool(warp_inputs)
        self.copy_X_train = copy_X_train
        self.random_state = check_random_state(random_state)
        self.noise = noise
        self.device = device
        self.max_batch = max_batch
        # exact single-ensemble sharding over the ranks of an initialised process group
        # (distributed.shard_log_prob; every rank must be constructed with the same random_state/data)
        self.shard_ensemble = bool(shard_ensemble)
        if mvn not in MVN_MODES:
            raise ValueError("mvn must be 'auto', 'reference', 'cholesky' or 'pathwise', got %r" % (mvn,))
        self.mvn = mvn
        # the ensemble sampler's whole run on the device (bgp_mcmc_run) where the priors and the kernel allow it; False: the
        # host-driven loop (one LML batch per half-step), whose priors are numpy's to the last bit
        self.resident_sampler = bool(resident_sampler)
        self._sampler = None
        self.chain_ = None
        self.pos_ = None
        self.kernel_ = None
        self.noise_ = None
        self._ctx_obj = None  # device context (ctypes handle; never pickled, rebuilt on demand)
        self._needs_rebuild = False
        self._plan = None
        self._backend = None  # _posterior.CanonicalPosterior | GramPosterior, chosen with the context
        self._post_theta = None  # theta the resident posterior (L_, alpha_, K_inv_) was built with
        self._L = self._K_inv = None
        self.alpha_ = None

    # ------------------------------------------------------------------ device plumbing
    @property
    def _ctx(self):
        """The device context.  After unpickling / deep-copying (the ctypes handle does not travel) it is
        rebuilt from the stored training data the first time something needs it."""
        if self._ctx_obj is None and self._needs_rebuild:
            self._needs_rebuild = False
            with self._keeping_posterior():
                self._ensure_context()
        return self._ctx_obj

    @_ctx.setter
    def _ctx(self, value):
        self._ctx_obj = value

    def __getstate__(self):
        state = dict(self.__dict__)
        state["_ctx_obj"] = None
        state["_sampler"] = None  # holds the bound (possibly rank-sharded) log-probability
        state["_backend"] = None  # (what it knows of the device does not travel: rebuilt with the context)
        state["_needs_rebuild"] = getattr(self, "_X_train_", None) is not None and self.kernel_ is not None
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)

    def _ensure_context(self, batch_hint=None):
        """(Re)create / update the device context for the current training set."""
        X, y = self._X_train_, self.y_train_
        alpha_diag = self._alpha_diag()
        plan = analyse_kernel(self.kernel_)
        want_batch = int(self.max_batch or batch_hint or getattr(self, "_batch_wish", None) or 64)
        ctx = self._ctx_obj
        if (ctx is None or ctx.d != X.shape[1] or ctx.form != plan.form or ctx.stationary != plan.stationary
                or ctx.max_batch < want_batch):
            if ctx is not None:
                ctx.close()
            ctx = _lib.Context(X, y, alpha_diag, form=plan.form, stationary=plan.stationary,
                               max_batch=max(want_batch, ctx.max_batch if ctx is not None else 0), device=self.device)
        else:
            ctx.update_data(X, y, alpha_diag)
        self._ctx, self._plan = ctx, plan
        self._backend = GramPosterior() if plan.generic else CanonicalPosterior()
        self._post_theta = None
        self._L = self._K_inv = None
        self._install_warp()
        return ctx

    def _alpha_diag(self):
        """The diagonal the device adds to K: ``alpha`` broadcast over the training points."""
        n = self._X_train_.shape[0]
        a = np.asarray(self.alpha, dtype=np.float64)
        a = a if np.iterable(self.alpha) else np.broadcast_to(a, (n,))
        if a.shape[0] != n:
            raise ValueError(f"alpha must be a scalar or an array with same number of entries as y. ({a.shape[0]} != {n})")
        return a

    @property
    def _post(self):
        """The posterior backend of the kernel (after an unpickle: rebuilt with the context first)."""
        self._ctx  # noqa: B018
        return self._backend

    def _warp_vector(self):
        """[wa_1..wa_d, wb_1..wb_d] of the current warpers, or None (identity)."""
        if self.warp_inputs and hasattr(self, "warp_alphas_"):
            return np.concatenate([self.warp_alphas_, self.warp_betas_])
        return None

    def _install_warp(self):
        """Make the device context see the training inputs (and later query points) through the current
        warpers -- the role of ``rewarp()`` in the reference (``bask/bayesgpr.py:284-295``)."""
        if self._ctx is not None:
            self._post_theta = None  # (first: a set_warp that raises leaves no posterior claimed under a warp it was not built with)
            self._L = self._K_inv = None
            self._backend.forget()
            self._ctx.set_warp(self._warp_vector())

    def _scratch_context(self):
        """A device context of its own on the training set, as large as the estimator's: what runs there leaves the estimator's
        context and its resident posteriors as they are."""
        return _lib.Context(self._X_train_, self.y_train_, self._alpha_diag(), form=self._plan.form,
                            stationary=self._plan.stationary, max_batch=self._ctx.max_batch, device=self.device)

    def _canonical(self, theta):
        return self._plan.canonical(theta, self._X_train_.shape[1])

    # ---- generic kernel expression trees (kernels.GramPlan; _posterior.GramPosterior): the kernel object on the host
    @property
    def _generic(self):
        return self._plan is not None and self._plan.generic

    def _kernel_at(self, theta):
        """The kernel object at ``theta`` (``kernel_.clone_with_theta``, sklearn/_gpr.py:571-576); log(0) noise levels pass."""
        with np.errstate(divide="ignore"):
            return self.kernel_.clone_with_theta(np.asarray(theta, dtype=np.float64))

    def _gram_stack(self, Thetas, X=None):
        """(B, n, n) stack of ``kernel(X_train)`` for every row of ``Thetas`` (no alpha: the device adds it)."""
        X = self.X_train_ if X is None else X
        return np.stack([self._kernel_at(t)(X) for t in np.atleast_2d(Thetas)])

    def _gram_lml(self, Thetas, Ws=None):
        """LML of every row (host kernel matrices, device factorisation).  ``Ws``: per-row input warps (B, 2d)."""
        Thetas = np.atleast_2d(Thetas)
        if Ws is None:
            K = self._gram_stack(Thetas)
        else:  # every walker sees the training inputs through its own Beta-CDF warp (bask/bayesgpr.py:353-365)
            K = np.stack([self._kernel_at(t)(self._ctx.beta_cdf(self._X_train_, w)) for t, w in zip(Thetas, Ws)])
        return self._ctx.lml_gram(K)

    def log_marginal_likelihood(self, theta=None, eval_gradient=False, clone_kernel=True):
        """``sklearn/_gpr.py:537-652`` on the device.  theta may be (p,) or a (B, p) block."""
        if theta is None:
            if eval_gradient:
                raise ValueError("Gradient can only be evaluated for theta!=None")
            return self.log_marginal_likelihood_value_
        theta = np.asarray(theta, dtype=np.float64)
        lml, grad = self._post.lml(self, np.atleast_2d(theta), eval_gradient)
        if theta.ndim == 1:
            return (float(lml[0]), grad[0]) if eval_gradient else float(lml[0])
        return (lml, grad) if eval_gradient else lml

    # ------------------------------------------------------------------ theta / posterior
    @property
    def theta(self):
        """Current (geometric-median) kernel hyper-parameters in log space
        (``bask/bayesgpr.py:182-198``)."""
        if self.kernel_ is not None:
            with np.errstate(divide="ignore"):
                return np.copy(self.kernel_.theta)
        return None

    @theta.setter
    def theta(self, theta):
        """Posterior build, ``bask/bayesgpr.py:200-217``: K, L_, K_inv_, alpha_ on the device."""
        theta = np.asarray(theta, dtype=np.float64)
        self.kernel_.theta = theta
        self._build_posterior(theta)

    def _build_posterior(self, theta):
        self.alpha_ = self._post.posterior(self, theta)
        self._post_theta = np.array(theta, copy=True)
        self._L = self._K_inv = None

    @contextmanager
    def _keeping_posterior(self, undo=None):
        """The one keeper of the median GP's bookkeeping: what the block does may forget it (a rebuilt
        context, another row's warp) although the median GP has not changed; on exit, however the block is left, ``undo()`` runs
        and then ``_post_theta`` / ``alpha_`` / ``L_`` / ``K_inv_`` are back.  An ``undo`` that raises leaves them forgotten."""
        saved = (self._post_theta, self.alpha_, self._L, self._K_inv)
        try:
            yield
        finally:
            if undo is not None:
                undo()
            self._post_theta, self.alpha_, self._L, self._K_inv = saved

    def _require_posterior(self, what="predict"):
        if self._post_theta is None or getattr(self, "_X_train_", None) is None:
            raise RuntimeError(what + " before fit is not supported on the MI355X path")

    def _y_scale(self):
        """(mean, std) of the y normalisation as two floats."""
        return float(np.ravel(self.y_train_mean_)[0]), float(np.ravel(self.y_train_std_)[0])

    def _fetch_factor(self, which):
        if self._post_theta is None:
            raise AttributeError("no posterior has been built yet")
        return self._post.factor(self, which)

    @property
    def L_(self):
        """Lower Cholesky factor of the kernel matrix (fetched from the device on demand)."""
        if self._L is None:
            self._L = self._fetch_factor("L")
        return self._L

    @L_.setter
    def L_(self, value):
        self._L = value

    @property
    def K_inv_(self):
        """Explicit inverse K^-1 (``bask/bayesgpr.py:207-208``), fetched on demand."""
        if self._K_inv is None:
            self._K_inv = self._fetch_factor("K_inv")
        return self._K_inv

    @K_inv_.setter
    def K_inv_(self, value):
        self._K_inv = value

    @property
    def X_train_(self):
        """Training inputs; the WARPED ones when ``warp_inputs`` and warpers exist
        (``bask/bayesgpr.py:219-235``)."""
        X = getattr(self, "_X_train_", None)
        if X is not None and self.warp_inputs and hasattr(self, "warp_alphas_") and self._ctx is not None:
            return self.warp(X)
        return X

    @X_train_.setter
    def X_train_(self, X_train):
        X_train = np.asarray(X_train, dtype=np.float64)
        self._X_train_ = np.copy(X_train) if self.copy_X_train else X_train

    # ------------------------------------------------------------------ input warping
    def warp(self, X):
        """Beta-CDF warp of X with the current warpers, evaluated on the device; identity when
        ``warp_inputs=False`` or before the first fit (``bask/bayesgpr.py:249-264``)."""
        w = self._warp_vector()
        if w is None or self._ctx is None:
            return X
        return self._ctx.beta_cdf(np.atleast_2d(np.asarray(X, dtype=np.float64)), w)

    def unwarp(self, X):
        """Inverse warp (Beta quantile function per column, ``bask/bayesgpr.py:266-282``).  Only used to
        GENERATE candidate points (``bask/optimizer.py:353-357``); host-side scipy."""
        if not (self.warp_inputs and hasattr(self, "warp_alphas_")):
            return X
        import scipy.stats as st

        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        out = np.empty_like(X)
        for col, (a_log, b_log) in enumerate(zip(self.warp_alphas_, self.warp_betas_)):
            out[:, col] = st.beta(a=np.exp(a_log), b=np.exp(b_log)).ppf(X[:, col])
        return out

    def rewarp(self):
        """Apply the current warpers to the resident training inputs again."""
        if self.warp_inputs:
            self._install_warp()

    def create_warpers(self, alphas, betas):
        """Set the Beta-CDF parameters (log space) of every input column
        (``bask/bayesgpr.py:297-316``).  ``warpers_`` / ``unwarpers_`` are kept as host callables for
        API compatibility; the device evaluates the warp itself."""
        if self.warp_inputs:
            import scipy.stats as st

            self.warp_alphas_ = np.copy(np.asarray(alphas, dtype=np.float64))
            self.warp_betas_ = np.copy(np.asarray(betas, dtype=np.float64))
            dists = [st.beta(a=np.exp(a), b=np.exp(b)) for a, b in zip(self.warp_alphas_, self.warp_betas_)]
            self.warpers_ = [dist.cdf for dist in dists]
            self.unwarpers_ = [dist.ppf for dist in dists]

    @contextmanager
    def noise_set_to_zero(self):
        """Context in which kernel_'s white-noise level is 0 WITHOUT recomputing alpha_ / L_ /
        K_inv_ (``bask/bayesgpr.py:318-336``)."""
        current_theta = self.theta
        try:
            present, white_param = param_for_white_kernel_in_sum(self.kernel_)
            self.kernel_.set_params(**{white_param: WhiteKernel(noise_level=0.0)})
            yield self
        finally:
            self.kernel_.theta = current_theta

    def _apply_noise_vector(self, n_instances, noise_vector):
        """``bask/bayesgpr.py:338-349``."""
        if noise_vector is not None:
            base = self.alpha if not np.iterable(self.alpha) else self._alpha
            if np.iterable(base):
                raise ValueError("alpha passed to the constructor must be a scalar when a noise_vector is used")
            alpha = np.ones(n_instances) * base
            alpha[: len(noise_vector)] += noise_vector
            self.alpha = alpha

    # ------------------------------------------------------------------ log posterior
    def _log_prob_batch(self, Theta, priors, warp_priors=None):
        """Vectorised ``_log_prob_fn`` (``bask/bayesgpr.py:351-379``): sum of priors (host) + LML
        (device) for a (Ns, p) block; non-finite -> -inf.  With ``warp_inputs`` the last 2d columns are
        the Beta-CDF parameters of each walker's own input warp (``:353-365``)."""
        return self._log_prob_finish(self._log_prob_begin(Theta, priors, warp_priors))

    def _log_prob_begin(self, Theta, priors, warp_priors=None):
        """First half of ``_log_prob_batch``: put the block's LML batch on the device and return at once with the
        priors of the same block (evaluated while the device factorises)."""
        Theta = np.atleast_2d(Theta)
        d = self._X_train_.shape[1] if self.warp_inputs else 0
        Tgp, W = (Theta[:, : Theta.shape[1] - 2 * d], Theta[:, Theta.shape[1] - 2 * d :]) if d else (Theta, None)
        pending = self._post.lml_begin(self, Tgp, W)
        try:
            lp = _eval_priors(priors, Tgp)
            if W is not None:
                lp = lp + _eval_warp_priors(warp_priors, W, d)
        except BaseException:
            if pending.submitted:
                self._ctx.lml_wait()
            raise
        return lp, pending

    def _log_prob_finish(self, token):
        lp, pending = token
        lml = self._post.lml_finish(self, pending)
        with np.errstate(invalid="ignore"):
            lp = lp + lml
        lp[~np.isfinite(lp)] = -np.inf
        return lp

    def _log_prob_fn(self, x, priors, warp_priors=None):
        return float(self._log_prob_batch(np.asarray(x, dtype=np.float64)[None, :], priors, warp_priors)[0])

    # ------------------------------------------------------------------ sample
    def sample(
        self,
        X=None,
        y=None,
        noise_vector=None,
        n_threads=1,
        n_desired_samples=100,
        n_burnin=0,
        n_thin=1,
        n_walkers_per_thread=100,
        progress=False,
        priors=None,
        warp_priors=None,
        position=None,
        add=False,
        **kwargs,
    ):
        """Sample the hyper-parameter posterior with the ensemble sampler
        (``bask/bayesgpr.py:381-548``; same arguments and derived quantities)."""
        if (X is None and self.X_train_ is None) or self.kernel_ is None:
            raise ValueError(
                "It looks like you are trying to sample from the GP posterior without data. "
                "Pass X and y, or ensure that you call fit before sample."
            )
        if priors is None:
            priors = guess_priors(self.kernel_)
        if warp_priors is None:
            import scipy.stats as st

            warp_priors = (st.norm(loc=0.0, scale=0.3).logpdf, st.norm(loc=0.0, scale=0.3).logpdf)

        if X is not None:
            X = np.asarray(X, dtype=np.float64)
            y = np.asarray(y, dtype=np.float64)
            if self.normalize_y:
                self._y_train_mean = np.mean(y, axis=0)
                self._y_train_std = np.std(y, axis=0)
            else:
                self._y_train_mean = np.zeros(1)
                self._y_train_std = 1
            self.y_train_std_ = self._y_train_std
            self.y_train_mean_ = self._y_train_mean
            y = (y - self.y_train_mean_) / self.y_train_std_
            if noise_vector is not None:
                noise_vector = np.array(noise_vector) / np.power(self.y_train_std_, 2)
            self.X_train_ = X
            self.y_train_ = np.copy(y) if self.copy_X_train else y

        self._apply_noise_vector(len(self.y_train_), noise_vector)

        n_dim = len(self.theta)
        n_walkers = n_threads * n_walkers_per_thread
        n_samples = int(np.ceil(n_desired_samples / n_walkers) + n_burnin)
        pos = None
        if position is not None:
            pos = position
        elif self.pos_ is not None:
            pos = self.pos_
        n_theta = n_dim
        if self.warp_inputs:
            added_dims = self._X_train_.shape[1] * 2
            n_dim += added_dims
        if pos is None:
            theta = self.theta
            theta[np.isinf(theta)] = np.log(self.noise_)
            if self.warp_inputs:
                theta = np.concatenate([theta, np.zeros(added_dims)])
            pos = [theta + 1e-2 * self.random_state.randn(n_dim) for _ in range(n_walkers)]

        if self.shard_ensemble:  # every rank must propose the same blocks: pin the start ensemble to rank 0's
            pos = distributed.broadcast_array(np.asarray(pos, dtype=np.float64))
        self._ensure_context(batch_hint=(n_walkers + 1) // 2)
        self._sampler = EnsembleSampler(
            nwalkers=n_walkers,
            ndim=n_dim,
            log_prob_fn=_ShardedLogProb(self) if self.shard_ensemble else _AsyncLogProb(self),
            kwargs=dict(priors=priors, warp_priors=warp_priors),
            threads=n_threads,
            **kwargs,
        )
        rng = np.random.RandomState(self.random_state.randint(0, np.iinfo(np.int32).max))
        self._sampler.random_state = rng.get_state()
        pos, prob, state = self._sampler.run_mcmc(pos, n_samples, progress=progress)
        chain = self._sampler.get_chain(flat=True, discard=n_burnin, thin=n_thin)
        if add and self.chain_ is not None:
            self.chain_ = np.concatenate([self.chain_, chain])
        else:
            self.chain_ = chain
        if self.warp_inputs:
            median = geometric_median(self.chain_)
            d = self._X_train_.shape[1]
            warp_params = median[n_theta:]
            self.create_warpers(warp_params[:d], warp_params[d:])
            self.rewarp()
            self.theta = median[:n_theta]
        else:
            self.theta = geometric_median(self.chain_)
        self.log_marginal_likelihood_value_ = self.log_marginal_likelihood(self.kernel_.theta, clone_kernel=False)
        self.pos_ = pos

    # ------------------------------------------------------------------ fit
    def fit(
        self,
        X,
        y,
        noise_vector=None,
        n_threads=1,
        n_desired_samples=100,
        n_burnin=10,
        n_walkers_per_thread=100,
        progress=True,
        priors=None,
        warp_priors=None,
        position=None,
        **kwargs,
    ):
        """MAP initialisation (L-BFGS-B on the device LML) followed by ``sample``
        (``bask/bayesgpr.py:550-620``)."""
        self.kernel = self._kernel
        X = np.asarray(X, dtype=np.float64)
        y = np.asarray(y, dtype=np.float64)
        if self.normalize_y and noise_vector is not None:
            y_std = np.std(y, axis=0)
            noise_vector = np.array(noise_vector) / np.power(y_std, 2)
        self._apply_noise_vector(len(y), noise_vector)
        # the context the MAP start creates is the one the sampler wants (a second allocation of the matrix workspace otherwise:
        # 2 x 15 ms + 5 ms of release at n = 2048 x 128 matrices, tools/fit_cprofile.py)
        self._batch_wish = max(64, (int(n_threads) * int(n_walkers_per_thread) + 1) // 2)  # (64: the default without a wish)
        self._map_fit(X, y)
        self.sample(
            n_threads=n_threads,
            n_desired_samples=n_desired_samples,
            n_burnin=n_burnin,
            n_walkers_per_thread=n_walkers_per_thread,
            progress=progress,
            priors=priors,
            warp_priors=warp_priors,
            position=position,
            add=False,
            **kwargs,
        )
        return self

    def _map_fit(self, X, y):
        """skopt GPR.fit -> sklearn GPR.fit restated (module docstring) with device LML/gradient."""
        if isinstance(self.noise, str) and self.noise != "gaussian":
            raise ValueError("expected noise to be 'gaussian', got %s" % self.noise)
        if self.kernel is None:
            self.kernel = ConstantKernel(1.0, constant_value_bounds="fixed") * _RBF(1.0, length_scale_bounds="fixed")
        if self.noise and not param_for_white_kernel_in_sum(self.kernel)[0]:
            if self.noise == "gaussian":
                self.kernel = self.kernel + WhiteKernel()
            else:
                self.kernel = self.kernel + WhiteKernel(noise_level=self.noise, noise_level_bounds="fixed")
        self.kernel_ = clone(self.kernel)

        if self.normalize_y:
            self._y_train_mean = np.mean(y, axis=0)
            std = np.std(y, axis=0)
            self._y_train_std = 1.0 if std == 0.0 else std  # _handle_zeros_in_scale
            y = (y - self._y_train_mean) / self._y_train_std
        else:
            self._y_train_mean = np.zeros(1)
            self._y_train_std = np.ones(1)
        if np.iterable(self.alpha) and np.shape(self.alpha)[0] != y.shape[0]:
            if np.shape(self.alpha)[0] == 1:
                self.alpha = self.alpha[0]
            else:
                raise ValueError(
                    "alpha must be a scalar or an array with same number of "
                    f"entries as y. ({np.shape(self.alpha)[0]} != {y.shape[0]})"
                )
        self.X_train_ = X
        self.y_train_ = np.copy(y) if self.copy_X_train else y
        self.y_train_std_ = self._y_train_std
        self.y_train_mean_ = self._y_train_mean
        self._ensure_context()

        if self.optimizer is not None and self.kernel_.n_dims > 0:
            def obj(theta):
                lml, grad = self.log_marginal_likelihood(theta, eval_gradient=True, clone_kernel=False)
                return -lml, -grad

            optima = [self._constrained_optimization(obj, self.kernel_.theta, self.kernel_.bounds)]
            if self.n_restarts_optimizer > 0:
                bounds = self.kernel_.bounds
                if not np.isfinite(bounds).all():
                    raise ValueError(
                        "Multiple optimizer restarts (n_restarts_optimizer>0) requires that all bounds are finite."
                    )
                for _ in range(self.n_restarts_optimizer):
                    theta_initial = self.random_state.uniform(bounds[:, 0], bounds[:, 1])
                    optima.append(self._constrained_optimization(obj, theta_initial, bounds))
            vals = [o[1] for o in optima]
            self.kernel_.theta = optima[int(np.argmin(vals))][0]
            self.log_marginal_likelihood_value_ = -np.min(vals)
        else:
            self.log_marginal_likelihood_value_ = self.log_marginal_likelihood(self.kernel_.theta)

        # factors built WITH the fitted noise ...
        self._build_posterior(self.kernel_.theta)
        # ... then kernel_'s WhiteKernel is zeroed (skopt's post-fit step)
        self.noise_ = None
        if self.noise:
            if isinstance(self.kernel_, WhiteKernel):
                self.kernel_.set_params(noise_level=0.0)
            else:
                present, white_param = param_for_white_kernel_in_sum(self.kernel_)
                if present:
                    self.noise_ = self.kernel_.get_params()[white_param].noise_level
                    self.kernel_.set_params(**{white_param: WhiteKernel(noise_level=0.0)})

    def _constrained_optimization(self, obj_func, initial_theta, bounds):
        if self.optimizer == "fmin_l_bfgs_b":
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res = scipy.optimize.minimize(obj_func, initial_theta, method="L-BFGS-B", jac=True, bounds=bounds)
            return res.x, res.fun
        if callable(self.optimizer):
            return self.optimizer(obj_func, initial_theta, bounds=bounds)
        raise ValueError(f"Unknown optimizer {self.optimizer}.")

    # ------------------------------------------------------------------ predict
    def _kernel_theta_for_predict(self):
        with np.errstate(divide="ignore"):
            return np.copy(self.kernel_.theta)

    def predict(self, X, return_std=False, return_cov=False, return_mean_grad=False, return_std_grad=False):
        """Predictive mean [, std | cov] (``bask/bayesgpr.py:622-635`` -> skopt predict)."""
        if return_std and return_cov:
            raise RuntimeError("Not returning standard deviation of predictions when returning full covariance.")
        if return_std_grad and not return_std:
            raise ValueError("Not returning std_gradient without returning the std.")
        if return_std_grad and not return_mean_grad:
            raise ValueError("Not returning std_gradient without returning the mean_gradient.")
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        if return_mean_grad and X.shape[0] > 1:
            raise NotImplementedError("Not implemented for n_samples > 1")
        if self.warp_inputs:
            validate_zeroone(X)  # the device warps the query points with the context-level warp
        self._require_posterior()
        mean, var, cov = self._post.predict(self, X, return_cov)
        y_mean = self.y_train_std_ * mean[0] + self.y_train_mean_
        if return_cov:
            return y_mean, cov[0] * self.y_train_std_**2
        y_std = np.sqrt(var[0] * self.y_train_std_**2)
        if return_mean_grad:
            grad_mean, grad_std = self._predict_gradients(X[0], y_std, return_std_grad)
            if return_std_grad:
                return y_mean, y_std, grad_mean, grad_std
            return (y_mean, y_std, grad_mean) if return_std else (y_mean, grad_mean)
        return (y_mean, y_std) if return_std else y_mean

    def _predict_gradients(self, x, y_std, want_std_grad):
        """Gradients of the predictive mean / std at ONE query point (skopt's
        ``GaussianProcessRegressor.predict(return_mean_grad, return_std_grad)``, the routine
        ``bask/bayesgpr.py:633`` forwards to): ``grad = kernel_.gradient_x(x, X_train_)`` (n, d),
        ``grad_mean = grad^T alpha_``, ``grad_std = -K_* K_inv_ grad / std``.  O(n d) + one O(n^2) product on
        the host from the device-built ``alpha_`` / ``K_inv_``; with input warping the derivative is with
        respect to the warped coordinates, as in the reference."""
        Xt = self.X_train_
        if self.warp_inputs:
            x = self.warp(x[None, :])[0]
        grad, k_trans = self._post.grad_x(self, x, Xt)
        grad_mean = (grad.T @ self.alpha_) * self.y_train_std_
        if not want_std_grad:
            return grad_mean, None
        grad_std = np.zeros(Xt.shape[1])
        if not np.allclose(y_std, 0.0):
            grad_std = -(k_trans @ (self.K_inv_ @ grad)) / y_std[0] * self.y_train_std_**2
        return grad_mean, grad_std

    def predict_gradients(self, X, return_std=True):
        """Predictive mean, std and their gradients at ANY number of query rows: ``(mean (m,), std (m,), grad_mean (m, d),
        grad_std (m, d))`` in y units, or ``(mean, grad_mean)`` with ``return_std=False`` -- what
        ``predict(x, return_std=True, return_mean_grad=True, return_std_grad=True)`` returns one point at a time (the reference
        raises for more than one row, and so does ``predict``).  Same normalisation, and the same rule for a vanishing std:
        where ``std <= 1e-8`` (``np.allclose(std, 0)``) ``grad_std`` is zero.  Canonical kernels in up to 32 dimensions without
        input warping: one device call for all rows (``bgp_predict_grad_batch``).  Warped inputs and
        generic kernel trees: the one-point routine row by row, with its results."""
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        if self.warp_inputs:
            validate_zeroone(X)
        self._require_posterior()
        if not (self._post.canonical and self._post.device_gradients(self)):
            rows = [self.predict(x[None, :], return_std=return_std, return_mean_grad=True, return_std_grad=return_std) for x in X]
            if return_std:
                return (np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]),
                        np.stack([r[2] for r in rows]), np.stack([r[3] for r in rows]))
            return np.concatenate([r[0] for r in rows]), np.stack([r[1] for r in rows])
        mean, var, dmean, dvar = self._post.predict_grad(self, X, want_dvar=return_std)
        y_mean = self.y_train_std_ * mean + self.y_train_mean_
        grad_mean = dmean * self.y_train_std_
        if not return_std:
            return y_mean, grad_mean
        y_std = np.sqrt(var * self.y_train_std_**2)
        grad_std = np.zeros_like(dvar)
        nz = ~(np.abs(y_std) <= 1e-8)  # (np.allclose(std, 0.0) of the one-point routine, row by row)
        grad_std[nz] = dvar[nz] / (2.0 * y_std[nz])[:, None] * self.y_train_std_**2
        return y_mean, y_std, grad_mean, grad_std

    def partial_dependence(self, Xs, grids, panels=None, thetas=None, return_path=False):
        """Partial dependence of the predictive mean: per panel the mean averaged over the sample rows ``Xs`` (S, d; transformed
        space) with the panel's coordinates replaced by grid values -- ``grids``: one 1-D array per dimension (transformed space, at
        most 256 values), ``panels``: ``k`` / ``(k,)`` / ``(k, -1)`` for a curve, ``(k1, k2)`` for a map, None for every dimension
        and every pair k1 < k2.  Returns a list with one array per panel, (G1,) or (G1, G2) in y units, for the median GP
        (``thetas=None``), or (B, G1) / (B, G1, G2) for a block of B chain rows.  Canonical kernels in up to 32 dimensions: ONE
        device call for all panels and rows (``bgp_partial_dependence``; the context-level warp of
        ``warp_inputs`` is applied to samples and grids on the device).  Generic kernel trees, more dimensions, and chain rows
        under ``warp_inputs``: ``predict`` on synthesised rows, said once on stderr.  ``return_path``: also "device" | "host"."""
        Xs = np.atleast_2d(np.asarray(Xs, dtype=np.float64))
        self._require_posterior()
        d = self._X_train_.shape[1]
        grids = [np.asarray(g, dtype=np.float64).reshape(-1) for g in grids]
        if Xs.shape[1] != d or len(grids) != d:
            raise ValueError(f"sample rows need {d} columns and one grid per dimension is needed")
        if self.warp_inputs:
            validate_zeroone(Xs)
            validate_zeroone(np.concatenate(grids))
        if panels is None:
            panels = [(k, -1) for k in range(d)] + [(a, b) for a in range(d) for b in range(a + 1, d)]
        pan = []
        for pnl in panels:
            pnl = tuple(int(v) for v in np.atleast_1d(pnl))
            pnl = (pnl[0], pnl[1] if len(pnl) > 1 else -1)
            if not (0 <= pnl[0] < d and -1 <= pnl[1] < d and pnl[0] != pnl[1]):
                raise ValueError(f"panel {pnl} is not a dimension or a pair of two different dimensions of {d}")
            pan.append(pnl)
        if not pan or Xs.shape[0] < 1 or any(not 1 <= len(g) <= 256 for g in grids):
            raise ValueError("partial_dependence needs a panel, a sample row and 1 .. 256 grid values per dimension")
        vals, path = self._post.partial_dependence(self, thetas, Xs, grids, pan)
        vals = [self.y_train_std_ * v + self.y_train_mean_ for v in vals]
        if thetas is None:
            vals = [v[0] for v in vals]
        return (vals, path) if return_path else vals

    def sensitivity(self, A, Bm, terms=None, thetas=None, return_path=False):
        """Variance-based (Sobol') sensitivity of the predictive mean by the pick-freeze design: ``A``, ``Bm`` are two independent
        sample matrices (N, d; transformed space), ``terms`` a list of dimensions or tuples of dimensions (default: every single
        dimension; the empty tuple and all dimensions are legal).  Returns ``(mean, variance, closed, total)`` in y units: the
        mean and the variance of the surrogate over the 2N rows and, per term, the closed effect (Saltelli et al. 2010: the
        variance explained by the term's dimensions alone, first order for one dimension) and the total effect (Jansen 1999:
        everything those dimensions take part in); the indices are ``closed / variance`` and ``total / variance``.  Scalars and
        (T,) arrays for the median GP (``thetas=None``), (B,) and (B, T) for a block of B chain rows.  Canonical kernels in up
        to 32 dimensions: ONE device call for all terms and rows (``bgp_sobol_indices``; the context-level
        warp of ``warp_inputs`` is applied to both matrices on the device).  Generic kernel trees, more dimensions, and chain
        rows under ``warp_inputs``: ``predict`` on synthesised rows, said once on stderr.  ``return_path``: also "device" |
        "host"."""
        A, Bm = np.atleast_2d(np.asarray(A, dtype=np.float64)), np.atleast_2d(np.asarray(Bm, dtype=np.float64))
        self._require_posterior()
        d = self._X_train_.shape[1]
        if A.shape[1] != d or Bm.shape != A.shape or A.shape[0] < 1:
            raise ValueError(f"A and Bm must both be (N, {d}) with N >= 1, got {A.shape} and {Bm.shape}")
        if self.warp_inputs:
            validate_zeroone(A)
            validate_zeroone(Bm)
        masks = sobol_masks([(k,) for k in range(d)] if terms is None else terms, d)
        (f0, V, closed, total), path = self._post.sensitivity(self, thetas, A, Bm, masks)
        y_mean, y_std = self._y_scale()
        out = (y_std * f0 + y_mean, y_std**2 * V, y_std**2 * closed, y_std**2 * total)
        if thetas is None:
            out = tuple(v[0] for v in out)
        return (*out, path) if return_path else out

    def _gradient_cov(self, X, thetas, want):
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        self._require_posterior()
        d = self._X_train_.shape[1]
        if X.shape[1] != d or X.shape[0] < 1:
            raise ValueError(f"the points must be (m, {d}) with m >= 1, got {X.shape}")
        return self._post.gradient_cov(self, thetas, X, want)

    def gradient_posterior(self, X, thetas=None, return_path=False):
        """The posterior distribution of the gradient of the latent function at the rows of ``X`` (m, d; transformed space):
        ``(grad_mean (m, d), grad_cov (m, d, d))`` in y units per unit of the transformed coordinate -- grad f(x) is normal with
        that mean (the ``grad_mean`` of ``predict_gradients``) and that covariance (exactly symmetric, diagonal clipped at 0), so
        ``grad_mean[:, k] / sqrt(grad_cov[:, k, k])`` says whether the slope in dimension k is distinguishable from zero.  For the
        median GP (``thetas=None``), or (B, m, d) and (B, m, d, d) for a block of B chain rows.  Canonical kernels in up to 32
        dimensions: ONE device call (``bgp_grad_cov``); more dimensions: numpy on the downloaded inverse,
        said once on stderr.  Matern 1/2 is not differentiable: ValueError.  Generic kernel trees and ``warp_inputs=True``:
        NotImplementedError.  ``return_path``: also "device" | "host"."""
        (dmean, cov, _), path = self._gradient_cov(X, thetas, (True, True, False))
        y_std = self._y_scale()[1]
        out = (y_std * dmean, y_std**2 * cov)
        if thetas is None:
            out = tuple(v[0] for v in out)
        return (*out, path) if return_path else out

    def active_subspace(self, Xs, thetas=None, return_path=False):
        """The two parts of the active-subspace matrix ``C = E_x[grad f grad f^T]`` over the sample rows ``Xs`` (m, d; transformed
        space): ``(C_mean, C_cov)``, the average of ``grad_mean grad_mean^T`` and of ``grad_cov`` (``gradient_posterior``), each
        (d, d) in y units squared per unit of transformed coordinate squared, or (B, d, d) for a block of B chain rows.  On the
        device path only the two sums come back.  Paths and refusals as ``gradient_posterior``."""
        (_, _, csum), path = self._gradient_cov(Xs, thetas, (False, False, True))
        y_std = self._y_scale()[1]
        out = (y_std**2 * csum[:, 0], y_std**2 * csum[:, 1])
        if thetas is None:
            out = tuple(v[0] for v in out)
        return (*out, path) if return_path else out

    def cross_validate(self, folds=None, n_folds=None, thetas=None, weights="is", random_state=None):
        """Does the surrogate predict the data it has not seen?  For every fold F of training indices, the predictive of the
        held-out OBSERVATIONS ``y_F`` given the remaining points -- without a refit: it follows from the resident ``K^-1`` and
        ``alpha`` alone (``bgp_cross_validate``), so canonical kernels, generic kernel trees and warped
        inputs are served alike.  The hyper-parameters stay those fitted on ALL points.  The predictive is that of the
        observation: its std includes the white level and the point's own ``alpha`` (``noise_vector``), which ``predict``'s
        std does not.

        ``folds``: a list of disjoint index arrays (1 .. 128 points each; they need not cover every point); ``n_folds=K``: a
        shuffled split into K near-equal folds seeded by ``random_state``; neither: leave-one-out.  ``thetas=None``: the median
        GP, as ``predict`` uses it; a (B, p) block of chain rows (under ``warp_inputs`` the rows carry their warps, as
        ``chain_`` holds them): every row's predictive, built ``max_batch`` rows at a time, and their combination --
        ``weights="is"``: rows weighted per fold by ``1 / p(y_F | y_-F, theta_b)``, the importance weights that carry the
        hyper-posterior from ``p(theta | y)`` to ``p(theta | y_-F)`` (``fold_lpd = -log mean_b exp(-lpd_bF)``); ``"equal"``:
        the plug-in mixture (``fold_lpd = log mean_b exp(lpd_bF)``).  With one row both coincide.

        Returns a dict, everything in y units: ``folds``; ``row_mean``, ``row_std`` (B, n) and ``row_fold_lpd`` (B, K) per row;
        the combined ``mean``, ``std``, ``point_lpd``, ``z = (y - mean) / std`` (n,; NaN where no fold covers the point),
        ``fold_lpd`` (K,; log density of the whole fold, correlations included), ``elpd = sum(fold_lpd)`` and the effective
        number of rows ``ess`` (K,) behind every fold's weights.  A fold whose block of the inverse is not numerically positive
        definite raises ``LinAlgError``."""
        self._require_posterior()
        if weights not in ("is", "equal"):
            raise ValueError(f"weights must be 'is' or 'equal', got {weights!r}")
        n = self._X_train_.shape[0]
        if folds is not None and n_folds is not None:
            raise ValueError("give folds or n_folds, not both")
        if folds is None:
            folds = split_folds(n, n if n_folds is None else n_folds, random_state)
        folds = check_folds(folds, n)
        post = self._post
        if thetas is None:
            out = post.cross_validate(self, None, folds)
        else:
            rows = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
            n_theta = len(self.kernel_.theta)
            if not self.warp_inputs:
                out = post.cross_validate(self, rows, folds)
            elif post.canonical:
                out = post.cross_validate(self, rows[:, :n_theta], folds, warps=np.ascontiguousarray(rows[:, n_theta:]))
            else:  # a generic kernel tree sees a row's warp through the estimator's warpers: one row after the other
                with self._row_warps() as install:
                    parts = [post.cross_validate(self, install(r), folds) for r in rows]
                out = tuple(np.concatenate([p[i] for p in parts]) for i in range(4))
        mean, var, lpd, status = out
        raise_if_not_pd(status.ravel(), self.kernel_)
        y_mean, y_std = self._y_scale()
        sizes = np.array([len(f) for f in folds], dtype=np.float64)
        row_mean, row_var = mean * y_std + y_mean, var * y_std**2
        row_lpd = lpd - sizes[None, :] * np.log(y_std)
        res = {"folds": folds, "row_mean": row_mean, "row_std": np.sqrt(row_var), "row_fold_lpd": row_lpd}
        res.update(combine_rows(row_mean, row_var, row_lpd, folds, np.asarray(self.y_train_) * y_std + y_mean,
                                "equal" if len(row_lpd) == 1 else weights))
        return res

    @contextmanager
    def _row_warps(self):
        """Yields ``install(row)``, which gives the estimator chain row ``row``'s own input warp (its own training inputs)
        and returns the row's kernel parameters as a (1, p) block; the current warpers are back on exit, however it is left
        (``bask/acquisition.py:142-145``), and behind them the median GP's posterior (``_keeping_posterior``)."""
        n_theta, d = len(self.kernel_.theta), self._X_train_.shape[1]
        backup = (np.copy(self.warp_alphas_), np.copy(self.warp_betas_))

        def install(row):
            self.create_warpers(row[n_theta : n_theta + d], row[n_theta + d :])
            self.rewarp()
            return row[None, :n_theta]

        def put_back():
            self.create_warpers(*backup)
            self.rewarp()

        with self._keeping_posterior(put_back):
            yield install

    def _warped_rows_moments(self, rows, X, noise_zero):
        """Normalised (mean, var), each (B, m), of the GPs of chain ``rows`` at ``X``, one row's warp after the other: one build +
        predict per row (``_row_warps``)."""
        mean, var = np.empty((len(rows), X.shape[0])), np.empty((len(rows), X.shape[0]))
        with self._row_warps() as install:
            for i, row in enumerate(rows):
                m, v, _ = self._post.rows_predict(self, install(row), X, noise_zero)
                mean[i], var[i] = m[0], v[0]
        return mean, var

    _warp_rows_path = "auto"  # "loop": hyper-posterior rows under input warping one at a time (tests compare the two)

    def _predict_hyper_samples(self, thetas, X, noise_zero=True):
        """Posterior build + predict for a whole batch of hyper-posterior draws (what
        ``evaluate_acquisitions`` does one ``gpr.theta = chain_[i]`` at a time,
        ``bask/acquisition.py:112-125``): ONE batched device build, ONE batched predict.  With input warping every draw
        carries its own warp, i.e. its own training inputs (``:113-119``); rows are then ``chain_`` rows, kernel parameters
        first and the 2d warp parameters behind them.  A canonical kernel still takes one build and one predict: the device
        warps the training inputs and the queries per row (``CanonicalPosterior.hyper_predict(..., warps=...)``, DESIGN.md
        section 17), and neither the estimator's warpers nor the context-level warp are touched.  A generic kernel tree, and
        ``_warp_rows_path = "loop"``, install one row's warp after the other: one build + predict per draw.  Same bits."""
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        rows = np.atleast_2d(thetas)
        if self.warp_inputs and self._post.canonical and self._warp_rows_path == "auto":
            validate_zeroone(X)
            n_theta = len(self.kernel_.theta)
            mean, var = self._post.hyper_predict(self, rows[:, :n_theta], X, noise_zero,
                                                 warps=np.ascontiguousarray(rows[:, n_theta:]))
        elif self.warp_inputs:
            validate_zeroone(X)
            mean, var = self._warped_rows_moments(rows, X, noise_zero)
        else:
            mean, var = self._post.hyper_predict(self, rows, X, noise_zero)
        return self.y_train_std_ * mean + self.y_train_mean_, np.sqrt(var * self.y_train_std_**2)

    def predict_marginal(self, X, thetas=None, n_samples=64, weights=None, quantiles=(0.05, 0.5, 0.95), at=None, noise=False,
                         random_state=None, return_path=False):
        """The fully Bayesian prediction at the rows of ``X`` (m, d; transformed space): the hyper-posterior mixture
        ``sum_b w_b N(mu_b(x), sigma_b(x)^2)`` over chain rows, i.e. the posterior predictive with the kernel hyper-parameters
        integrated out -- ``predict`` uses the ONE GP at the chain's geometric median.  Rows: ``thetas`` (B, p; under
        ``warp_inputs`` they carry their warps, as ``chain_`` holds them), or ``n_samples`` rows of ``chain_`` drawn without
        replacement from ``random_state`` as ``evaluate_acquisitions`` draws them (fewer if the chain is shorter).  ``weights``
        (B,): importance weights, default equal; a row with weight 0 or a non-finite moment anywhere is left out and the rest
        renormalised.  ``noise=False``: the latent function, as the acquisitions see it; ``noise=True`` keeps every row's own
        white level: the predictive of an observation.

        Returns a dict in y units: ``mean``; ``std`` with its two parts ``std_within`` ("the GPs are unsure") and ``std_between``
        ("the hyper-parameters are unsure": ``std^2 = std_within^2 + std_between^2``); ``quantiles`` (Q, m) of the MIXTURE at
        ``probs`` (not ``mean + z std``: the two differ as soon as the rows disagree); with ``at`` (a value per point or one for
        all) ``cdf`` = P(f(x) <= at), ``sf`` = P(f(x) > at) (each accurate in its own tail) and ``logpdf``, the log predictive
        density of ``at``; ``n_used`` and the ``rows``.  Canonical kernels with at most ``max_batch`` rows: ONE batched build and ONE
        device call (``bgp_predict_mixture``; under ``warp_inputs`` the per-row-warped build and
        ``bgp_predict_mixture_warped``) -- the B x m moments never leave the device.  Generic kernel trees, and more rows than
        ``max_batch``: the rows' moments chunk by chunk through the existing predict paths, then the same pass on them
        (``bgp_mixture_values``), said once on stderr.  ``return_path``: also "device" | "chunks"."""
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        if self.warp_inputs:
            validate_zeroone(X)
        self._require_posterior()
        if thetas is None:
            chain = np.asarray(self.chain_)
            rng = check_random_state(random_state)
            rows = chain[rng.choice(len(chain), replace=False, size=min(int(n_samples), len(chain)))]
        else:
            rows = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
        probs = np.asarray(quantiles if quantiles is not None else [], dtype=np.float64).ravel()
        y_mean, y_std = self._y_scale()
        post, ctx = self._post, self._ctx
        if post.canonical and len(rows) <= ctx.max_batch and self._warp_rows_path == "auto":
            if self.warp_inputs:
                n_theta = len(self.kernel_.theta)
                H = self._canonical(rows[:, :n_theta])
                status = ctx.posterior(H, want_alpha=False, warps=np.ascontiguousarray(rows[:, n_theta:]))["status"]
                raise_if_not_pd(status, self.kernel_)
            else:
                H = post.build_rows(self, rows)
            out = ctx.predict_mixture(H if noise else noise_off(H), X, y_mean, y_std, probs, at=at, weights=weights,
                                      warped=bool(self.warp_inputs))
            path = "device"
        else:
            _marginal_tell_once("generic kernel tree" if not post.canonical else "more rows than the context's max_batch")
            step = max(1, int(ctx.max_batch))
            parts = [self._predict_hyper_samples(rows[b0:b0 + step], X, noise_zero=not noise) for b0 in range(0, len(rows), step)]
            mu, sd = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
            out = ctx.mixture_values(mu, sd * sd, 0.0, 1.0, probs, at=at, weights=weights)  # (already in y units)
            path = "chunks"
        within, between = out.pop("within"), out.pop("between")
        out.update(std=np.sqrt(within + between), std_within=np.sqrt(within), std_between=np.sqrt(between), rows=rows)
        if "quantiles" not in out:
            out["quantiles"] = np.empty((0, X.shape[0]))
        return (out, path) if return_path else out

    def _acq_hyper_samples(self, thetas, X, kinds, params, n_samples, noise_zero=True):
        """Closed-form acquisition values averaged over a batch of hyper-posterior draws, entirely on the device:
        batched posterior build, batched predict and the acquisition / averaging pass of
        ``evaluate_acquisitions`` (``bask/acquisition.py:112-139``) -- only (len(kinds), m) numbers come back."""
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        H = self._post.build_rows(self, thetas)
        return self._ctx.acq(noise_off(H) if noise_zero else H, X, *self._y_scale(), kinds, params, n_samples)

    def _pvrs(self, X, thompson_points, has_alpha_vec):
        """Device side of PVRS / VarianceReduction (``bask/acquisition.py:287-300,328-338``)."""
        return self._post.pvrs(self, np.atleast_2d(X), np.atleast_2d(thompson_points), has_alpha_vec)

    # ---- batch proposals (Optimizer.ask(n_points > 1))
    def _fantasy_batch(self, X, first, q, acq, rows, n_samples, acq_kwargs, lie, thompson=None, replay=None, path="auto",
                       want_moments=False):
        """Greedy batch over the candidates ``X`` of a proposal whose argmax was ``first``: point j + 1 maximises ``acq``
        for the GPs of the same chain ``rows`` (PVRS / VR and other whole-GP acquisitions: the median GP; PVRS with the
        same ``thompson`` points) conditioned on the j points chosen so far with their fantasy observations.  ``lie``:
        the fantasy value in y units, or None for the kriging believer (every GP's own posterior mean).
        Hyper-parameters, warps and the y normalisation stay fixed; a fantasy point carries the noise a ``tell`` with
        noise 0 would give it (the scalar alpha + the row's white level; for PVRS / VR alpha enters only as a vector,
        with 0 appended, as the reference does for the candidate row).  A whole-GP acquisition other than PVRS / VR is
        called itself on the conditioned median GP with ``replay``, the generator state the proposal handed it.
        Returns (q indices into X, the (q - 1, m) step values, "fast" | "fallback", info) with info["step_ms"] the
        wall time of every step; on the fast path also info["begin_ms"] / ["end_ms"], info["device"] (its counters)
        and, with ``want_moments``, info["moments"] (the conditioned latent means, variances)."""
        from . import acquisition as A

        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        if not 1 <= q <= X.shape[0]:
            raise ValueError(f"a batch of {q} points from {X.shape[0]} candidates")
        y_mean, y_std = self._y_scale()
        lie_n = None if lie is None else (float(lie) - y_mean) / y_std
        spec = A._device_acq_spec(acq, acq_kwargs) if isinstance(acq, A.UncertaintyAcquisition) else None
        fast = (path != "fallback" and spec is not None and A.DEVICE_ACQUISITIONS and not self.warp_inputs
                and self._post.canonical and X.shape[1] <= 32)
        if isinstance(acq, A.UncertaintyAcquisition) and (rows is None or len(rows) == 0):
            # no hyper-posterior draws (n_samples=0): every value is 0, np.argmax takes the lowest index left
            rest = [i for i in range(X.shape[0]) if i != first][: q - 1]
            return [int(first)] + rest, np.zeros((q - 1, X.shape[0])), "fallback", {"step_ms": []}
        if fast:
            return self._fantasy_fast(X, first, q, spec, rows, n_samples, lie_n, want_moments)
        _fantasy_tell_once()
        return self._fantasy_fallback(X, first, q, acq, rows, n_samples, acq_kwargs, lie_n, thompson, replay)

    def _fantasy_base_alpha(self):
        return float(self.alpha if not np.iterable(self.alpha) else self._alpha)

    def _fantasy_fast(self, X, first, q, spec, rows, n_samples, lie_n, want_moments):
        """The uncertainty family on the device (bgp_fantasy_*), on a context of its own: the estimator's context and its
        resident posteriors are left as they are."""
        import time

        H = self._canonical(np.atleast_2d(rows))
        ctx = self._scratch_context()
        info = {"step_ms": []}
        try:
            raise_if_not_pd(ctx.posterior(H, want_alpha=False)["status"], self.kernel_)
            Hk = noise_off(H)
            noise = self._fantasy_base_alpha() + np.exp(H[:, -1])
            t0 = time.perf_counter()
            ctx.fantasy_begin(Hk, noise, X, *self._y_scale(), [spec[0]], [spec[1]], n_samples, max(q - 1, 1))
            info["begin_ms"] = (time.perf_counter() - t0) * 1e3
            picks, values = [int(first)], []
            for _ in range(q - 1):
                t0 = time.perf_counter()
                nxt, vals = ctx.fantasy_step(picks[-1], lie_n, want_values=True)
                info["step_ms"].append((time.perf_counter() - t0) * 1e3)
                picks.append(nxt)
                values.append(vals[0])
            if want_moments:
                info["moments"] = ctx.fantasy_moments()
            info["device"] = ctx.fantasy_stats()
            t0 = time.perf_counter()
            ctx.fantasy_end()
            info["end_ms"] = (time.perf_counter() - t0) * 1e3
        finally:
            ctx.close()
        return picks, np.array(values).reshape(q - 1, X.shape[0]), "fast", info

    def _fantasy_fallback(self, X, first, q, acq, rows, n_samples, acq_kwargs, lie_n, thompson, replay):
        """Any kernel, warp and acquisition: a scratch copy of the estimator holds the training set plus the chosen
        points and their lies on a context of its own, and the existing device calls evaluate every step."""
        import copy
        import time

        from . import acquisition as A

        scratch = copy.copy(self)  # (__getstate__: no context, no sampler travel)
        scratch._needs_rebuild = False
        scratch.kernel_ = copy.deepcopy(self.kernel_)
        full = isinstance(acq, A.FullGPAcquisition)
        own = full and type(acq) not in (A.PVRS, A.VarianceReduction)  # a whole-GP acquisition evaluated as itself
        X0, y0, (y_mean, y_std) = self._X_train_, self.y_train_, self._y_scale()
        alpha0 = np.asarray(self.alpha, dtype=np.float64) if np.iterable(self.alpha) else None
        picks, values, info = [int(first)], [], {"step_ms": []}
        try:
            mus0 = None
            if lie_n is None and not (full and not own):
                # kriging believer: the lie is each GP's own mean, so the conditioned means ARE the unconditioned ones
                scratch._ensure_context()
                if own:
                    scratch.theta = scratch.theta
                    mus0 = scratch.predict(X)[None, :]
                else:
                    mus0, _ = scratch._predict_hyper_samples(rows, X, noise_zero=True)
            for j in range(1, q):
                t0 = time.perf_counter()
                scratch._X_train_ = np.vstack([X0, X[picks]])
                if own and lie_n is None:  # the median GP's own means at the chosen points, normalised
                    lies = (mus0[0, picks] - y_mean) / y_std
                else:  # (PVRS / VR and the variances do not read y)
                    lies = np.full(j, 0.0 if lie_n is None else lie_n)
                scratch.y_train_ = np.concatenate([y0, lies])
                if alpha0 is not None:
                    extra = np.zeros(j) if full and not own else np.full(j, self._fantasy_base_alpha())
                    scratch.alpha = np.concatenate([alpha0, extra])
                scratch._ensure_context()
                if own:
                    scratch.theta = scratch.theta  # the median GP's posterior on the augmented set
                    rng = np.random.RandomState()
                    rng.set_state(replay)
                    vals = np.asarray(acq(X, scratch, random_state=rng, **acq_kwargs), dtype=np.float64)
                    vals = vals if np.all(np.isfinite(vals)) else np.zeros(X.shape[0])
                elif full:
                    vals = scratch._pvrs(X, X if thompson is None else thompson, alpha0 is not None)
                    vals = vals if np.all(np.isfinite(vals)) else np.zeros_like(vals)
                else:
                    mus, stds = scratch._predict_hyper_samples(rows, X, noise_zero=True)
                    vals = A._average_uncertainty(scratch, acq, mus if mus0 is None else mus0, stds, n_samples,
                                                  acq_kwargs)
                values.append(vals)
                v = np.array(vals, copy=True)
                v[picks] = -np.inf
                picks.append(int(np.argmax(v)))
                info["step_ms"].append((time.perf_counter() - t0) * 1e3)
        finally:
            if scratch._ctx_obj is not None:
                scratch._ctx_obj.close()
                scratch._ctx_obj = None
        return picks, np.array(values).reshape(q - 1, X.shape[0]), "fallback", info

    def _pathwise_obstacle(self):
        """Why pathwise draws cannot run on this estimator (None: they can)."""
        if self.warp_inputs:
            return "warped inputs"
        if not self._post.canonical:
            return "a generic kernel tree"
        if self._X_train_.shape[1] > 32:
            return "more than 32 input dimensions"
        return None

    def _mvn_mode(self, m, mvn=None, noise=False):
        """'reference' (numpy's SVD draw on the host from the device-built mean / covariance), 'cholesky' (device) or
        'pathwise' (``sample_paths``; only when asked for, and only where it can run)."""
        mode = self.__dict__.get("mvn", "auto") if mvn is None else mvn
        if mode not in MVN_MODES:
            raise ValueError("mvn must be 'auto', 'reference', 'cholesky' or 'pathwise', got %r" % (mode,))
        if mode == "pathwise":
            why = "noisy draws (noise=True)" if noise else self._pathwise_obstacle()
            if why is None:
                return mode
            _pathwise_tell_once(why)
            mode = "auto"
        if mode == "auto":
            mode = "reference" if m <= self.MVN_REFERENCE_MAX_POINTS else "cholesky"
        if not self._post.canonical:
            # the device draw builds the predictive covariance from the canonical hyper-parameters; a generic tree has none:
            # mean / covariance through the host-evaluated kernel, the reference's own SVD draw on the host
            mode = "reference"
        return mode

    def sample_y(self, X, sample_mean=False, noise=False, n_samples=1, random_state=0, mvn=None):
        """Function realisations of the GP(s) (``bask/bayesgpr.py:637-718``).  Predictive means and
        covariances are built on the device; the multivariate normal draw is numpy's legacy SVD draw on the
        host (``mvn="reference"``: the reference's own variates, ``sklearn/_gpr.py:522-526``) or
        ``mean + chol(cov) z`` on the device (``mvn="cholesky"``: same distribution, other variates).
        ``mvn=None`` takes the estimator's setting (default ``"auto"``: reference variates up to
        ``MVN_REFERENCE_MAX_POINTS`` query points)."""
        rng = check_random_state(random_state)
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        mode = self._mvn_mode(X.shape[0], mvn, noise)
        if mode == "pathwise":
            with self.sample_paths(n_paths=n_samples, sample_mean=sample_mean, random_state=rng) as paths:
                return paths(X)
        if sample_mean:
            cm = nullcontext(self) if noise else self.noise_set_to_zero()
            with cm:
                if mode == "reference":
                    # sklearn's sample_y: predict(return_cov=True), then rng.multivariate_normal(mean, cov, n).T
                    y_mean, y_cov = self.predict(X, return_cov=True)
                    return _legacy_mvn(rng, y_mean, y_cov, n_samples).T
                return self._draw(X, n_samples, rng)
        # hyper-posterior draws: one chain row (with replacement) and one function per sample.  The generator is
        # consumed in the reference's order -- all row indices first, then one normal vector per sample -- and the
        # device builds all posteriors and predictive covariances in batched calls.
        ind = rng.choice(len(self.chain_), size=n_samples, replace=True)
        if mode == "reference":
            return self._draw_rows_reference(self.chain_[ind], X, rng, noise).T
        Z = np.vstack([rng.standard_normal((1, X.shape[0])) for _ in range(n_samples)])
        return self._draw_rows(self.chain_[ind], X, Z, noise).T

    def _sample_hyper_rows(self, n_draws, X, rng):
        """The sample acquisitions of ``evaluate_acquisitions``: per draw the reference calls
        ``gpr.sample_y(X, random_state=rng)`` (``bask/acquisition.py:132-136``), i.e. ONE function of ONE freshly
        chosen chain row with the noise off -- same generator consumption here (row index, then the normal vector,
        per draw), one batched device call for all draws.  Returns (n_draws, m)."""
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        mode = self._mvn_mode(X.shape[0])
        if mode == "pathwise":
            with self.sample_paths(n_paths=n_draws, random_state=rng) as paths:
                return np.ascontiguousarray(paths(X).T)
        if mode == "reference":
            # row index and MVN draw alternate on the generator, as in the reference's loop: the rows cannot be chosen
            # ahead of the draws, so every draw is one device predict (mean, covariance) + one host SVD
            out = np.empty((n_draws, X.shape[0]))
            for i in range(n_draws):
                row = self.chain_[rng.choice(len(self.chain_), size=1, replace=True)[0]]
                out[i] = self._draw_rows_reference(row[None, :], X, rng, noise=False)[0]
            return out
        rows, Z = [], []
        for _ in range(n_draws):
            rows.append(self.chain_[rng.choice(len(self.chain_), size=1, replace=True)[0]])
            Z.append(rng.standard_normal((1, X.shape[0])))
        return self._draw_rows(np.array(rows), X, np.vstack(Z), noise=False)

    def sample_paths(self, n_paths=1, sample_mean=False, n_features=1024, random_state=0):
        """``n_paths`` posterior function draws as FUNCTIONS (a ``PosteriorPaths``): Matheron's rule on ``n_features`` random
        Fourier features per path.  ``paths(X)`` is (m, n_paths) in y units -- the shape ``sample_y``
        returns --, ``paths.gradient(X)`` (m, n_paths, d); the object can be evaluated anywhere, any number of times, with
        consistent values.  ``sample_mean=True``: every path belongs to the median GP; otherwise each path takes one chain
        row drawn with replacement (ONE batched posterior build over the distinct rows).  The paths are the latent function
        (noise off).  The generator is consumed in this order: all row indices first (``choice``, none with
        ``sample_mean``); then per path the omega normals (F x d), for Matern kernels F chi-square variates with 2 nu
        degrees of freedom, F phases (uniform on [0, 2 pi)), F + 1 weights and n noise normals.  Runs on a device context of
        its own: the estimator's resident posterior is not disturbed.  Canonical kernels in up to 32 dimensions without input
        warping; ``ValueError`` otherwise."""
        why = None if getattr(self, "_X_train_", None) is None else self._pathwise_obstacle()
        if why is not None:
            raise ValueError("sample_paths does not support %s" % why)
        self._require_posterior("sample_paths")
        n_paths, F = int(n_paths), int(n_features)
        if n_paths < 1 or not 1 <= F <= 65536:
            raise ValueError("sample_paths needs n_paths >= 1 and 1 <= n_features <= 65536")
        rng = check_random_state(random_state)
        n_theta = len(self.kernel_.theta)
        if sample_mean:
            thetas = np.tile(np.asarray(self._post_theta, dtype=np.float64)[None, :n_theta], (n_paths, 1))
        else:
            thetas = self.chain_[rng.choice(len(self.chain_), size=n_paths, replace=True)][:, :n_theta]
        return self._paths_of_thetas(thetas, F, rng)

    def _sample_paths_rows(self, thetas, n_per_row, n_features, rng):
        """``n_per_row`` pathwise draws for EACH row of ``thetas`` (B, n_theta), as ``sample_paths`` draws them: path
        ``b * n_per_row + j`` is draw j of row b.  The generator ``rng`` is consumed per path as ``sample_paths`` documents (no row
        indices are drawn here).  ``ValueError`` with ``sample_paths``' own reason where the pathwise draws cannot run."""
        why = None if getattr(self, "_X_train_", None) is None else self._pathwise_obstacle()
        if why is not None:
            raise ValueError("sample_paths does not support %s" % why)
        n_per_row, F = int(n_per_row), int(n_features)
        if n_per_row < 1 or not 1 <= F <= 65536:
            raise ValueError("sample_paths needs n_paths >= 1 and 1 <= n_features <= 65536")
        n_theta = len(self.kernel_.theta)
        thetas = np.repeat(np.atleast_2d(np.asarray(thetas, dtype=np.float64))[:, :n_theta], n_per_row, axis=0)
        return self._paths_of_thetas(thetas, F, rng)

    def _paths_of_thetas(self, thetas, F, rng):
        """One pathwise draw per row of ``thetas`` (the common tail of ``sample_paths`` and ``_sample_paths_rows``)."""
        n_paths = len(thetas)
        H = self._canonical(thetas)
        n, d = self._X_train_.shape
        omega, phase, w, eps = draw_path_variates(rng, n_paths, F, d, n, self._plan.stationary)
        uniq, inverse = np.unique(H, axis=0, return_inverse=True)  # repeated chain rows share one posterior build
        ctx = self._scratch_context()
        try:
            raise_if_not_pd(ctx.posterior(uniq, want_alpha=False)["status"], self.kernel_)
            ctx.paths_begin(np.asarray(inverse, dtype=np.int32).ravel(), noise_off(H), H[:, -1], omega, phase, w, eps)
        except BaseException:
            ctx.close()
            raise
        return PosteriorPaths(ctx, *self._y_scale(), n_paths, d)

    def _draw_rows_reference(self, rows, X, rng, noise):
        """The reference's per-sample loop (``bask/bayesgpr.py:679-706``) with the device doing what the theta setter
        and ``predict(return_cov=True)`` do there -- ONE batched posterior build over the distinct chain rows, the
        predictive means / covariances in chunks -- and the host doing what numpy does there: one legacy
        ``multivariate_normal`` (SVD) per sample, in sample order, on the caller's generator.  (len(rows), m)."""
        rows = np.atleast_2d(rows)
        m = X.shape[0]
        out = np.empty((len(rows), m))
        if self.warp_inputs:
            validate_zeroone(X)
            with self._row_warps() as install:
                for i, row in enumerate(rows):  # every draw has its own warped training inputs
                    mean, cov = self._mean_cov_rows(install(row), X, noise)
                    out[i] = _legacy_mvn(rng, mean[0], cov[0], 1)[0]
            return out
        # the covariances of a chunk of samples at a time (m^2 doubles each)
        chunk = max(1, int((256 << 20) // (8 * m * m)))
        for lo in range(0, len(rows), chunk):
            mean, cov = self._mean_cov_rows(rows[lo : lo + chunk, : len(self.kernel_.theta)], X, noise)
            for i in range(mean.shape[0]):
                out[lo + i] = _legacy_mvn(rng, mean[i], cov[i], 1)[0]
        return out

    def _mean_cov_rows(self, thetas, X, noise):
        """Predictive mean and covariance (y units) of the GP of every chain row: batched device posterior build over the
        distinct rows + batched device predict with the full covariance; ``theta`` / ``alpha_`` / ``L_`` stay untouched."""
        mean, _var, cov = self._post.rows_predict(self, np.atleast_2d(thetas), X, not noise, return_cov=True)
        return self.y_train_std_ * mean + self.y_train_mean_, cov * self.y_train_std_**2

    def _draw_rows(self, rows, X, Z, noise):
        """f_i = mean_i + chol(cov_i) Z[i] for the GP of chain row i (kernel parameters and, with input warping, its
        own warp); (len(rows), m) in the units of y.  The resident posterior of ``theta`` is rebuilt lazily by the
        next call that needs it (``make_resident``), so ``theta`` / ``alpha_`` / ``L_`` / ``K_inv_`` are untouched."""
        rows = np.atleast_2d(rows)
        if self.warp_inputs:
            validate_zeroone(X)
            out = np.empty((len(rows), X.shape[0]))
            with self._row_warps() as install:
                for i, row in enumerate(rows):  # every draw has its own warped training inputs
                    out[i] = self._draw_rows_device(install(row), X, Z[i : i + 1], noise)[0]
            return out
        return self._draw_rows_device(rows[:, : len(self.kernel_.theta)], X, Z, noise)

    def _draw_rows_device(self, thetas, X, Z, noise):
        H = self._canonical(thetas)
        uniq, inverse = np.unique(H, axis=0, return_inverse=True)  # repeated chain rows share one posterior build
        raise_if_not_pd(self._ctx.posterior(uniq, want_alpha=False)["status"], self.kernel_)
        Hk = H if noise else noise_off(H)  # noise_set_to_zero(): the factors keep the noise, the predictive kernel drops it
        pidx = np.asarray(inverse, dtype=np.int32).ravel()
        out = np.empty_like(Z)
        todo = np.arange(len(H))
        jitter = 1e-10
        while len(todo):
            o, st = self._ctx.sample_y_batch(pidx[todo], Hk[todo], X, Z[todo], jitter=jitter)
            ok = st == 0
            out[todo[ok]] = o[ok]
            todo = todo[~ok]
            # numpy's SVD-based draw tolerates a numerically semi-definite covariance; the Cholesky-based draw
            # needs a growing diagonal jitter instead
            jitter *= 100.0
            if len(todo) and jitter > 1e-2:
                raise _lib.NotPositiveDefinite("predictive covariance not positive definite (jitter %.3g)" % jitter)
        return self.y_train_std_ * out + self.y_train_mean_

    def _draw(self, X, n_samples, rng):
        self._post.make_resident(self)
        Hk = self._canonical(self._kernel_theta_for_predict())
        z = rng.standard_normal((n_samples, X.shape[0]))
        jitter = 1e-10
        while True:
            try:
                out = self._ctx.sample_y(0, Hk, X, z, jitter=jitter)
                break
            except _lib.NotPositiveDefinite:
                # numpy's SVD-based draw tolerates a numerically semi-definite covariance; the
                # Cholesky-based draw needs a growing diagonal jitter instead
                jitter *= 100.0
                if jitter > 1e-2:
                    raise
        return (self.y_train_std_ * out + self.y_train_mean_).T

    def __del__(self):
        ctx = self.__dict__.get("_ctx_obj")
        if ctx is not None:
            try:
                ctx.close()
            except Exception:
                pass


MATERN_NU = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}


def draw_path_variates(rng, n_paths, F, d, n, stationary):
    """The random numbers of ``n_paths`` pathwise draws, in the documented order -- per path: omega normals (F, d), for a Matern
    kernel F chi-square variates with 2 nu degrees of freedom (omega rows times sqrt(2 nu / chi2): the multivariate t that is
    the spectral density of the unit-length-scale Matern kernel; nu = 1/2: Cauchy tails), F phases on [0, 2 pi), F + 1 weights,
    n noise normals.  Returns omega (P, F, d), phase (P, F), w (P, F + 1), eps (P, n)."""
    omega, phase = np.empty((n_paths, F, d)), np.empty((n_paths, F))
    w, eps = np.empty((n_paths, F + 1)), np.empty((n_paths, n))
    nu = MATERN_NU.get(stationary)
    for p in range(n_paths):
        z = rng.standard_normal((F, d))
        if nu is not None:
            z = z * np.sqrt(2.0 * nu / rng.chisquare(2.0 * nu, size=F))[:, None]
        omega[p] = z
        phase[p] = rng.uniform(0.0, 2.0 * np.pi, size=F)
        w[p] = rng.standard_normal(F + 1)
        eps[p] = rng.standard_normal(n)
    return omega, phase, w, eps


class PosteriorPaths:
    """Posterior function draws of a ``BayesGPR`` (``sample_paths``), resident on a device context of their own
    (``bgp_paths_*``).  ``paths(X)``: (m, n_paths) in y units; ``paths.gradient(X)``: (m, n_paths, d).  A value does not depend
    on the other rows of the call: evaluating twice, or on a superset, gives the same bits.  ``paths.minimize(...)``: every
    path's minimiser over a box, searched on the device.  ``close()`` (or leaving the ``with`` block) frees the device
    state."""

    def __init__(self, ctx, y_mean, y_std, n_paths, d):
        self._ctx, self._y_mean, self._y_std = ctx, y_mean, y_std
        self.n_paths, self.d = n_paths, d

    def _X(self, X):
        if self._ctx is None:
            raise RuntimeError("the paths have been closed")
        X = np.atleast_2d(np.asarray(X, dtype=np.float64))
        if X.shape[1] != self.d:
            raise ValueError("query points must have %d columns, got %d" % (self.d, X.shape[1]))
        return X

    def __call__(self, X):
        X = self._X(X)
        out, _ = self._ctx.paths_eval(X)
        return (self._y_std * out + self._y_mean).T

    def gradient(self, X):
        X = self._X(X)
        _, dout = self._ctx.paths_eval(X, want_grad=True)
        return np.ascontiguousarray(np.transpose(self._y_std * dout, (1, 0, 2)))

    def minimize(self, bounds=(0.0, 1.0), n_candidates=2000, n_starts=8, X0=None, random_state=0, gtol=1e-5, max_iter=200):
        """The minimiser of every path over the box ``bounds`` = (low, high) (scalars or d values each), searched on the device:
        one workgroup per (start, path) runs a bounded quasi-Newton iteration on the path and its analytic gradient
        (``bgp_paths_minimize``) until the projected gradient is below ``gtol`` (y units) or ``max_iter``
        iterations.  ``X0=None``: ``n_candidates`` uniform points of the box are drawn -- the generator is consumed by ONE
        ``uniform(size=(n_candidates, d))`` call, nothing else --, all paths are evaluated there in ONE call, and each path
        starts from its ``n_starts`` lowest rows (stable argsort, so ties keep the row order).  ``X0``: (S, d) starts shared
        by all paths, or (n_paths, S, d); no generator is used.  Returns a dict: ``x`` (n_paths, d) the best end point per path and
        ``fun`` (n_paths,) its value in y units -- never above the path's lowest candidate row --; per start ``x_all``
        (n_paths, S, d), ``fun_all``, ``status`` (0 converged, 1 ``max_iter``, 2 no decrease), ``iters``, ``evals``
        (n_paths, S); ``best`` (n_paths,) the index of the best start."""
        if self._ctx is None:
            raise RuntimeError("the paths have been closed")
        d, P = self.d, self.n_paths
        lo = np.ascontiguousarray(np.broadcast_to(np.asarray(bounds[0], dtype=np.float64), (d,)))
        hi = np.ascontiguousarray(np.broadcast_to(np.asarray(bounds[1], dtype=np.float64), (d,)))
        if not np.all(lo <= hi):
            raise ValueError("minimize needs low <= high in every dimension")
        if X0 is None:
            n_candidates, n_starts = int(n_candidates), int(n_starts)
            if not 1 <= n_starts <= n_candidates:
                raise ValueError("minimize needs 1 <= n_starts <= n_candidates")
            cand = lo + (hi - lo) * check_random_state(random_state).uniform(size=(n_candidates, d))
            f, _ = self._ctx.paths_eval(cand)
            X0 = np.stack([cand[np.argsort(f[p], kind="stable")[:n_starts]] for p in range(P)])
        else:
            X0 = np.asarray(X0, dtype=np.float64)
            if X0.ndim == 2:
                X0 = np.broadcast_to(X0[None], (P,) + X0.shape)
            if X0.ndim != 3 or X0.shape[0] != P or X0.shape[1] < 1 or X0.shape[2] != d:
                raise ValueError("X0 must be (S, d) or (n_paths, S, d) with S >= 1 and d = %d, got %r" % (d, X0.shape))
        out = self._ctx.paths_minimize(X0, lo, hi, gtol=float(gtol) / self._y_std, max_iter=max_iter)
        fun_all = self._y_std * out["fun"] + self._y_mean
        best = np.argmin(fun_all, axis=1)
        rows = np.arange(P)
        return {"x": out["x"][rows, best], "fun": fun_all[rows, best], "x_all": out["x"], "fun_all": fun_all,
                "status": out["status"], "iters": out["iters"], "evals": out["evals"], "best": best}

    def select_batch(self, X, q, kind="improvement", incumbent="paths", forced=(), return_values=False):
        """``q`` rows of ``X`` picked greedily on the JOINT draw of the paths over {training inputs, rows of X}, on the device
        (``bgp_paths_select``); the draw matrix does not leave it.  ``kind="improvement"``: step j picks the
        row that adds most to the Monte-Carlo q-EI ``mean_s max(0, c_s - min_{k chosen} f_s(x_k))`` -- greedy on a monotone
        submodular set function --, ties to the lower index; ``incumbent="paths"``: c_s is path s's own minimum over the training
        inputs (the incumbent of noisy EI: uncertain, and integrated over whatever hyper-posterior rows the paths carry); a
        number: that value, in y units, for every path.  ``kind="thompson"``: step j picks path ``j mod n_paths``'s lowest row
        among those left.  ``forced``: row indices taken as chosen before the first step (points under evaluation): they lower
        the incumbents and are never picked.  Returns a dict: ``picks`` (q,), ``incumbents`` (n_paths,) in y units (before the
        forced rows lower them) and ``values`` (q, m) in y units -- the step's gain of every row, or ``-f`` of the step's path
        for Thompson; chosen rows included -- or None without ``return_values``."""
        X = self._X(X)
        if kind not in _lib.SELECT_KINDS:
            raise ValueError("kind must be one of %r, got %r" % (tuple(_lib.SELECT_KINDS), kind))
        if isinstance(incumbent, str):
            if incumbent != "paths":
                raise ValueError("incumbent must be 'paths' or a number in y units, got %r" % (incumbent,))
            inc = None
        else:
            inc = (float(incumbent) - self._y_mean) / self._y_std
        picks, values, incs = self._ctx.paths_select(X, q, kind=kind, incumbent=inc, forced=forced, want_values=return_values)
        if values is not None:
            values = self._y_std * values if kind == "improvement" else -(self._y_std * (-values) + self._y_mean)
        return {"picks": picks.astype(np.intp), "values": values, "incumbents": self._y_std * incs + self._y_mean}

    def close(self):
        ctx, self._ctx = self._ctx, None
        if ctx is not None:
            ctx.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_pathwise_told = []


def _pathwise_tell_once(why):
    """One line on stderr, once per process: mvn="pathwise" asked for where the pathwise draws cannot run."""
    if not _pathwise_told:
        _pathwise_told.append(True)
        print("[bayes_skopt_amd] mvn='pathwise': not available for %s; drawing as mvn='auto' does" % why, file=sys.stderr,
              flush=True)


_marginal_told = []


def _marginal_tell_once(why):
    """One line on stderr, once per process: a hyper-posterior mixture whose rows' moments came back to the host in chunks."""
    if not _marginal_told:
        _marginal_told.append(True)
        print("[bayes_skopt_amd] predict_marginal: the rows' moments chunk by chunk through predict, then the mixture pass on them "
              "(%s)" % why, file=sys.stderr, flush=True)


_fantasy_told = []


def _fantasy_tell_once():
    """One line on stderr, once per process: a batch proposal conditioned through whole device passes per point."""
    if not _fantasy_told:
        _fantasy_told.append(True)
        print("[bayes_skopt_amd] ask(n_points > 1): fantasy points through the fallback path (one posterior build + "
              "evaluation per point on an augmented training set)", file=sys.stderr, flush=True)


def _legacy_mvn(rng, mean, cov, n_samples):
    """``rng.multivariate_normal(mean, cov, n_samples)`` -- numpy's legacy SVD-based draw, the call scikit-learn's
    ``sample_y`` makes (``sklearn/_gpr.py:522-526``); (n_samples, m).  Its "covariance is not symmetric positive-
    semidefinite" warning is the reference's too (noise-free predictive covariances are numerically singular)."""
    return np.atleast_2d(rng.multivariate_normal(np.ravel(mean), cov, n_samples))


def _eval_warp_priors(warp_priors, W, d):
    """Log-prior of the warp parameters (``bask/bayesgpr.py:360-365``): a pair of callables applied to
    every (alpha_k, beta_k), or one callable of both."""
    lp = np.zeros(W.shape[0])
    A, Bm = W[:, :d], W[:, d:]
    if isinstance(warp_priors, (list, tuple)):
        for k in range(d):
            lp += _vec_call(warp_priors[0], A[:, k]) + _vec_call(warp_priors[1], Bm[:, k])
    else:
        for k in range(d):
            lp += np.array([float(warp_priors(a, b)) for a, b in zip(A[:, k], Bm[:, k])])
    return lp


class _ShardedLogProb:
    """``log_prob_fn`` of the exact single-ensemble sharding (SURVEY.md 8e option 1; the reference runs ONE ensemble on
    one RNG, ``bask/bayesgpr.py:490-530``): every rank is handed the same (B, p) block, evaluates the LML of its own
    rows [r B/G, (r+1) B/G) on its device and the log-priors of ALL rows on the host meanwhile; ``finish`` gathers the B
    log-likelihoods device to device (``distributed.allgather_lml``: one RCCL all-gather of B doubles per half-step).
    Same arithmetic per row as ``_AsyncLogProb``: the chain equals the single-GPU chain bit for bit."""

    def __init__(self, gp):
        self._gp = gp

    def __call__(self, Theta, priors, warp_priors=None):
        return self.finish(self.begin(Theta, priors, warp_priors))

    def begin(self, Theta, priors, warp_priors=None):
        gp = self._gp
        Theta = np.atleast_2d(np.asarray(Theta, dtype=np.float64))
        if distributed.backend() is None:
            return ("single", gp._log_prob_begin(Theta, priors, warp_priors))
        rank, _lr, ws = distributed.world()
        B = Theta.shape[0]
        lo, hi = distributed.shard_rows(B, rank, ws)
        # From here on every rank is committed to ONE collective in ``finish``.  Whatever fails locally in between -- the
        # priors raising, a failed submit, a device error -- is carried in the token and reported THROUGH that collective
        # (status word next to the values): a rank that raised here would leave its peers blocked in the all-gather.
        if gp.warp_inputs or not gp._post.canonical:  # per-walker warps / host kernels: finished values gathered via the host
            try:
                return ("host", B, gp._log_prob_begin(Theta[lo:hi], priors, warp_priors) if hi > lo else None, None)
            except Exception as exc:
                return ("host", B, None, exc)
        # decided from what every rank sees alike (same block, same context settings): all ranks gather the same way
        can_async = not gp._ctx._timing and -(-B // ws) <= gp._ctx.max_batch
        native = distributed.backend() == "rccl" and can_async
        submitted, lp, H, failure = False, None, None, None
        try:
            H = gp._canonical(Theta[lo:hi])
            submitted = gp._ctx.lml_submit(H) if (can_async and hi > lo) else False
            lp = _eval_priors(priors, Theta)  # all rows on every rank, while the device factorises this rank's
        except Exception as exc:
            failure = exc
        except BaseException:
            # KeyboardInterrupt / SystemExit: this rank is going down and will never enter the collective.  Collect the pending
            # batch (otherwise every later call on the context answers BGP_ERR_STATE) and take the group down with it, so that the
            # peers fail at once instead of sitting in the all-gather until BGP_COMM_TIMEOUT_S.
            try:
                if submitted or gp._ctx.has_pending():
                    gp._ctx.lml_wait()
            except Exception:
                pass
            distributed.abort_process_group()
            raise
        return ("dev", B, lp, H, submitted, native, hi > lo, failure)

    def finish(self, token):
        gp = self._gp
        if token[0] == "single":
            return gp._log_prob_finish(token[1])
        if token[0] == "host":
            _k, B, tok, failure = token
            local = np.zeros(0)
            if failure is None and tok is not None:
                try:
                    local = gp._log_prob_finish(tok)
                except Exception as exc:
                    failure = exc
            return self._gather(None, B, local, failure)
        _k, B, lp, H, submitted, native, has_rows, failure = token
        if native:
            lml = self._gather(gp._ctx, B, None, failure)
        else:  # gloo group (CPU tests, ranks sharing one GPU) or a batch that could not go asynchronously
            local = np.zeros(0)
            try:
                if submitted:
                    local = gp._ctx.lml_wait()  # (also when the priors failed: the pending batch must be collected)
                elif has_rows and failure is None:
                    local = gp._ctx.lml(H)
            except Exception as exc:
                failure = failure or exc
            lml = self._gather(None, B, local, failure)
        with np.errstate(invalid="ignore"):
            lp = lp + lml
        lp[~np.isfinite(lp)] = -np.inf
        return lp

    def resident(self, n_walkers, n_dim, priors=None, warp_priors=None):
        """The sharded ensemble's run resident on every rank's device (``bgp_mcmc_begin_ex`` with the group's communicator):
        the step kernel replicated, each rank's rows of a half-step factorised on its GPU, the all-gather of the
        log-likelihoods ON THE STREAM between the batch and the next step kernel -- no host synchronisation per half-step
        (``bask/bayesgpr.py:510-530`` on G GPUs).  Over gloo (CPU tests, ranks sharing a GPU) the host-driven exchange stays."""
        if distributed.backend() is None:
            run, self.resident_reason = _resident_run(self._gp, n_walkers, n_dim, priors, warp_priors, None)
            return run
        if distributed.backend() != "rccl":
            run, self.resident_reason = None, "the process group is a gloo group: the exchange goes through the host"
            return run
        run, self.resident_reason = _resident_run(self._gp, n_walkers, n_dim, priors, warp_priors, distributed.communicator())
        return run

    @staticmethod
    def _gather(ctx, B, local, failure):
        try:
            return distributed.allgather_lml(ctx, B, local=local, error=0 if failure is None else 1)
        except distributed.ShardedEvaluationError as err:
            if failure is not None:
                raise err from failure
            raise


class _AsyncLogProb:
    """``log_prob_fn`` of the ensemble sampler: callable like ``_log_prob_batch`` and, for the sampler's overlap of
    its own bookkeeping with the device, split into ``begin`` (enqueue) / ``finish`` (collect)."""

    def __init__(self, gp):
        self._gp = gp

    def __call__(self, Theta, priors, warp_priors=None):
        return self._gp._log_prob_batch(Theta, priors, warp_priors)

    def begin(self, Theta, priors, warp_priors=None):
        return self._gp._log_prob_begin(Theta, priors, warp_priors)

    def finish(self, token):
        return self._gp._log_prob_finish(token)

    def resident(self, n_walkers, n_dim, priors=None, warp_priors=None):
        """The sampler asks: can the whole run stay on the device (``bgp_mcmc_begin`` / ``_steps`` / ``_end``)?  An object
        with begin(coords, log_prob, nsteps) / steps(plan segment) / progress() / end() / abandon() when it can, else None with
        the reason in ``resident_reason`` (the host-driven loop runs and says so once)."""
        run, self.resident_reason = _resident_run(self._gp, n_walkers, n_dim, priors, warp_priors, None)
        return run


def _device_prior(fn):
    """(kind, five parameters) of a log-prior the step kernel of the resident sampler can evaluate (``include/bgp.h``,
    ``bgp_mcmc_begin_ex``), or None: the two families ``guess_priors`` hands out carry theirs (``_bgp_device``); a frozen
    ``scipy.stats.norm(loc, scale).logpdf`` -- the reference's default warp priors, ``bask/bayesgpr.py:463-466`` -- is kind 3."""
    dev = getattr(fn, "_bgp_device", None)
    if dev is not None:
        return dev
    frozen = getattr(fn, "__self__", None)
    dist = getattr(frozen, "dist", None)
    if getattr(fn, "__name__", "") != "logpdf" or getattr(dist, "name", None) != "norm":
        return None
    try:
        args, loc, scale = dist._parse_args(*frozen.args, **frozen.kwds)
        loc, scale = float(loc), float(scale)
    except Exception:
        return None
    if args or not (np.isfinite(loc) and np.isfinite(scale) and scale > 0.0):
        return None
    # scipy: x = (t - loc) / scale;  -x**2 / 2.0 - log(sqrt(2 pi)) - log(scale), with numpy's constants
    return 3, (loc, scale, float(np.log(np.sqrt(2 * np.pi))), float(np.log(np.asarray(scale))), 0.0)


def _resident_run(gp, n_walkers, n_dim, priors, warp_priors, comm):
    """(run object, None) when the ensemble sampler's whole run can stay on the device, (None, reason) otherwise.
    ``comm``: the communicator of a sharded ensemble (every rank decides from the same facts: the same answer everywhere)."""
    if not getattr(gp, "resident_sampler", True):
        return None, None  # (asked for: not a fallback)
    if not gp._post.canonical:
        return None, "the kernel tree has no canonical device form: its matrices are evaluated on the host"
    if n_walkers % 2:
        return None, "an odd number of walkers: the two halves of a step differ in size"
    ctx = gp._ctx
    if ctx._timing:
        return None, "per-launch timing is on"
    Ns = n_walkers // 2
    world = comm.world if comm is not None else 1
    if -(-Ns // world) > ctx.max_batch:
        return None, "a half-step's proposals exceed max_batch"
    if callable(priors) or priors is None:
        return None, "the prior is one callable of the whole parameter vector"
    priors = list(priors)
    d = gp._X_train_.shape[1]
    nwarp = 2 * d if gp.warp_inputs else 0
    n_theta = n_dim - nwarp
    if len(priors) != n_theta:
        return None, "the number of priors differs from the number of kernel hyper-parameters"
    table = [_device_prior(f) for f in priors]
    if nwarp:
        if not isinstance(warp_priors, (list, tuple)) or len(warp_priors) != 2:
            return None, "the warp prior is one callable of (alpha, beta)"
        wa, wb = _device_prior(warp_priors[0]), _device_prior(warp_priors[1])
        table += [wa] * d + [wb] * d
    if any(t is None for t in table):
        return None, "a prior is not one of the families the device evaluates (guess_priors' two, scipy.stats.norm)"
    try:  # the canonical map as an index table: probe it with the positions themselves
        probe = gp._canonical(np.arange(n_theta, dtype=np.float64)[None, :] + 0.25)[0]
        fixed = gp._canonical(np.arange(n_theta, dtype=np.float64)[None, :] + 0.75)[0]
    except Exception:
        return None, "the kernel's hyper-parameters do not map onto the canonical vector entry by entry"
    src = np.where(probe != fixed, np.floor(probe).astype(np.int64), -1)
    if probe.shape != (d + 2,) or np.any(src >= n_theta):
        return None, "the kernel's hyper-parameters do not map onto the canonical vector entry by entry"
    kind = np.array([t[0] for t in table], dtype=np.int32)
    par = np.array([t[1] for t in table], dtype=np.float64)
    h_fixed = np.where(src < 0, probe, 0.0)

    class _Run:  # (the sampler hands the plan over in segments and draws the next one while the device works)
        @staticmethod
        def begin(coords, log_prob, nsteps):
            ctx.mcmc_begin(coords, log_prob, nsteps, src, h_fixed, kind, par, comm=comm, nwarp=nwarp)

        steps = staticmethod(ctx.mcmc_steps)
        progress = staticmethod(ctx.mcmc_progress)
        end = staticmethod(ctx.mcmc_end)
        abandon = staticmethod(ctx.mcmc_abandon)

    return _Run, None


def _vec_call(fn, col):
    try:
        with np.errstate(all="ignore"):
            v = np.asarray(fn(col), dtype=np.float64)
        if v.shape == col.shape:
            return v
    except Exception:
        pass
    with np.errstate(all="ignore"):
        return np.array([float(fn(t)) for t in col])


def _eval_priors(priors, Theta):
    """Sum of log-priors for a (Ns, p) block.  A list holds one callable per hyper-parameter
    (``bask/bayesgpr.py:368-370``), evaluated column-wise when the callable broadcasts and
    element-wise otherwise; a single callable receives each full parameter vector (:371-372)."""
    Ns, p = Theta.shape
    if callable(priors):
        return np.array([float(priors(row)) for row in Theta])
    priors = list(priors)
    if len(priors) != p:
        raise ValueError(f"zip() argument 2 is {'shorter' if p < len(priors) else 'longer'} than argument 1: "
                         f"{len(priors)} priors for {p} hyper-parameters")
    lp = np.zeros(Ns)
    k = 0
    while k < p:
        prior = priors[k]
        k1 = k + 1
        while k1 < p and priors[k1] is prior:  # guess_priors puts the SAME callable on every length scale
            k1 += 1
        block = Theta[:, k:k1]
        vals = None
        try:  # one elementwise call for the whole run of columns ...
            with np.errstate(all="ignore"):
                v = np.asarray(prior(block if k1 - k > 1 else block[:, 0]), dtype=np.float64)
            if v.shape == block.shape or (k1 - k == 1 and v.shape == (Ns,)):
                vals = v.reshape(Ns, k1 - k)
        except Exception:
            vals = None
        if vals is None:
            with np.errstate(all="ignore"):
                vals = np.array([[float(prior(t)) for t in row] for row in block])
        for j in range(k1 - k):  # ... added column by column, i.e. in the reference's summation order
            lp += vals[:, j]
        k = k1
    return lp
