"""Batch proposals: ``Optimizer.ask(n_points > 1, strategy=...)`` by fantasy conditioning.

The oracle below restates the semantics with numpy / scipy alone: per hyper-posterior row, the kernel on the training set plus
the chosen points with their lies, a Cholesky factorisation, the latent prediction, the closed form and the average over the
rows; PVRS / VR by the reference's loop body on the augmented training set."""
import numpy as np
import pytest
import scipy.linalg as sla
from scipy.special import ndtr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bask():
    import bayes_skopt_amd as bask

    assert bask._lib.device_count() >= 1
    return bask


def branin_like(x):
    return float(np.sin(3.0 * x[0]) + (x[1] - 0.3) ** 2 + 0.5 * np.cos(2.0 * x[0] * x[1]))


def fitted(bask, acq, n=40, d=2, m=300, n_samples=8, kwargs=None, seed=0, gp_samples=60, **okw):
    """An optimizer past its initial design: n random points told at once (one MCMC fit + one proposal)."""
    opt = bask.Optimizer(dimensions=[(-1.0, 1.0)] * d, n_points=m, n_initial_points=n, init_strategy="r2", acq_func=acq,
                         acq_func_kwargs=kwargs, random_state=seed, **okw)
    rng = np.random.RandomState(seed)
    X = rng.uniform(-1.0, 1.0, size=(n, d)).tolist()
    y = [branin_like(x) + 0.01 * rng.randn() for x in X]
    opt.tell(X, y, n_samples=n_samples, gp_samples=gp_samples, gp_burnin=2)
    assert opt.gp.kernel_ is not None and opt._last_candidates is not None
    return opt


# ------------------------------------------------------------------ the oracle
def _stationary(r2, name):
    r = np.sqrt(r2)
    if name == "rbf":
        return np.exp(-0.5 * r2)
    if name == "matern12":
        return np.exp(-r)
    if name == "matern32":
        t = np.sqrt(3.0) * r
        return (1.0 + t) * np.exp(-t)
    t = np.sqrt(5.0) * r
    return (1.0 + t + t * t / 3.0) * np.exp(-t)


def _k(A, B, h, plan):
    """Latent kernel of canonical h = [log c, log l_1..d, log s2] (no white term)."""
    d = A.shape[1]
    ell = np.exp(h[1 : 1 + d])
    r2 = (((A[:, None, :] - B[None, :, :]) / ell) ** 2).sum(-1)
    s = _stationary(r2, plan.stationary)
    return np.exp(h[0]) * s if plan.form == "product" else np.exp(h[0]) + s


def _prior_var(h, plan):
    return np.exp(h[0]) if plan.form == "product" else np.exp(h[0]) + 1.0


def _latent(Xa, ya, noise_a, h, Xc, plan):
    """Latent mean / variance at Xc of the GP with training data (Xa, ya), diagonal noise_a + the white level."""
    K = _k(Xa, Xa, h, plan) + np.diag(noise_a + np.exp(h[-1]))
    L = sla.cholesky(K, lower=True)
    Ks = _k(Xc, Xa, h, plan)
    mu = Ks @ sla.cho_solve((L, True), ya)
    V = sla.solve_triangular(L, Ks.T, lower=True)
    var = np.maximum(_prior_var(h, plan) - (V * V).sum(0), 0.0)
    return mu, var


def _closed_form(name, mu, std, kw):
    def ei(mu, std, y_opt):
        out = np.zeros_like(mu)
        ok = std > 0
        z = (y_opt - mu[ok]) / std[ok]
        out[ok] = (z * ndtr(z) + np.exp(-z * z / 2.0) / np.sqrt(2.0 * np.pi)) * std[ok]
        return out

    if name == "ei":
        y_opt = kw.get("y_opt")
        return ei(mu, std, mu.min() if y_opt is None else y_opt)
    if name == "lcb":
        return kw.get("alpha", 1.96) * std - mu
    if name == "mean":
        return -mu
    if name == "ttei":
        e = ei(mu, std, mu.min())
        top = np.argmax(e)
        out = np.zeros_like(mu)
        ok = std > 0
        sp = np.sqrt(std[ok] ** 2 + std[top] ** 2)
        z = (mu[top] - mu[ok]) / sp
        out[ok] = sp * (z * ndtr(z) + np.exp(-z * z / 2.0) / np.sqrt(2.0 * np.pi))
        return out
    raise KeyError(name)


def oracle_batch(opt, name, q, strategy):
    """(picks, step values) of the batch semantics, restated."""
    gp = opt.gp
    plan = gp._plan
    cand, first = opt._last_candidates, int(np.argmax(opt._last_acq_values))
    X0, y0 = gp._X_train_, gp.y_train_
    ym, ys = float(np.ravel(gp.y_train_mean_)[0]), float(np.ravel(gp.y_train_std_)[0])
    # (tell() hands BayesGPR a noise vector: alpha is the scalar base + 0 per point; a fantasy point gets the scalar base)
    alpha_vec = np.broadcast_to(np.asarray(gp.alpha, dtype=np.float64), (len(X0),))
    base_alpha = float(gp._alpha)
    picks, values = [first], []
    if name in ("pvrs", "vr"):
        h = gp._canonical(gp.theta)[0]
        T = cand if name == "vr" else opt._last_batch_state["thompson"][0]
        for _ in range(q - 1):
            Xa = np.vstack([X0, cand[picks]])
            covs = np.empty(len(cand))
            for i in range(len(cand)):  # the reference's loop body on X_train_ + chosen points
                Xi = np.vstack([Xa, cand[i : i + 1]])
                Kaug = _k(Xi, Xi, h, plan) + np.exp(h[-1]) * np.eye(len(Xi))
                if np.iterable(gp.alpha):  # alpha added only as a vector, 0 for the chosen and the candidate rows
                    Kaug += np.diag(np.concatenate([alpha_vec, np.zeros(len(Xi) - len(X0))]))
                Kt = _k(T, Xi, h, plan)
                covs[i] = np.trace(Kt @ np.linalg.solve(Kaug, Kt.T))
            values.append(covs)
            v = covs.copy()
            v[picks] = -np.inf
            picks.append(int(np.argmax(v)))
        return picks, np.array(values)
    rows = opt._last_batch_state["rows"]
    n_samples = opt._last_batch_state["n_samples"]
    H = gp._canonical(rows)
    kw = opt.acq_func_kwargs
    lie_y = {"cl_min": np.min, "cl_mean": np.mean, "cl_max": np.max}.get(strategy)
    lie_y = None if lie_y is None else float(lie_y(opt.yi))
    base = [_latent(X0, y0, alpha_vec, h, cand, plan) for h in H]
    for _ in range(q - 1):
        P = cand[picks]
        Xa = np.vstack([X0, P])
        na = np.concatenate([alpha_vec, np.full(len(picks), base_alpha)])
        acc = np.zeros(len(cand))
        for b, h in enumerate(H):
            if lie_y is None:  # kriging believer: the row's own mean at each chosen point
                lies = base[b][0][picks]
            else:
                lies = np.full(len(picks), (lie_y - ym) / ys)
            mu, var = _latent(Xa, np.concatenate([y0, lies]), na, h, cand, plan)
            tmp = _closed_form(name, ys * mu + ym, np.sqrt(var * ys * ys), kw)
            if np.all(np.isfinite(tmp)):
                acc += tmp / n_samples
        values.append(acc)
        v = acc.copy()
        v[picks] = -np.inf
        picks.append(int(np.argmax(v)))
    return picks, np.array(values)


UNCERTAINTY = [("ei", None), ("ei", {"y_opt": -0.5}), ("lcb", None), ("mean", None), ("ttei", None)]


@pytest.mark.parametrize("name,kwargs", UNCERTAINTY)
def test_uncertainty_batches_match_the_oracle(bask, name, kwargs):
    opt = fitted(bask, name, kwargs=kwargs, n=40, m=300, n_samples=8)
    for strategy in ("cl_min", "cl_mean", "cl_max", "kb"):
        pts = opt.ask(4, strategy=strategy)
        info = opt._last_batch_info
        assert info["path"] == ("fallback" if name == "ttei" else "fast")
        picks, values = oracle_batch(opt, name, 4, strategy)
        assert info["picks"] == picks, (strategy, info["picks"], picks)
        scale = np.abs(values).max()
        np.testing.assert_allclose(info["values"], values, rtol=0, atol=1e-9 * scale)
        assert len(pts) == 4


@pytest.mark.parametrize("name", ["pvrs", "vr"])
def test_pvrs_batches_match_the_oracle(bask, name):
    opt = fitted(bask, name, n=30, d=3, m=300, n_samples=0)
    pts = opt.ask(4)
    info = opt._last_batch_info
    picks, values = oracle_batch(opt, name, 4, "cl_min")
    assert info["picks"] == picks
    np.testing.assert_allclose(info["values"], values, rtol=0, atol=1e-9 * np.abs(values).max())
    assert opt.ask(4, strategy="kb") == pts  # PVRS does not read y


# ------------------------------------------------------------------ fast path against fallback path
@pytest.mark.parametrize("name,strategy", [("ei", "cl_mean"), ("lcb", "kb"), ("mean", "cl_max")])
def test_fast_path_equals_fallback_path(bask, name, strategy):
    opt = fitted(bask, name, n=500, d=3, m=2000, n_samples=32, gp_samples=64)
    fast = opt.ask(8, strategy=strategy)
    f_info = opt._last_batch_info
    assert f_info["path"] == "fast" and f_info["device"]["steps"] == 7
    opt._batch_path = "fallback"
    slow = opt.ask(8, strategy=strategy)
    s_info = opt._last_batch_info
    assert s_info["path"] == "fallback"
    assert f_info["picks"] == s_info["picks"]
    # (rank-1 updates against a refactorised augmented set: the explicit-inverse variances cancel differently, measured
    # up to 3e-8 of the largest value at n = 500)
    np.testing.assert_allclose(f_info["values"], s_info["values"], rtol=0, atol=1e-7 * np.abs(s_info["values"]).max())
    assert [list(map(float, p)) for p in fast] == [list(map(float, p)) for p in slow]


def _valid_batch(opt, pts, q):
    assert len(pts) == q
    assert len({tuple(np.round(p, 15)) for p in pts}) == q
    for p in pts:
        assert all(dim.low <= v <= dim.high for v, dim in zip(p, opt.space.dimensions))


def test_fallback_batches_for_warped_inputs_and_generic_trees(bask):
    import sklearn.gaussian_process.kernels as sk

    opt = fitted(bask, "ei", n=20, d=2, m=200, n_samples=4, gp_kwargs=dict(warp_inputs=True), seed=1)
    pts = opt.ask(4)
    assert opt._last_batch_info["path"] == "fallback"
    _valid_batch(opt, pts, 4)
    opt = fitted(bask, "lcb", n=20, d=2, m=200, n_samples=4, seed=2,
                 gp_kernel=sk.ConstantKernel(1.0, (0.1, 10.0)) * sk.Matern(0.5, (0.05, 5.0), nu=2.5)
                 * sk.RBF(1.0, (0.05, 5.0)))
    assert opt.gp._generic
    pts = opt.ask(4)
    assert opt._last_batch_info["path"] == "fallback"
    _valid_batch(opt, pts, 4)


# ------------------------------------------------------------------ invariants
def test_batch_invariants(bask):
    opt = fitted(bask, "ei", n=40, m=300, n_samples=8, seed=3)
    single = opt.ask()
    state = opt.rng.get_state()
    batch = opt.ask(5)
    assert list(batch[0]) == list(single)
    assert opt.ask(5) == batch
    after = opt.rng.get_state()
    assert after[0] == state[0] and np.array_equal(after[1], state[1]) and after[2:] == state[2:]
    _valid_batch(opt, batch, 5)
    # kriging believer: the conditioned means are the unconditioned ones
    assert "moments" not in opt._last_batch_info and not hasattr(opt.gp, "_fantasy_last_moments")
    opt._batch_moments = True
    opt.ask(4, strategy="kb")
    mean_kb, _ = opt._last_batch_info["moments"]
    opt.ask(4, strategy="cl_max")
    mean_cl, _ = opt._last_batch_info["moments"]
    rows = opt._last_batch_state["rows"]
    mu0, _ = opt.gp._predict_hyper_samples(rows, opt._last_candidates, noise_zero=True)
    ym, ys = float(np.ravel(opt.gp.y_train_mean_)[0]), float(np.ravel(opt.gp.y_train_std_)[0])
    np.testing.assert_allclose(ys * mean_kb + ym, mu0, rtol=1e-12, atol=1e-12 * np.abs(mu0).max())
    assert not np.allclose(mean_cl, mean_kb)
    with pytest.raises(ValueError):
        opt.ask(3, strategy="cl_median")
    with pytest.raises(ValueError, match="candidates"):
        opt.ask(301)


def test_tell_after_batch_continues_like_a_single_ask(bask):
    a = fitted(bask, "ei", n=30, m=300, n_samples=6, seed=4)
    b = fitted(bask, "ei", n=30, m=300, n_samples=6, seed=4)
    batch = a.ask(4)
    x = b.ask()
    assert list(batch[0]) == list(x)
    ra = a.tell(batch[0], branin_like(batch[0]), n_samples=6, gp_samples=60, gp_burnin=2)
    rb = b.tell(x, branin_like(x), n_samples=6, gp_samples=60, gp_burnin=2)
    assert list(a.ask()) == list(b.ask())
    assert np.array_equal(a._last_acq_values, b._last_acq_values)
    assert ra.x == rb.x


class NegMean:
    """A whole-GP acquisition of the user's own: the median GP's predicted mean, negated (lowest mean first)."""

    def __call__(self, X, gp, *args, random_state=None, **kwargs):
        return -gp.predict(X)


def test_user_full_gp_acquisition_is_evaluated_as_itself(bask):
    """A FullGPAcquisition without a device form is called itself on the conditioned median GP, not replaced by VR."""
    from bayes_skopt_amd.acquisition import FullGPAcquisition

    neg_mean = type("NegMeanAcq", (NegMean, FullGPAcquisition), {})()
    opt = fitted(bask, neg_mean, n=40, m=300, n_samples=0, seed=7)
    gp = opt.gp
    cand = opt._last_candidates
    h = gp._canonical(gp.theta)[0]
    ym, ys = float(np.ravel(gp.y_train_mean_)[0]), float(np.ravel(gp.y_train_std_)[0])
    alpha_vec = np.broadcast_to(np.asarray(gp.alpha, dtype=np.float64), (len(gp._X_train_),))
    for strategy in ("cl_min", "cl_max", "kb"):
        pts = opt.ask(4, strategy=strategy)
        info = opt._last_batch_info
        assert info["path"] == "fallback"
        _valid_batch(opt, pts, 4)
        # restated: the median GP (its white level included, as predict sees it) on X + chosen points with the lies
        picks = [int(np.argmax(opt._last_acq_values))]
        lie = {"cl_min": min(opt.yi), "cl_max": max(opt.yi)}.get(strategy)
        mu0 = _latent(gp._X_train_, gp.y_train_, alpha_vec, h, cand, plan=gp._plan)[0]
        for _ in range(3):
            Xa = np.vstack([gp._X_train_, cand[picks]])
            lies = mu0[picks] if lie is None else np.full(len(picks), (lie - ym) / ys)
            na = np.concatenate([alpha_vec, np.full(len(picks), float(gp._alpha))])
            mu = _latent(Xa, np.concatenate([gp.y_train_, lies]), na, h, cand, plan=gp._plan)[0]
            v = -(ys * mu + ym)
            v[picks] = -np.inf
            picks.append(int(np.argmax(v)))
        assert info["picks"] == picks, (strategy, info["picks"], picks)


def test_pvrs_subclass_and_sample_acquisitions(bask):
    from bayes_skopt_amd.acquisition import PVRS, SampleAcquisition

    class MyPVRS(PVRS):
        pass

    opt = fitted(bask, MyPVRS(), n=30, m=200, n_samples=0, seed=8)
    first = opt.ask()
    pts = opt.ask(3)
    assert opt._last_batch_info["path"] == "fallback" and list(pts[0]) == list(first)
    _valid_batch(opt, pts, 3)
    assert opt.ask(3) == pts  # (the Thompson draws replay the proposal's generator state)

    class Flat(SampleAcquisition):
        def __call__(self, gp_sample, *args, **kwargs):
            return -gp_sample

    opt = fitted(bask, Flat(), n=20, m=100, n_samples=2, seed=9)
    with pytest.raises(NotImplementedError, match="sample acquisitions"):
        opt.ask(2)


def test_thompson_sampling_has_no_batch(bask):
    opt = fitted(bask, "ts", n=20, m=100, n_samples=2, seed=5)
    with pytest.raises(NotImplementedError, match="Thompson"):
        opt.ask(2)
    assert opt.ask(1) is not None


# ------------------------------------------------------------------ the initial design
def test_r2_batch_is_the_next_design_points(bask):
    one = bask.Optimizer(dimensions=[(-1.0, 1.0)] * 2, n_initial_points=6, init_strategy="r2", random_state=0)
    many = bask.Optimizer(dimensions=[(-1.0, 1.0)] * 2, n_initial_points=6, init_strategy="r2", random_state=0)
    seq = []
    for _ in range(4):
        x = one.ask()
        seq.append(list(x))
        one.tell(x, branin_like(x), fit=False)
    assert [list(p) for p in many.ask(4)] == seq
    many.tell(many.ask(4), [0.0] * 4, fit=False)
    tail = many.ask(5)  # 2 design points left, 3 random ones
    assert [list(p) for p in tail[:2]] == [list(many._initial_points[1]), list(many._initial_points[0])]
    _valid_batch(many, tail, 5)


@pytest.mark.parametrize("init_strategy", ["sb", "random"])
def test_design_batches_are_distinct_points_in_the_space(bask, init_strategy):
    opt = bask.Optimizer(dimensions=[(-1.0, 1.0)] * 2, n_initial_points=4, init_strategy=init_strategy, random_state=0)
    pts = opt.ask(3)
    _valid_batch(opt, pts, 3)
    opt.tell(pts, [branin_like(p) for p in pts], fit=False)
    pts = opt.ask(3)  # one design point left, two random ones
    _valid_batch(opt, pts, 3)


# ------------------------------------------------------------------ end to end
def test_batch_loop(bask):
    opt = bask.Optimizer(dimensions=[(-1.0, 1.0)] * 2, n_points=500, n_initial_points=8, acq_func="ei", random_state=0)
    for _ in range(6):
        xs = opt.ask(4)
        res = opt.tell(xs, [branin_like(x) for x in xs], n_samples=8, gp_samples=60, gp_burnin=2)
    assert len(opt.Xi) == 24 and len({tuple(x) for x in opt.Xi}) == 24
    assert res.fun == min(opt.yi)


def test_bayes_search_cv_with_batches(bask):
    from sklearn.datasets import load_iris
    from sklearn.svm import SVC

    X, y = load_iris(return_X_y=True)
    search = bask.BayesSearchCV(SVC(), {"C": bask.space.Real(1e-3, 1e3, prior="log-uniform"),
                                        "gamma": bask.space.Real(1e-4, 1e1, prior="log-uniform")},
                                n_iter=9, n_points=3, cv=3, random_state=0,
                                optimizer_kwargs=dict(n_initial_points=3, gp_samples=40, n_points=200))
    search.fit(X, y)
    assert len(search.cv_results_["params"]) == 9
    assert set(search.best_params_) == {"C", "gamma"}
    assert search.best_score_ >= 0.9


# ------------------------------------------------------------------ the device path at config E shape
def test_fast_path_runs_at_config_e_shape(bask):
    opt = fitted(bask, "ei", n=974, d=6, m=10000, n_samples=128, gp_samples=160, seed=6)
    pts = opt.ask(4)
    info = opt._last_batch_info
    assert info["path"] == "fast" and info["device"] == {"begins": 1, "steps": 3}
    _valid_batch(opt, pts, 4)
    pv = fitted(bask, "pvrs", n=974, d=6, m=10000, n_samples=0, gp_samples=160, seed=6)
    pts = pv.ask(2)
    _valid_batch(pv, pts, 2)
