"""The device-resident optimum search (bgp_minimize_starts, utils.expected_optimum, Optimizer.expected_optimum; DESIGN.md section
13) on three surrogates -- n = 60 / d = 3 / 21 starts, n = 300 / d = 4 / 21 starts, n = 974 / d = 8 / 101 starts; Matern 5/2, ARD,
with a white term -- for the mean (kappa = 0) and, on the last two, the upper bound mean + 1.96 std.  The reference is
``utils.expected_minimum`` as it stands (kappa = 0) and the same scipy loop over ``predict(return_std=True)`` otherwise, with the
same ``random_state`` and therefore the same starts.  Per-start end points are NOT compared: the two methods legitimately end in
different basins from the same start."""
import numpy as np
import pytest
from sklearn.utils import check_random_state

pytestmark = pytest.mark.gpu

GTOL = 1e-5
SEED = 7
PROBLEMS = {"n60_d3": (60, 3, 21), "n300_d4": (300, 4, 21), "n974_d8": (974, 8, 101)}
CASES = [("n60_d3", 0.0), ("n300_d4", 0.0), ("n300_d4", 1.96), ("n974_d8", 0.0), ("n974_d8", 1.96)]


@pytest.fixture(scope="module")
def bask():
    import bayes_skopt_amd as bask

    assert bask._lib.device_count() >= 1
    return bask


_cache = {}


def _surrogate(bask, name):
    """(res, gp, space) of a fitted surrogate on a box that is not the unit box."""
    if name in _cache:
        return _cache[name]
    from bayes_skopt_amd.space import Space, create_result

    n, d, _ = PROBLEMS[name]
    rng = np.random.RandomState(100 + n)
    space = Space([(-2.0, 3.0)] * d)
    Xt = rng.uniform(size=(n, d))
    y = np.sin(3.0 * Xt.sum(axis=1)) + np.sum((Xt - 0.4) ** 2, axis=1) + 0.5 * np.cos(7.0 * Xt[:, 0]) + 0.05 * rng.randn(n)
    Xi = space.inverse_transform(Xt)
    gp = bask.BayesGPR(kernel=bask.construct_default_kernel(list(range(d))), normalize_y=True, random_state=1)
    gp.fit(space.transform(Xi), y, n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
    assert gp._post.canonical and gp.noise_ is not None  # (ARD Matern 5/2 with a white term)
    _cache[name] = (create_result(Xi, list(y), space, models=[gp]), gp, space)
    return _cache[name]


def _starts(res, space, S):
    rng = check_random_state(SEED)
    return space.transform([res.x] + space.rvs(S - 1, random_state=rng))


def _objective(gp, mean, var, kappa):
    y_mean, y_std = float(np.ravel(gp.y_train_mean_)[0]), float(np.ravel(gp.y_train_std_)[0])
    return y_mean + y_std * mean + kappa * (y_std * np.sqrt(var))


def _scipy_upper_bound(res, kappa, n_random_starts, random_state):
    """``utils.expected_minimum``'s loop on mean + kappa std: the reference for kappa != 0."""
    from scipy.optimize import minimize

    space, reg = res.space, res.models[-1]
    bounds = np.asarray(space.bounds, dtype=np.float64)
    d = len(bounds)
    eps = np.sqrt(np.finfo(np.float64).eps)

    def fun_and_grad(x):
        h = eps * np.maximum(1.0, np.abs(x))
        sign = np.where(x + h > bounds[:, 1], -1.0, 1.0)
        pts = np.tile(x, (d + 1, 1))
        pts[1:, :][np.arange(d), np.arange(d)] += sign * h
        mu, sd = reg.predict(space.transform(pts.tolist()), return_std=True)
        vals = np.asarray(mu) + kappa * np.asarray(sd)
        return float(vals[0]), (vals[1:] - vals[0]) / (sign * h)

    rng = check_random_state(random_state)
    xs = [res.x] + space.rvs(n_random_starts, random_state=rng)
    best = np.inf
    for x0 in xs:
        best = min(best, minimize(fun_and_grad, x0=np.asarray(x0, dtype=np.float64), jac=True, bounds=space.bounds,
                                  method="L-BFGS-B").fun)
    return float(best)


def _projected_gradient(gp, x, kappa):
    """inf-norm of the projected gradient of mean + kappa std at x (unit box), from the existing host one-point gradient."""
    _m, _s, gm, gs = gp.predict(x[None, :], return_std=True, return_mean_grad=True, return_std_grad=True)
    g = gm + kappa * gs
    g = np.where(((x <= 0.0) & (g > 0.0)) | ((x >= 1.0) & (g < 0.0)), 0.0, g)
    return float(np.abs(g).max())


@pytest.mark.parametrize("name,kappa", CASES)
def test_every_start_and_the_best_value(bask, name, kappa):
    from bayes_skopt_amd import utils as U

    res, gp, space = _surrogate(bask, name)
    S = PROBLEMS[name][2]
    x, value, info = U.expected_optimum(res, kappa=kappa, n_random_starts=S - 1, random_state=SEED, gtol=GTOL)
    assert info["path"] == "device"
    X0 = _starts(res, space, S)
    xt, st = info["x_transformed"], info["status"]
    assert xt.shape == X0.shape and np.all(xt >= 0.0) and np.all(xt <= 1.0)
    assert set(np.unique(st)) <= {0, 1, 2}
    # the end points' moments are the bits of predict_grad there; the objective never rises from a start
    mean, var, _dm, _dv = gp._post.predict_grad(gp, xt)
    np.testing.assert_array_equal(mean, info["mean"])
    np.testing.assert_array_equal(var, info["var"])
    np.testing.assert_array_equal(_objective(gp, mean, var, kappa), info["fun"])
    m0, v0, _dm, _dv = gp._post.predict_grad(gp, X0)
    f0 = _objective(gp, m0, v0, kappa)
    assert np.all(info["fun"] <= f0), (info["fun"] - f0).max()
    # converged starts: the projected gradient, recomputed on the host
    worst = max([_projected_gradient(gp, xt[i], kappa) for i in np.flatnonzero(st == 0)] + [0.0])
    conv = int(np.sum(st == 0))
    print("OPTIMUM %-8s kappa %.2f  converged %d / %d  status %s  iters max %d  evals mean %.1f max %d  worst |pg| %.2e"
          % (name, kappa, conv, S, np.bincount(st, minlength=3).tolist(), info["iters"].max(), info["evals"].mean(),
             info["evals"].max(), worst))
    assert worst <= 2 * GTOL
    if S == 21:
        assert conv == S, st
    else:
        assert conv >= 0.95 * S, st
    assert st[info["best"]] == 0
    # best value against the scipy reference
    if kappa == 0.0:
        ref = U.expected_minimum(res, n_random_starts=S - 1, random_state=SEED)[1]
    else:
        ref = _scipy_upper_bound(res, kappa, S - 1, SEED)
    print("OPTIMUM %-8s kappa %.2f  device %.12g  scipy %.12g  diff %.2e" % (name, kappa, value, ref, value - ref))
    assert value == info["fun"][info["best"]] == info["fun"].min()
    assert value <= ref + 1e-6 * np.ptp(res.func_vals)
    # x is the best end point in the original space
    np.testing.assert_allclose(space.transform([x])[0], xt[info["best"]], rtol=0, atol=1e-12)


@pytest.mark.parametrize("kappa", [0.0, 1.96])
def test_determinism_and_independence_of_the_starts(bask, kappa):
    res, gp, space = _surrogate(bask, "n300_d4")
    X0 = _starts(res, space, 21)
    a = gp._post.minimize(gp, kappa, X0, 0.0, 1.0, gtol=GTOL, max_iter=200)
    b = gp._post.minimize(gp, kappa, X0, 0.0, 1.0, gtol=GTOL, max_iter=200)
    first = gp._post.minimize(gp, kappa, X0[:5], 0.0, 1.0, gtol=GTOL, max_iter=200)
    for key in ("x", "mean", "var", "iters", "evals", "status"):
        np.testing.assert_array_equal(a[key], b[key])
        np.testing.assert_array_equal(a[key][:5], first[key])
    # every loop is capped: with max_iter = 3 the search stops there, inside the box, not above its start
    capped = gp._post.minimize(gp, kappa, X0, 0.0, 1.0, gtol=GTOL, max_iter=3)
    assert np.all(capped["iters"] <= 3) and np.all(capped["evals"] <= 2 + 3 * 30)
    assert np.all(capped["iters"][capped["status"] == 1] == 3)
    assert np.all(capped["x"] >= 0.0) and np.all(capped["x"] <= 1.0)
    # a box smaller than the unit box is respected exactly
    lo, hi = np.full(4, 0.25), np.array([0.5, 0.75, 0.3, 1.0])
    boxed = gp._post.minimize(gp, kappa, X0, lo, hi, gtol=GTOL, max_iter=200)
    assert np.all(boxed["x"] >= lo) and np.all(boxed["x"] <= hi)


def test_optimizer_expected_optimum_and_the_diagnostics(bask):
    opt = bask.Optimizer(dimensions=[(-2.0, 2.0), (0, 10)], n_initial_points=6, random_state=0)
    opt.run(lambda x: float(np.sin(2.0 * x[0]) + 0.05 * (x[1] - 4) ** 2), n_iter=12, n_samples=1, gp_samples=40, gp_burnin=5)
    res = opt._result()
    x, value, info = opt.expected_optimum(n_random_starts=20, random_state=3)
    assert info["path"] == "device" and len(info["status"]) == 21
    assert -2.0 <= x[0] <= 2.0 and 0.0 <= x[1] <= 10.0 and isinstance(x[1], float)  # (un-rounded, as expected_minimum's)
    at_best = opt.gp.predict_gradients(opt.space.transform([res.x]), return_std=False)[0][0]
    assert value <= at_best
    xu, vu, _ = opt.expected_optimum(kappa=1.96, n_random_starts=20, random_state=3)
    assert np.isfinite(vu) and -2.0 <= xu[0] <= 2.0 and 0.0 <= xu[1] <= 10.0
    kw = dict(n_space_samples=60, n_gp_samples=40, n_random_starts=10, random_state=1)
    p_dev = opt.probability_of_optimality(0.1, minimizer="device", **kw)
    assert 0.0 <= p_dev <= 1.0
    p1, p2 = opt.probability_of_optimality(0.1, **kw), opt.probability_of_optimality(0.1, **kw)
    assert p1 == p2 == opt.probability_of_optimality(0.1, minimizer="scipy", **kw) and 0.0 <= p1 <= 1.0
    gap = opt.expected_optimality_gap(n_probabilities=10, minimizer="device", **kw)
    assert np.isfinite(gap) and gap >= 0.0
    with pytest.raises(ValueError):
        opt.probability_of_optimality(0.1, minimizer="host", **kw)


def test_categorical_spaces_raise(bask):
    from bayes_skopt_amd import utils as U
    from bayes_skopt_amd.space import Space, create_result

    res = create_result([[0.1, "a"]], [1.0], Space([(0.0, 1.0), ["a", "b"]]), models=[None])
    with pytest.raises(ValueError, match="categorical"):
        U.expected_optimum(res)


def test_the_fallback_says_so_once(bask, capfd, monkeypatch):
    """A warped surrogate takes the host loop: expected_minimum's result for kappa = 0, the same loop on mean + kappa std
    otherwise, and one line on stderr for the process."""
    from bayes_skopt_amd import utils as U
    from bayes_skopt_amd.space import Space, create_result

    monkeypatch.setattr(U, "_told", set())
    rng = np.random.RandomState(0)
    space = Space([(-1.0, 1.0)])
    Xt = rng.uniform(size=(40, 1))
    y = np.sin(6.0 * Xt[:, 0]) + 0.05 * rng.randn(40)
    gp = bask.BayesGPR(kernel=bask.construct_default_kernel([0]), random_state=1, warp_inputs=True, normalize_y=True)
    gp.fit(Xt, y, n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
    res = create_result(space.inverse_transform(Xt), list(y), space, models=[gp])
    capfd.readouterr()
    x, value, info = U.expected_optimum(res, n_random_starts=3, random_state=2)
    assert info == {"path": "host"}
    xr, vr = U.expected_minimum(res, n_random_starts=3, random_state=2)
    assert x == xr and value == vr
    xu, vu, _ = U.expected_optimum(res, kappa=1.96, n_random_starts=3, random_state=2)
    assert vu == _scipy_upper_bound(res, 1.96, 3, 2)
    err = capfd.readouterr().err
    assert err.count("expected_optimum: this search is driven from the host") == 1, err
