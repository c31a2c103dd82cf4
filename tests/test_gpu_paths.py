"""Pathwise posterior function draws on the device (bgp_paths_*, BayesGPR.sample_paths, mvn="pathwise"):
device values and gradients against the long-double reference of tests/_pathref.py at the tolerance class
tests/test_cpu_paths_reference.py qualifies, the degenerate paths against ``bgp_predict_batch`` and a hand formula, bitwise
independence of a (path, row) from what shares its call, states and limits, the API, the ensemble moments, the optimiser.
Lines start with ``PRECISION``."""
import numpy as np
import pytest

import _pathref as R
import _precision as P
from conftest import synth
from test_cpu_paths_reference import MOMENT_CASES, MOMENT_F, MOMENT_PATHS, MOMENT_SEED, moment_deviations, moment_problem

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)


@pytest.fixture(scope="module")
def bask():
    import bayes_skopt_amd as bask

    assert bask._lib.device_count() >= 1
    return bask


def _check(tag, quantity, err, t):
    print("PRECISION %-52s %-6s err/tol %.3e" % (tag, quantity, err / t))
    assert err <= t, "%s %s: error %.3e > tol %.3e (%.1fx)" % (tag, quantity, err, t, err / t)


def _begin(bask, cid, **over):
    """A context with the case's posteriors resident and its paths begun; returns (ctx, problem dict)."""
    from bayes_skopt_amd._posterior import noise_off

    c, pr = R.ALL[cid], dict(R.problem(cid), **over)
    ctx = bask._lib.Context(pr["X"], pr["y"], pr["alpha"], form=c["form"], stationary=c["stationary"], max_batch=2)
    assert np.all(ctx.posterior(pr["H"])["status"] == 0)
    Hp = pr["H"][pr["pidx"]]
    ctx.paths_begin(pr["pidx"], noise_off(Hp), Hp[:, -1], pr["omega"], pr["phase"], pr["w"], pr["eps"])
    return ctx, pr


# ---- 1. values and gradients against the extended-precision reference ----------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES])
def test_device_paths_against_the_extended_precision_reference(bask, cid):
    ctx, pr = _begin(bask, cid)
    f, df = ctx.paths_eval(pr["Xq"], want_grad=True)
    f2, none = ctx.paths_eval(pr["Xq"])
    ctx.close()
    assert none is None and f.shape == (R.ALL[cid]["P"], R.ALL[cid]["m"]) and df.shape == f.shape + (R.ALL[cid]["d"],)
    np.testing.assert_array_equal(f, f2)  # (the same bits with and without the gradient)
    assert np.all(np.isfinite(f)) and np.all(np.isfinite(df))
    ev, eg = R.err(f, df, R.ref_paths(cid))
    _check(cid, "f", ev, R.case_tol(cid))
    _check(cid, "df", eg, R.case_tol(cid))


# ---- 2. degenerate paths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [R.CASES[1]["id"], R.CASES[4]["id"], R.CASES[9]["id"]])
def test_a_path_without_randomness_is_the_predictive_mean(bask, cid):
    """w = 0, eps = 0: f0 = 0, r = y, v = K^-1 y = alpha -- the path is ``bgp_predict_batch``'s mean, at the "mean" tolerance."""
    from bayes_skopt_amd._posterior import noise_off
    from oracle import hp_oracle as HP

    c, pr = R.ALL[cid], R.problem(cid)
    ctx, _ = _begin(bask, cid, w=np.zeros_like(pr["w"]), eps=np.zeros_like(pr["eps"]))
    f, _ = ctx.paths_eval(pr["Xq"])
    mean, _var = ctx.predict(noise_off(pr["H"]), pr["Xq"])
    ctx.close()
    for p, b in enumerate(pr["pidx"]):
        post = HP.posterior(pr["X"], pr["y"], pr["alpha"], pr["H"][b], c["stationary"], c["form"])
        Ks = HP.gram(pr["Xq"], pr["H"][b], c["stationary"], c["form"], Y=pr["X"])
        scale = float(np.abs(Ks * post["alpha"][None, :]).sum(axis=1).max())
        _check("%s path %d" % (cid, p), "mean", P.err_rel_max(f[p], mean[b], scale), P.tol("mean", pr["kappa"][b], c["n"]))


def test_one_training_point_without_data_is_the_hand_formula(bask):
    """n = 1, y = 0, eps = 0: f(x) = f0(x) - k(x, X_0) f0(X_0) / (c + s2 + alpha)."""
    X, alpha = np.array([[0.3, 0.6]]), 1e-3
    h = np.array([np.log(1.7), np.log(0.4), np.log(0.7), np.log(0.05)])
    rng = np.random.RandomState(5)
    omega, phase, w, _ = R.draw_variates(rng, 1, 5, 2, 1, "matern32")
    Xq = rng.uniform(size=(4, 2))
    ctx = bask._lib.Context(X, np.zeros(1), alpha, form="product", stationary="matern32", max_batch=1)
    assert np.all(ctx.posterior(h[None])["status"] == 0)
    hk = h.copy()
    hk[-1] = -np.inf
    ctx.paths_begin([0], hk[None], h[-1:], omega, phase, w, np.zeros((1, 1)))
    f, _ = ctx.paths_eval(Xq)
    ctx.close()
    cst, ell, s2 = np.exp(h[0]), np.exp(h[1:3]), np.exp(h[3])

    def f0(Z):
        return np.sqrt(2 * cst / 5) * (np.cos(phase[0][None, :] + (Z / ell) @ omega[0].T) @ w[0][:5])

    t = np.sqrt(3.0) * np.sqrt((((Xq - X) / ell) ** 2).sum(axis=1))
    want = f0(Xq) - cst * (1 + t) * np.exp(-t) * f0(X)[0] / (cst + s2 + alpha)
    np.testing.assert_allclose(f[0], want, rtol=1e-12, atol=1e-13)


# ---- 3. bits --------------------------------------------------------------------------------------------------------------
def test_a_value_does_not_depend_on_what_shares_the_call(bask):
    """A row alone, inside 257 rows, with and without the other paths; and after the resident posteriors have been rebuilt with
    other hyper-parameters: identical bits."""
    from bayes_skopt_amd._posterior import noise_off

    cid = R.CASES[4]["id"]  # 257 rows, three paths on two posteriors, F = 200, n = 130
    ctx, pr = _begin(bask, cid)
    Xq = pr["Xq"]
    f, df = ctx.paths_eval(Xq, want_grad=True)
    for i in (0, 100, 255, 256):
        fi, dfi = ctx.paths_eval(Xq[i : i + 1], want_grad=True)
        np.testing.assert_array_equal(fi[:, 0], f[:, i])
        np.testing.assert_array_equal(dfi[:, 0], df[:, i])
    lo, _ = ctx.paths_eval(Xq[:100])
    hi, _ = ctx.paths_eval(Xq[100:])
    np.testing.assert_array_equal(np.concatenate([lo, hi], axis=1), f)
    H2 = pr["H"] + 0.05
    assert np.all(ctx.posterior(H2)["status"] == 0)
    after, dafter = ctx.paths_eval(Xq, want_grad=True)
    np.testing.assert_array_equal(after, f)
    np.testing.assert_array_equal(dafter, df)
    assert np.all(ctx.posterior(pr["H"])["status"] == 0)
    Hp = pr["H"][pr["pidx"]]
    for p in range(3):  # every path alone, on a state of its own
        ctx.paths_begin(pr["pidx"][p : p + 1], noise_off(Hp[p : p + 1]), Hp[p : p + 1, -1], pr["omega"][p : p + 1],
                        pr["phase"][p : p + 1], pr["w"][p : p + 1], pr["eps"][p : p + 1])
        alone, dalone = ctx.paths_eval(Xq, want_grad=True)
        np.testing.assert_array_equal(alone[0], f[p])
        np.testing.assert_array_equal(dalone[0], df[p])
    ctx.close()


# ---- 4. states and limits ---------------------------------------------------------------------------------------------------
def test_states_and_limits_are_errors_not_crashes(bask):
    lib = bask._lib
    X, y = synth(40, 2, 3)
    h = np.array([0.0, np.log(0.4), np.log(0.4), np.log(1e-2)])
    hk = np.array([0.0, np.log(0.4), np.log(0.4), -np.inf])
    om, ph, w, eps = R.draw_variates(np.random.RandomState(1), 1, 8, 2, 40, "matern52")
    ctx = lib.Context(X, y, 1e-8, max_batch=1)
    assert ctx.paths_stats() == {"begins": 0, "evals": 0}
    with pytest.raises(lib.BgpError, match=r"code 4.*bgp_paths_begin first"):
        ctx.paths_eval(X[:3])
    with pytest.raises(lib.BgpError, match=r"code 4.*no resident posteriors"):
        ctx.paths_begin([0], hk[None], h[-1:], om, ph, w, eps)
    ctx.posterior(h[None])
    with pytest.raises(lib.BgpError, match=r"code 4.*names posterior 1"):
        ctx.paths_begin([1], hk[None], h[-1:], om, ph, w, eps)
    with pytest.raises(lib.BgpError, match=r"code 1.*0 features"):
        ctx.paths_begin([0], hk[None], h[-1:], np.empty((1, 0, 2)), np.empty((1, 0)), np.zeros((1, 1)), eps)
    ctx.set_warp(np.zeros(4))
    ctx.posterior(h[None])
    with pytest.raises(lib.BgpError, match=r"code 1.*warped inputs"):
        ctx.paths_begin([0], hk[None], h[-1:], om, ph, w, eps)
    ctx.set_warp(None)
    ctx.posterior(h[None])
    ctx.paths_begin([0], hk[None], h[-1:], om, ph, w, eps)
    f, _ = ctx.paths_eval(X[:3])
    f2, _ = ctx.paths_eval(X[:3])
    np.testing.assert_array_equal(f, f2)
    assert ctx.paths_stats() == {"begins": 1, "evals": 2}
    ctx.update_data(X[:30], y[:30], 1e-8)
    with pytest.raises(lib.BgpError, match=r"code 4.*bgp_paths_begin first"):
        ctx._paths_P = 1
        ctx.paths_eval(X[:3])
    ctx.posterior(h[None])
    ctx.paths_begin([0], hk[None], h[-1:], om, ph, w, eps[:, :30])
    ctx.paths_end()
    with pytest.raises(lib.BgpError, match="code 4"):
        ctx._paths_P = 1
        ctx.paths_eval(X[:3])
    assert ctx.paths_stats() == {"begins": 2, "evals": 2}
    ctx.close()
    X, y = synth(40, 33, 3)
    h = np.concatenate([[0.0], np.full(33, np.log(2.0)), [np.log(1e-2)]])
    ctx = lib.Context(X, y, 1e-8, max_batch=1)
    ctx.posterior(h[None])
    om, ph, w, eps = R.draw_variates(np.random.RandomState(1), 1, 8, 33, 40, "matern52")
    with pytest.raises(lib.BgpError, match=r"code 1.*d > 32"):
        ctx.paths_begin([0], h[None], h[-1:], om, ph, w, eps)
    ctx.close()


# ---- 5. the API ---------------------------------------------------------------------------------------------------------------
def _kernels():
    from bayes_skopt_amd.kernels import RBF, ConstantKernel, Matern

    return {
        "matern52": ConstantKernel(1.0, (0.1, 2.0)) * Matern([0.4, 0.3, 0.5], (0.2, 0.8), nu=2.5),
        "rbf": ConstantKernel(1.0, (0.1, 2.0)) * RBF([0.4, 0.3, 0.5], (0.2, 0.8)),
        "sum_matern12": ConstantKernel(0.5, (0.1, 2.0)) + Matern(0.6, (0.2, 0.9), nu=0.5),
    }


def _data():
    """60 points in three dimensions, targets shifted by 5 and scaled by 3: far from normalised."""
    rng = np.random.RandomState(3)
    X = rng.uniform(size=(60, 3))
    return X, 5.0 + 3.0 * (np.sin(3.0 * X.sum(axis=1)) + 0.05 * rng.randn(60))


@pytest.fixture(scope="module")
def fitted(bask):
    """kind -> a BayesGPR fitted to ``_data()`` (fitted once per kind)."""
    cache = {}

    def get(kind):
        if kind not in cache:
            X, y = _data()
            gp = bask.BayesGPR(kernel=_kernels()[kind], random_state=0, normalize_y=True)
            gp.fit(X, y, n_desired_samples=40, n_burnin=5, n_walkers_per_thread=20, progress=False)
            cache[kind] = gp
        return cache[kind]

    return get


@pytest.mark.parametrize("kind, sample_mean", [("matern52", False), ("sum_matern12", False), ("rbf", True)])
def test_sample_paths_is_the_restatement_seeded_alike(bask, fitted, kind, sample_mean):
    """Shapes, y units, and every path reproduced from the seed alone by the long-double restatement (rows first, then the
    variates per path) at the tolerance of the C-ABI test."""
    gp = fitted(kind)
    Xq = np.random.RandomState(9).uniform(-0.05, 1.05, size=(20, 3))
    n_paths, F, seed = 3, 64, 17
    with gp.sample_paths(n_paths=n_paths, sample_mean=sample_mean, n_features=F, random_state=seed) as paths:
        f, g = paths(Xq), paths.gradient(Xq)
    assert f.shape == (20, n_paths) and g.shape == (20, n_paths, 3)
    with pytest.raises(RuntimeError):
        paths(Xq)
    rng = np.random.RandomState(seed)
    n_theta = len(gp.kernel_.theta)
    if sample_mean:
        thetas = np.tile(gp._post_theta[None, :n_theta], (n_paths, 1))
    else:
        thetas = gp.chain_[rng.choice(len(gp.chain_), size=n_paths, replace=True)][:, :n_theta]
    H = gp._canonical(thetas)
    X, y, alpha = gp._X_train_, gp.y_train_, gp._alpha_diag()
    omega, phase, w, eps = R.draw_variates(rng, n_paths, F, 3, len(X), gp._plan.stationary)
    ym, ys = float(np.ravel(gp.y_train_mean_)[0]), float(np.ravel(gp.y_train_std_)[0])
    yraw = _data()[1]  # (y units: the estimator's normalisation is that of the raw targets, which are far from normalised)
    np.testing.assert_allclose([ym, ys], [yraw.mean(), yraw.std()], rtol=1e-12)
    assert abs(ym) > 3.0 * ys / np.sqrt(len(yraw)) and abs(ys - 1.0) > 0.5
    for p in range(n_paths):
        rf, rdf, s, sg = R._path(hp.LD, R._solve_ld, X, y, alpha, H[p], omega[p], phase[p], w[p], eps[p], Xq, gp._plan.stationary,
                                 gp._plan.form)
        t = R.tol(P.kappa_of(X, alpha, H[p], gp._plan.stationary, gp._plan.form), len(X))
        ev = float((np.abs(f[:, p] - P.f(ys * rf + ym)) / (ys * P.f(s))).max())
        eg = float((np.abs(g[:, p] - P.f(ys * rdf)) / (ys * np.maximum(P.f(sg), 1e-300))).max())
        _check("%s path %d" % (kind, p), "f", ev, t)
        _check("%s path %d" % (kind, p), "df", eg, t)


def test_sample_y_pathwise_is_sample_paths_and_an_object_is_a_function(bask, fitted):
    gp = fitted("matern52")
    rng = np.random.RandomState(4)
    Xq = rng.uniform(size=(30, 3))
    for sample_mean in (False, True):
        a = gp.sample_y(Xq, sample_mean=sample_mean, n_samples=4, random_state=21, mvn="pathwise")
        with gp.sample_paths(n_paths=4, sample_mean=sample_mean, random_state=21) as paths:
            b = paths(Xq)
            again = paths(Xq)
            superset = paths(np.vstack([rng.uniform(size=(300, 3)), Xq]))
        assert a.shape == (30, 4)
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(b, again)
        np.testing.assert_array_equal(b, superset[300:])
    assert gp.sample_y(Xq, n_samples=2, random_state=1).shape == (30, 2) and gp.mvn == "auto"  # ("auto" is untouched)
    rows = gp.__class__._sample_hyper_rows
    gp.mvn = "pathwise"
    try:
        got = rows(gp, 3, Xq, np.random.RandomState(8))
    finally:
        gp.mvn = "auto"
    with gp.sample_paths(n_paths=3, random_state=np.random.RandomState(8)) as paths:
        np.testing.assert_array_equal(got, paths(Xq).T)


@pytest.mark.parametrize("kind", ["matern52", "rbf", "sum_matern12"])
def test_path_gradients_match_central_differences(bask, fitted, kind):
    """``paths.gradient`` against central differences of the same object, at the rtol of
    ``test_predict_gradients_match_finite_differences`` (2e-5; its atol 1e-7 scaled by the 3.0 of these targets)."""
    gp = fitted(kind)
    x0 = np.array([[0.37, 0.52, 0.61], [0.8, 0.1, 0.4]])
    with gp.sample_paths(n_paths=2, n_features=32, random_state=2) as paths:
        g = paths.gradient(x0)
        h, fd = 1e-5, np.zeros((2, 2, 3))
        for k in range(3):
            e = np.zeros(3)
            e[k] = h
            fd[:, :, k] = (paths(x0 + e) - paths(x0 - e)) / (2 * h)
    np.testing.assert_allclose(g, fd, rtol=2e-5, atol=3e-7)


# ---- 6. the ensemble of paths has predict's moments ----------------------------------------------------------------------
@pytest.mark.parametrize("stationary,form", MOMENT_CASES)
def test_ensemble_moments_match_predict(bask, stationary, form):
    """4096 paths of the median GP (n = 23, d = 3, m = 9, F = 64): ensemble mean within 5 standard errors of ``predict``, ensemble
    variance within 5 standard errors of ``predict``'s variance with the noise off; every row counts."""
    from bayes_skopt_amd.kernels import ConstantKernel, Matern

    X, y, _alpha, _h, Xq = moment_problem(stationary, form)
    nu = R.NU[stationary]
    if form == "product":
        kernel = ConstantKernel(1.0, (0.1, 2.0)) * Matern([0.4, 0.3, 0.5], (0.2, 0.8), nu=nu)
    else:
        kernel = ConstantKernel(0.5, (0.1, 2.0)) + Matern(0.6, (0.2, 0.9), nu=nu)
    gp = bask.BayesGPR(kernel=kernel, random_state=0, normalize_y=True)
    gp.fit(X, y, n_desired_samples=40, n_burnin=5, n_walkers_per_thread=20, progress=False)
    with gp.sample_paths(n_paths=MOMENT_PATHS, sample_mean=True, n_features=MOMENT_F, random_state=MOMENT_SEED) as paths:
        f = paths(Xq).T
    with gp.noise_set_to_zero():
        mean, std = gp.predict(Xq, return_std=True)
    zm, zv = moment_deviations(f, mean, std**2)
    print("PRECISION moments %s %s: ensemble mean %.2f, ensemble variance %.2f standard errors" % (stationary, form, zm, zv))
    assert zm <= 5.0 and zv <= 5.0, (zm, zv)


# ---- 7. the optimiser ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("acq", ["ts", "pvrs"])
def test_optimizer_proposes_with_pathwise_draws(bask, acq):
    rng = np.random.RandomState(0)
    opt = bask.Optimizer(dimensions=[(0.0, 1.0)] * 2, n_points=2000, n_initial_points=6, init_strategy="r2", acq_func=acq,
                         random_state=0)
    opt.gp.mvn = "pathwise"
    seen = []
    real = opt.gp.sample_paths

    def spy(*a, **k):
        seen.append(k.get("n_paths"))
        return real(*a, **k)

    opt.gp.sample_paths = spy
    for _ in range(7):
        x = opt.ask()
        opt.tell(x, float(np.sin(3 * np.sum(x)) + 0.05 * rng.randn()), gp_samples=40, gp_burnin=2, n_samples=3)
    nxt = opt.ask()
    assert len(nxt) == 2 and all(0.0 <= v <= 1.0 for v in nxt)
    assert len(seen) >= 2 and opt._last_candidates.shape == (2000, 2)  # (every proposal drew its functions pathwise)


def test_warped_inputs_fall_back_with_one_line(bask, capfd):
    from bayes_skopt_amd import bayesgpr

    X, y = synth(60, 2, 8)
    gp = bask.BayesGPR(kernel=bask.construct_default_kernel([0, 1]), random_state=1, warp_inputs=True, normalize_y=True,
                       mvn="pathwise")
    gp.fit(X, y, n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
    Xq = np.random.RandomState(2).uniform(0.1, 0.9, size=(6, 2))
    del bayesgpr._pathwise_told[:]
    capfd.readouterr()
    a = gp.sample_y(Xq, n_samples=2, random_state=3)
    b = gp.sample_y(Xq, n_samples=2, random_state=3)
    c = gp.sample_y(Xq, n_samples=2, random_state=3, mvn="auto")
    err = capfd.readouterr().err
    assert err.count("mvn='pathwise': not available for warped inputs") == 1
    np.testing.assert_array_equal(a, c)
    np.testing.assert_array_equal(a, b)
    with pytest.raises(ValueError, match="warped inputs"):
        gp.sample_paths()
