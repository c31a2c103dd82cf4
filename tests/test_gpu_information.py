"""bgp_info.hip against the long-double reference of tests/_inforef.py at its tolerance: the three entry points,
the exact rules, a point's independence of its neighbours, and the Python layer.  ``pytest -s`` prints ``PRECISION`` lines."""
import numpy as np
import pytest

import _inforef as R
from conftest import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bask():
    import bayes_skopt_amd as bask
    assert bask._lib.device_count() >= 1
    return bask


@pytest.fixture(scope="module")
def problem():
    rng = np.random.RandomState(11)
    X, y = synth(40, 2, 5)
    H = np.array([0.0, -1.2, -1.0, -3.0]) + 0.2 * rng.randn(5, 4)
    return X, y, H, rng.uniform(-0.7, 0.7, size=(5, 4)), rng.uniform(size=(33, 2))


@pytest.fixture(scope="module")
def ctx(bask, problem):
    c = bask._lib.Context(problem[0], problem[1], np.full(40, 1e-10), max_batch=5)
    yield c
    c.close()


def _against_reference(name, out, mean, var, w, y_mean, y_std, Q):
    mu, sd, wn = R.columns(mean, var, w, y_mean, y_std)
    t, om = R.rule(Q)
    assert out["n_used"] == len(wn)
    worst = [0.0, 0.0]
    for i in range(mu.shape[1]):
        ref = R.reference(mu[:, i], sd[:, i], wn, t, om)
        if not np.isfinite(ref[1]):  # an atom: never a number that looks converged
            assert np.isnan(out["information"][i]) and out["entropy"][i] == -np.inf
            continue
        tol = R.tolerance(sd[:, i], wn, t)
        for k, key in enumerate(("information", "entropy")):
            worst[k] = max(worst[k], abs(float(out[key][i] - ref[k])) / tol)
    print("PRECISION info %s: device vs long double (tol) information %.3g entropy %.3g" % (name, worst[0], worst[1]))
    assert max(worst) <= 1.0, worst
    return mu, sd, wn, t


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%s-B%d-Q%d-m%d" % c)
def test_information_values_against_the_long_double_reference(ctx, case):
    content, B, Q, m = case
    mean, var, w, y_mean, y_std = R.moments(content, B, m)
    out = ctx.information_values(mean, var, y_mean, y_std, n_nodes=Q, weights=w)
    _mu, sd, wn, t = _against_reference(str(case), out, mean, var, w, y_mean, y_std, Q)
    assert out["n_used"] == (B - 2 if content == "dropped" else B)
    assert B > 1 or (out["information"] == 0.0).all()  # one row: exactly 0
    tol = np.array([R.tolerance(sd[:, i], wn, t) for i in range(m)])
    if content == "identical":
        assert (out["information"] <= tol).all() and (out["information"] >= 0.0).all()
    if content == "apart":
        assert (np.abs(out["information"] - np.log(B)) <= tol).all()
    if content.startswith("ystd"):  # the information does not see the scale, the entropy moves by its log
        one = ctx.information_values(mean, var, y_mean, 1.0, n_nodes=Q, weights=w)
        tol1 = np.array([R.tolerance(sd[:, i] / y_std, wn, t) for i in range(m)])
        assert (np.abs(out["information"] - one["information"]) <= tol + tol1).all()
        assert (np.abs(out["entropy"] - one["entropy"] - np.log(y_std)) <= tol + tol1).all()


def test_a_point_does_not_see_its_neighbours(ctx):
    mean, var, w, y_mean, y_std = R.moments("random", 5, 257)
    crowd = ctx.information_values(mean, var, y_mean, y_std, weights=w)
    perm = np.random.RandomState(3).permutation(257)
    mixed = ctx.information_values(mean[:, perm], var[:, perm], y_mean, y_std, weights=w)
    for key in ("information", "entropy"):
        assert np.array_equal(mixed[key], crowd[key][perm]), key
        for i in (0, 3, 4, 255, 256):
            alone = ctx.information_values(mean[:, i:i + 1], var[:, i:i + 1], y_mean, y_std, weights=w)
            assert alone[key][0] == crowd[key][i], (key, i)


@pytest.mark.parametrize("warped", [False, True])
def test_the_resident_entry_is_predict_followed_by_information_values(bask, ctx, problem, monkeypatch, warped):
    _X, _y, H, W, Xq = problem
    assert np.all(ctx.posterior(H, want_alpha=False, warps=W if warped else None)["status"] == 0)
    w = np.linspace(0.5, 1.5, 5)
    if not warped:
        monkeypatch.setenv("BGP_ITEM_CHUNK", "2")  # three chunks of posteriors in front of the pass
    out = ctx.hyper_information(H, Xq, 0.25, 1.5, weights=w, warped=warped)
    monkeypatch.delenv("BGP_ITEM_CHUNK", raising=False)
    mean, var = ctx.predict_warped(H, Xq) if warped else ctx.predict(H, Xq)
    want = ctx.information_values(mean, var, 0.25, 1.5, weights=w)
    assert out["n_used"] == 5 and np.array_equal(out["information"], want["information"]) and np.array_equal(out["entropy"], want["entropy"])
    _against_reference("resident warped=%s" % warped, out, mean, var, w, 0.25, 1.5, 32)
    with pytest.raises(bask._lib.BgpError, match="code 1"):
        ctx.information_values(mean, var, 0.25, 1.5, n_nodes=65)


@pytest.mark.parametrize("kind", ["canonical", "generic"])
def test_the_estimator_against_the_reference_on_the_rows_moments(bask, capfd, monkeypatch, kind):
    from bayes_skopt_amd import bayesgpr
    from sklearn.gaussian_process import kernels as sk
    X, y = synth(40, 2, 5)
    Xq = np.random.RandomState(2).uniform(size=(20, 2))
    kernel = (bask.construct_default_kernel([0, 1]) if kind == "canonical" else
              sk.Matern(length_scale=0.4, nu=2.5) * sk.RBF(length_scale=0.7) + sk.WhiteKernel(0.05))
    gp = bask.BayesGPR(kernel=kernel, normalize_y=True, random_state=3)
    gp.fit(X, y, n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
    rows = np.asarray(gp.chain_)[:8]
    monkeypatch.setattr(bayesgpr, "_information_told", [])
    capfd.readouterr()
    out, path = gp.hyper_information(Xq, thetas=rows, return_path=True)
    gp.hyper_information(Xq, thetas=rows)
    said = capfd.readouterr().err.count("hyper_information: the rows' moments chunk by chunk")
    if kind == "canonical":
        assert path == "device" and said == 0
        mean, var = gp._ctx.predict(gp._post.build_rows(gp, rows), Xq)
        scale = gp._y_scale()
    else:
        assert path == "chunks" and said == 1
        mu, sd = gp._predict_hyper_samples(rows, Xq, noise_zero=False)
        mean, var, scale = mu, sd * sd, (0.0, 1.0)
    _mu, sd, wn, t = _against_reference("estimator " + kind, out, mean, var, None, scale[0], scale[1], 32)
    tol = np.array([R.tolerance(sd[:, i], wn, t) for i in range(len(Xq))])
    assert (out["information"] >= 0.0).all() and (out["information"] <= np.log(out["n_used"]) + tol).all()
    assert (np.abs(out["information"] - (out["entropy"] - out["entropy_within"])) <= tol).all()


def test_the_bald_acquisition_proposes_the_most_informative_candidate(bask):
    from bayes_skopt_amd.space import Real
    opt = bask.Optimizer(dimensions=[Real(-2.0, 2.0), Real(0.0, 1.0)], n_points=60, n_initial_points=8, acq_func="bald", random_state=0)
    f = lambda x: float(np.sin(2.0 * x[0]) + x[1] ** 2)  # noqa: E731
    opt.run(f, n_iter=10, n_samples=4, gp_samples=40, gp_burnin=5)
    info = opt.hyper_information()
    assert info["n_used"] == 4 and np.array_equal(info["information"], opt._last_acq_values)
    best = opt._last_candidates[np.argmax(info["information"])]
    assert np.array_equal(opt.space.transform([opt.ask()])[0], opt.space.transform(opt.space.inverse_transform(best[None, :]))[0])
    two = opt.ask(2)
    assert len(two) == 2 and list(two[0]) == list(opt.ask()) and list(two[1]) != list(two[0])
    assert opt._last_batch_info["path"] == "fallback"
    with pytest.raises(ValueError, match="single GP about its own hyper-parameters is zero"):
        opt.tell(two[0], f(two[0]), n_samples=0)
