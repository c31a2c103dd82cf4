"""The pathwise posterior draws without a GPU: the tolerance class "path" of tests/_pathref.py is right --
reachable by a correct fp64 computation, missed by a single-precision slip -- on every case of tests/test_gpu_paths.py; the host's
spectral draws reproduce the four stationary kernels; ``mvn="pathwise"`` is accepted and never chosen by ``"auto"``; and the
ensemble of paths has ``predict``'s mean and variance."""
import numpy as np
import pytest

import _pathref as R
import _precision as P

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

MARGIN = 10.0


@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES])
def test_tolerance_is_reachable_and_bites(cid):
    ref, t = R.ref_paths(cid), R.case_tol(cid)
    reach = max(R.err(*R.path64(cid), ref)) / t
    bite = min(R.err(*R.path64(cid, round32=True), ref)) / t
    print("%-52s kappa %.2e  reachable err/tol %.2e   bites err/tol %.1e" % (cid, R.problem(cid)["kappa"].max(), reach, bite))
    assert reach <= 1 / MARGIN, (cid, reach)
    assert bite >= MARGIN, (cid, bite)


def test_cases_cover_the_tile_edges_and_the_degenerate_shapes():
    get = lambda k: {c[k] for c in R.CASES}  # noqa: E731
    assert get("n") == {1, 63, 64, 65, 130} and get("d") == {1, 3, 17, 32} and get("F") == {1, 63, 64, 65, 200}
    assert get("m") == {1, 255, 257} and get("P") == {1, 3} and get("vec_alpha") == {False, True}
    assert {(c["stationary"], c["form"]) for c in R.CASES} == set(P.FAMILIES)
    assert any(c.get("no_constant") and c["form"] == "sum" for c in R.CASES) and any(c.get("no_white") for c in R.CASES)
    assert any(c.get("dup_query") and c["stationary"] == "matern12" for c in R.CASES)
    for c in R.CASES:
        assert R.problem(c["id"])["kappa"].max() <= P.KAPPA_MAX


@pytest.mark.parametrize("stationary", ["rbf", "matern12", "matern32", "matern52"])
def test_spectral_draws_reproduce_the_kernel(stationary):
    """E cos(omega . delta) = S(|delta|) for omega from the host's spectral draw: 200 000 draws at r = 0.1, 1, 3 within five
    Monte-Carlo standard errors (sd / sqrt(F), the sd from the same cosine samples)."""
    from bayes_skopt_amd.bayesgpr import draw_path_variates

    F, d = 200_000, 3
    omega = draw_path_variates(np.random.RandomState(11), 1, F, d, 1, stationary)[0][0]
    u = np.array([2.0, -1.0, 2.0]) / 3.0
    for r in (0.1, 1.0, 3.0):
        cs = np.cos(omega @ (r * u))
        S = float(hp._S(hp.LD(r * r), stationary))
        se = cs.std(ddof=1) / np.sqrt(F)
        print("%-9s r = %.1f  S %.6f  estimate %.6f  (%.2f standard errors)" % (stationary, r, S, cs.mean(), (cs.mean() - S) / se))
        assert abs(cs.mean() - S) <= 5.0 * se, (stationary, r, cs.mean(), S, se)


def test_the_library_draw_and_the_reference_draw_consume_the_generator_alike():
    from bayes_skopt_amd.bayesgpr import draw_path_variates

    for st in ("rbf", "matern12"):
        a = draw_path_variates(np.random.RandomState(3), 2, 5, 3, 4, st)
        b = R.draw_variates(np.random.RandomState(3), 2, 5, 3, 4, st)
        for x, z in zip(a, b):
            np.testing.assert_array_equal(x, z)


def test_mvn_mode_accepts_pathwise_and_auto_never_returns_it():
    import bayes_skopt_amd as bask
    from bayes_skopt_amd._posterior import CanonicalPosterior

    gp = bask.BayesGPR(mvn="pathwise")
    gp._backend = CanonicalPosterior()
    gp._X_train_ = np.zeros((5, 3))
    assert gp._mvn_mode(10) == "pathwise" and gp._mvn_mode(100_000) == "pathwise"
    assert gp._mvn_mode(10, "auto") == "reference" and gp._mvn_mode(100_000, "auto") == "cholesky"
    gp.mvn = "auto"
    assert {gp._mvn_mode(m) for m in (1, 512, 513, 10_000, 1_000_000)} == {"reference", "cholesky"}
    assert gp._mvn_mode(7, "pathwise") == "pathwise"
    with pytest.raises(ValueError, match="pathwise"):
        gp._mvn_mode(7, "svd")
    with pytest.raises(ValueError):
        bask.BayesGPR(mvn="svd")


MOMENT_CASES = [("matern52", "product"), ("matern12", "sum")]
MOMENT_SEED, MOMENT_PATHS, MOMENT_F = 2024, 4096, 64


def moment_problem(stationary, form):
    """n = 23, d = 3, m = 9: (X, y, alpha, h, Xq)."""
    rng = np.random.RandomState(77)
    X = rng.uniform(size=(23, 3))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.randn(23)
    y = (y - y.mean()) / y.std()
    h = np.array([0.2, -1.0, -0.8, -1.2, np.log(1e-2)])
    return X, y, 1e-8, h, rng.uniform(size=(9, 3))


def moment_deviations(paths, mean, var):
    """Worst |ensemble mean - mean| and |ensemble variance - var| in their standard errors (sd / sqrt(P), the variance's sd from the
    squared deviations); no row excluded."""
    Pn = paths.shape[0]
    em = paths.mean(axis=0)
    dev2 = (paths - em) ** 2
    zm = np.abs(em - mean) / (paths.std(axis=0, ddof=1) / np.sqrt(Pn))
    zv = np.abs(dev2.mean(axis=0) - var) / (dev2.std(axis=0, ddof=1) / np.sqrt(Pn))
    return float(zm.max()), float(zv.max())


@pytest.mark.parametrize("stationary,form", MOMENT_CASES)
def test_ensemble_moments_of_the_restatement(stationary, form):
    """4096 paths of one GP (n = 23, d = 3, m = 9, F = 64), the seed of the GPU test: mean and variance of the ensemble within 3.5
    standard errors of the predictive mean and latent variance -- headroom under the GPU test's bound of 5."""
    from oracle import gp_oracle as O

    X, y, alpha, h, Xq = moment_problem(stationary, form)
    paths = R.moments_restated(X, y, alpha, h, stationary, form, Xq, MOMENT_PATHS, MOMENT_F, MOMENT_SEED)
    mean, std = O.predict(X, y, np.full(len(X), alpha), h, Xq, stationary, form, noise_zero=True)
    zm, zv = moment_deviations(paths, mean, std**2)
    print("%s %s: worst deviation of the ensemble mean %.2f, of the ensemble variance %.2f standard errors" % (stationary, form, zm, zv))
    assert zm <= 3.5 and zv <= 3.5, (zm, zv)
