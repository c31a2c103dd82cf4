"""The bounds of tests/test_gpu_shapley.py qualified without a device (tests/_shapref.py: the fp64 replica within 1 / 10, fp32 inputs
miss by >= 10); the host route on a function with a known attribution; the binding's argument checks.  ``pytest -s``: PRECISION."""
import numpy as np
import pytest

import _pdref as PD
import _precision as P
import _shapref as R

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)


@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES])
def test_fp64_reaches_the_bounds_and_fp32_inputs_miss_them(cid):
    c, (X, y, alpha, H, kap, Xp, Z) = R.ALL[cid], R.problem(cid)
    st, fm, reach, bite = c["stationary"], c["form"], 0.0, np.inf
    for b in range(c["Buse"]):
        ref, t = R.reference(cid, b), P.tol("mean", kap[b], c["n"])
        e64 = R.errs(R.replica64(X, PD.alpha64(X, y, alpha, H[b], st, fm), H[b], Xp, Z, st, fm), ref, t, c["d"])
        X32 = P.to32(X)
        e32 = R.errs(R.replica64(X32, PD.alpha64(X32, y, alpha, H[b], st, fm), H[b], P.to32(Xp), P.to32(Z), st, fm), ref, t, c["d"])
        reach, bite = max(reach, max(e64.values())), min(bite, max(e32.values()))
    print("PRECISION shapley %s kappa %.3g: fp64 replica %.4f of the bounds, fp32 inputs %.4g" % (cid, kap[: c["Buse"]].max(), reach, bite))
    assert reach <= 0.1 and bite >= 10.0


class _Known:  # an estimator whose mean is f(x) = a . x + c x_0 x_1, as means_by_predict reads one
    a, c = np.array([1.0, -2.0, 0.5, 0.25]), 3.0
    _post = property(lambda self: self)

    def predict(self, gp, X, return_cov):
        return (X @ self.a + self.c * X[:, 0] * X[:, 1])[None, :], None, None

    def phi(self, x, z):  # against one baseline z: a_k (x_k - z_k); the product's x_0 x_1 - z_0 z_1 in two equal-order halves
        return self.a * (x - z) + 0.5 * self.c * np.array([(x[0] - z[0]) * (z[1] + x[1]), (x[1] - z[1]) * (z[0] + x[0]), 0.0, 0.0])


def test_the_host_route_on_a_function_with_a_known_attribution(monkeypatch):
    from bayes_skopt_amd import _posterior as post

    gp, rng = _Known(), np.random.RandomState(0)
    Xp, Z = rng.uniform(size=(2, 4)), rng.uniform(size=(1, 4))
    want = np.stack([gp.phi(x, Z[0]) for x in Xp])
    phi, base, value, inter, se = post.shapley_by_predict(gp, None, Xp, Z, "test", interactions=True)
    want_inter = np.zeros((2, 4, 4))
    want_inter[:, 0, 1] = want_inter[:, 1, 0] = gp.c * (Xp[:, 0] - Z[0, 0]) * (Xp[:, 1] - Z[0, 1])
    for got, ref in ((phi[0], want), (phi[0].sum(axis=1), value[0] - base[0]), (inter[0], want_inter)):  # (round-off: |f| < 8)
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-14)
    assert se is None
    # past the enumeration limit: the permutation estimate, within 5 of its own standard errors (fixed seed); no interactions
    monkeypatch.setattr(post, "SHAP_EXACT_ROWS", 8)
    phi, base2, value2, inter, se = post.shapley_by_predict(gp, None, Xp, Z, "test", True, 400, np.random.RandomState(1))
    assert inter is None and np.array_equal(base2, base) and np.array_equal(value2, value)
    assert np.all(np.abs(phi[0] - want) <= 5.0 * se[0] + 1e-14) and se[0][:, :2].min() > 0.0 and np.all(se[0][:, 2:] < 1e-14)


def test_argument_checks_of_the_binding():
    import bayes_skopt_amd as bask
    from bayes_skopt_amd import _lib

    assert "bgp_shapley" in _lib.SIGNATURES and "shapley_values" in bask.utils.__all__
    ctx = _lib.Context.__new__(_lib.Context)
    ctx.d, ctx.p = 3, 5
    for H, Xp, Z in ((5, 2, 3), (5, 3, 4), (4, 3, 3)):  # the columns of the points, of the background, of H
        with pytest.raises(ValueError, match="3 columns|d\\+2"):
            ctx.shapley(np.zeros((1, H)), np.zeros((1, Xp)), np.zeros((4, Z)))
