"""Prediction gradients for many query rows (bgp_predict_grad_batch, BayesGPR.predict_gradients): the
device mean / var / dmean / dvar against the long-double references of tests/_gradref.py at the tolerance classes
tests/test_cpu_predgrad_reference.py qualifies, the rows against the existing one-point routine, the zero-std and r = 0 rules,
bitwise independence of a row from what shares its call, the host fallbacks, the limits.  Lines start with ``PRECISION``."""
import numpy as np
import pytest

import _gradref as G
import _precision as P
from conftest import synth

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
    print("PRECISION %-40s %-6s err/tol %.3e" % (tag, quantity, err / t))
    assert err <= t, "%s %s: error %.3e > tol %.3e (%.1fx)" % (tag, quantity, err, t, err / t)


@pytest.mark.parametrize("noise_zero", [False, True])
@pytest.mark.parametrize("cid", [c["id"] for c in P.POST_CASES])
def test_device_gradients_against_the_extended_precision_reference(bask, cid, noise_zero):
    from bayes_skopt_amd._posterior import noise_off

    c = P.ALL[cid]
    X, y, alpha, H, kap = P.problem(cid)
    n, k = len(X), kap[0]
    ctx = bask._lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=1)
    assert np.all(ctx.posterior(H[:1])["status"] == 0)
    Hk = noise_off(H[:1]) if noise_zero else H[:1]
    mean, var, dmean, dvar = ctx.predict_grad(Hk, P.query(cid))
    mean2, var2, dmean2, none = ctx.predict_grad(Hk, P.query(cid), want_dvar=False)
    ctx.close()
    assert none is None
    for a, b in ((mean, mean2), (var, var2), (dmean, dmean2)):
        np.testing.assert_array_equal(a, b)
    pr, ref = P.ref_predict(cid, noise_zero), G.ref_gradients(cid)
    tag = cid + ("_noise0" if noise_zero else "_noise")
    _check(tag, "mean", P.err_rel_max(mean[0], pr["mean"], P.mean_scale(cid)), P.tol("mean", k, n))
    _check(tag, "var", P.err_rel_max(var[0], pr["var"], P.prior_var(cid, noise_zero)), P.tol("var", k, n))
    _check(tag, "dmean", G.err_dmean(dmean[0], ref), P.tol("mean", k, n))
    _check(tag, "dvar", G.err_dvar(dvar[0], ref), P.tol("var", k, n))


def _fd_kernels():
    from bayes_skopt_amd.kernels import RBF, ConstantKernel, Matern

    # (the four kernels of tests/test_gpu_bayesgpr.py::test_predict_gradients_match_finite_differences)
    return {
        "matern52": ConstantKernel(1.0, (0.1, 2.0)) * Matern([0.4, 0.3, 0.5], (0.2, 0.8), nu=2.5),
        "matern32": ConstantKernel(1.0, (0.1, 2.0)) * Matern(0.4, (0.2, 0.8), nu=1.5),
        "rbf": ConstantKernel(1.0, (0.1, 2.0)) * RBF([0.4, 0.3, 0.5], (0.2, 0.8)),
        "sum_matern12": ConstantKernel(0.5, (0.1, 2.0)) + Matern(0.6, (0.2, 0.9), nu=0.5),
    }


def _fit(bask, kernel, X, y, **kw):
    gp = bask.BayesGPR(kernel=kernel, random_state=0, normalize_y=True, **kw)
    gp.fit(X, y, n_desired_samples=40, n_burnin=5, n_walkers_per_thread=20, progress=False)
    return gp


def _one_point_rows(gp, Xq):
    rows = [gp.predict(x[None, :], return_std=True, return_mean_grad=True, return_std_grad=True) for x in Xq]
    return (np.concatenate([r[0] for r in rows]), np.concatenate([r[1] for r in rows]), np.stack([r[2] for r in rows]),
            np.stack([r[3] for r in rows]))


@pytest.mark.parametrize("kind", ["matern52", "matern32", "rbf", "sum_matern12"])
def test_rows_match_the_one_point_routine(bask, kind):
    """``predict_gradients(X)`` against ``predict(x, return_std, return_mean_grad, return_std_grad)`` row by row (host
    contraction of numpy gradients with the device-built alpha_ / K_inv_): both fp64, so 2 tol on the metrics of _gradref,
    in y units."""
    rng = np.random.RandomState(3)
    X = rng.uniform(size=(60, 3))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.05 * rng.randn(60)
    gp = _fit(bask, _fd_kernels()[kind], X, y)
    Xq = np.vstack([[0.37, 0.52, 0.61], rng.uniform(-0.05, 1.05, size=(12, 3))])
    ys = float(np.ravel(gp.y_train_std_)[0])
    for zero in (False, True):
        if zero:
            with gp.noise_set_to_zero():
                got, want = gp.predict_gradients(Xq), _one_point_rows(gp, Xq)
                mu_only = gp.predict_gradients(Xq, return_std=False)
                scales = [gp._post.grad_x(gp, x, gp.X_train_) for x in Xq]
                prior = float(gp.kernel_.diag(Xq[:1])[0])
        else:
            got, want = gp.predict_gradients(Xq), _one_point_rows(gp, Xq)
            mu_only = gp.predict_gradients(Xq, return_std=False)
            scales = [gp._post.grad_x(gp, x, gp.X_train_) for x in Xq]
            prior = float(gp.kernel_.diag(Xq[:1])[0])
        np.testing.assert_array_equal(mu_only[0], got[0])
        np.testing.assert_array_equal(mu_only[1], got[2])
        assert got[0].shape == (13,) and got[1].shape == (13,) and got[2].shape == (13, 3) and got[3].shape == (13, 3)
        Ki, a = gp.K_inv_, gp.alpha_
        kappa, n = float(np.linalg.cond(Ki)), len(X)
        s_mean = max(float(np.abs(k * a).sum()) for _g, k in scales) * ys
        s_dmean = max(float(np.abs(g * a[:, None]).sum(axis=0).max()) for g, _k in scales) * ys
        # grad_std = dvar / (2 std): the dvar metric, row by row on the row's own std
        e_dstd = max(float(np.abs(got[3][i] - want[3][i]).max() * 2.0 * want[1][i] /
                           (2.0 * np.abs((k @ Ki)[:, None] * g).sum(axis=0).max() * ys**2))
                     for i, (g, k) in enumerate(scales))
        tag = "%s_%s" % (kind, "noise0" if zero else "noise")
        _check(tag, "mean", float(np.abs(got[0] - want[0]).max()) / s_mean, 2 * P.tol("mean", kappa, n))
        _check(tag, "var", float(np.abs(got[1] ** 2 - want[1] ** 2).max()) / (prior * ys**2), 2 * P.tol("var", kappa, n))
        _check(tag, "dmean", float(np.abs(got[2] - want[2]).max()) / s_dmean, 2 * P.tol("mean", kappa, n))
        _check(tag, "dstd", e_dstd, 2 * P.tol("var", kappa, n))


def test_query_row_at_a_training_point(bask):
    """Noise off, a query row ON a training point.  Matern 1/2: fac(0) = 0, so every gradient is finite and the row agrees with
    the one-point routine (which applies the same rule).  Where the std is <= 1e-8 in y units -- targets of scale 1e-9 --
    ``grad_std`` is exactly zero, as ``np.allclose(std, 0)`` makes it in the one-point routine."""
    from bayes_skopt_amd.kernels import ConstantKernel, Matern

    rng = np.random.RandomState(5)
    X = rng.uniform(size=(50, 2))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.05 * rng.randn(50)
    Xq = np.vstack([X[7], X[7] + 1e-3, X[20]])
    gp = _fit(bask, ConstantKernel(0.5, (0.1, 2.0)) + Matern(0.6, (0.2, 0.9), nu=0.5), X, y)
    with gp.noise_set_to_zero():
        got, want = gp.predict_gradients(Xq), _one_point_rows(gp, Xq)
        mean, var, dmean, dvar = gp._post.predict_grad(gp, Xq)
    assert all(np.all(np.isfinite(a)) for a in (mean, var, dmean, dvar) + tuple(got))
    np.testing.assert_allclose(got[2], want[2], rtol=1e-9, atol=1e-11 * np.abs(want[2]).max())
    np.testing.assert_allclose(got[3], want[3], rtol=1e-6, atol=1e-9 * np.abs(want[3]).max())
    # the training point's own term contributes nothing: dropping it from the host sum changes nothing
    g, _k = gp._post.grad_x(gp, Xq[0], gp.X_train_)
    assert np.all(g[7] == 0.0)
    tiny = _fit(bask, ConstantKernel(1.0, (0.1, 2.0)) * Matern([0.4, 0.3], (0.2, 0.8), nu=2.5), X, 1e-9 * y)
    with tiny.noise_set_to_zero():
        mu, sd, gm, gs = tiny.predict_gradients(Xq)
        one = _one_point_rows(tiny, Xq)
    assert np.all(sd <= 1e-8) and np.all(gs == 0.0) and np.all(one[3] == 0.0)
    assert np.all(np.isfinite(gm)) and np.abs(gm).max() > 0.0


def test_rows_do_not_depend_on_what_shares_the_call(bask):
    """Three posteriors in one call == each alone, and m = 257 rows == the same rows in two calls: bit for bit."""
    X, y, alpha, H = P._problem(200, 4, 41, "matern52", "product", 3, False)
    H[:, -1] = np.log(1e-2)
    Xq = np.random.RandomState(8).uniform(-0.1, 1.1, size=(257, 4))
    ctx = bask._lib.Context(X, y, alpha, max_batch=4)
    assert np.all(ctx.posterior(H)["status"] == 0)
    together = ctx.predict_grad(H, Xq)
    again = ctx.predict_grad(H, Xq)
    split = [ctx.predict_grad(H, Xq[:100]), ctx.predict_grad(H, Xq[100:])]
    for q in range(4):
        np.testing.assert_array_equal(together[q], again[q])
        np.testing.assert_array_equal(together[q], np.concatenate([split[0][q], split[1][q]], axis=1))
    for b in range(3):
        assert np.all(ctx.posterior(H[b : b + 1])["status"] == 0)
        alone = ctx.predict_grad(H[b : b + 1], Xq)
        for q in range(4):
            np.testing.assert_array_equal(alone[q][0], together[q][b])
    ctx.close()


def test_more_training_points_than_the_lds_rows_hold(bask):
    """n = 3100: the k / g rows of a workgroup live in device scratch instead of LDS; against fp64 numpy / LAPACK on the
    metrics of _gradref at 2 tol (both fp64)."""
    from oracle import gp_oracle as O

    n, d = 3100, 2
    X, y = synth(n, d, 12)
    h = np.array([0.1, np.log(0.3), np.log(0.4), np.log(1e-2)])
    Xq = np.random.RandomState(2).uniform(size=(5, d))
    ctx = bask._lib.Context(X, y, 1e-8, max_batch=1)
    assert np.all(ctx.posterior(h[None])["status"] == 0)
    mean, var, dmean, dvar = ctx.predict_grad(h[None], Xq)
    pm, pv = ctx.predict(h[None], Xq)
    ctx.close()
    K = O.gram_with_jitter(X, np.full(n, 1e-8), h, "matern52", "product")
    w = np.linalg.eigvalsh(K)
    kappa = float(w[-1] / w[0])
    dm, dv, sm, sv = G.gradients64(X, y, 1e-8, h, Xq, "matern52", "product", return_scales=True)
    _check("scratch_rows_n3100", "dmean", float(np.abs(dmean[0] - dm).max() / sm), 2 * P.tol("mean", kappa, n))
    _check("scratch_rows_n3100", "dvar", float(np.abs(dvar[0] - dv).max() / sv), 2 * P.tol("var", kappa, n))
    np.testing.assert_allclose(mean, pm, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(var, pv, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("which", ["warped", "generic"])
def test_fallbacks_equal_the_one_point_routine(bask, which):
    """Warped inputs / a generic kernel tree: the one-point routine row by row, array_equal."""
    from sklearn.gaussian_process import kernels as sk

    X, y = synth(80, 2, 8)
    if which == "warped":
        gp = bask.BayesGPR(kernel=bask.construct_default_kernel([0, 1]), random_state=1, warp_inputs=True, normalize_y=True)
    else:
        gp = bask.BayesGPR(kernel=sk.Matern(length_scale=0.5, nu=2.5) + sk.Matern(length_scale=2.0, nu=1.5), random_state=4,
                           normalize_y=True)
    gp.fit(X, y, n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
    assert gp.warp_inputs or gp._generic
    Xq = np.random.RandomState(2).uniform(0.1, 0.9, size=(4, 2))
    got, want = gp.predict_gradients(Xq), _one_point_rows(gp, Xq)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    mu, gm = gp.predict_gradients(Xq, return_std=False)
    np.testing.assert_array_equal(mu, want[0])
    np.testing.assert_array_equal(gm, want[2])
    with pytest.raises(NotImplementedError):
        gp.predict(Xq, return_mean_grad=True)


def test_limits_are_errors_not_crashes(bask):
    """d = 33, or a context-level warp: BGP_ERR_INVALID from both entry points (the Python layer checks first and never relies
    on it); no resident posterior: BGP_ERR_STATE."""
    lib = bask._lib
    X, y = synth(40, 33, 3)
    h = np.concatenate([[0.0], np.full(33, np.log(2.0)), [np.log(1e-2)]])
    ctx = lib.Context(X, y, 1e-8, max_batch=1)
    ctx.posterior(h[None])
    with pytest.raises(lib.BgpError, match="code 1"):
        ctx.predict_grad(h[None], X[:3])
    with pytest.raises(lib.BgpError, match="code 1"):
        ctx.minimize_starts(0, h[None], 0.0, 1.0, 0.0, X[:3], 0.0, 1.0)
    ctx.close()
    X, y = synth(40, 2, 3)
    h = np.array([0.0, np.log(0.4), np.log(0.4), np.log(1e-2)])
    ctx = lib.Context(X, y, 1e-8, max_batch=1)
    with pytest.raises(lib.BgpError, match="code 4"):
        ctx.predict_grad(h[None], X[:3])
    ctx.set_warp(np.zeros(4))
    ctx.posterior(h[None])
    with pytest.raises(lib.BgpError, match="code 1"):
        ctx.predict_grad(h[None], X[:3])
    with pytest.raises(lib.BgpError, match="code 1"):
        ctx.minimize_starts(0, h[None], 0.0, 1.0, 0.0, X[:3], 0.0, 1.0)
    ctx.set_warp(None)
    ctx.posterior(h[None])
    assert np.all(np.isfinite(ctx.predict_grad(h[None], X[:3])[2]))
    ctx.close()
