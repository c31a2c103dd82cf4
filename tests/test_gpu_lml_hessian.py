"""Hessian of the log marginal likelihood on the device (``bgp_lml_hess_batch``, bgp_lmlhess.hip) through
``_lib.Context.lml_hess`` on the cases of tests/_lmlhessref.py: the long-double reference, exact symmetry, the gradient call's bits,
independence of batch, position and chunk, the context-level warp as a fixed warp, the limits, the failed row (PRECISION lines: -s)."""
import numpy as np
import pytest

import _lmlhessref as R
import _precision as P

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)


@pytest.fixture(scope="module")
def lib():
    from bayes_skopt_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _ctx(lib, cid, **kw):
    c = R.ALL[cid]
    X, y, alpha, H, _ = R.problem(cid)
    return lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=len(H), **kw), H


@pytest.mark.parametrize("cid", list(R.ALL))
def test_against_the_long_double_reference(lib, cid, monkeypatch):
    c, kap = R.ALL[cid], R.problem(cid)[4]
    ctx, H = _ctx(lib, cid)
    try:
        lml, grad, hess, st = ctx.lml_hess(H)
        lml_g, grad_g, st_g = ctx.lml_grad(H)
        assert hess.shape == (c["B"], c["d"] + 2, c["d"] + 2) and np.all(st == 0) and np.isfinite(hess).all()
        assert np.array_equal(hess, np.swapaxes(hess, 1, 2))
        assert np.array_equal(lml, lml_g) and np.array_equal(grad, grad_g) and np.array_equal(st, st_g)
        for b in range(c["B"]):
            e = R.err(hess[b], R.reference(cid, b)) / R.tol(kap[b], c["n"])
            print("PRECISION lmlhess %s b%d kappa %.3g: device vs long double %.4f tol" % (cid, b, kap[b], e))
            assert e <= 1.0
        if c["B"] > 1:  # a matrix alone, at another position, and under a forced chunk (3 matrices as 2 + 1)
            assert all(np.array_equal(ctx.lml_hess(H[b])[2][0], hess[b]) for b in range(c["B"]))
            assert np.array_equal(ctx.lml_hess(H[::-1])[2], hess[::-1])
            monkeypatch.setenv("BGP_LMLHESS_CHUNK", "2")  # (read at every call)
            assert np.array_equal(ctx.lml_hess(H)[2], hess)
    finally:
        ctx.close()


def test_context_level_warp_is_a_fixed_warp(lib):
    c = P.WARP_CASES[0]
    X, y, alpha, H, _ = P.problem(c["id"])
    w = P.warp_params(c["id"])[0]
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=len(H))
    try:
        ctx.set_warp(w)
        got = ctx.lml_hess(H)
        Xw = ctx.beta_cdf(X, w)
    finally:
        ctx.close()
    ctx = lib.Context(Xw, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=len(H))
    try:  # the same numbers as un-warped training inputs of another context: the same bits
        assert all(np.array_equal(a, b) for a, b in zip(got, ctx.lml_hess(H)))
    finally:
        ctx.close()


def test_more_than_16_dimensions_is_an_error_code_and_python_takes_the_host_path(lib, capfd):
    import bayes_skopt_amd as bask
    from bayes_skopt_amd.kernels import RBF, ConstantKernel, WhiteKernel

    rng = np.random.RandomState(3)
    X = rng.uniform(size=(40, 17))
    y = np.sin(X.sum(axis=1))
    y = (y - y.mean()) / y.std()
    theta = np.concatenate([[0.1], np.log(0.8) + 0.1 * rng.randn(17), [np.log(1e-2)]])
    ctx = lib.Context(X, y, 1e-8, stationary="rbf", max_batch=1)
    try:
        with pytest.raises(lib.BgpError, match="d > 16"):
            ctx.lml_hess(theta)
        assert np.isfinite(ctx.lml(theta)).all()  # (nothing was launched: the context is usable)
    finally:
        ctx.close()
    gp = bask.BayesGPR(kernel=ConstantKernel(1.0) * RBF(np.ones(17)) + WhiteKernel(1e-2), alpha=1e-8, normalize_y=False)
    gp.kernel_ = gp.kernel
    gp._X_train_, gp.y_train_ = X, y
    gp._ensure_context()
    try:
        gp._post_theta = theta
        out = gp.hyper_laplace(theta=theta, priors=[lambda t: 0.0 * t] * 19)
        ref = R.hessian(X, y, 1e-8, theta, "rbf", "product")
        assert out["path"] == "host" and "numpy on the downloaded inverse" in capfd.readouterr().err
        assert R.err(out["hessian"], ref) <= R.tol(P.kappa_of(X, 1e-8, theta, "rbf", "product"), 40)
    finally:
        gp._ctx.close()


def test_a_failed_row_gives_zeros_and_the_per_row_warped_state_ends(lib):
    X, y, alpha, H, _ = R.problem(R.CASES[3]["id"])
    X = X.copy()
    X[1] = X[0]  # a duplicated point: singular without noise and without alpha_diag
    bad = H[1].copy()
    bad[-1] = -np.inf
    Hb = np.array([H[0], bad, H[2]])
    ctx = lib.Context(X, y, 0.0, max_batch=3)
    try:
        lml, grad, hess, st = ctx.lml_hess(Hb)
        assert st[1] != 0 and lml[1] == -np.inf and not grad[1].any() and not hess[1].any() and st[0] == 0 and st[2] == 0
        for b in (0, 2):
            assert all(np.array_equal(a[0], f[b]) for a, f in zip(ctx.lml_hess(Hb[b]), (lml, grad, hess, st)))
        W = np.zeros((3, 2 * X.shape[1]))
        ctx.posterior(Hb[[0, 2, 0]], want_alpha=False, warps=W)
        ctx.predict_warped(Hb[[0, 2, 0]], X[:5])  # (the per-row-warped posteriors are readable ...)
        ctx.lml_hess(Hb[0])
        with pytest.raises(lib.BgpError, match="not per-row warped"):  # (... until the call ends that state)
            ctx.predict_warped(Hb[[0, 2, 0]], X[:5])
    finally:
        ctx.close()
