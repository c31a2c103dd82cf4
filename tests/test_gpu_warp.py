"""Input warping (warp_inputs=True, bask/bayesgpr.py:219-316,353-365): device Beta-CDF warp, per-walker
warped LML, context-level warp for posterior/predict, and the BayesGPR / Optimizer surface."""
import numpy as np
import pytest
from scipy.stats import beta as sbeta

from conftest import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import bayes_skopt_amd  # noqa: F401
    from bayes_skopt_amd import _lib

    assert _lib.device_count() >= 1
    return _lib


@pytest.fixture(scope="module")
def O():
    from oracle import gp_oracle

    return gp_oracle


def test_device_beta_cdf_matches_scipy(lib):
    n, d = 500, 4
    X = np.random.RandomState(0).uniform(size=(n, d))
    X[0] = 0.0
    X[1] = 1.0
    X[2] = 1e-12
    X[3] = 1 - 1e-12
    ctx = lib.Context(X, np.zeros(n), 1e-10, max_batch=2)
    for seed, scale in ((1, 0.3), (2, 1.0), (3, 2.0)):
        w = scale * np.random.RandomState(seed).randn(2 * d)
        got = ctx.beta_cdf(X, w)
        ref = np.column_stack([sbeta(np.exp(w[k]), np.exp(w[d + k])).cdf(X[:, k]) for k in range(d)])
        np.testing.assert_allclose(got, ref, rtol=1e-11, atol=1e-15)
    ctx.close()


def test_per_walker_warped_lml(lib, O):
    n, d, B = 260, 3, 10
    X, y = synth(n, d, 12)
    rng = np.random.RandomState(13)
    H = np.array([0.0, -1.0, -1.1, -0.9, -3.5]) + 0.15 * rng.randn(B, d + 2)
    W = 0.3 * rng.randn(B, 2 * d)
    ctx = lib.Context(X, y, 1e-10, max_batch=4)  # chunked
    got = ctx.lml_warped(H, W)
    ref = np.array([O.lml_warped(X, y, np.full(n, 1e-10), H[b], W[b]) for b in range(B)])
    np.testing.assert_allclose(got, ref, rtol=1e-6)
    # zero warp parameters = Beta(1, 1) = identity
    np.testing.assert_allclose(ctx.lml_warped(H, np.zeros_like(W)), ctx.lml(H), rtol=1e-12)
    ctx.close()


def test_context_level_warp_posterior_predict(lib, O):
    n, d, m = 150, 2, 60
    X, y = synth(n, d, 21)
    Xq = np.random.RandomState(22).uniform(size=(m, d))
    th = np.array([0.1, -1.0, -1.2, -3.0])
    w = np.array([0.2, -0.3, 0.4, 0.1])
    ctx = lib.Context(X, y, 1e-10, max_batch=2)
    ctx.set_warp(w)
    np.testing.assert_allclose(ctx.lml(th)[0], O.lml_warped(X, y, np.full(n, 1e-10), th, w), rtol=1e-6)
    ctx.posterior(th)
    mean, var = ctx.predict(th, Xq)
    mo, so = O.predict(O.warp_inputs(X, w), y, np.full(n, 1e-10), th, O.warp_inputs(Xq, w))
    np.testing.assert_allclose(mean[0], mo, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(np.sqrt(var[0]), so, rtol=1e-6, atol=1e-8)
    ctx.set_warp(None)
    np.testing.assert_allclose(ctx.lml(th)[0], O.lml(X, y, np.full(n, 1e-10), th), rtol=1e-6)
    ctx.close()


def test_bayesgpr_with_warping_end_to_end(O):
    """A function that is stationary only after a monotone warp of its input: the warped GP must run,
    keep the reference's chain layout (p + 2d columns) and predict consistently with the oracle."""
    import bayes_skopt_amd as bask

    rng = np.random.RandomState(0)
    n, d = 80, 1
    X = rng.uniform(size=(n, d))
    y = np.sin(12.0 * X[:, 0] ** 3) + 0.05 * rng.randn(n)
    y = (y - y.mean()) / y.std()
    gp = bask.BayesGPR(kernel=bask.construct_default_kernel([0]), random_state=1, warp_inputs=True)
    gp.fit(X, y, n_desired_samples=60, n_burnin=5, n_walkers_per_thread=30, progress=False)
    assert gp.chain_.shape == (60, 3 + 2 * d)
    assert gp.warp_alphas_.shape == (d,) and gp.warp_betas_.shape == (d,)
    w = np.concatenate([gp.warp_alphas_, gp.warp_betas_])
    np.testing.assert_allclose(gp.X_train_, O.warp_inputs(X, w), rtol=1e-10, atol=1e-14)
    Xq = np.linspace(0.01, 0.99, 25)[:, None]
    mean, std = gp.predict(Xq, return_std=True)
    mo, so = O.predict(O.warp_inputs(X, w), y, np.full(n, 1e-10), gp.theta, O.warp_inputs(Xq, w))
    np.testing.assert_allclose(mean, mo, rtol=1e-6, atol=1e-8)
    from conftest import assert_variance_close

    assert_variance_close(std**2, so**2, O.predict_variance_selfdiff(O.warp_inputs(X, w), y, np.full(n, 1e-10), gp.theta,
                                                                      O.warp_inputs(Xq, w)))
    with pytest.raises(ValueError):
        gp.predict(np.array([[1.5]]))
    np.testing.assert_allclose(gp.unwarp(gp.warp(Xq)), Xq, rtol=1e-8)
    # acquisition driver with per-draw warps, then everything is restored
    acq = bask.acquisition.evaluate_acquisitions(Xq, gp, [bask.acquisition.ExpectedImprovement(),
                                                        bask.acquisition.PVRS()], n_samples=3, random_state=0)
    assert acq.shape == (2, 25) and np.all(np.isfinite(acq))
    np.testing.assert_allclose(np.concatenate([gp.warp_alphas_, gp.warp_betas_]), w)
    s = gp.sample_y(Xq, n_samples=2, random_state=1)
    assert s.shape == (25, 2) and np.all(np.isfinite(s))
    np.testing.assert_allclose(np.concatenate([gp.warp_alphas_, gp.warp_betas_]), w)


def test_optimizer_with_warping():
    import bayes_skopt_amd as bask

    rng = np.random.RandomState(0)
    opt = bask.Optimizer(dimensions=[(0.0, 1.0)] * 2, n_points=200, n_initial_points=6, init_strategy="r2",
                         gp_kwargs=dict(warp_inputs=True), acq_func="pvrs", random_state=0)
    for _ in range(8):
        x = opt.ask()
        opt.tell(x, float(np.sin(5 * x[0] ** 2) + x[1] + 0.01 * rng.randn()), gp_samples=100, gp_burnin=2)
    assert opt.gp.chain_.shape == (100, 4 + 4)
    nxt = opt.ask()
    assert all(0.0 <= v <= 1.0 for v in nxt)


def test_warped_device_chain_equals_oracle_chain(O):
    """warp_inputs=True through the sampler's asynchronous path (bgp_lml_batch_warped_submit / _wait: the per-walker
    Beta parameters are extra chain columns, bask/bayesgpr.py:353-365): the device-driven chain must coincide with the
    per-walker oracle replay (warp -> LML, default priors + N(0, 0.3) warp priors) on the same RandomState stream --
    one accept/reject flip would make them diverge."""
    import scipy.stats as st

    import bayes_skopt_amd as bask

    rng = np.random.RandomState(4)
    n, d, W, steps = 50, 2, 20, 25
    X = rng.uniform(size=(n, d))
    y = np.sin(9.0 * X[:, 0] ** 2) + X[:, 1] + 0.05 * rng.randn(n)
    y = (y - y.mean()) / y.std()
    ad = np.full(n, 1e-10)
    gp = bask.BayesGPR(kernel=bask.construct_default_kernel(list(range(d))), random_state=7, warp_inputs=True,
                       resident_sampler=False)  # (the host-driven loop: the resident form has its own test, test_gpu_resident.py)
    gp.fit(X, y, n_desired_samples=W, n_burnin=0, n_walkers_per_thread=W, progress=False)
    start = np.array(gp.pos_, copy=True)
    assert start.shape == (W, d + 2 + 2 * d)
    submitted = []
    real = gp._ctx.lml_warped_submit

    def spy(H, Wp):
        ok = real(H, Wp)
        submitted.append((len(H), ok))
        return ok

    gp._ctx.lml_warped_submit = spy
    gp.random_state = np.random.RandomState(321)
    gp.sample(n_desired_samples=W * steps, n_burnin=0, n_walkers_per_thread=W, position=start)
    dev_chain = gp._sampler.get_chain()
    assert len(submitted) == 1 + 2 * steps
    assert all(ok for b, ok in submitted if b == W // 2)  # every half-step block went through submit / wait
    seed = np.random.RandomState(321).randint(0, np.iinfo(np.int32).max)
    wp = st.norm(loc=0.0, scale=0.3).logpdf

    def log_prob(theta):
        th, w = theta[: d + 2], theta[d + 2:]
        lp = float(O.default_log_prior(th[None, :], d)[0]) + float(np.sum(wp(w)))
        lp += O.lml_warped(X, y, ad, th, w)
        return lp if np.isfinite(lp) else -np.inf

    ref_chain, ref_lp, _, _, _ = O.stretch_move_sampler(log_prob, start, steps, np.random.RandomState(seed))
    np.testing.assert_allclose(dev_chain, ref_chain, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(gp._sampler.get_log_prob(), ref_lp, rtol=1e-7)


# ------------------------------------------------------------------------------------------------------------------------------
# the Beta CDF at its edges (tests/_warpref.py; tests/test_cpu_warp_reference.py qualifies grid, reference and tolerance)
# ------------------------------------------------------------------------------------------------------------------------------
_GRID = {}


def _device_grid(lib):
    """``beta_cdf`` on the edge grid and on its mirror image (1 - x with the parameters swapped), four parameter pairs per call
    on ONE context of 8 points in d = 4; computed once for the tests below."""
    if not _GRID:
        import _warpref as WR

        X, _T, _A, _B = WR.grid()
        d = 4
        ctx = lib.Context(np.full((8, d), 0.5), np.zeros(8), 1e-10, max_batch=2)
        got, mirror = np.empty_like(X), np.empty_like(X)
        try:
            for j0 in range(0, len(WR.PAIRS), d):
                js = [min(j, len(WR.PAIRS) - 1) for j in range(j0, j0 + d)]  # (the last call repeats the last pair)
                wa, wb = [WR.PAIRS[j][0] for j in js], [WR.PAIRS[j][1] for j in js]
                got[js] = ctx.beta_cdf(X[js].T, np.array(wa + wb)).T
                mirror[js] = ctx.beta_cdf(1.0 - X[js].T, np.array(wb + wa)).T
        finally:
            ctx.close()
        _GRID.update(got=got, mirror=mirror)
    return _GRID["got"], _GRID["mirror"]


def _warpref():
    hp = pytest.importorskip("oracle.hp_oracle")
    if not hp.available():
        pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference")
    pytest.importorskip("mpmath")
    import _warpref as WR

    return WR


def test_beta_cdf_on_the_edge_grid_meets_the_absolute_tolerance(lib):
    """``beta_cdf`` against mpmath at 50 digits on the 121 x 20 grid of tests/_warpref.py, parameters up to e^+-6 and x from the
    smallest normal double to 1 - 2^-53, at the absolute tolerance ``_warpref.tol`` (K = 8; the host restatement of the same
    arithmetic holds a quarter of it); exactly 0 at x = 0 and exactly 1 at x = 1 for every (a, b).
    Measured on the device: worst err / tol 0.203, at w = (-0.3, -1), x = 0.55998 (the switch point; absolute error 1.0e-15);
    worst absolute error 2.2e-13; the device's values are those of the host restatement bit for bit on 1326 of the 2420
    points (host: worst err / tol 0.243).  The switch-point test below: largest decrease 0.087 of its 2 tol; the symmetry
    test: 0.059 of its 2 tol over 1154 points."""
    WR = _warpref()
    X, T, _A, _B = WR.grid()
    got, _mirror = _device_grid(lib)
    ref = WR.reference()
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    inner = T > 0.0
    ratio = np.where(inner, err / np.where(inner, T, 1.0), 0.0)
    j, i = np.unravel_index(np.argmax(ratio), ratio.shape)
    host = np.abs(WR.restated()[0].astype(np.longdouble) - ref).astype(np.float64)
    print("PRECISION beta_cdf edge grid: worst err / tol %.3f at w = (%g, %g), x = %.17g (abs err %.3e); worst abs err %.3e; host "
          "restatement worst err / tol %.3f; device == host restatement on %d of %d points"
          % (ratio[j, i], WR.PAIRS[j][0], WR.PAIRS[j][1], X[j, i], err[j, i], err.max(), float((host[inner] / T[inner]).max()),
             int((got == WR.restated()[0]).sum()), got.size))
    assert np.all(got[:, 0] == 0.0) and np.all(got[:, 1] == 1.0)
    assert np.all(np.isfinite(got)) and np.all((got >= 0.0) & (got <= 1.0))
    assert np.all(err <= T), "worst err / tol %.3f" % ratio[j, i]


def test_beta_cdf_is_monotone_across_the_switch_point(lib):
    """The two continued fractions meet at x = (a + 1) / (a + b + 2): for every (a, b) of the grid the device values at the
    switch point and its two fp64 neighbours are non-decreasing within 2 tol."""
    WR = _warpref()
    _X, T, _A, _B = WR.grid()
    got, _mirror = _device_grid(lib)
    s, t = got[:, WR.SWITCH], T[:, WR.SWITCH]
    step = np.diff(s, axis=1)
    lim = 2.0 * np.maximum(t[:, :-1], t[:, 1:])
    print("PRECISION beta_cdf switch point: largest decrease / (2 tol) %.3f" % float((-step / lim).max()))
    assert np.all(step >= -lim)


def test_beta_cdf_symmetry(lib):
    """I_x(a, b) + I_{1-x}(b, a) = 1 within 2 tol at every grid point whose 1 - x is exact in fp64."""
    from fractions import Fraction

    WR = _warpref()
    X, T, A, B = WR.grid()
    got, mirror = _device_grid(lib)
    worst, count = 0.0, 0
    for j in range(X.shape[0]):
        for i in range(X.shape[1]):
            x = float(X[j, i])
            if 0.0 < x < 1.0 and Fraction(1) - Fraction(x) == Fraction(1.0 - x):
                lim = 2.0 * max(T[j, i], WR.tol(B[j], A[j], 1.0 - x))
                worst, count = max(worst, abs(got[j, i] + mirror[j, i] - 1.0) / lim), count + 1
    print("PRECISION beta_cdf symmetry: worst |I_x(a, b) + I_{1-x}(b, a) - 1| / (2 tol) %.3f over %d points" % (worst, count))
    assert count >= 121 * 6 and worst <= 1.0


def test_the_three_warp_entry_points_give_the_same_bits(lib):
    """``beta_cdf``, the context-level warp and the per-walker warp run ONE kernel behind three launches (one matrix without a
    stride; B matrices behind a row stride, in chunks of ``max_batch``).  n d = 900 is no multiple of the 256 threads of a
    block, B = 9 > max_batch = 4 (chunks of 4 / 4 / 1).  No accessor reads a warped design matrix back, so the log-likelihood
    carries the bits: a context built on ``beta_cdf(X, w)`` without a warp, ``set_warp(w)`` on the context of X, and
    ``lml_warped`` rows that share w, row by row."""
    n, d, B = 300, 3, 9
    X, y = synth(n, d, 31)
    rng = np.random.RandomState(32)
    H = np.array([0.0, -1.0, -1.1, -0.9, -3.5]) + 0.1 * rng.randn(B, d + 2)
    H[4] = H[8] = H[0]  # the first row of every chunk: the same problem behind three offsets
    w = np.array([0.4, -0.3, 0.2, -0.5, 0.1, 0.6])
    ctx = lib.Context(X, y, 1e-10, max_batch=4)
    try:
        rows, st = ctx.lml_warped(H, np.tile(w, (B, 1)), return_status=True)
        Xw = ctx.beta_cdf(X, w)
        ctx.set_warp(w)
        ctxwarp = np.array([ctx.lml(H[b:b + 1])[0] for b in range(B)])
        ctx.set_warp(None)
    finally:
        ctx.close()
    ctx2 = lib.Context(Xw, y, 1e-10, max_batch=4)
    try:
        plain = np.array([ctx2.lml(H[b:b + 1])[0] for b in range(B)])
    finally:
        ctx2.close()
    assert np.all(st == 0) and np.all(np.isfinite(rows)) and rows[0] == rows[4] == rows[8]
    assert np.array_equal(ctxwarp, plain), "set_warp and beta_cdf: max |d| %.3e" % np.abs(ctxwarp - plain).max()
    assert np.array_equal(rows, ctxwarp), "lml_warped and set_warp: max |d| %.3e" % np.abs(rows - ctxwarp).max()


def test_warp_parameters_outside_the_domain_give_minus_inf_not_nan(lib):
    """Outside |w| <= 15 (include/bgp.h at ``bgp_beta_cdf``) a per-walker warped LML is a finite number or -inf with a non-zero
    status, never NaN; where ``exp(w)`` is 0 or inf it is -inf with a non-zero status -- the Beta CDF is NaN there by
    construction, whatever x is; and the other rows of the batch keep the bits they have alone.  n = 60: one block column, so
    a matrix of NaN is factorised by one workgroup that waits for nothing but its own barriers (the argument is written out
    at ``test_device_run_equals_the_replay_of_its_plan`` of tests/test_gpu_mcmc_replay.py)."""
    n, d = 60, 2
    X, y = synth(n, d, 41)
    X = 0.05 + 0.9 * (X - X.min(axis=0)) / (X.max(axis=0) - X.min(axis=0))  # strictly inside (0, 1)
    assert X.min() > 0.0 and X.max() < 1.0
    rng = np.random.RandomState(42)
    far = [20.0, -20.0, 700.0, -700.0, 800.0, -800.0]
    W = 0.3 * rng.randn(3 * len(far), 2 * d)
    bad = {}
    for k, v in enumerate(far):  # rows 3 k: an ALPHA entry of column 0; rows 3 k + 1: a BETA entry of column 1; rows 3 k + 2: inside
        W[3 * k, 0], W[3 * k + 1, d + 1] = v, v
        bad[3 * k], bad[3 * k + 1] = v, v
    H = np.array([0.0, -1.0, -1.1, -3.5]) + 0.1 * rng.randn(len(W), d + 2)
    good = [b for b in range(len(W)) if b not in bad]
    ctx = lib.Context(X, y, 1e-10, max_batch=5)  # (18 rows in chunks of 5 / 5 / 5 / 3)
    try:
        got, st = ctx.lml_warped(H, W, return_status=True)
        alone = np.array([ctx.lml_warped(H[b:b + 1], W[b:b + 1])[0] for b in good])
        cdf = ctx.beta_cdf(X, np.array([800.0, 0.1, -0.2, -800.0]))
        half = [ctx.beta_cdf(np.full((1, d), 0.5), np.array([v, 0.0, v, 0.0]))[0] for v in (15.0, 20.0)]
    finally:
        ctx.close()
    for b, v in bad.items():
        print("PRECISION warp parameter %6g in row %2d: lml %s status %d" % (v, b, got[b], st[b]))
    assert not np.any(np.isnan(got))
    for b, v in bad.items():
        assert np.isfinite(got[b]) or (got[b] == -np.inf and st[b] != 0), (b, v, got[b], st[b])
        if abs(v) > 745.0:  # exp(v) is 0 or inf in fp64
            assert got[b] == -np.inf and st[b] != 0, (b, v, got[b], st[b])
    assert np.all(np.isfinite(got[good])) and np.all(st[good] == 0)
    assert np.array_equal(got[good], alone)
    assert np.all(np.isnan(cdf))  # exp(800) = inf on column 0, exp(-800) = 0 on column 1: NaN at every x
    # the slowest point of the continued fraction, a = b and x = 0.5, where the answer is 0.5 by symmetry: at the edge of the
    # domain (778 iterations in host fp64) within the tolerance; at w = (20, 20) the cap is reached -- NaN, not the 0.4826 that
    # the unconverged fraction gives.  (Column 1 is Beta(1, 1): the identity.)  Measured on the device: 0.49999999958113872 at
    # e^15, 4.2e-10 from 0.5 against a tolerance of 3.4e-7; NaN at e^20; w = +-20 in ONE entry converges (status 0), w = 700 gives
    # -inf with status 2 like +-800.
    import _warpref as WR

    a15 = float(np.exp(15.0))
    print("PRECISION beta_cdf at a = b = e^15, x = 0.5: %.17g (tol %.3e); at a = b = e^20: %s" % (half[0][0], WR.tol(a15, a15, 0.5), half[1][0]))
    assert abs(half[0][0] - 0.5) <= WR.tol(a15, a15, 0.5) and np.isnan(half[1][0])
    assert abs(half[0][1] - 0.5) <= WR.tol(1.0, 1.0, 0.5) and abs(half[1][1] - 0.5) <= WR.tol(1.0, 1.0, 0.5)
