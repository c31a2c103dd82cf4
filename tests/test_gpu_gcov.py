"""Posterior covariance of the surrogate's gradient and the active-subspace sums on the device (``bgp_grad_cov``, bgp_gcov.hip;
DESIGN.md section 22), driven through ``_lib.Context`` on the cases of tests/_gcovref.py -- the six differentiable (family, form)
pairs, n = 1 and on both sides of the 64-point training tile and of the 128-pad, d = 1 and at the padded widths 8 / 16 / 32 and
just past them, m d at a 128-row tile edge, m at the 256-point reduction chunk - 1, exact, + 1 and over several chunks, fewer items
than resident posteriors, a query that is a training point, one 1e-8 from it, one far outside the data -- and through the Python
layer (``BayesGPR.gradient_posterior`` / ``active_subspace``, ``utils.active_subspace``, ``Optimizer.active_subspace``).

* dmean, cov and both sums against the long-double reference at the tolerances tests/test_cpu_gcov_reference.py qualifies; exact
  symmetry; the smallest eigenvalue of Sigma / scale >= -d tol; the sums against the fixed-order sum of the per-point outputs;
* bitwise: a point alone and in a crowd, B = 1 against a batch, two identical calls, a forced small point chunk against the
  default, every combination of NULL outputs;
* the limits, which are error codes, and the resident posteriors afterwards.

Lines printed with ``pytest -s`` start with ``PRECISION``."""
import functools

import numpy as np
import pytest

import _gcovref as R
import _precision as P

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

CIDS = [c["id"] for c in R.CASES]


@pytest.fixture(scope="module")
def lib():
    import bayes_skopt_amd  # noqa: F401
    from bayes_skopt_amd import _lib

    assert _lib.device_count() >= 1
    return _lib


@pytest.fixture(scope="module")
def bask():
    import bayes_skopt_amd as bask

    assert bask._lib.device_count() >= 1
    return bask


def _context(lib, cid, rows=slice(None)):
    c = R.ALL[cid]
    X, y, alpha, H, _kap, _Xq = R.problem(cid)
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=len(H))
    assert np.all(ctx.posterior(H[rows], want_alpha=False)["status"] == 0)
    return ctx


def _run(lib, cid, calls, rows=slice(None)):
    """One context and posterior build (rows ``rows`` of H) of the case; ``calls``: (H rows of the call, Xq, wants) per device call."""
    ctx = _context(lib, cid, rows)
    try:
        return [ctx.grad_cov(Hc, Xq, *want) for Hc, Xq, want in calls]
    finally:
        ctx.close()


ALL3 = (True, True, True)


@functools.lru_cache(maxsize=None)
def _cached(lib, cid):
    """The case's own call: its first Buse posteriors, every output."""
    c = R.ALL[cid]
    H, Xq = R.problem(cid)[3], R.problem(cid)[5]
    return _run(lib, cid, [(H[: c["Buse"]], Xq, ALL3)])[0]


def _device_order_sums(dmean, cov):
    """The sums of bgp_gcov.hip from fp64 per-point values, in ITS order: chunks of 256 points; inside a chunk the butterfly of a
    64-lane wave (lanes i and i + w added, w = 32 .. 1), the four waves in ascending order; chunk partials in ascending order; one
    division by m."""
    m, d = dmean.shape
    vals = np.concatenate([(dmean[:, :, None] * dmean[:, None, :]).reshape(m, d * d), cov.reshape(m, d * d)], axis=1)
    acc = np.zeros(2 * d * d)
    for i0 in range(0, m, R.RC):
        v = np.zeros((R.RC, 2 * d * d))
        v[: min(R.RC, m - i0)] = vals[i0 : i0 + R.RC]
        w = v.reshape(4, 64, -1)
        width = 32
        while width >= 1:
            w = w[:, :width] + w[:, width : 2 * width]
            width //= 2
        w = w[:, 0]
        acc = acc + (((w[0] + w[1]) + w[2]) + w[3])
    out = (acc / m).reshape(2, d, d)
    return out[0], out[1]


@pytest.mark.parametrize("cid", CIDS)
def test_against_the_long_double_reference(lib, cid):
    c = R.ALL[cid]
    kap = R.problem(cid)[4]
    dmean, cov, csum = _cached(lib, cid)
    B, m, d = c["Buse"], c["m"], c["d"]
    assert dmean.shape == (B, m, d) and cov.shape == (B, m, d, d) and csum.shape == (B, 2, d, d)
    assert np.array_equal(cov, np.swapaxes(cov, 2, 3)) and np.array_equal(csum, np.swapaxes(csum, 2, 3))
    assert (cov[:, :, np.arange(d), np.arange(d)] >= 0.0).all()
    for b in range(B):
        ref = R.reference(cid, b)
        t_var, t_mean = P.tol("var", kap[b], c["n"]), P.tol("mean", kap[b], c["n"])
        e_cov, e_dm = R.err_cov(cov[b], ref) / t_var, R.err_dmean(dmean[b], ref) / t_mean
        r_mean, r_cov = R.csum_ratio(csum[b, 0], csum[b, 1], ref, t_mean, t_var)
        eig = R.min_eig_scaled(cov[b], ref)
        own = _device_order_sums(dmean[b], cov[b])
        s_mean, s_cov = R.csum_ratio(csum[b, 0], csum[b, 1], dict(ref, C_mean=own[0], C_cov=own[1]), t_mean, t_var)
        print("PRECISION gcov %s b%d kappa %.3g: device vs long double cov %.4f dmean %.4f C_mean %.4f C_cov %.4f tol; smallest "
              "eigenvalue of Sigma / scale %.4g; sums vs the fixed-order sum of the outputs %.2g %.2g tol, bitwise %s"
              % (cid, b, kap[b], e_cov, e_dm, r_mean, r_cov, eig, s_mean, s_cov,
                 np.array_equal(csum[b, 0], own[0]) and np.array_equal(csum[b, 1], own[1])))
        assert max(e_cov, e_dm, r_mean, r_cov) <= 1.0
        assert eig >= -d * t_var
        assert max(s_mean, s_cov) <= 1.0
        assert np.array_equal(csum[b, 0], own[0]) and np.array_equal(csum[b, 1], own[1])


def test_a_training_point_its_near_twin_and_a_far_point(lib):
    cid = "gc_special_n129_d3"
    c = R.ALL[cid]
    kap = R.problem(cid)[4]
    dmean, cov, _ = _cached(lib, cid)
    ref = R.reference(cid, 0)
    t_var, t_mean = P.tol("var", kap[0], c["n"]), P.tol("mean", kap[0], c["n"])
    sc = R.h0_scale(ref)
    # far outside the data every fac underflows: Sigma is H0, g is 0 -- within the tolerances, here exactly
    assert (np.abs(cov[0, R.FAR] - np.diag(P.f(ref["H0"]))) / sc).max() <= t_var
    assert np.abs(dmean[0, R.FAR]).max() <= t_mean * ref["scale_dmean"]
    for s in (0, 1):  # the training point and its twin 1e-8 away: each within tolerance of its own reference, and of each other
        assert (np.abs(cov[0, s] - P.f(ref["cov"][s])) / sc).max() <= t_var
    assert np.all(np.isfinite(cov)) and np.all(np.isfinite(dmean))


BITS_CIDS = ["gc1_n63_d3_m255_matern32_product", "gc4_n129_d8_m17_matern32_sum", "gc7_n65_d17_m9_matern32_product",
             "gc8_n129_d32_m4_matern52_product", "gc12_n64_d1_m600_rbf_product"]


@pytest.mark.parametrize("cid", BITS_CIDS)
def test_bits_do_not_depend_on_the_company_the_outputs_asked_for_or_the_call(lib, cid):
    c = R.ALL[cid]
    H, Xq = R.problem(cid)[3], R.problem(cid)[5]
    m = c["m"]
    pick = sorted({0, m // 2, m - 1})
    wants = [(True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)]
    calls = [(H[:1], Xq, ALL3)] + [(H[:1], Xq[s : s + 1], ALL3) for s in pick] + [(H[:1], Xq, w) for w in wants]
    out = _run(lib, cid, calls)
    dmean, cov, csum = _cached(lib, cid)
    again = out[0]
    assert np.array_equal(again[0], dmean) and np.array_equal(again[1], cov) and np.array_equal(again[2], csum)  # two calls
    for s, (dm1, cv1, cs1) in zip(pick, out[1 : 1 + len(pick)]):  # a point alone: m = 1
        assert np.array_equal(dm1[0, 0], dmean[0, s]) and np.array_equal(cv1[0, 0], cov[0, s])
        assert np.array_equal(cs1[0, 0], np.outer(dm1[0, 0], dm1[0, 0])) and np.array_equal(cs1[0, 1], cv1[0, 0])
    for w, got in zip(wants, out[1 + len(pick) :]):  # NULL outputs
        for have, g, full in zip(w, got, (dmean, cov, csum)):
            assert (g is None) == (not have)
            if have:
                assert np.array_equal(g, full)


@pytest.mark.parametrize("cid", ["gc12_n64_d1_m600_rbf_product", "gc11_n65_d2_m257_matern32_sum", "gc1_n63_d3_m255_matern32_product"])
def test_a_forced_small_point_chunk_gives_the_bits_of_the_default(lib, cid, monkeypatch):
    """BGP_GCOV_CHUNK=256 (read at every call): m = 600 runs as 256 + 256 + 88 points, m = 257 as 256 + 1, m = 255 as one chunk."""
    H, Xq = R.problem(cid)[3], R.problem(cid)[5]
    dmean, cov, csum = _cached(lib, cid)
    monkeypatch.setenv("BGP_GCOV_CHUNK", "256")
    got = _run(lib, cid, [(H[:1], Xq, ALL3), (H[:1], Xq, (False, False, True))])
    monkeypatch.delenv("BGP_GCOV_CHUNK")
    assert np.array_equal(got[0][0], dmean) and np.array_equal(got[0][1], cov) and np.array_equal(got[0][2], csum)
    assert np.array_equal(got[1][2], csum)


def test_an_item_alone_and_inside_a_batch(lib):
    cid = "gc_B3_n65_d3"
    H, Xq = R.problem(cid)[3], R.problem(cid)[5]
    dmean, cov, csum = _cached(lib, cid)  # 2 of 3 resident posteriors
    one = _run(lib, cid, [(H[:1], Xq, ALL3), (H, Xq, ALL3)])
    for got, full in zip(one[0], (dmean, cov, csum)):
        assert np.array_equal(got[0], full[0])
    for got, full in zip(one[1], (dmean, cov, csum)):  # all three
        assert got.shape[0] == 3 and np.array_equal(got[:2], full)
    alone = _run(lib, cid, [(H[1:2], Xq, ALL3)], rows=slice(1, 2))[0]  # posterior 1 built and used alone
    for got, full in zip(alone, (dmean, cov, csum)):
        assert np.array_equal(got[0], full[1])


def test_limits_are_error_codes_and_leave_the_posteriors_usable(lib):
    cid = "gc8_n129_d32_m4_matern52_product"
    c = R.ALL[cid]
    X, y, alpha, H, _kap, Xq = R.problem(cid)
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=2)
    m12 = lib.Context(X, y, alpha, form=c["form"], stationary="matern12", max_batch=1)
    rng = np.random.RandomState(0)
    X33 = rng.uniform(size=(20, 33))
    big = lib.Context(X33, rng.randn(20), 1e-6, max_batch=1)
    try:
        with pytest.raises(lib.BgpError, match=r"code 4"):  # nothing built
            ctx.grad_cov(H[:1], Xq)
        assert np.all(ctx.posterior(H[:1], want_alpha=False)["status"] == 0)
        before = ctx.predict(H[:1], Xq)
        with pytest.raises(lib.BgpError, match=r"code 4"):  # more items than resident posteriors
            ctx.grad_cov(np.repeat(H[:1], 2, axis=0), Xq)
        with pytest.raises(lib.BgpError, match=r"code 1"):  # no output asked for
            ctx.grad_cov(H[:1], Xq, False, False, False)
        with pytest.raises(lib.BgpError, match=r"code 1.*exceeds"):  # m d over 2^24 (nothing is read)
            ctx.grad_cov(H[:1], np.zeros(((1 << 24) // c["d"] + 1, c["d"])), False, False, True)
        with pytest.raises(ValueError):
            ctx.grad_cov(H[:1], Xq[:, :3])
        after = ctx.predict(H[:1], Xq)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        good = ctx.grad_cov(H[:1], Xq)
        assert np.array_equal(good[0], _cached(lib, cid)[0]) and np.array_equal(good[1], _cached(lib, cid)[1])
        # a context-level warp: refused as by the other gradient entry points
        ctx.set_warp(np.zeros(2 * c["d"]))
        assert np.all(ctx.posterior(H[:1], want_alpha=False)["status"] == 0)
        with pytest.raises(lib.BgpError, match=r"code 1.*warped inputs"):
            ctx.grad_cov(H[:1], np.clip(Xq, 0.0, 1.0))
        assert np.all(np.isfinite(ctx.predict(H[:1], np.clip(Xq, 0.0, 1.0))[0]))
        # Matern 1/2 is not differentiable: refused, never approximated
        assert np.all(m12.posterior(H[:1], want_alpha=False)["status"] == 0)
        with pytest.raises(lib.BgpError, match=r"code 1.*not differentiable"):
            m12.grad_cov(H[:1], Xq)
        assert np.all(np.isfinite(m12.predict(H[:1], Xq)[0]))
        h33 = np.concatenate([[0.0], np.zeros(33), [-4.0]])[None, :]
        assert np.all(big.posterior(h33, want_alpha=False)["status"] == 0)
        with pytest.raises(lib.BgpError, match=r"code 1.*d > 32"):
            big.grad_cov(h33, X33[:2])
    finally:
        ctx.close()
        m12.close()
        big.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the Python layer
# ------------------------------------------------------------------------------------------------------------------------------
def _model_tolerances(bask, gp, X):
    """(bound on |d grad_mean|, bound matrix on |d grad_cov_kl|, bounds on C_mean / C_cov) in y units for a fitted canonical model
    at the rows X: tol("mean") / tol("var") at kappa of its training Gram matrix on the metrics of tests/_gcovref.py, evaluated
    with the fp64 host forms."""
    Kt = gp.kernel_(gp.X_train_) + np.diag(np.broadcast_to(gp.alpha, (len(gp.X_train_),)))
    w = np.linalg.eigvalsh(Kt)
    kappa, n = float(w[-1] / w[0]), len(Kt)
    hk = gp._canonical(gp._kernel_theta_for_predict())[0]
    G, h0 = bask.gradcov.cross_gradient(hk, gp.X_train_, X, gp._plan.stationary, gp._plan.form)
    a = np.ravel(gp.alpha_)
    y_std = float(np.ravel(gp.y_train_std_)[0])
    scale = float(np.abs(G * a[None, :, None]).sum(axis=1).max())
    b_dmean = P.tol("mean", kappa, n) * scale * y_std
    b_cov = P.tol("var", kappa, n) * np.sqrt(h0[:, None] * h0[None, :]) * y_std**2
    g = np.abs(np.einsum("sjk,j->sk", G, a)).mean(axis=0)
    b_cmean = P.tol("mean", kappa, n) * scale * (g[:, None] + g[None, :]) * y_std**2
    return b_dmean, b_cov, b_cmean


def _angle(u, v):
    return float(np.arccos(min(1.0, abs(float(u @ v)) / (np.linalg.norm(u) * np.linalg.norm(v)))))


def test_optimizer_active_subspace_and_gradient_posterior(bask, monkeypatch, capfd):
    from bayes_skopt_amd import _posterior, gradcov
    from bayes_skopt_amd.space import Real

    dims = [Real(-1.0, 1.0), Real(-1.0, 1.0), Real(0.0, 1.0)]
    opt = bask.Optimizer(dimensions=dims, n_initial_points=12, random_state=0)
    f = lambda x: float(np.sin(1.5 * (x[0] + x[1])))  # (varies along x_0 + x_1 only)
    opt.run(f, n_iter=20, n_samples=1, gp_samples=40, gp_burnin=5)
    gp, space = opt.gp, opt.space
    assert gp._post.canonical
    N = 300
    Xs = space.rvs_transformed(N, random_state=np.random.RandomState(5))
    b_dmean, b_cov, b_cmean = _model_tolerances(bask, gp, Xs)
    # gradient_posterior: the mean is predict_gradients' grad_mean (both carry the tolerance), the covariance is symmetric and PSD
    gm, gc, path = gp.gradient_posterior(Xs, return_path=True)
    assert path == "device" and gm.shape == (N, 3) and gc.shape == (N, 3, 3)
    assert np.abs(gm - gp.predict_gradients(Xs, return_std=False)[1]).max() <= 2.0 * b_dmean
    assert np.array_equal(gc, np.swapaxes(gc, 1, 2))
    # the active subspace: utils / Optimizer are the estimator's two sums, assembled
    out = opt.active_subspace(n_samples=N, random_state=5)
    C_mean, C_cov = gp.active_subspace(Xs)
    assert out["path"] == "device" and np.array_equal(out["C_mean"], C_mean) and np.array_equal(out["C_cov"], C_cov)
    assert np.array_equal(out["C"], C_mean + C_cov) and np.all(np.diff(out["eigenvalues"]) <= 0.0)
    # device against the forced host path: gradient_posterior, and the sums
    capfd.readouterr()
    monkeypatch.setattr(gradcov, "_told", [])
    monkeypatch.setattr(_posterior.CanonicalPosterior, "gradient_cov_path", "host")
    hm, hc, hpath = gp.gradient_posterior(Xs, return_path=True)
    host = opt.active_subspace(n_samples=N, random_state=5)
    monkeypatch.setattr(_posterior.CanonicalPosterior, "gradient_cov_path", "auto")
    err = capfd.readouterr().err
    assert hpath == "host" and host["path"] == "host" and err.count("gradient covariance: numpy on the downloaded inverse") == 1
    assert np.abs(gm - hm).max() <= 2.0 * b_dmean and np.all(np.abs(gc - hc) <= 2.0 * b_cov[None])
    assert np.all(np.abs(out["C_mean"] - host["C_mean"]) <= 2.0 * b_cmean) and np.all(np.abs(out["C_cov"] - host["C_cov"]) <= 2.0 * b_cov)
    # the leading direction: as close to (1, 1, 0) / sqrt 2 as the fp64 host path on the same model finds it, plus the first-order
    # rotation of an eigenvector under the matrices' tolerances, ||dC||_F / (lambda_1 - lambda_2) with |dC_kl| <= 2 (bounds)
    target = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0)
    a_host = _angle(host["eigenvectors"][:, 0], target)
    gap = float(host["eigenvalues"][0] - host["eigenvalues"][1])
    rot = float(np.linalg.norm(2.0 * (b_cmean + b_cov))) / gap
    a_dev = _angle(out["eigenvectors"][:, 0], target)
    print("PRECISION gcov active subspace: leading direction %.4f rad from (1, 1, 0) / sqrt 2 on the device, %.4f on the host path; "
          "first-order rotation bound %.3g; explained %s" % (a_dev, a_host, rot, np.round(out["explained"], 4)))
    assert a_dev <= a_host + rot
    v = out["eigenvectors"][:, 0]
    assert v[np.argmax(np.abs(v))] > 0.0
    # the fully Bayesian matrices: the mean of per-row calls, with the band of the ranked eigenvalues
    fb = bask.utils.active_subspace(opt._result(), n_samples=N, n_gp_samples=4, random_state=11)
    r11 = np.random.RandomState(11)
    X2 = space.rvs_transformed(N, random_state=r11)
    rows = np.asarray(gp.chain_)[r11.randint(0, len(gp.chain_), size=4)]
    per = [gp.active_subspace(X2, thetas=r[None, :]) for r in rows]  # (an item's bits do not depend on what shares the build or the call)
    assert fb["path"] == "device"
    assert np.array_equal(fb["C_mean"], np.stack([p[0][0] for p in per]).mean(axis=0))
    assert np.array_equal(fb["C_cov"], np.stack([p[1][0] for p in per]).mean(axis=0))
    lo, hi = fb["band"]
    assert lo.shape == hi.shape == (3,) and np.all(lo <= hi)
    gmB, gcB = gp.gradient_posterior(X2[:7], thetas=rows)
    assert gmB.shape == (4, 7, 3) and gcB.shape == (4, 7, 3, 3)
    # more rows than one batched build holds: a build and a call per max_batch rows, every row with the bits it has alone
    chain = np.asarray(gp.chain_)
    many = chain[np.arange(int(gp._ctx.max_batch) + 6) % len(chain)]
    cmB, ccB = gp.active_subspace(X2[:20], thetas=many)
    assert cmB.shape == ccB.shape == (len(many), 3, 3)
    for sl in (slice(0, 3), slice(len(many) - 6, len(many))):
        cm1, cc1 = gp.active_subspace(X2[:20], thetas=many[sl])
        assert np.array_equal(cmB[sl], cm1) and np.array_equal(ccB[sl], cc1)
    # given samples in the original space
    pts = space.inverse_transform(X2[:50])
    giv = bask.utils.active_subspace(opt._result(), samples=pts)
    cm, cc = gp.active_subspace(space.transform(pts))
    assert np.array_equal(giv["C_mean"], cm) and np.array_equal(giv["C_cov"], cc)
    with pytest.raises(ValueError):
        gp.gradient_posterior(Xs[:, :2])
    with pytest.raises(RuntimeError):
        bask.BayesGPR(kernel=bask.construct_default_kernel([0])).gradient_posterior(Xs)


def test_what_is_refused_and_the_host_path_beyond_32_dimensions(bask, capfd, monkeypatch):
    import sklearn.gaussian_process.kernels as sk

    from bayes_skopt_amd import gradcov

    rng = np.random.RandomState(0)
    n = 30
    Xt = rng.uniform(size=(n, 2))
    y = np.sin(5.0 * Xt[:, 0]) + Xt[:, 1] ** 2 + 0.05 * rng.randn(n)
    fit = dict(n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
    # Matern 1/2: no mean-square derivative
    g12 = bask.BayesGPR(kernel=sk.ConstantKernel(1.0) * sk.Matern([0.5, 0.5], nu=0.5) + sk.WhiteKernel(0.05), normalize_y=True,
                        random_state=1)
    g12.fit(Xt, y, **fit)
    assert g12._post.canonical
    with pytest.raises(ValueError, match="not differentiable"):
        g12.gradient_posterior(Xt[:3])
    with pytest.raises(ValueError, match="not differentiable"):
        g12.active_subspace(Xt[:3])
    # a generic kernel tree: no closed-form cross derivative
    gen = bask.BayesGPR(kernel=sk.Matern(length_scale=0.4, nu=2.5) * sk.RBF(length_scale=0.7) + sk.WhiteKernel(0.05),
                        normalize_y=True, random_state=4)
    gen.fit(Xt, y, **fit)
    assert not gen._post.canonical
    with pytest.raises(NotImplementedError, match="generic kernel tree"):
        gen.gradient_posterior(Xt[:3])
    # warped inputs: the chain rule through the Beta pdf is not built
    gw = bask.BayesGPR(kernel=bask.construct_default_kernel([0, 1]), random_state=1, warp_inputs=True, normalize_y=True)
    gw.fit(Xt, y, **fit)
    with pytest.raises(NotImplementedError, match="warp_inputs"):
        gw.active_subspace(Xt[:3])
    assert np.all(np.isfinite(gw.predict(Xt[:3])))
    # 33 dimensions: numpy on the downloaded inverse, said once
    monkeypatch.setattr(gradcov, "_told", [])
    capfd.readouterr()
    X33 = rng.uniform(size=(24, 33))
    y33 = np.sin(X33[:, 0] + X33[:, 1]) + 0.05 * rng.randn(24)
    g33 = bask.BayesGPR(kernel=bask.construct_default_kernel(list(range(33))), normalize_y=True, random_state=2)
    g33.fit(X33, y33, **dict(fit, n_walkers_per_thread=80))  # (the ensemble move wants >= 2 walkers per parameter: 35 here)
    gm, gc, path = g33.gradient_posterior(X33[:5] + 0.01, return_path=True)
    cm, cc, path2 = g33.active_subspace(X33[:5] + 0.01, return_path=True)
    assert path == path2 == "host" and gm.shape == (5, 33) and gc.shape == (5, 33, 33)
    assert np.array_equal(gc, np.swapaxes(gc, 1, 2)) and (gc[:, np.arange(33), np.arange(33)] >= 0.0).all()
    np.testing.assert_allclose(cc, gc.mean(axis=0), rtol=1e-13, atol=0)
    assert capfd.readouterr().err.count("gradient covariance: numpy on the downloaded inverse (more than 32 dimensions)") == 1
