"""Knowledge-gradient acquisition on the device (``bgp_knowledge_gradient``, bgp_kg.hip), driven through
``_lib.Context`` on the cases of tests/_kgref.py -- the eight (family, form) pairs, n = 1 and on both sides of the 64-column tile
and of the 128-pad, d = 1 .. 32, M = 0, 1, either side of a 64-lane wave and 255, m = 1, 255 / 256 / 257 and three candidate chunks,
fewer rows than resident posteriors, a candidate that is a reference point, one that is a training point, its twin 1e-8 away, one
far outside the data, coinciding reference points, a noise-free posterior with noise 0 -- and through the Python layer
(``acquisition.KnowledgeGradient``, ``Optimizer(acq_func="kg")``).

* per row and averaged against the long-double reference at the derived tolerance of tests/_kgref.py; >= 0 everywhere; exactly 0 at
  M = 0 and where the device's own s is <= 0;
* bitwise: a candidate alone and in a crowd, B = 1 against a batch, two identical calls, a forced small candidate chunk against the
  default, every combination of NULL outputs, the average against the fixed-order host average of the returned rows;
* the limits, which are error codes, and the resident posteriors afterwards.

Lines printed with ``pytest -s`` start with ``PRECISION``."""
import ctypes
import functools

import numpy as np
import pytest

import _kgref as R
import _precision as P

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

CIDS = [c["id"] for c in R.CASES]
NS = 5  # n_samples of the average (deliberately not the number of rows)


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


def _hk(H):
    Hk = np.array(H, dtype=np.float64, copy=True)
    Hk[:, -1] = -np.inf
    return Hk


def _context(lib, cid, rows=slice(None)):
    c = R.ALL[cid]
    X, y, alpha, H = R.problem(cid)[:4]
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=len(H))
    assert np.all(ctx.posterior(H[rows], want_alpha=False)["status"] == 0)
    return ctx


def _run(lib, cid, calls, rows=slice(None)):
    """One context and posterior build (rows ``rows`` of H) of the case; ``calls``: (H rows, noise, Xc, A) per device call."""
    ctx = _context(lib, cid, rows)
    try:
        return [ctx.knowledge_gradient(_hk(Hc), nz, Xc, A, R.Y_STD, NS) for Hc, nz, Xc, A in calls]
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def _cached(lib, cid):
    """The case's own call on its first Buse posteriors: (kg (Buse, m), avg (m,), the device's latent variance (Buse, m))."""
    c = R.ALL[cid]
    H, Xc, A, noise = R.problem(cid)[3], R.problem(cid)[5], R.problem(cid)[6], R.problem(cid)[7]
    B = c["Buse"]
    ctx = _context(lib, cid)
    try:
        kg, avg = ctx.knowledge_gradient(_hk(H[:B]), noise[:B], Xc, A, R.Y_STD, NS)
        var = ctx.predict(_hk(H[:B]), Xc)[1]
    finally:
        ctx.close()
    return kg, avg, var


def _host_average(kg):
    s = np.zeros(kg.shape[1])
    for b in range(kg.shape[0]):
        s = s + kg[b] / float(NS)
    return s


@pytest.mark.parametrize("cid", CIDS)
def test_against_the_long_double_reference(lib, cid):
    c = R.ALL[cid]
    kap, noise = R.problem(cid)[4], R.problem(cid)[7]
    kg, avg, var = _cached(lib, cid)
    B, m = c["Buse"], c["m"]
    assert kg.shape == (B, m) and avg.shape == (m,)
    assert np.all(np.isfinite(kg)) and (kg >= 0.0).all() and (avg >= 0.0).all()
    ref_avg, tol_avg = np.zeros(m), np.zeros(m)
    for b in range(B):
        ref = R.reference(cid, b)
        r = R.ratio(kg[b] / R.Y_STD, ref)
        print("PRECISION kg %s b%d kappa %.3g: device vs long double %.4f tol (largest KG %.3g, smallest finite tol %.3g)"
              % (cid, b, kap[b], r, float(ref["kg"].max()), float(ref["tol"].min())))
        assert r <= 1.0
        assert np.all(kg[b][var[b] + noise[b] <= 0.0] == 0.0)  # the rule where the device's own s is not positive
        ref_avg += R.Y_STD * P.f(ref["kg"]) / NS
        tol_avg += R.Y_STD * ref["tol"] / NS
    if c["M"] == 0:
        assert np.all(kg == 0.0) and np.all(avg == 0.0)
    err = np.abs(avg - ref_avg)
    with np.errstate(invalid="ignore"):
        assert np.all((err <= tol_avg) | (err == 0.0))
    assert np.array_equal(avg, _host_average(kg))


def test_the_special_points(lib):
    cid = "kg_special_n129_d3"
    kg, _avg, _var = _cached(lib, cid)
    ref = R.reference(cid, 0)
    X, y, alpha, H, kap, Xc, A, noise = R.problem(cid)
    # far outside the data every cross-covariance is below 1e-100: of the reference lines only the lowest counts (they are flat), and the
    # value is the two-line closed form of that constant and the candidate's own line, q_M f(-|mu(x) - p*| / q_M)
    from scipy.special import ndtr

    p, q = P.f(ref["p"][R.FAR]), P.f(ref["q"][R.FAR])
    assert np.abs(q[:-1]).max() <= 1e-100
    z = -abs(p[-1] - p[:-1].min()) / q[-1]
    two = q[-1] * (z * ndtr(z) + np.exp(-0.5 * z * z) / np.sqrt(2.0 * np.pi))
    assert abs(kg[0, R.FAR] - R.Y_STD * two) <= R.Y_STD * ref["tol"][R.FAR]
    # the training point and its twin 1e-8 away: each within tolerance of its own reference (asserted above), and close to each other
    assert abs(kg[0, R.TRAIN] - kg[0, R.TWIN]) <= R.Y_STD * (ref["tol"][R.TRAIN] + ref["tol"][R.TWIN]) + 1e-6 * kg[0, R.TRAIN]
    # the coinciding reference points: the second copy owns nothing (exact duplicates: the lower index wins) -- dropping it moves
    # the other lines to other lanes, i.e. changes the order of the sum and nothing else
    keep = [0, 1, 3, 4, 5]
    one = _run(lib, cid, [(H[:1], noise[:1], Xc, A[keep])])[0]
    assert np.all(np.abs(one[0] - kg) <= R.Y_STD * ref["tol"][None, :])
    assert np.abs(one[0] - kg).max() <= 64 * P.EPS * kg.max()


def test_a_noise_free_posterior_at_a_training_point(lib):
    cid = "kg_noisefree_n5_d2"
    kg, _avg, var = _cached(lib, cid)
    print("PRECISION kg %s: the device's latent variance at the training point %.3g, KG there %.3g" % (cid, var[0, 0], kg[0, 0]))
    c, kap, H = R.ALL[cid], R.problem(cid)[4], R.problem(cid)[3]
    assert var[0, 0] <= P.tol("var", kap[0], c["n"]) * float(np.exp(H[0, 0]))  # s at rounding level: within the variance's tolerance of 0
    if var[0, 0] <= 0.0:
        assert kg[0, 0] == 0.0
    assert np.all(np.isfinite(kg)) and (kg >= 0.0).all() and (kg[0, 1:] > 0.0).any()


BITS_CIDS = ["kg1_n63_d8_M1_m255_matern12_product", "kg2_n64_d17_M62_m9_matern32_product", "kg6_n65_d3_M255_m6_matern32_sum",
             "kg7_n63_d2_M5_m257_matern52_sum"]


def _raw(lib, ctx, H, noise, Xc, A, want_kg, want_avg):
    """The C call itself with either output NULL."""
    from bayes_skopt_amd._lib import _c, _p

    H, noise, Xc, A = _c(_hk(H)), _c(noise), _c(Xc), _c(np.asarray(A, dtype=np.float64).reshape(-1, Xc.shape[1]))
    B, m, M = len(H), len(Xc), len(A)
    kg, avg = np.full((B, m), np.nan), np.full(m, np.nan)
    null = ctypes.cast(None, ctypes.POINTER(ctypes.c_double))
    rc = ctx._lib.bgp_knowledge_gradient(ctx._h, B, _p(H), _p(noise), m, _p(Xc), M, _p(A) if M else null, R.Y_STD, NS,
                                         _p(kg) if want_kg else null, _p(avg) if want_avg else null)
    return rc, kg, avg


@pytest.mark.parametrize("cid", BITS_CIDS)
def test_bits_do_not_depend_on_the_company_the_outputs_asked_for_or_the_call(lib, cid):
    c = R.ALL[cid]
    H, Xc, A, noise = R.problem(cid)[3], R.problem(cid)[5], R.problem(cid)[6], R.problem(cid)[7]
    m = c["m"]
    kg, avg, _ = _cached(lib, cid)
    pick = sorted({0, m // 2, m - 1})
    out = _run(lib, cid, [(H[:1], noise[:1], Xc, A)] + [(H[:1], noise[:1], Xc[s : s + 1], A) for s in pick])
    assert np.array_equal(out[0][0], kg) and np.array_equal(out[0][1], avg)  # two calls
    for s, (k1, a1) in zip(pick, out[1:]):  # a candidate alone: m = 1
        assert np.array_equal(k1[0, 0], kg[0, s]) and np.array_equal(a1[0], avg[s])
    ctx = _context(lib, cid)
    try:
        rc, k, a = _raw(lib, ctx, H[:1], noise[:1], Xc, A, True, False)
        assert rc == 0 and np.array_equal(k, kg) and np.isnan(a).all()
        rc, k, a = _raw(lib, ctx, H[:1], noise[:1], Xc, A, False, True)
        assert rc == 0 and np.array_equal(a, avg) and np.isnan(k).all()
        rc, k, a = _raw(lib, ctx, H[:1], noise[:1], Xc, A, True, True)
        assert rc == 0 and np.array_equal(k, kg) and np.array_equal(a, avg)
        assert _raw(lib, ctx, H[:1], noise[:1], Xc, A, False, False)[0] == 1  # no output asked for: BGP_ERR_INVALID
    finally:
        ctx.close()


@pytest.mark.parametrize("cid", ["kg8_n64_d2_M3_m300_matern52_product", "kg7_n63_d2_M5_m257_matern52_sum",
                                 "kg1_n63_d8_M1_m255_matern12_product", "kg4_n129_d1_M64_m256_rbf_sum"])
def test_a_forced_small_candidate_chunk_gives_the_bits_of_the_default(lib, cid, monkeypatch):
    """BGP_KG_CHUNK=128 (read at every call): m = 300 runs as 128 + 128 + 44 candidates, m = 257 as 128 + 128 + 1, m = 256 and 255 as
    two chunks; by default each is one chunk."""
    H, Xc, A, noise = R.problem(cid)[3], R.problem(cid)[5], R.problem(cid)[6], R.problem(cid)[7]
    kg, avg, _ = _cached(lib, cid)
    monkeypatch.setenv("BGP_KG_CHUNK", str(R.CHUNK))
    got = _run(lib, cid, [(H[:1], noise[:1], Xc, A)])[0]
    monkeypatch.delenv("BGP_KG_CHUNK")
    assert np.array_equal(got[0], kg) and np.array_equal(got[1], avg)


def test_a_row_alone_and_inside_a_batch(lib):
    cid = "kg_B3_n65_d3"
    H, Xc, A, noise = R.problem(cid)[3], R.problem(cid)[5], R.problem(cid)[6], R.problem(cid)[7]
    kg, avg, _ = _cached(lib, cid)  # 2 of 3 resident posteriors
    one, three = _run(lib, cid, [(H[:1], noise[:1], Xc, A), (H, noise, Xc, A)])
    assert np.array_equal(one[0][0], kg[0]) and np.array_equal(one[1], kg[0] / float(NS))
    assert three[0].shape[0] == 3 and np.array_equal(three[0][:2], kg) and np.array_equal(three[1], _host_average(three[0]))
    alone = _run(lib, cid, [(H[1:2], noise[1:2], Xc, A)], rows=slice(1, 2))[0]  # posterior 1 built and used alone
    assert np.array_equal(alone[0][0], kg[1])


def test_limits_are_error_codes_and_leave_the_posteriors_usable(lib):
    cid = "kg3_n65_d32_M63_m5_matern52_product"
    c = R.ALL[cid]
    X, y, alpha, H, _kap, Xc, A, noise = R.problem(cid)
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=2)
    rng = np.random.RandomState(0)
    X33 = rng.uniform(size=(20, 33))
    big = lib.Context(X33, rng.randn(20), 1e-6, max_batch=1)
    call = lambda *a: ctx.knowledge_gradient(*a, R.Y_STD, NS)  # noqa: E731
    try:
        with pytest.raises(lib.BgpError, match=r"code 4"):  # nothing built
            call(_hk(H[:1]), noise[:1], Xc, A)
        assert np.all(ctx.posterior(H[:1], want_alpha=False)["status"] == 0)
        before = ctx.predict(H[:1], Xc)
        with pytest.raises(lib.BgpError, match=r"code 4"):  # more rows than resident posteriors
            call(_hk(np.repeat(H[:1], 2, axis=0)), np.repeat(noise[:1], 2), Xc, A)
        with pytest.raises(lib.BgpError, match=r"code 1.*exceed"):  # M = 256
            call(_hk(H[:1]), noise[:1], Xc, rng.uniform(size=(256, c["d"])))
        with pytest.raises(lib.BgpError, match=r"code 1"):  # n_samples = 0
            ctx.knowledge_gradient(_hk(H[:1]), noise[:1], Xc, A, R.Y_STD, 0)
        with pytest.raises(ValueError):
            call(_hk(H[:1]), noise[:1], Xc[:, :3], A[:, :3])
        after = ctx.predict(H[:1], Xc)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        good = call(_hk(H[:1]), noise[:1], Xc, A)
        assert np.array_equal(good[0], _cached(lib, cid)[0]) and np.array_equal(good[1], _cached(lib, cid)[1])
        after = ctx.predict(H[:1], Xc)  # a successful call leaves them untouched too
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        # the posteriors rebuilt as per-row-warped ones: only predict_warped reads those
        assert np.all(ctx.posterior(H[:1], want_alpha=False, warps=np.zeros((1, 2 * c["d"])))["status"] == 0)
        with pytest.raises(lib.BgpError, match=r"code 4.*per-row warped"):
            call(_hk(H[:1]), noise[:1], Xc, A)
        assert np.all(ctx.posterior(H[:1], want_alpha=False)["status"] == 0)
        after = ctx.predict(H[:1], Xc)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        # a context-level warp: refused as by the gradient entry points
        ctx.set_warp(np.zeros(2 * c["d"]))
        assert np.all(ctx.posterior(H[:1], want_alpha=False)["status"] == 0)
        with pytest.raises(lib.BgpError, match=r"code 1.*warped inputs"):
            call(_hk(H[:1]), noise[:1], np.clip(Xc, 0.0, 1.0), np.clip(A, 0.0, 1.0))
        assert np.all(np.isfinite(ctx.predict(H[:1], np.clip(Xc, 0.0, 1.0))[0]))
        h33 = np.concatenate([[0.0], np.zeros(33), [-4.0]])[None, :]
        assert np.all(big.posterior(h33, want_alpha=False)["status"] == 0)
        with pytest.raises(lib.BgpError, match=r"code 1.*d > 32"):
            big.knowledge_gradient(_hk(h33), [1e-3], X33[:2], X33[2:4], 1.0, 1)
        assert np.all(np.isfinite(big.predict(h33, X33[:2])[0]))
    finally:
        ctx.close()
        big.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the Python layer
# ------------------------------------------------------------------------------------------------------------------------------
FIT = dict(n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)


def _toy(n=30, d=2, seed=0):
    rng = np.random.RandomState(seed)
    Xt = rng.uniform(size=(n, d))
    y = np.sin(5.0 * Xt[:, 0]) + Xt[:, 1] ** 2 + 0.05 * rng.randn(n)
    return Xt, y, rng.uniform(size=(70, d))


@pytest.fixture(scope="module")
def fitted_gp(bask):
    Xt, y, Xc = _toy()
    gp = bask.BayesGPR(kernel=bask.construct_default_kernel([0, 1]), normalize_y=True, random_state=1)
    gp.fit(Xt, y, **FIT)
    assert gp._post.canonical
    return gp, Xc


def _python_tolerance(gp, thetas, Xc, A):
    """The derived tolerance (tests/_kgref.py) in y units for the rows ``thetas`` of a fitted canonical model, averaged over the rows,
    from fp64 quantities: the lines from the device's predictive covariance, kappa of the row's Gram matrix, the mean's scale over
    [A; x] and the prior variance."""
    from oracle import gp_oracle as O

    st, fm = gp._plan.stationary, gp._plan.form
    Xt, d, n = gp._X_train_, gp._X_train_.shape[1], gp._X_train_.shape[0]
    y_std = float(np.ravel(gp.y_train_std_)[0])
    H = gp._canonical(np.atleast_2d(thetas))
    ad = np.broadcast_to(gp._alpha_diag(), (n,))
    Q = np.vstack([A, Xc])
    M = len(A)
    assert np.all(gp._ctx.posterior(H, want_alpha=True)["status"] == 0)
    mean, var, cov = gp._ctx.predict(_hk(H), Q, return_cov=True)
    total = np.zeros(len(Xc))
    for b in range(len(H)):
        a = np.linalg.solve(O.gram_with_jitter(Xt, ad, H[b], st, fm), gp.y_train_)
        sc = np.abs(O.kernel_matrix(Q, _hk(H)[b], st, fm, Y=Xt) * a[None, :]).sum(axis=1)
        mean_scale = np.maximum(sc[:M].max() if M else 0.0, sc[M:])
        pv = float(O.kernel_diag(1, _hk(H)[b], d, fm)[0])
        kap = P.kappa_of(Xt, ad, H[b], st, fm)
        t_mean, t_var = P.tol("mean", kap, n), P.tol("var", kap, n)
        s = var[b, M:] + gp._fantasy_base_alpha() + np.exp(H[b, -1])
        qmax = np.abs(np.concatenate([cov[b, :M, M:].T, var[b, M:, None]], axis=1)).max(axis=1) / np.sqrt(s)
        total += y_std * (2.0 * t_mean * mean_scale + R.SQ2PI * (t_var * pv / np.sqrt(s) + qmax * t_var * pv / (2.0 * s))) / len(H)
    return total


@pytest.mark.parametrize("n_gp_samples", [0, 4])
def test_device_path_equals_host_path(bask, fitted_gp, n_gp_samples, monkeypatch):
    gp, Xc = fitted_gp
    KG = bask.acquisition.KnowledgeGradient()
    dev, path = KG(Xc, gp, n_reference=9, n_gp_samples=n_gp_samples, random_state=3, return_path=True)
    monkeypatch.setattr(bask.acquisition.KnowledgeGradient, "path", "host")
    host, hpath = KG(Xc, gp, n_reference=9, n_gp_samples=n_gp_samples, random_state=3, return_path=True)
    monkeypatch.undo()
    assert (path, hpath) == ("device", "host") and dev.shape == host.shape == (len(Xc),)
    assert (dev >= 0.0).all() and np.all(np.isfinite(dev)) and dev.max() > 0.0
    A = Xc[np.argsort(gp.predict(Xc), kind="stable")[:9]]
    rows = gp._post_theta[None, :] if n_gp_samples == 0 else gp.chain_[
        np.random.RandomState(3).choice(len(gp.chain_), replace=False, size=n_gp_samples)]
    tol = _python_tolerance(gp, rows, Xc, A)
    r = float((np.abs(dev - host) / tol).max())
    print("PRECISION kg python n_gp_samples=%d: device vs host path %.4f tol (largest value %.3g, smallest tol %.3g)"
          % (n_gp_samples, r, dev.max(), tol.min()))
    assert r <= 1.0
    # explicit reference points are taken as given, and M = 0 gives zeros
    again = KG(Xc, gp, reference_points=A, n_gp_samples=n_gp_samples, random_state=3)
    assert np.array_equal(again, dev)
    assert np.all(KG(Xc, gp, n_reference=0) == 0.0)
    assert np.all(np.isfinite(gp.predict(Xc)))  # the estimator's own posterior is back where a consumer needs it


def test_generic_trees_and_warped_inputs_take_the_host_path_and_say_so_once(bask, capfd, monkeypatch):
    import sklearn.gaussian_process.kernels as sk

    Xt, y, Xc = _toy(n=20)
    Xc = Xc[:24]
    monkeypatch.setattr(bask.acquisition, "_kg_told", [])
    capfd.readouterr()
    KG = bask.acquisition.KnowledgeGradient()
    gen = bask.BayesGPR(kernel=sk.Matern(length_scale=0.4, nu=2.5) * sk.RBF(length_scale=0.7) + sk.WhiteKernel(0.05),
                        normalize_y=True, random_state=4)
    gen.fit(Xt, y, **FIT)
    assert not gen._post.canonical
    v1, p1 = KG(Xc, gen, n_reference=5, return_path=True)
    v2, p2 = KG(Xc, gen, n_reference=5, n_gp_samples=2, random_state=0, return_path=True)
    gw = bask.BayesGPR(kernel=bask.construct_default_kernel([0, 1]), random_state=1, warp_inputs=True, normalize_y=True)
    gw.fit(Xt, y, **FIT)
    v3, p3 = KG(Xc, gw, n_reference=5, return_path=True)
    v4, p4 = KG(Xc, gw, n_reference=5, n_gp_samples=2, random_state=0, return_path=True)
    assert p1 == p2 == p3 == p4 == "host"
    for v in (v1, v2, v3, v4):
        assert v.shape == (len(Xc),) and np.all(np.isfinite(v)) and (v >= 0.0).all() and v.max() > 0.0
    err = capfd.readouterr().err
    assert err.count("knowledge_gradient: on the host") == 1
    assert np.all(np.isfinite(gw.predict(Xc))) and np.all(np.isfinite(gen.predict(Xc)))


def test_optimizer_with_the_knowledge_gradient(bask):
    f = lambda x: (x[0] - 0.3) ** 2 + (x[1] + 0.2) ** 2  # noqa: E731
    opt = bask.Optimizer(dimensions=[(-1.0, 1.0)] * 2, n_points=60, n_initial_points=10, init_strategy="r2", acq_func="kg",
                         acq_func_kwargs=dict(n_reference=7), random_state=0)
    assert isinstance(opt.acq_func, bask.acquisition.KnowledgeGradient)
    rng = np.random.RandomState(0)
    X0 = rng.uniform(-1.0, 1.0, size=(10, 2)).tolist()
    opt.tell(X0, [f(x) + 0.01 * rng.randn() for x in X0], gp_samples=40, gp_burnin=2)
    for _ in range(2):
        x = opt.ask()
        assert all(-1.0 <= v <= 1.0 for v in x)
        opt.tell(x, f(x) + 0.01 * rng.randn(), gp_samples=40, gp_burnin=2)
    assert len(opt.Xi) == 12
    x = opt.ask()
    assert all(-1.0 <= v <= 1.0 for v in x)
    # the proposal is the argmax of the values the acquisition returns for the recorded candidates
    cand, vals = opt._last_candidates, opt._last_acq_values
    own = opt.acq_func(cand, opt.gp, n_reference=7)
    assert np.array_equal(own, vals) and vals.max() > 0.0
    assert list(map(float, x)) == list(map(float, opt.space.inverse_transform(cand[np.argmax(own)].reshape(1, -1))[0]))
    pts = opt.ask(n_points=3)
    assert opt._last_batch_info["path"] == "fallback"
    assert len(pts) == 3 and len({tuple(map(float, p)) for p in pts}) == 3
    assert all(-1.0 <= v <= 1.0 for p in pts for v in p)
    assert list(map(float, pts[0])) == list(map(float, x))
