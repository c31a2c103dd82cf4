"""Joint entropy search acquisition on the device (``bgp_joint_entropy``, bgp_jes.hip), driven through
``_lib.Context`` on the cases of tests/_jesref.py -- the eight (family, form) pairs, n = 1 and on both sides of the 64-column tile and
of the 128-pad, d = 1 .. 32, R = 1, 2, 5, either side of a 64-lane wave and 255, m = 1, 255 / 256 / 257 and three candidate chunks,
fewer rows than resident posteriors with an optimum set per posterior, a candidate that is an optimum point, one that is a training
point, its twin 1e-8 away, one far outside the data, coinciding optimum points, a sample with z ~ 1e3, a near-noise-free posterior
with tau = 0 and an optimum point on a training point -- and through the Python layer (``acquisition.JointEntropySearch``,
``Optimizer(acq_func="jes")``).

* per row and averaged against the long-double reference at the derived tolerance of tests/_jesref.py; the invariants
  ``0 <= gain <= 1/2 log1p(v / nu)`` on the device's own variance;
* bitwise: a candidate alone and in a crowd, B = 1 against a batch, two identical calls, a forced small candidate chunk against the
  default, every combination of NULL outputs, the average against the fixed-order host average of the returned rows; a following
  predict returns its earlier bits;
* the limits, which are error codes, and the resident posteriors afterwards.

Lines printed with ``pytest -s`` start with ``PRECISION``."""
import ctypes
import functools

import numpy as np
import pytest

import _jesref as R
import _precision as P

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

CIDS = [c["id"] for c in R.CASES]
NS = R.NS


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
    """One context and posterior build (rows ``rows`` of H) of the case; ``calls``: (H rows, noise, Xc, A, f) per device call."""
    tau = R.problem(cid)[9]
    ctx = _context(lib, cid, rows)
    try:
        return [ctx.joint_entropy(_hk(Hc), nz, Xc, A, f, tau, NS) for Hc, nz, Xc, A, f in calls]
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def _cached(lib, cid):
    """The case's own call on its first Buse posteriors: (gain (Buse, m), avg (m,), the device's latent variance (Buse, m), and
    whether a following predict returned the bits of one before the call)."""
    c = R.ALL[cid]
    X, y, alpha, H, kap, Xc, A, f, noise, tau = R.problem(cid)
    B = c["Buse"]
    ctx = _context(lib, cid)
    try:
        before = ctx.predict(_hk(H[:B]), Xc)
        gain, avg = ctx.joint_entropy(_hk(H[:B]), noise[:B], Xc, A[:B], f[:B], tau, NS)
        after = ctx.predict(_hk(H[:B]), Xc)
    finally:
        ctx.close()
    same = np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    return gain, avg, after[1], same


def _host_average(gain):
    s = np.zeros(gain.shape[1])
    for b in range(gain.shape[0]):
        s = s + gain[b] / float(NS)
    return s


@pytest.mark.parametrize("cid", CIDS)
def test_against_the_long_double_reference(lib, cid):
    c = R.ALL[cid]
    kap, noise = R.problem(cid)[4], R.problem(cid)[8]
    gain, avg, var, same = _cached(lib, cid)
    B, m = c["Buse"], c["m"]
    assert gain.shape == (B, m) and avg.shape == (m,)
    assert same  # a following bgp_predict_batch returns its earlier bits
    assert np.all(np.isfinite(gain)) and (gain >= 0.0).all() and (avg >= 0.0).all()
    ref_avg, tol_avg = np.zeros(m), np.zeros(m)
    for b in range(B):
        ref = R.reference(cid, b)
        r = R.ratio(gain[b], ref)
        fin = ref["tol"][np.isfinite(ref["tol"])]
        print("PRECISION jes %s b%d kappa %.3g: device vs long double %.4f tol (largest gain %.3g, smallest finite tol %.3g, rule entries %d)"
              % (cid, b, kap[b], r, float(ref["gain"].max()), float(fin.min()) if fin.size else float("nan"), int(ref["rule"].sum())))
        assert r <= 1.0
        # the invariants on the device's own variance (a few ulp for the two logs and the division by R)
        cap = 0.5 * np.log1p(var[b] / noise[b])
        assert np.all(gain[b] <= cap * (1.0 + 8 * P.EPS) + 8 * P.EPS)
        assert set(np.flatnonzero(ref["rule"]).tolist()) <= R.designated(cid)
        ref_avg += P.f(ref["gain"]) / NS
        tol_avg += ref["tol"] / NS
    err = np.abs(avg - ref_avg)
    with np.errstate(invalid="ignore"):
        assert np.all((err <= tol_avg) | (err == 0.0))
    assert np.array_equal(avg, _host_average(gain))


def test_the_special_points(lib):
    cid = "jes_special_n129_d3"
    gain, _avg, var, _same = _cached(lib, cid)
    ref = R.reference(cid, 0)
    X, y, alpha, H, kap, Xc, A, f, noise, tau = R.problem(cid)
    assert not ref["rule"].any()  # tau > 0 keeps every candidate regular: all of them are held to the reference above
    # far outside the data every cross-covariance vanishes: nothing is conditioned, and the value is the truncation's alone --
    # the mean over r of 1/2 [log(v + nu) - log(v F((f_r - mu) / sqrt v) + nu)] from the candidate's own two moments
    assert np.abs(P.f(ref["cov"][R.FAR])).max() <= 1e-100
    mu, v = float(ref["mu"][R.FAR]), float(ref["v"][R.FAR])
    alone = np.mean(0.5 * (np.log(v + noise[0]) - np.log(v * R.F64((f[0] - mu) / np.sqrt(v)) + noise[0])))
    assert abs(gain[0, R.FAR] - alone) <= ref["tol"][R.FAR]
    # the training point and its twin 1e-8 away: each within tolerance of its own reference (asserted above), and close to each other
    assert abs(gain[0, R.TRAIN] - gain[0, R.TWIN]) <= ref["tol"][R.TRAIN] + ref["tol"][R.TWIN] + 1e-6 * gain[0, R.TRAIN]
    # the candidate that IS an optimum point: that sample pins f(x) to f_0 up to tau, its term is nearly the whole cap
    g_same = float(ref["g"][R.SAME_OPT, 0])
    assert g_same >= 0.9 * float(ref["cap"][R.SAME_OPT]) and gain[0, R.SAME_OPT] >= g_same / A.shape[1] - ref["tol"][R.SAME_OPT]
    # the coinciding optimum points are two samples (each has its own f_r): nothing is merged -- dropping one changes the value
    keep = [0, 1, 3, 4, 5]
    one = _run(lib, cid, [(H[:1], noise[:1], Xc, A[:1, keep], f[:1, keep])])[0][0]
    assert one.shape == gain.shape and not np.array_equal(one, gain)
    # the sample with z ~ 1e3: the continued fraction's branch, finite and inside the invariants (asserted above for every candidate)
    assert (P.f(ref["z"])[:, R.BIG_Z] > 300.0).any()


def test_a_near_noise_free_posterior_with_an_optimum_point_on_a_training_point(lib):
    cid = "jes_noisefree_n5_d2"
    gain, _avg, var, _same = _cached(lib, cid)
    c, H, kap, noise = R.ALL[cid], R.problem(cid)[3], R.problem(cid)[4], R.problem(cid)[8]
    ref = R.reference(cid, 0)
    # every candidate is a rule entry here (w_0 = v_0 at a training point, tau = 0: the sign of a rounded 0) and no other case has one
    assert ref["rule"].all() and sum(int(R.reference(k, b)["rule"].sum()) for k in CIDS for b in range(R.ALL[k]["Buse"])) == c["m"]
    print("PRECISION jes %s: device gain %s, reference %s, cap %s" % (cid, gain[0], P.f(ref["gain"]), 0.5 * np.log1p(var[0] / noise[0])))
    assert np.all(np.isfinite(gain)) and (gain >= 0.0).all() and (gain > 0.0).any()
    assert np.all(gain[0] <= 0.5 * np.log1p(var[0] / noise[0]) * (1.0 + 8 * P.EPS) + 8 * P.EPS)


BITS_CIDS = ["jes1_n63_d8_R2_m255_matern12_product", "jes2_n64_d17_R62_m9_matern32_product", "jes6_n65_d3_R255_m4_matern32_sum",
             "jes7_n63_d2_R5_m257_matern52_sum"]


def _raw(lib, ctx, H, noise, Xc, A, f, tau, want_gain, want_avg, R_=None, ns=NS, m_=None, B_=None):
    """The C call itself with either output NULL (``R_``, ``m_``, ``B_``: a count other than the arrays', for the limits that are
    refused before anything is read)."""
    from bayes_skopt_amd._lib import _c, _p

    H, noise, Xc, A, f = _c(_hk(H)), _c(noise), _c(Xc), _c(np.asarray(A, dtype=np.float64)), _c(np.asarray(f, dtype=np.float64))
    B, m = len(H), len(Xc)
    Rr = f.shape[1] if R_ is None else R_
    gain, avg = np.full((B, m), np.nan), np.full(m, np.nan)
    null = ctypes.cast(None, ctypes.POINTER(ctypes.c_double))
    rc = ctx._lib.bgp_joint_entropy(ctx._h, B if B_ is None else B_, _p(H), _p(noise), m if m_ is None else m_, _p(Xc), Rr, _p(A), _p(f), float(tau), ns,
                                    _p(gain) if want_gain else null, _p(avg) if want_avg else null)
    return rc, gain, avg


@pytest.mark.parametrize("cid", BITS_CIDS)
def test_bits_do_not_depend_on_the_company_the_outputs_asked_for_or_the_call(lib, cid):
    c = R.ALL[cid]
    X, y, alpha, H, kap, Xc, A, f, noise, tau = R.problem(cid)
    m = c["m"]
    gain, avg, _, _ = _cached(lib, cid)
    pick = sorted({0, m // 2, m - 1})
    out = _run(lib, cid, [(H[:1], noise[:1], Xc, A[:1], f[:1])] + [(H[:1], noise[:1], Xc[s : s + 1], A[:1], f[:1]) for s in pick])
    assert np.array_equal(out[0][0], gain) and np.array_equal(out[0][1], avg)  # two calls
    for s, (g1, a1) in zip(pick, out[1:]):  # a candidate alone: m = 1
        assert np.array_equal(g1[0, 0], gain[0, s]) and np.array_equal(a1[0], avg[s])
    ctx = _context(lib, cid)
    try:
        rc, g, a = _raw(lib, ctx, H[:1], noise[:1], Xc, A[:1], f[:1], tau, True, False)
        assert rc == 0 and np.array_equal(g, gain) and np.isnan(a).all()
        rc, g, a = _raw(lib, ctx, H[:1], noise[:1], Xc, A[:1], f[:1], tau, False, True)
        assert rc == 0 and np.array_equal(a, avg) and np.isnan(g).all()
        rc, g, a = _raw(lib, ctx, H[:1], noise[:1], Xc, A[:1], f[:1], tau, True, True)
        assert rc == 0 and np.array_equal(g, gain) and np.array_equal(a, avg)
        assert _raw(lib, ctx, H[:1], noise[:1], Xc, A[:1], f[:1], tau, False, False)[0] == 1  # no output asked for: BGP_ERR_INVALID
    finally:
        ctx.close()


@pytest.mark.parametrize("cid", ["jes8_n64_d2_R3_m300_matern52_product", "jes7_n63_d2_R5_m257_matern52_sum",
                                 "jes1_n63_d8_R2_m255_matern12_product", "jes9_n63_d3_R1_m256_rbf_product"])
def test_a_forced_small_candidate_chunk_gives_the_bits_of_the_default(lib, cid, monkeypatch):
    """BGP_JES_CHUNK=128 (read at every call): m = 300 runs as 128 + 128 + 44 candidates, m = 257 as 128 + 128 + 1, m = 256 and 255 as
    two chunks; by default each is one chunk."""
    X, y, alpha, H, kap, Xc, A, f, noise, tau = R.problem(cid)
    gain, avg, _, _ = _cached(lib, cid)
    monkeypatch.setenv("BGP_JES_CHUNK", str(R.CHUNK))
    got = _run(lib, cid, [(H[:1], noise[:1], Xc, A[:1], f[:1])])[0]
    monkeypatch.delenv("BGP_JES_CHUNK")
    assert np.array_equal(got[0], gain) and np.array_equal(got[1], avg)


def test_a_row_alone_and_inside_a_batch_each_with_its_own_optimum_set(lib):
    cid = "jes_B3_n65_d3"
    X, y, alpha, H, kap, Xc, A, f, noise, tau = R.problem(cid)
    gain, avg, _, _ = _cached(lib, cid)  # 2 of 3 resident posteriors
    one, three = _run(lib, cid, [(H[:1], noise[:1], Xc, A[:1], f[:1]), (H, noise, Xc, A, f)])
    assert np.array_equal(one[0][0], gain[0]) and np.array_equal(one[1], gain[0] / float(NS))
    assert three[0].shape[0] == 3 and np.array_equal(three[0][:2], gain) and np.array_equal(three[1], _host_average(three[0]))
    alone = _run(lib, cid, [(H[1:2], noise[1:2], Xc, A[1:2], f[1:2])], rows=slice(1, 2))[0]  # posterior 1 built and used alone
    assert np.array_equal(alone[0][0], gain[1])
    # posterior 1 with posterior 0's optimum set is another value: the sets are not shared
    swapped = _run(lib, cid, [(H[:2], noise[:2], Xc, A[[0, 0]], f[[0, 0]])])[0]
    assert np.array_equal(swapped[0][0], gain[0]) and not np.array_equal(swapped[0][1], gain[1])


def test_limits_are_error_codes_and_leave_the_posteriors_usable(lib):
    cid = "jes3_n65_d32_R63_m5_matern52_product"
    c = R.ALL[cid]
    X, y, alpha, H, _kap, Xc, A, f, noise, tau = R.problem(cid)
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=2)
    rng = np.random.RandomState(0)
    X33 = rng.uniform(size=(20, 33))
    big = lib.Context(X33, rng.randn(20), 1e-6, max_batch=1)
    H1, n1, A1, f1 = H[:1], noise[:1], A[:1], f[:1]
    call = lambda *a, tau=tau, ns=NS: ctx.joint_entropy(*a, tau, ns)  # noqa: E731
    try:
        with pytest.raises(lib.BgpError, match=r"code 4"):  # nothing built
            call(_hk(H1), n1, Xc, A1, f1)
        assert np.all(ctx.posterior(H1, want_alpha=False)["status"] == 0)
        before = ctx.predict(H1, Xc)
        with pytest.raises(lib.BgpError, match=r"code 4"):  # more rows than resident posteriors
            call(_hk(np.repeat(H1, 2, axis=0)), np.repeat(n1, 2), Xc, np.repeat(A1, 2, axis=0), np.repeat(f1, 2, axis=0))
        with pytest.raises(lib.BgpError, match=r"code 1.*exceed"):  # R = 256
            call(_hk(H1), n1, Xc, rng.uniform(size=(1, 256, c["d"])), np.zeros((1, 256)))
        assert _raw(lib, ctx, H1, n1, Xc, A1, f1, tau, True, True, R_=0)[0] == 1  # R = 0
        for kw in (dict(m_=0), dict(m_=(1 << 24) + 1), dict(B_=0), dict(B_=65536)):  # m and B outside their ranges
            assert _raw(lib, ctx, H1, n1, Xc, A1, f1, tau, True, True, **kw)[0] == 1, kw
        assert _raw(lib, ctx, H1, n1, Xc, A1, f1, tau, True, True)[0] == 0
        with pytest.raises(lib.BgpError, match=r"code 1"):  # n_samples = 0
            call(_hk(H1), n1, Xc, A1, f1, ns=0)
        for bad in (0.0, -1e-3, np.inf, np.nan):  # the observation noise: > 0 and finite
            with pytest.raises(lib.BgpError, match=r"code 1.*noise"):
                call(_hk(H1), np.array([bad]), Xc, A1, f1)
        for bad in (-1e-9, np.inf, np.nan):  # tau: >= 0 and finite
            with pytest.raises(lib.BgpError, match=r"code 1.*tau"):
                call(_hk(H1), n1, Xc, A1, f1, tau=bad)
        for bad in (np.inf, np.nan):  # every optimum value finite
            fb = f1.copy()
            fb[0, -1] = bad
            with pytest.raises(lib.BgpError, match=r"code 1.*fopt"):
                call(_hk(H1), n1, Xc, A1, fb)
        with pytest.raises(ValueError):
            call(_hk(H1), n1, Xc[:, :3], A1[:, :, :3], f1)
        with pytest.raises(ValueError):
            call(_hk(H1), n1, Xc, A1[:, :5], f1)
        after = ctx.predict(H1, Xc)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        good = call(_hk(H1), n1, Xc, A1, f1)
        assert np.array_equal(good[0], _cached(lib, cid)[0]) and np.array_equal(good[1], _cached(lib, cid)[1])
        assert np.array_equal(call(_hk(H1), n1, Xc, A1, f1, tau=0.0)[0].shape, good[0].shape)  # tau = 0 is inside the limits
        after = ctx.predict(H1, Xc)  # a successful call leaves them untouched too
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        # the posteriors rebuilt as per-row-warped ones: only predict_warped reads those
        assert np.all(ctx.posterior(H1, want_alpha=False, warps=np.zeros((1, 2 * c["d"])))["status"] == 0)
        with pytest.raises(lib.BgpError, match=r"code 4.*per-row warped"):
            call(_hk(H1), n1, Xc, A1, f1)
        assert np.all(ctx.posterior(H1, want_alpha=False)["status"] == 0)
        after = ctx.predict(H1, Xc)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        # a context-level warp: refused as by the gradient entry points
        ctx.set_warp(np.zeros(2 * c["d"]))
        assert np.all(ctx.posterior(H1, want_alpha=False)["status"] == 0)
        with pytest.raises(lib.BgpError, match=r"code 1.*warped inputs"):
            call(_hk(H1), n1, np.clip(Xc, 0.0, 1.0), np.clip(A1, 0.0, 1.0), f1)
        assert np.all(np.isfinite(ctx.predict(H1, np.clip(Xc, 0.0, 1.0))[0]))
        h33 = np.concatenate([[0.0], np.zeros(33), [-4.0]])[None, :]
        assert np.all(big.posterior(h33, want_alpha=False)["status"] == 0)
        with pytest.raises(lib.BgpError, match=r"code 1.*d > 32"):
            big.joint_entropy(_hk(h33), [1e-3], X33[:2], X33[None, 2:4], np.zeros((1, 2)), 1e-6, 1)
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


def _optima(gp, Xc, B, Rr=6, seed=5):
    """Explicit optimum samples: points of the unit box and values a little below the posterior mean there (y units), per row."""
    rng = np.random.RandomState(seed)
    A = rng.uniform(size=(B, Rr, Xc.shape[1]))
    f = np.stack([gp.predict(A[b]) for b in range(B)]) - rng.uniform(0.0, 0.5, size=(B, Rr))
    return A, f


def _python_tolerance(gp, thetas, Xc, A, f_norm, tau):
    """The derived tolerance (tests/_jesref.py) in nats for the rows ``thetas`` of a fitted canonical model, averaged over the rows,
    from fp64 quantities: the joint moments from the device's predictive covariance, kappa of the row's Gram matrix, the mean's
    scales and the prior variance."""
    from oracle import gp_oracle as O

    st, fm = gp._plan.stationary, gp._plan.form
    Xt, d, n = gp._X_train_, gp._X_train_.shape[1], gp._X_train_.shape[0]
    H = gp._canonical(np.atleast_2d(thetas))
    ad = np.broadcast_to(gp._alpha_diag(), (n,))
    Rr = A.shape[1]
    total = np.zeros(len(Xc))
    assert np.all(gp._ctx.posterior(H, want_alpha=True)["status"] == 0)
    for b in range(len(H)):
        Q = np.vstack([A[b], Xc])
        mean, var, cov = (a[b] for a in gp._ctx.predict(_hk(H), Q, return_cov=True))
        a = np.linalg.solve(O.gram_with_jitter(Xt, ad, H[b], st, fm), gp.y_train_)
        sc = np.abs(O.kernel_matrix(Q, _hk(H)[b], st, fm, Y=Xt) * a[None, :]).sum(axis=1)
        pv = float(O.kernel_diag(1, _hk(H)[b], d, fm)[0])
        kap = P.kappa_of(Xt, ad, H[b], st, fm)
        nu = gp._fantasy_base_alpha() + np.exp(H[b, -1])
        total += R.tolerance64(mean[Rr:], var[Rr:], mean[:Rr], var[:Rr], cov[:Rr, Rr:].T, f_norm[b], nu, tau, sc[Rr:], sc[:Rr], pv,
                               P.tol("mean", kap, n), P.tol("var", kap, n)) / len(H)
    return total


@pytest.mark.parametrize("n_gp_samples", [0, 4])
def test_device_path_equals_host_path(bask, fitted_gp, n_gp_samples, monkeypatch):
    gp, Xc = fitted_gp
    B = max(n_gp_samples, 1)
    A, f = _optima(gp, Xc, B)
    JES = bask.acquisition.JointEntropySearch()
    dev, path = JES(Xc, gp, optimum_samples=(A, f), n_gp_samples=n_gp_samples, random_state=3, return_path=True)
    monkeypatch.setattr(bask.acquisition.JointEntropySearch, "path", "host")
    host, hpath = JES(Xc, gp, optimum_samples=(A, f), n_gp_samples=n_gp_samples, random_state=3, return_path=True)
    monkeypatch.undo()
    assert (path, hpath) == ("device", "host") and dev.shape == host.shape == (len(Xc),)
    assert (dev >= 0.0).all() and np.all(np.isfinite(dev)) and dev.max() > 0.0
    rows = gp._post_theta[None, :] if n_gp_samples == 0 else gp.chain_[
        np.random.RandomState(3).choice(len(gp.chain_), replace=False, size=n_gp_samples)]
    f_norm = (f - float(np.ravel(gp.y_train_mean_)[0])) / float(np.ravel(gp.y_train_std_)[0])
    tol = _python_tolerance(gp, rows, Xc, A, f_norm, 1e-6)
    r = float((np.abs(dev - host) / tol).max())
    print("PRECISION jes python n_gp_samples=%d: device vs host path %.4f tol (largest value %.3g, smallest tol %.3g)"
          % (n_gp_samples, r, dev.max(), tol.min()))
    assert r <= 0.1
    # one optimum set (R, d) / (R,) is shared by the rows
    shared = JES(Xc, gp, optimum_samples=(A[0], f[0]), n_gp_samples=n_gp_samples, random_state=3)
    assert shared.shape == dev.shape and (np.array_equal(shared, dev) if B == 1 else not np.array_equal(shared, dev))
    with pytest.raises(ValueError):
        JES(Xc, gp, optimum_samples=(A[:, :, :1], f), n_gp_samples=n_gp_samples, random_state=3)
    assert np.all(np.isfinite(gp.predict(Xc)))  # the estimator's own posterior is back where a consumer needs it


def test_seeded_draws_give_the_same_bits(bask, fitted_gp):
    gp, Xc = fitted_gp
    JES = bask.acquisition.JointEntropySearch()
    kw = dict(n_optima=5, n_features=128, n_candidates=200, n_starts=2)
    for n_gp_samples in (0, 2):
        a, pa = JES(Xc, gp, n_gp_samples=n_gp_samples, random_state=7, return_path=True, **kw)
        b = JES(Xc, gp, n_gp_samples=n_gp_samples, random_state=7, **kw)
        c = JES(Xc, gp, n_gp_samples=n_gp_samples, random_state=8, **kw)
        assert pa == "device" and np.array_equal(a, b) and not np.array_equal(a, c)
        assert a.shape == (len(Xc),) and np.all(np.isfinite(a)) and (a >= 0.0).all() and a.max() > 0.0
    # sample_paths itself keeps its generator consumption: the helper beside it draws no row indices
    rng1, rng2 = np.random.RandomState(11), np.random.RandomState(11)
    with gp.sample_paths(n_paths=3, sample_mean=True, n_features=64, random_state=rng1) as p1:
        with gp._sample_paths_rows(gp._post_theta[None, :], 3, 64, rng2) as p2:
            assert np.array_equal(p1(Xc[:5]), p2(Xc[:5]))
    assert rng1.uniform() == rng2.uniform()


def test_generic_trees_and_warped_inputs_take_the_host_path_and_say_so_once(bask, capfd, monkeypatch):
    import sklearn.gaussian_process.kernels as sk

    Xt, y, Xc = _toy(n=20)
    Xc = Xc[:24]
    monkeypatch.setattr(bask.acquisition, "_jes_told", [])
    capfd.readouterr()
    JES = bask.acquisition.JointEntropySearch()
    gen = bask.BayesGPR(kernel=sk.Matern(length_scale=0.4, nu=2.5) * sk.RBF(length_scale=0.7) + sk.WhiteKernel(0.05),
                        normalize_y=True, random_state=4)
    gen.fit(Xt, y, **FIT)
    assert not gen._post.canonical
    A1, f1 = _optima(gen, Xc, 1)
    A2, f2 = _optima(gen, Xc, 2)
    v1, p1 = JES(Xc, gen, optimum_samples=(A1, f1), return_path=True)
    v2, p2 = JES(Xc, gen, optimum_samples=(A2, f2), n_gp_samples=2, random_state=0, return_path=True)
    gw = bask.BayesGPR(kernel=bask.construct_default_kernel([0, 1]), random_state=1, warp_inputs=True, normalize_y=True)
    gw.fit(Xt, y, **FIT)
    A3, f3 = _optima(gw, Xc, 1)
    A4, f4 = _optima(gw, Xc, 2)
    v3, p3 = JES(Xc, gw, optimum_samples=(A3, f3), return_path=True)
    v4, p4 = JES(Xc, gw, optimum_samples=(A4, f4), n_gp_samples=2, random_state=0, return_path=True)
    assert p1 == p2 == p3 == p4 == "host"
    for v in (v1, v2, v3, v4):
        assert v.shape == (len(Xc),) and np.all(np.isfinite(v)) and (v >= 0.0).all() and v.max() > 0.0
    err = capfd.readouterr().err
    assert err.count("joint_entropy: on the host") == 1
    # without explicit samples the draws cannot run there: sample_paths' own reason
    with pytest.raises(ValueError, match="sample_paths does not support a generic kernel tree"):
        JES(Xc, gen)
    with pytest.raises(ValueError, match="sample_paths does not support warped inputs"):
        JES(Xc, gw, n_gp_samples=2, random_state=0)
    assert np.all(np.isfinite(gw.predict(Xc))) and np.all(np.isfinite(gen.predict(Xc)))


def test_optimizer_with_joint_entropy_search(bask):
    f = lambda x: (x[0] - 0.3) ** 2 + (x[1] + 0.2) ** 2  # noqa: E731

    def run():
        opt = bask.Optimizer(dimensions=[(-1.0, 1.0)] * 2, n_points=200, n_initial_points=5, init_strategy="r2", acq_func="jes",
                             acq_func_kwargs=dict(n_optima=8, n_features=128, n_candidates=200, n_starts=2), random_state=0)
        assert isinstance(opt.acq_func, bask.acquisition.JointEntropySearch)
        rng = np.random.RandomState(0)
        X0 = rng.uniform(-1.0, 1.0, size=(5, 2)).tolist()
        opt.tell(X0, [f(x) + 0.05 * rng.randn() for x in X0], gp_samples=40, gp_burnin=2)
        asked = []
        for _ in range(3):
            x = opt.ask()
            assert all(-1.0 <= v <= 1.0 for v in x) and np.all(np.isfinite(x))
            asked.append(list(map(float, x)))
            opt.tell(x, f(x) + 0.05 * rng.randn(), gp_samples=40, gp_burnin=2)
        return opt, asked

    opt, asked = run()
    assert len(opt.Xi) == 8
    assert run()[1] == asked  # reproducible under a seed
    vals = opt._last_acq_values
    assert np.all(np.isfinite(vals)) and vals.max() > 0.0
    pts = opt.ask(n_points=2)
    assert opt._last_batch_info["path"] == "fallback"
    assert len(pts) == 2 and len({tuple(map(float, p)) for p in pts}) == 2
    assert all(-1.0 <= v <= 1.0 for p in pts for v in p)
