"""Cross-validation from the resident inverses on the device (``bgp_cross_validate``, bgp_cv.hip), through
``_lib.Context`` on the cases of tests/_cvref.py -- folds of 1, 2, 63, 64, 65, 127 and 128 points, mixed sizes in one call, shuffled
and contiguous index sets across the row blocks of the padded inverse, partitions and lists that leave points uncovered, every
kernel family, fewer rows than resident posteriors -- and through the Python layer (``BayesGPR``, ``utils``, ``Optimizer``).

* mean, variance and fold log density of every (row, fold, point) against the long-double REFIT on the remaining points at the
  tolerance tests/test_cpu_cv_reference.py qualifies; ``status`` zero everywhere -- asserted, never masked;
* one-point folds through the leave-one-out kernel and through the fold kernel; bitwise: fold order, a row alone and in a batch, a
  build in more than one chunk; the entry point's contract (error codes, NaN at uncovered points, the end of residency);
* per-row-warped residents, a generic kernel tree, and the estimator's result against actually refitting on the remaining points.

Lines printed with ``pytest -s`` start with ``PRECISION``."""
import functools

import numpy as np
import pytest

import _cvref as R
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


def _context(lib, cid, max_batch=None, build=True):
    c = R.ALL[cid]
    X, y, alpha, H, _ = R.problem(cid)
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=max_batch or len(H))
    if build:
        assert np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)
    return ctx


@functools.lru_cache(maxsize=None)
def _cached(lib, cid):
    """The case's own call: its first Buse resident rows, its fold list."""
    c = R.ALL[cid]
    ctx = _context(lib, cid)
    try:
        return ctx.cross_validate(c["Buse"], c["folds"])
    finally:
        ctx.close()


def _ratios(got_folds, ref, kappa, n, sens=None):
    """Per quantity the worst err / tol over the folds of one row."""
    out = {q: 0.0 for q in R.QUANTITIES}
    for k, (g, r) in enumerate(zip(got_folds, ref)):
        e = R.errs(g, r)
        for q in R.QUANTITIES:
            out[q] = max(out[q], e[q] / R.tol(q, kappa, n, sens=0.0 if sens is None else sens[k][q], amp=r["amp"]))
    return out


def _same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _code(excinfo):
    text = str(excinfo.value)
    return int(text.split("(code ")[1].split(")")[0]), text


ERR_INVALID, ERR_STATE = 1, 4  # include/bgp.h


@pytest.mark.parametrize("cid", CIDS)
def test_against_the_long_double_refit(lib, cid):
    c = R.ALL[cid]
    n, folds = c["n"], c["folds"]
    kap = R.problem(cid)[4]
    mean, var, lpd, status = _cached(lib, cid)
    assert mean.shape == var.shape == (c["Buse"], n) and lpd.shape == status.shape == (c["Buse"], len(folds))
    assert not status.any(), status
    cov = R.covered(folds, n)
    assert np.all(np.isnan(mean[:, ~cov])) and np.all(np.isnan(var[:, ~cov]))
    assert np.all(np.isfinite(mean[:, cov])) and np.all(var[:, cov] > 0.0) and np.all(np.isfinite(lpd))
    worst = {q: 0.0 for q in R.QUANTITIES}
    for b in range(c["Buse"]):
        r = _ratios(R.device_folds(mean, var, lpd, b, folds), R.reference(cid, b), kap[b], n)
        worst = {q: max(worst[q], r[q]) for q in R.QUANTITIES}
    print("PRECISION cv %s kappa %.3g: device vs long-double refit %s tol (mean / var / lpd)"
          % (cid, kap[: c["Buse"]].max(), " / ".join("%.4f" % worst[q] for q in R.QUANTITIES)))
    assert max(worst.values()) <= 1.0, worst


def test_one_point_folds_through_both_kernels(lib):
    """The leave-one-out case as it is (every fold one point: the per-point kernel) and with one two-point fold added to the call,
    which sends every fold through the workgroup kernel: both meet the tolerance on the one-point folds."""
    cid = R.LOO_CASE
    c = R.ALL[cid]
    n, folds = c["n"], c["folds"]
    kap = R.problem(cid)[4]
    loo = _cached(lib, cid)
    ctx = _context(lib, cid)
    try:
        mixed = ctx.cross_validate(c["Buse"], folds + [R.LOO_PAIR])
    finally:
        ctx.close()
    assert not loo[3].any() and not mixed[3].any()
    for name, (mean, var, lpd, _st) in (("loo kernel", loo), ("fold kernel", mixed)):
        worst = {q: 0.0 for q in R.QUANTITIES}
        for b in range(c["Buse"]):
            r = _ratios(R.device_folds(mean, var, lpd[:, : len(folds)], b, folds), R.reference(cid, b), kap[b], n)
            worst = {q: max(worst[q], r[q]) for q in R.QUANTITIES}
        print("PRECISION cv %s one-point folds, %s: %s tol" % (cid, name, " / ".join("%.4f" % worst[q] for q in R.QUANTITIES)))
        assert max(worst.values()) <= 1.0, (name, worst)
    assert np.all(np.isfinite(mixed[0][:, R.LOO_PAIR])) and np.all(np.isnan(loo[0][:, R.LOO_PAIR]))


def test_bits_do_not_depend_on_fold_order_batch_or_chunking(lib):
    cid = CIDS[2]  # n = 65, three rows, folds of 63 and 1
    c = R.ALL[cid]
    H = R.problem(cid)[3]
    folds = c["folds"] + [np.array([int(np.setdiff1d(np.arange(c["n"]), np.concatenate(c["folds"]))[0])])]
    ctx = _context(lib, cid)
    try:
        fwd = ctx.cross_validate(3, folds)
        rev = ctx.cross_validate(3, folds[::-1])
        two = ctx.cross_validate(2, folds)
        assert np.all(ctx.posterior(H[1:2], want_alpha=False)["status"] == 0)
        alone = ctx.cross_validate(1, folds)
    finally:
        ctx.close()
    assert _same(fwd[0], rev[0]) and _same(fwd[1], rev[1]) and _same(fwd[2], rev[2][:, ::-1])
    assert not fwd[3].any() and not rev[3].any()
    for i in range(3):  # row 1 read in a two-row call against a build of that row alone; the rows of a shorter call
        assert _same(two[i][1], alone[i][0]) and _same(two[i], fwd[i][:2])
    small = _context(lib, cid, max_batch=2)  # the three-row build takes two chunks here
    try:
        chunked = small.cross_validate(3, folds)
    finally:
        small.close()
    for i in range(3):
        assert _same(chunked[i], fwd[i])
    assert not chunked[3].any()


def test_contract(lib):
    cid = CIDS[4]  # n = 129
    c = R.ALL[cid]
    n, folds = c["n"], c["folds"]
    X, y, alpha, H, _ = R.problem(cid)
    ctx = _context(lib, cid, build=False)
    try:
        with pytest.raises(lib.BgpError) as e:
            ctx.cross_validate(1, folds)
        code, text = _code(e)
        assert code == ERR_STATE and "bgp_cross_validate" in text and "resident" in text
        assert np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)
        good = ctx.cross_validate(1, folds)
        assert not good[3].any()
        with pytest.raises(lib.BgpError) as e:  # more rows than are resident
            ctx.cross_validate(2, folds)
        assert _code(e)[0] == ERR_STATE and "resident" in _code(e)[1]
        assert ctx.lml_submit(H)
        with pytest.raises(lib.BgpError) as e:
            ctx.cross_validate(1, folds)
        assert _code(e)[0] == ERR_STATE and "pending" in _code(e)[1]
        ctx.lml_wait()
        assert np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)  # (an LML batch overwrites the workspace, not the residents)
        bad = [([np.arange(129)], 1, "128"), ([np.array([3, 7]), np.array([7])], 1, "two folds"), ([np.array([5, 5])], 1, "two folds"),
               ([np.array([0, n])], 1, "out of range"), ([np.array([-1])], 1, "out of range"),
               ([np.array([1]), np.array([], dtype=np.int64)], 1, "empty"), (folds, 0, "B")]
        for fl, B, word in bad:
            with pytest.raises(lib.BgpError) as e:
                ctx.cross_validate(B, fl)
            code, text = _code(e)
            assert code == ERR_INVALID and "bgp_cross_validate" in text and word in text, (word, text)
            again = ctx.cross_validate(1, folds)  # the next valid call is right: the same bits as before
            assert all(_same(u, v) for u, v in zip(again[:3], good[:3])) and not again[3].any()
        ctx.update_data(X, y, alpha)  # new training data ends residency for this consumer too
        with pytest.raises(lib.BgpError) as e:
            ctx.cross_validate(1, folds)
        assert _code(e)[0] == ERR_STATE and "resident" in _code(e)[1]
    finally:
        ctx.close()


def test_invalid_arguments_go_before_the_residency_answer(lib):
    cid = CIDS[2]
    ctx = _context(lib, cid, build=False)
    try:
        with pytest.raises(lib.BgpError) as e:
            ctx.cross_validate(1, [np.array([1, 1])])
        assert _code(e)[0] == ERR_INVALID
    finally:
        ctx.close()


def test_per_row_warped_residents(lib):
    """WARP_CASES[1] built with ``bgp_posterior_batch_warped``: the reference on the long-double warped inputs, the tolerance at
    kappa of the warped Gram matrix plus the Beta-CDF budget."""
    c = P.ALL[R.WARP_CID]
    X, y, alpha, H, _ = P.problem(R.WARP_CID)
    W = P.warp_params(R.WARP_CID)
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=len(H))
    try:
        assert np.all(ctx.posterior(H, want_alpha=False, warps=W)["status"] == 0)
        mean, var, lpd, status = ctx.cross_validate(len(H), R.WARP_FOLDS)
    finally:
        ctx.close()
    assert not status.any()
    worst = {q: 0.0 for q in R.QUANTITIES}
    for b in range(len(H)):
        ref, kap, sens = R.warp_reference(b)
        r = _ratios(R.device_folds(mean, var, lpd, b, R.WARP_FOLDS), ref, kap, c["n"], sens)
        worst = {q: max(worst[q], r[q]) for q in R.QUANTITIES}
    print("PRECISION cv %s per-row warped: %s tol" % (R.WARP_CID, " / ".join("%.4f" % worst[q] for q in R.QUANTITIES)))
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------------------------------------
# the Python layer
# ------------------------------------------------------------------------------------------------------------------------------
def _refit(bask, gp, folds):
    """(mean, std) in y units of the held-out observations by ACTUALLY refitting: per fold an estimator with the same kernel at the
    same fixed theta (no optimiser, no sampling) on the remaining points -- in the full fit's normalised units, which is the model
    the folds share -- and its ``predict(X_F, return_std=True)``.  ``predict``'s std is that of the latent function here (the fit
    zeroes ``kernel_``'s white level), so the white level and the held-out points' own alpha are added in quadrature."""
    X, yn, a = gp._X_train_, np.asarray(gp.y_train_), np.asarray(gp._alpha_diag())
    y_mean, y_std = float(np.ravel(gp.y_train_mean_)[0]), float(np.ravel(gp.y_train_std_)[0])
    kernel = gp._kernel_at(gp._post_theta)
    mean, std = np.full(len(yn), np.nan), np.full(len(yn), np.nan)
    for F in folds:
        rest = np.setdiff1d(np.arange(len(yn)), F)
        clone = bask.BayesGPR(kernel=kernel, alpha=a[rest], optimizer=None, normalize_y=False, random_state=0)
        clone._map_fit(X[rest], yn[rest])
        m, s = clone.predict(X[F], return_std=True)
        mean[F] = m * y_std + y_mean
        std[F] = np.sqrt(s**2 + clone.noise_ + a[F]) * y_std
        clone._ctx.close()
    return mean, std


def _data(n, d, seed):
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(n, d))
    y = 3.0 + 2.0 * (np.sin(5.0 * X[:, 0]) + X[:, -1] ** 2) + 0.1 * rng.randn(n)
    return X, y, rng.uniform(0.005, 0.02, size=n)


@pytest.fixture(scope="module")
def fitted(bask):
    X, y, nv = _data(60, 2, 11)
    gp = bask.BayesGPR(kernel=bask.construct_default_kernel([0, 1]), normalize_y=True, random_state=3)
    gp.fit(X, y, noise_vector=nv, n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
    return gp, X, y


def test_estimator_against_refitting(bask, fitted):
    gp, X, y = fitted
    out = gp.cross_validate(n_folds=5, random_state=7)
    folds = out["folds"]
    assert len(folds) == 5 and sorted(np.concatenate(folds)) == list(range(60))
    mean, std = _refit(bask, gp, folds)
    np.testing.assert_allclose(out["mean"], mean, rtol=1e-6)
    np.testing.assert_allclose(out["std"], std, rtol=1e-6)
    np.testing.assert_allclose(out["z"], (y - mean) / std, rtol=1e-5, atol=1e-6)
    assert out["row_mean"].shape == out["row_std"].shape == (1, 60) and out["row_fold_lpd"].shape == (1, 5)
    assert np.array_equal(out["fold_lpd"], out["row_fold_lpd"][0]) and out["elpd"] == out["fold_lpd"].sum()
    assert np.array_equal(out["ess"], np.ones(5))
    # one-point folds: the fold's log density is the point's
    loo = gp.cross_validate()
    assert len(loo["folds"]) == 60 and all(len(f) == 1 for f in loo["folds"])
    np.testing.assert_allclose(loo["point_lpd"][np.concatenate(loo["folds"])], loo["fold_lpd"], rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(loo["point_lpd"], -0.5 * (loo["z"] ** 2 + np.log(2 * np.pi * loo["std"] ** 2)), rtol=1e-10, atol=1e-12)
    # the median GP still predicts afterwards (its posterior is rebuilt on demand)
    assert np.all(np.isfinite(gp.predict(X[:3])))


def test_estimator_with_chain_rows(bask, fitted):
    gp, X, y = fitted
    rows = np.asarray(gp.chain_)[:8]
    folds = [np.array([5, 50, 7]), np.arange(20, 40), np.array([0])]
    out = {w: gp.cross_validate(folds=folds, thetas=rows, weights=w) for w in ("is", "equal")}
    for o in out.values():
        assert o["row_mean"].shape == o["row_std"].shape == (8, 60) and o["row_fold_lpd"].shape == (8, 3)
        assert o["mean"].shape == o["std"].shape == o["z"].shape == o["point_lpd"].shape == (60,)
        assert o["fold_lpd"].shape == o["ess"].shape == (3,) and o["elpd"] == o["fold_lpd"].sum()
        cov = R.covered(folds, 60)
        assert np.all(np.isnan(o["mean"][~cov])) and np.all(np.isfinite(o["mean"][cov])) and np.all(o["std"][cov] > 0)
        assert np.all(o["ess"] >= 1.0 - 1e-12) and np.all(o["ess"] <= 8.0 + 1e-12)
    assert np.all(out["is"]["fold_lpd"] <= out["equal"]["fold_lpd"] + 1e-12)
    assert _same(out["is"]["row_fold_lpd"], out["equal"]["row_fold_lpd"])
    # a row of the block is what the row gives alone
    one = gp.cross_validate(folds=folds, thetas=rows[3:4])
    assert _same(one["row_mean"][0], out["is"]["row_mean"][3]) and _same(one["row_fold_lpd"][0], out["is"]["row_fold_lpd"][3])
    with pytest.raises(ValueError):
        gp.cross_validate(folds=folds, n_folds=3)
    with pytest.raises(ValueError):
        gp.cross_validate(folds=[np.arange(60), np.array([0])])
    with pytest.raises(ValueError):
        gp.cross_validate(weights="uniform")


def test_generic_kernel_tree_against_refitting(bask):
    from sklearn.gaussian_process import kernels as sk

    X, y, _nv = _data(40, 2, 12)
    gp = bask.BayesGPR(kernel=sk.RBF(length_scale=0.3) + sk.RBF(length_scale=1.5) + sk.WhiteKernel(0.05), normalize_y=True,
                       random_state=4)
    gp.fit(X, y, n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
    assert not gp._post.canonical
    out = gp.cross_validate(n_folds=4, random_state=1)
    mean, std = _refit(bask, gp, out["folds"])
    np.testing.assert_allclose(out["mean"], mean, rtol=1e-6)
    np.testing.assert_allclose(out["std"], std, rtol=1e-6)
    hyp = gp.cross_validate(n_folds=4, thetas=np.asarray(gp.chain_)[:3], random_state=1)
    assert hyp["row_mean"].shape == (3, 40) and np.all(np.isfinite(hyp["mean"]))


def _optimizer(bask, warp):
    from bayes_skopt_amd.space import Real

    opt = bask.Optimizer(dimensions=[Real(-2.0, 2.0), Real(0.0, 1.0)], n_initial_points=8, random_state=0,
                         gp_kwargs=dict(warp_inputs=True) if warp else None)
    opt.run(lambda x: float(np.sin(2.0 * x[0]) + x[1] ** 2), n_iter=14, n_samples=1, gp_samples=40, gp_burnin=5)
    return opt


@pytest.mark.parametrize("warp", [False, True])
def test_optimizer_cross_validate(bask, warp):
    opt = _optimizer(bask, warp)
    gp = opt.gp
    assert gp.warp_inputs == warp
    before = opt.rng.get_state()
    a = opt.cross_validate(n_folds=4, n_samples=5, random_state=6)
    b = opt.cross_validate(n_folds=4, n_samples=5, random_state=6)
    after = opt.rng.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    n = len(opt.Xi)
    assert a["row_mean"].shape == (5, n) and a["row_fold_lpd"].shape == (5, 4) and a["ess"].shape == (4,)
    for key in ("mean", "std", "z", "point_lpd", "fold_lpd", "row_mean", "row_std", "row_fold_lpd", "ess"):
        assert _same(a[key], b[key]), key
    assert a["elpd"] == b["elpd"] and all(np.array_equal(u, v) for u, v in zip(a["folds"], b["folds"]))
    assert np.all(np.isfinite(a["mean"])) and np.all(a["std"] > 0)
    # the median GP, leave-one-out, against the textbook formula on the downloaded inverse (context-level warp included)
    loo = opt.cross_validate()
    y_mean, y_std = float(np.ravel(gp.y_train_mean_)[0]), float(np.ravel(gp.y_train_std_)[0])
    dK = np.diag(gp.K_inv_)
    np.testing.assert_allclose(loo["mean"], (np.asarray(gp.y_train_) - gp.alpha_ / dK) * y_std + y_mean, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(loo["std"], np.sqrt(1.0 / dK) * y_std, rtol=1e-6)
    assert bask.utils.cross_validate is not None and "cross_validate" in bask.utils.__all__
