"""Sobol' sensitivity of the surrogate mean on the device (``bgp_sobol_indices``, bgp_sobol.hip), driven
through ``_lib.Context`` on the cases of tests/_sobolref.py -- every kernel family, n on both sides of the 64-point training tile,
d = 1 and at the padded row widths 8 / 16 / 32 and past them, N at the 256-sample chunk - 1, exact, + 1 and over several chunks,
T = 1 and T = d, singletons + pairs, the empty and the full mask, repeated terms, fewer items than resident posteriors, r = 0 --
and through the Python layer (``BayesGPR.sensitivity``, ``utils.sensitivity_indices``, ``Optimizer.sensitivity_indices``).

* f0, V and every term's C, J against the long-double reference on the synthesised rows at ``tol("mean", kappa, n)`` and its
  first-order image through the estimator, the tolerance tests/test_cpu_sobol_reference.py qualifies; against ``ctx.predict`` on
  the synthesised rows through the numpy estimator within 2 tol;
* bitwise: the empty mask, the full mask, A == Bm; a term alone, repeated, reordered; one item alone and inside a batch; two
  identical calls;
* a context-level warp against ``hp_oracle.warp_inputs`` on the synthesised rows; the limits, which are error codes.

Lines printed with ``pytest -s`` start with ``PRECISION``."""
import ctypes as C
import functools

import numpy as np
import pytest

import _pdref as PD
import _precision as P
import _sobolref as R

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

ERR_INVALID, ERR_STATE = 1, 4  # include/bgp.h
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


def _noise_off(H):
    Hk = np.array(H, dtype=np.float64, copy=True)
    Hk[:, -1] = -np.inf
    return Hk


def _run(lib, cid, calls, predict=False):
    """One context and posterior build of the case; ``calls``: (rows of H, A, Bm, masks) per device call.  With ``predict``: also
    the means of ``ctx.predict`` on the (T + 2) N synthesised rows of the case, (Buse, T + 2, N)."""
    c = R.ALL[cid]
    X, y, alpha, H, _kap, A, Bm = R.problem(cid)
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=len(H))
    try:
        assert np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)
        out = [ctx.sobol_indices(_noise_off(H[rows]), a, b, masks) for rows, a, b, masks in calls]
        via = None
        if predict:
            Hk, rows = _noise_off(H[: c["Buse"]]), R.all_rows(A, Bm, R.masks_of(c["terms"]))
            via = np.concatenate([ctx.predict(Hk, rows[r0:r0 + 4096])[0] for r0 in range(0, len(rows), 4096)], axis=1)
            via = via.reshape(c["Buse"], len(c["terms"]) + 2, len(A))
    finally:
        ctx.close()
    return out, via


@functools.lru_cache(maxsize=None)
def _cached(lib, cid):
    """The case's own call (its first Buse posteriors, its term list) and the predict route, shared by the tests that read them."""
    c = R.ALL[cid]
    _X, _y, _alpha, _H, _kap, A, Bm = R.problem(cid)
    out, via = _run(lib, cid, [(slice(0, c["Buse"]), A, Bm, R.masks_of(c["terms"]))], predict=True)
    return out[0], via


def _item(got, b):
    return tuple(v[b] for v in got)


@pytest.mark.parametrize("cid", CIDS)
def test_against_the_long_double_reference(lib, cid):
    c = R.ALL[cid]
    kap = R.problem(cid)[4]
    got, _via = _cached(lib, cid)
    B, T = c["Buse"], len(c["terms"])
    assert [v.shape for v in got] == [(B,), (B,), (B, T), (B, T)]
    worst = {}
    for b in range(B):
        e = R.errs(_item(got, b), R.reference(cid, b), P.tol("mean", kap[b], c["n"]))
        worst = {k: max(worst.get(k, 0.0), v) for k, v in e.items()}
    print("PRECISION sobol %s kappa %.3g: device vs long double f0 %.4f V %.4f C %.4f J %.4f tol"
          % (cid, kap[:B].max(), worst["f0"], worst["V"], worst["C"], worst["J"]))
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("cid", CIDS)
def test_against_predict_on_the_synthesised_rows(lib, cid):
    c = R.ALL[cid]
    kap = R.problem(cid)[4]
    got, via = _cached(lib, cid)
    worst = 0.0
    for b in range(c["Buse"]):
        f0, V, Cv, J = R.estimator(via[b], chunk=R.RC)
        other = dict(R.reference(cid, b), f0=f0, V=V, C=Cv, J=J)  # (the reference's scales and images, predict's values)
        worst = max(worst, R.worst(_item(got, b), other, P.tol("mean", kap[b], c["n"])))
    print("PRECISION sobol %s: device vs predict on synthesised rows %.4f tol (2 allowed)" % (cid, worst))
    assert worst <= 2.0


def _same(a, b):
    a, b = np.atleast_1d(a), np.atleast_1d(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("cid", ["sb_mixed_B3", "sb_twin_matern12", "sb5_n129_d4_N600_T10_matern12_sum"])
def test_bitwise_invariants(lib, cid):
    c = R.ALL[cid]
    _X, _y, _alpha, _H, _kap, A, Bm = R.problem(cid)
    masks, B = R.masks_of(c["terms"]), c["Buse"]
    T, full = len(masks), (1 << c["d"]) - 1
    order = list(range(T))[::-1]
    every = slice(0, B)
    calls = [(every, A, Bm, masks), (every, A, Bm, masks), (every, A, Bm, [masks[i] for i in order])]
    calls += [(every, A, Bm, [m]) for m in masks]
    calls += [(slice(0, 1), A, Bm, masks), (every, A, Bm, [0, full]), (every, Bm, A, [full]), (every, A, A, masks + [0, full])]
    out, _ = _run(lib, cid, calls)
    ref = out[0]
    assert all(_same(a, b) for a, b in zip(ref, out[1]))                                   # two identical calls
    assert _same(ref[0], out[2][0]) and _same(ref[1], out[2][1])                           # a reordered list
    assert _same(ref[2][:, order], out[2][2]) and _same(ref[3][:, order], out[2][3])
    for i in range(T):                                                                     # a term alone
        alone = out[3 + i]
        assert _same(ref[0], alone[0]) and _same(ref[1], alone[1])
        assert _same(ref[2][:, i], alone[2][:, 0]) and _same(ref[3][:, i], alone[3][:, 0])
    for i in range(T):                                                                     # a repeated term: the same bits twice
        for j in range(i):
            if masks[j] == masks[i]:
                assert _same(ref[2][:, i], ref[2][:, j]) and _same(ref[3][:, i], ref[3][:, j])
    assert all(_same(a[:1], b) for a, b in zip(ref, out[3 + T]))                           # item 0 alone (B = 1 on row 0)
    ends, swapped, equal = out[4 + T], out[5 + T], out[6 + T]
    assert np.all(ends[2][:, 0] == 0.0) and np.all(ends[3][:, 0] == 0.0)                   # the empty mask IS fA: no effect at all
    # the full mask IS fB: with A and Bm exchanged its row is the old fA, so (fA - fB)^2 and the symmetric f0, V keep their bits
    assert _same(ends[3][:, 1], swapped[3][:, 0]) and _same(ends[0], swapped[0]) and _same(ends[1], swapped[1])
    assert np.all(ends[3][:, 1] > 0.0)
    assert np.all(equal[2] == 0.0) and np.all(equal[3] == 0.0) and np.all(equal[1] > 0.0)  # A == Bm: exact zeros


def test_b1_on_row0_equals_item0_of_b3(lib):
    cid = "sb_twin_matern12"
    c = R.ALL[cid]
    assert c["B"] == c["Buse"] == 3
    _X, _y, _alpha, _H, _kap, A, Bm = R.problem(cid)
    masks = R.masks_of(c["terms"])
    out, _ = _run(lib, cid, [(slice(0, 3), A, Bm, masks), (slice(0, 1), A, Bm, masks)])
    assert all(_same(a[:1], b) for a, b in zip(*out))


def test_context_level_warp(lib):
    """Both matrices go through the context-level warp as predict's queries do: WARP_CASES[0]'s problem and warp, against the
    long-double reference on rows synthesised from the mpmath-warped matrices; the Beta-CDF budget as in
    ``_precision.ref_set_warp`` (``sens``: the fp64 replica's error of a mean with the warped inputs rounded to fp32, over 2^-24)."""
    cid = P.WARP_CASES[0]["id"]
    c = P.ALL[cid]
    st, fm, d = c["stationary"], c["form"], c["d"]
    X, y, alpha, H, _ = P.problem(cid)
    Xw, W, kap = P.warped_problem(cid)
    rng = np.random.RandomState(c["seed"] + 9)
    A, Bm = rng.uniform(size=(41, d)), rng.uniform(size=(41, d))
    masks = R.masks_of(R._singles(d) + [tuple(range(d))])
    ref = R.reference_of(X, y, alpha, H[0], A, Bm, masks, st, fm, warp=W[0])
    Aw, Bw = P.f(hp.warp_inputs(A, W[0])), P.f(hp.warp_inputs(Bm, W[0]))
    X32 = P.to32(P.f(Xw[0]))
    a32 = PD.alpha64(X32, y, alpha, H[0], st, fm)
    e32 = float(np.abs(R.means64(X32, a32, H[0], P.to32(Aw), P.to32(Bw), masks, st, fm) - P.f(ref["F"])).max() / ref["scale"])
    t = P.tol("mean", float(kap[0]), len(X), e32 / P.F32)
    ctx = lib.Context(X, y, alpha, form=fm, stationary=st, max_batch=len(H))
    try:
        ctx.set_warp(W[0])
        assert ctx.posterior(H[:1], want_alpha=False)["status"][0] == 0
        got = ctx.sobol_indices(_noise_off(H[:1]), A, Bm, masks)
        ctx.set_warp(None)
    finally:
        ctx.close()
    e = R.errs(_item(got, 0), ref, t)
    print("PRECISION sobol %s context warp: f0 %.4f V %.4f C %.4f J %.4f tol (tol %.3g, of which Beta CDF %.3g)"
          % (cid, e["f0"], e["V"], e["C"], e["J"], t, P.CDF_REL * e32 / P.F32))
    assert max(e.values()) <= 1.0


def _raw(ctx, B, H, A, Bm, masks, N=None, T=None):
    """The C entry itself (limits that ``Context.sobol_indices`` cannot express); returns the code."""
    H, A, Bm = (np.ascontiguousarray(a, dtype=np.float64) for a in (H, A, Bm))
    masks = np.ascontiguousarray(masks, dtype=np.uint32)
    nT = max(1, len(masks))
    f0, V, cl, to = np.zeros(max(1, B)), np.zeros(max(1, B)), np.zeros(max(1, B) * nT), np.zeros(max(1, B) * nT)
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint)
    return ctx._lib.bgp_sobol_indices(ctx._h, B, H.ctypes.data_as(dp), len(A) if N is None else N, A.ctypes.data_as(dp),
                                      Bm.ctypes.data_as(dp), len(masks) if T is None else T, masks.ctypes.data_as(up),
                                      f0.ctypes.data_as(dp), V.ctypes.data_as(dp), cl.ctypes.data_as(dp), to.ctypes.data_as(dp))


def test_error_codes(lib):
    rng = np.random.RandomState(5)
    n, d = 12, 3
    X, y = rng.uniform(size=(n, d)), rng.randn(n)
    H = np.column_stack([np.zeros(2), np.full((2, d), -1.0), np.full(2, -4.0)])
    A, Bm = rng.uniform(size=(5, d)), rng.uniform(size=(5, d))
    ok = dict(B=1, H=H[:1], A=A, Bm=Bm, masks=[1, 6, 0, 7])
    ctx = lib.Context(X, y, 1e-8, max_batch=2)
    big = lib.Context(rng.uniform(size=(n, 33)), y, 1e-8, max_batch=1)
    try:
        assert _raw(ctx, **ok) == ERR_STATE  # before any posterior build
        assert "resident" in lib.load().bgp_last_error().decode()
        assert np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)
        H33 = np.zeros((1, 35))
        assert np.all(big.posterior(H33, want_alpha=False)["status"] == 0)
        assert _raw(big, 1, H33, rng.uniform(size=(4, 33)), rng.uniform(size=(4, 33)), [1]) == ERR_INVALID  # d > 32
        bad = [dict(masks=[1, 8]), dict(masks=[1 << 31]), dict(N=0), dict(N=(1 << 24) + 1), dict(T=0), dict(T=R.TMAX + 1), dict(B=0),
               dict(N=-1), dict(T=-1)]
        for kw in bad:
            assert _raw(ctx, **{**ok, **kw}) == ERR_INVALID, kw
        assert _raw(ctx, **{**ok, "B": 3, "H": np.vstack([H, H[:1]])}) == ERR_STATE  # more than are resident
        # ... and the context still works: the valid call, against its own route through the wrapper
        assert _raw(ctx, **ok) == 0
        f0, V, cl, to = ctx.sobol_indices(H[:2], A, Bm, [1, 6, 0, 7])
        assert cl.shape == to.shape == (2, 4) and all(np.all(np.isfinite(v)) for v in (f0, V, cl, to)) and np.all(V > 0.0)
        with pytest.raises(lib.BgpError, match="dimension"):
            ctx.sobol_indices(H[:1], A, Bm, [8])
        with pytest.raises(lib.BgpError, match="T <="):
            ctx.sobol_indices(H[:1], A, Bm, [])
        with pytest.raises(ValueError):
            ctx.sobol_indices(H[:1], A, Bm[:, :2], [1])
        mean, _var = ctx.predict(H[:1], A)  # the resident posteriors are as they were
        assert np.all(np.isfinite(mean))
    finally:
        ctx.close()
        big.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the Python layer
# ------------------------------------------------------------------------------------------------------------------------------
def _brute(gp, A, Bm, terms, thetas=None):
    """predict on hand-built rows and the numpy estimator: (mean, variance, closed, total) in y units (a leading axis per chain row)
    and the bounds of the comparison (f0, V, C, J): both sides carry tol("mean", kappa, n) on the mean's absolute-sum scale over
    these rows, taken with the median GP's kernel_ and alpha_, and its first-order image through the estimator (tests/_sobolref.py)."""
    from bayes_skopt_amd._posterior import sobol_estimator, sobol_masks

    rows = R.all_rows(A, Bm, sobol_masks(terms, A.shape[1]))
    Kt = gp.kernel_(gp.X_train_) + np.diag(np.broadcast_to(gp.alpha, (len(gp.X_train_),)))
    w = np.linalg.eigvalsh(Kt)
    scale = float(np.abs(gp.kernel_(gp.warp(rows) if gp.warp_inputs else rows, gp.X_train_) * np.ravel(gp.alpha_)[None, :]).sum(axis=1).max())
    dmu = 2.0 * P.tol("mean", float(w[-1] / w[0]), len(Kt)) * scale * float(np.ravel(gp.y_train_std_)[0])
    if thetas is None:
        F = np.asarray(gp.predict(rows)).reshape(len(terms) + 2, len(A))
    else:
        F = gp._predict_hyper_samples(thetas, rows)[0].reshape(len(thetas), len(terms) + 2, len(A))
    fA, fB, fT = F[..., 0, :], F[..., 1, :], F[..., 2:, :]
    f0, V, Cv, J = sobol_estimator(fA, fB, fT)
    N = len(A)
    ca, cb, dt = np.abs(fA - f0[..., None]), np.abs(fB - f0[..., None]), np.abs(fT - fA[..., None, :])
    bounds = (dmu, dmu * (ca + cb).sum(axis=-1) / N, dmu * 2.0 * (dt.sum(axis=-1) + cb.sum(axis=-1)[..., None]) / N,
              dmu * 2.0 * dt.sum(axis=-1) / N)
    return (f0, V, Cv, J), bounds, (fA, fB, fT)


def _close(got, want, bounds):
    return all(np.all(np.abs(np.asarray(g) - w) <= b) for g, w, b in zip(got, want, bounds))


def test_optimizer_sensitivity_indices(bask):
    from bayes_skopt_amd.space import Real

    dims = [Real(-2.0, 2.0), Real(0.0, 1.0), Real(-1.0, 1.0)]
    opt = bask.Optimizer(dimensions=dims, n_initial_points=10, random_state=0)
    f = lambda x: float(np.sin(2.0 * x[0]) + 2.0 * x[1] ** 2 + x[0] * x[1])  # (dimension 2 is ignored)
    opt.run(f, n_iter=16, n_samples=1, gp_samples=40, gp_burnin=5)
    gp, space = opt.gp, opt.space
    N = 300
    out = opt.sensitivity_indices(n_samples=N, pairs="all", random_state=3)
    assert out["path"] == "device" and sorted(out["first"]) == sorted(out["total"]) == [0, 1, 2]
    assert sorted(out["interaction"]) == [(0, 1), (0, 2), (1, 2)]
    rng = np.random.RandomState(3)
    A, Bm = space.rvs_transformed(N, random_state=rng), space.rvs_transformed(N, random_state=rng)
    terms = [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2)]
    got = gp.sensitivity(A, Bm, terms)
    want, bounds, (fA, fB, fT) = _brute(gp, A, Bm, terms)
    assert _close(got, want, bounds)
    mean, var, closed, total = got
    assert out["mean"] == mean and out["variance"] == var
    for k in range(3):  # (the same call: exact)
        assert out["first"][k] == closed[k] / var and out["total"][k] == total[k] / var
    assert out["interaction"][(0, 1)] == closed[3] / var - closed[0] / var - closed[1] / var
    assert min(out["total"], key=out["total"].get) == 2
    # total >= first up to the Monte-Carlo error of the two estimates: 5 standard errors of their summands, from the sample
    f0 = want[0]
    for k in range(3):
        se = 5.0 * (np.std((fB - f0) * (fT[k] - fA)) + np.std(0.5 * (fA - fT[k]) ** 2)) / np.sqrt(N) / var
        assert out["total"][k] >= out["first"][k] - se, (k, out["total"][k], out["first"][k], se)
    # the default: every single dimension, no pairs
    plain = bask.utils.sensitivity_indices(opt._result(), n_samples=N, random_state=3)
    assert plain["first"] == out["first"] and plain["total"] == out["total"] and plain["interaction"] == {}
    # the fully Bayesian indices: the mean of per-row calls, with the band
    fb = bask.utils.sensitivity_indices(opt._result(), dims=[0, 2], pairs=[(2, 1)], n_samples=N, n_gp_samples=5, random_state=11)
    r11 = np.random.RandomState(11)
    A2, B2 = space.rvs_transformed(N, random_state=r11), space.rvs_transformed(N, random_state=r11)
    rows = np.asarray(gp.chain_)[r11.randint(0, len(gp.chain_), size=5)]
    assert fb["path"] == "device" and sorted(fb["first"]) == [0, 2] and list(fb["interaction"]) == [(2, 1)]
    terms2 = [(0,), (2,), (1,), (2, 1)]
    per_row = [gp.sensitivity(A2, B2, terms2, thetas=r[None, :]) for r in rows]
    S = np.stack([p[2][0] / p[1][0] for p in per_row])   # (an item's bits do not depend on what shares the build or the call)
    Tt = np.stack([p[3][0] / p[1][0] for p in per_row])
    for i, k in enumerate([0, 2]):
        assert fb["first"][k] == S[:, i].mean() and fb["total"][k] == Tt[:, i].mean()
        for name, vals in (("first", S[:, i]), ("total", Tt[:, i])):
            lo, hi = fb["band"][name][k]
            assert (lo, hi) == tuple(np.percentile(vals, [5.0, 95.0]))
            assert lo <= fb[name][k] <= hi
    assert fb["interaction"][(2, 1)] == (S[:, 3] - S[:, 1] - S[:, 2]).mean()
    want, bounds, _ = _brute(gp, A2, B2, terms2, thetas=rows)
    assert _close([np.stack([p[j][0] for p in per_row]) for j in range(4)], want, bounds)
    # argument checks reach the caller as ValueError before the device is asked
    with pytest.raises(ValueError, match="outside"):
        gp.sensitivity(A, Bm, [(3,)])
    with pytest.raises(ValueError, match="at least one term"):
        gp.sensitivity(A, Bm, [])
    with pytest.raises(ValueError):
        gp.sensitivity(A, Bm[:5])
    with pytest.raises(RuntimeError):
        bask.BayesGPR(kernel=bask.construct_default_kernel([0])).sensitivity(A, Bm)


def test_the_fallbacks_agree_with_brute_force_and_say_so_once(bask, capfd, monkeypatch):
    import sklearn.gaussian_process.kernels as sk

    from bayes_skopt_amd import _posterior
    from bayes_skopt_amd.space import Space, create_result

    monkeypatch.setattr(_posterior, "_sens_told", [])
    rng = np.random.RandomState(0)
    d, n, N = 2, 40, 50
    Xt = rng.uniform(size=(n, d))
    y = np.sin(5.0 * Xt[:, 0]) + Xt[:, 1] ** 2 + 0.05 * rng.randn(n)
    space = Space([(-1.0, 1.0), (0.0, 4.0)])
    terms = [(0,), (1,), (0, 1)]
    capfd.readouterr()
    # a generic kernel tree: the host route for the median GP and for chain rows
    gp = bask.BayesGPR(kernel=sk.Matern(length_scale=0.4, nu=2.5) * sk.RBF(length_scale=0.7) + sk.WhiteKernel(0.05),
                       normalize_y=True, random_state=4)
    gp.fit(Xt, y, n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
    assert not gp._post.canonical
    res = create_result(space.inverse_transform(Xt), list(y), space, models=[gp])
    out = bask.utils.sensitivity_indices(res, pairs="all", n_samples=N, random_state=2)
    assert out["path"] == "host"
    r = np.random.RandomState(2)
    A, Bm = space.rvs_transformed(N, random_state=r), space.rvs_transformed(N, random_state=r)
    want, bounds, _ = _brute(gp, A, Bm, terms)
    assert _close(gp.sensitivity(A, Bm, terms), want, bounds)
    np.testing.assert_allclose([out["first"][0], out["first"][1], out["total"][0], out["total"][1]],
                               [want[2][0] / want[1], want[2][1] / want[1], want[3][0] / want[1], want[3][1] / want[1]], rtol=1e-9)
    hyp = bask.utils.sensitivity_indices(res, dims=[1], n_samples=N, n_gp_samples=2, random_state=2)
    r1 = np.random.RandomState(2)
    A1, B1 = space.rvs_transformed(N, random_state=r1), space.rvs_transformed(N, random_state=r1)
    rows1 = np.asarray(gp.chain_)[r1.randint(0, len(gp.chain_), size=2)]
    assert hyp["path"] == "host" and hyp["interaction"] == {} and list(hyp["first"]) == [1]
    want, bounds, _ = _brute(gp, A1, B1, [(1,)], thetas=rows1)
    np.testing.assert_allclose(hyp["first"][1], (want[2][:, 0] / want[1]).mean(), rtol=1e-9)
    # warp_inputs: the median GP stays on the device (context-level warp); chain rows carry their own warps and go by predict
    gw = bask.BayesGPR(kernel=bask.construct_default_kernel([0, 1]), random_state=1, warp_inputs=True, normalize_y=True)
    gw.fit(Xt, y, n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
    resw = create_result(space.inverse_transform(Xt), list(y), space, models=[gw])
    med = bask.utils.sensitivity_indices(resw, pairs="all", n_samples=N, random_state=2)
    assert med["path"] == "device"
    want, bounds, _ = _brute(gw, A, Bm, terms)
    assert _close(gw.sensitivity(A, Bm, terms), want, bounds)
    hyp = bask.utils.sensitivity_indices(resw, n_samples=N, n_gp_samples=3, random_state=2)
    assert hyp["path"] == "host" and set(hyp["band"]["first"]) == set(hyp["band"]["total"]) == {0, 1}
    r2 = np.random.RandomState(2)
    A2, B2 = space.rvs_transformed(N, random_state=r2), space.rvs_transformed(N, random_state=r2)
    rows = np.asarray(gw.chain_)[r2.randint(0, len(gw.chain_), size=3)]
    want, bounds, _ = _brute(gw, A2, B2, [(0,), (1,)], thetas=rows)
    *got, path = gw.sensitivity(A2, B2, [(0,), (1,)], thetas=rows, return_path=True)
    assert path == "host" and _close(got, want, bounds)
    np.testing.assert_allclose([hyp["total"][0], hyp["total"][1]], (want[3] / want[1][:, None]).mean(axis=0), rtol=1e-9)
    err = capfd.readouterr().err
    assert err.count("sensitivity: through predict on synthesised rows") == 1, err
