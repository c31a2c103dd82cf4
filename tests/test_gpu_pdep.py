"""Partial dependence of the surrogate mean on the device (``bgp_partial_dependence``, bgp_pdep.hip), driven
through ``_lib.Context`` on the cases of tests/_pdref.py -- every kernel family, n = 1, d = 1, d = 32, the 32-point training tile,
the 16-sample chunk and the 16 x 16 grid tile each at size - 1, size, size + 1, grids of 1 and 256 values, a pair listed with
k1 > k2, a repeated panel, fewer items than resident posteriors, r = 0 -- and through the Python layer (``BayesGPR``,
``utils.partial_dependence``, ``Optimizer.partial_dependence``).

* every panel against the long-double reference on the synthesised rows at ``tol("mean", kappa, n)``, the tolerance
  tests/test_cpu_pdep_reference.py qualifies; against ``ctx.predict`` on the synthesised rows within 2 tol;
* bitwise: a panel alone, inside a list, in a reordered list; one item alone and inside a batch; two identical calls;
* a context-level warp against ``hp_oracle.warp_inputs`` on the synthesised rows; the limits, which are error codes.

Lines printed with ``pytest -s`` start with ``PRECISION``."""
import ctypes as C
import functools

import numpy as np
import pytest

import _pdref as R
import _precision as P

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
    """One context and posterior build of the case; ``calls``: (rows of H, panels) per device call.  With ``predict``: also the
    means of ``ctx.predict`` on the synthesised rows, averaged in numpy, per panel of the case."""
    c = R.ALL[cid]
    X, y, alpha, H, _kap, Xs, grids = R.problem(cid)
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=len(H))
    try:
        assert np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)
        out = [ctx.partial_dependence(_noise_off(H[rows]), Xs, grids, panels) for rows, panels in calls]
        via = None
        if predict:
            via, Hk = [], _noise_off(H[: c["Buse"]])
            for panel in c["panels"]:
                axes = R.panel_axes(panel, grids)
                shape, cells = R._cells(axes)
                step = max(1, 4096 // len(Xs))
                parts = [ctx.predict(Hk, R.synth_rows(Xs, axes, cells[c0:c0 + step]))[0].reshape(len(Hk), -1, len(Xs)).mean(axis=2)
                         for c0 in range(0, len(cells), step)]
                via.append(np.concatenate(parts, axis=1).reshape((len(Hk),) + shape))
    finally:
        ctx.close()
    return out, via


@functools.lru_cache(maxsize=None)
def _cached(lib, cid):
    """The case's own call (its first Buse posteriors, its panel list) and the predict route, shared by the tests that read them."""
    c = R.ALL[cid]
    out, via = _run(lib, cid, [(slice(0, c["Buse"]), c["panels"])], predict=True)
    return out[0], via


@pytest.mark.parametrize("cid", CIDS)
def test_against_the_long_double_reference(lib, cid):
    c = R.ALL[cid]
    kap = R.problem(cid)[4]
    got, _via = _cached(lib, cid)
    assert len(got) == len(c["panels"])
    worst = 0.0
    for b in range(c["Buse"]):
        ref = R.reference(cid, b)
        for (k1, k2), g, (v, _s) in zip(c["panels"], got, ref):
            assert g.shape == (c["Buse"],) + v.shape == (c["Buse"],) + ((c["ng"][k1],) if k2 < 0 else (c["ng"][k1], c["ng"][k2]))
        worst = max(worst, max(R.errs([g[b] for g in got], ref)) / P.tol("mean", kap[b], c["n"]))
    print("PRECISION pdep %s kappa %.3g: device vs long double %.4f tol" % (cid, kap[: c["Buse"]].max(), worst))
    assert worst <= 1.0


@pytest.mark.parametrize("cid", CIDS)
def test_against_predict_on_the_synthesised_rows(lib, cid):
    c = R.ALL[cid]
    kap = R.problem(cid)[4]
    got, via = _cached(lib, cid)
    worst = 0.0
    for b in range(c["Buse"]):
        ref = R.reference(cid, b)  # (its scales)
        e = [float(np.abs(g[b] - v[b]).max() / s) for g, v, (_r, s) in zip(got, via, ref)]
        worst = max(worst, max(e) / P.tol("mean", kap[b], c["n"]))
    print("PRECISION pdep %s: device vs predict on synthesised rows %.4f tol (2 allowed)" % (cid, worst))
    assert worst <= 2.0


def _same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("cid", ["pd_ragged_B3", "pd_twin_matern12", "pd_edge+1"])
def test_bitwise_invariants(lib, cid):
    c = R.ALL[cid]
    panels, B = c["panels"], c["Buse"]
    order = list(range(len(panels)))[::-1]
    every = slice(0, B)
    calls = [(every, panels), (every, panels), (every, [panels[i] for i in order])] + [(every, [p]) for p in panels]
    calls += [(slice(0, 1), panels)]
    out, _ = _run(lib, cid, calls)
    full = out[0]
    assert all(_same(a, b) for a, b in zip(full, out[1]))                    # two identical calls
    assert all(_same(full[i], g) for i, g in zip(order, out[2]))             # a reordered list
    assert all(_same(full[i], out[3 + i][0]) for i in range(len(panels)))    # a panel alone
    assert all(_same(a[:1], b) for a, b in zip(full, out[-1]))               # item 0 alone (B = 1 on row 0)
    for i, p in enumerate(panels):                                           # a repeated panel: the same block twice
        for j in range(i):
            if panels[j] == p:
                assert _same(full[i], full[j])


def test_b1_on_row0_equals_item0_of_b3(lib):
    cid = "pd_twin_matern12"
    c = R.ALL[cid]
    assert c["B"] == c["Buse"] == 3
    out, _ = _run(lib, cid, [(slice(0, 3), c["panels"]), (slice(0, 1), c["panels"])])
    assert all(_same(a[:1], b) for a, b in zip(*out))


def test_context_level_warp(lib):
    """Samples and grid rows go through the context-level warp as predict's queries do: WARP_CASES[0]'s problem and warp, against
    the long-double reference on rows synthesised from the mpmath-warped samples and grids; the Beta-CDF budget as in
    ``_precision.ref_set_warp`` (``sens``: the fp64 replica's error with the warped inputs rounded to fp32, over 2^-24)."""
    cid = P.WARP_CASES[0]["id"]
    c = P.ALL[cid]
    st, fm, d = c["stationary"], c["form"], c["d"]
    X, y, alpha, H, _ = P.problem(cid)
    Xw, W, kap = P.warped_problem(cid)
    rng = np.random.RandomState(c["seed"] + 9)
    Xs = rng.uniform(size=(21, d))
    grids = [np.linspace(0.0, 1.0, 9), np.linspace(0.05, 0.95, 17)]
    panels = [(0, -1), (1, -1), (1, 0)]
    ref = R.reference_of(X, y, alpha, H[0], Xs, grids, tuple(panels), st, fm, warp=W[0])
    Xsw = P.f(hp.warp_inputs(Xs, W[0]))
    gw = [P.f(hp.warp_inputs(np.column_stack([g] * d), W[0]))[:, k] for k, g in enumerate(grids)]
    X32 = P.to32(P.f(Xw[0]))
    a32 = R.alpha64(X32, y, alpha, H[0], st, fm)
    e32 = max(R.errs(R.replica64(X32, a32, H[0], P.to32(Xsw), [P.to32(g) for g in gw], panels, st, fm), ref))
    t = P.tol("mean", float(kap[0]), len(X), e32 / P.F32)
    ctx = lib.Context(X, y, alpha, form=fm, stationary=st, max_batch=len(H))
    try:
        ctx.set_warp(W[0])
        assert ctx.posterior(H[:1], want_alpha=False)["status"][0] == 0
        got = ctx.partial_dependence(_noise_off(H[:1]), Xs, grids, panels)
        ctx.set_warp(None)
    finally:
        ctx.close()
    e = max(R.errs([g[0] for g in got], ref))
    print("PRECISION pdep %s context warp: %.4f tol (tol %.3g, of which Beta CDF %.3g)" % (cid, e / t, t, P.CDF_REL * e32 / P.F32))
    assert e <= t


def _raw(lib, ctx, B, H, Xs, gmax, ng, grid, panels, P_=None, S=None):
    """The C entry itself (limits that ``Context.partial_dependence`` cannot express); returns the code."""
    H, Xs, grid = (np.ascontiguousarray(a, dtype=np.float64) for a in (H, Xs, grid))
    ng, panels = (np.ascontiguousarray(a, dtype=np.int32) for a in (ng, panels))
    out = np.zeros(max(1, B) * 70000)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    return ctx._lib.bgp_partial_dependence(ctx._h, B, H.ctypes.data_as(dp), len(Xs) if S is None else S, Xs.ctypes.data_as(dp), gmax,
                                           ng.ctypes.data_as(ip), grid.ctypes.data_as(dp), len(panels) if P_ is None else P_,
                                           panels.reshape(-1).ctypes.data_as(ip), out.ctypes.data_as(dp))


def test_error_codes(lib):
    rng = np.random.RandomState(5)
    n, d = 12, 3
    X, y = rng.uniform(size=(n, d)), rng.randn(n)
    H = np.column_stack([np.zeros(2), np.full((2, d), -1.0), np.full(2, -4.0)])
    Xs, grid = rng.uniform(size=(4, d)), rng.uniform(size=(5, d))
    ok = dict(B=1, H=H[:1], Xs=Xs, gmax=5, ng=[5, 3, 1], grid=grid, panels=[[0, -1], [2, 1]])
    ctx = lib.Context(X, y, 1e-8, max_batch=2)
    big = lib.Context(rng.uniform(size=(n, 33)), y, 1e-8, max_batch=1)
    try:
        assert _raw(lib, ctx, **ok) == ERR_STATE  # before any posterior build
        assert "resident" in lib.load().bgp_last_error().decode()
        assert np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)
        H33 = np.zeros((1, 35))
        assert np.all(big.posterior(H33, want_alpha=False)["status"] == 0)
        assert _raw(lib, big, 1, H33, rng.uniform(size=(4, 33)), 5, [5] * 33, rng.uniform(size=(5, 33)), [[0, -1]]) == ERR_INVALID
        bad = [dict(ng=[5, 0, 1]), dict(ng=[5, 6, 1]), dict(gmax=257, ng=[5, 3, 1], grid=rng.uniform(size=(257, d))),
               dict(panels=[[0, -1], [3, 1]]), dict(panels=[[-1, 1]]), dict(panels=[[0, -2]]), dict(panels=[[1, 1]]), dict(S=0),
               dict(P_=0), dict(B=0)]
        for kw in bad:
            assert _raw(lib, ctx, **{**ok, **kw}) == ERR_INVALID, kw
        assert _raw(lib, ctx, **{**ok, "B": 3, "H": np.vstack([H, H[:1]])}) == ERR_STATE  # more than are resident
        # ... and the context still works: the valid call, against its own route through the wrapper
        assert _raw(lib, ctx, **ok) == 0
        got = ctx.partial_dependence(H[:1], Xs, [grid[:5, 0], grid[:3, 1], grid[:1, 2]], [(0, -1), (2, 1)])
        assert [g.shape for g in got] == [(1, 5), (1, 1, 3)] and all(np.all(np.isfinite(g)) for g in got)
        with pytest.raises(lib.BgpError, match="gmax"):
            ctx.partial_dependence(H[:1], Xs, [np.linspace(0, 1, 257)] * d, [(0, -1)])
    finally:
        ctx.close()
        big.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the Python layer
# ------------------------------------------------------------------------------------------------------------------------------
def _brute(gp, Xs, grids, panel, thetas=None):
    """predict on hand-built rows, the mean over the samples: (G1[, G2]) in y units, or (B, ...) per chain row -- and the
    tolerance of the comparison in y units: both sides carry tol("mean", kappa, n) on the mean's absolute-sum scale over these
    rows, max_rows sum_j |k(row, X_j) alpha_j|, taken with the median GP's kernel_ and alpha_."""
    axes = R.panel_axes(panel, grids)
    shape, cells = R._cells(axes)
    rows = R.synth_rows(Xs, axes, cells)
    Kt = gp.kernel_(gp.X_train_) + np.diag(np.broadcast_to(gp.alpha, (len(gp.X_train_),)))
    w = np.linalg.eigvalsh(Kt)
    scale = float(np.abs(gp.kernel_(gp.warp(rows) if gp.warp_inputs else rows, gp.X_train_) * np.ravel(gp.alpha_)[None, :]).sum(axis=1).max())
    t = 2.0 * P.tol("mean", float(w[-1] / w[0]), len(Kt)) * scale * float(np.ravel(gp.y_train_std_)[0])
    if thetas is None:
        return np.asarray(gp.predict(rows)).reshape(len(cells), len(Xs)).mean(axis=1).reshape(shape), t
    mu = gp._predict_hyper_samples(thetas, rows)[0]
    return mu.reshape(len(thetas), len(cells), len(Xs)).mean(axis=2).reshape((len(thetas),) + shape), t


def _close(got, want_t):
    want, t = want_t
    return float(np.abs(got - want).max()) <= t


def test_optimizer_partial_dependence(bask):
    from bayes_skopt_amd.space import Categorical, Integer, Real, Space

    dims = [Real(-2.0, 2.0), Real(1e-3, 1.0, prior="log-uniform"), Integer(0, 5), Categorical(["a", "b", "c"])]
    opt = bask.Optimizer(dimensions=dims, n_initial_points=8, random_state=0)
    f = lambda x: float(np.sin(2.0 * x[0]) + np.log10(x[1]) ** 2 + 0.1 * (x[2] - 2) ** 2 + {"a": 0.0, "b": 0.3, "c": -0.2}[x[3]])
    opt.run(f, n_iter=14, n_samples=1, gp_samples=40, gp_burnin=5)
    gp, space = opt.gp, opt.space
    out = opt.partial_dependence(n_samples=23, n_points=7, random_state=3)
    assert out["path"] == "device" and sorted(out["dims"]) == [0, 1, 2, 3] and len(out["pairs"]) == 6
    np.testing.assert_allclose(out["dims"][0][0], np.linspace(-2.0, 2.0, 7))
    np.testing.assert_allclose(out["dims"][1][0], np.logspace(-3.0, 0.0, 7))
    assert list(out["dims"][2][0]) == [0, 1, 2, 3, 4, 5] and list(out["dims"][3][0]) == ["a", "b", "c"]
    assert out["pairs"][(1, 3)][2].shape == (7, 3) and out["pairs"][(0, 2)][2].shape == (7, 6)
    Xs = space.rvs_transformed(23, random_state=np.random.RandomState(3))
    grids = [np.asarray(Space([dm]).transform([[v] for v in out["dims"][k][0]]))[:, 0] for k, dm in enumerate(dims)]
    for k in range(4):
        assert _close(out["dims"][k][1], _brute(gp, Xs, grids, (k, -1)))
    for (a, b), (_g1, _g2, v) in out["pairs"].items():
        assert _close(v, _brute(gp, Xs, grids, (a, b)))
    # given samples (original space), chosen panels, and the fully Bayesian curve: the mean of per-row calls, with its band
    samples = space.rvs(9, random_state=5)
    rng = np.random.RandomState(11)
    rows = np.asarray(gp.chain_)[rng.randint(0, len(gp.chain_), size=5)]
    fb = bask.utils.partial_dependence(opt._result(), dims=[1, 3], pairs=[(3, 1)], n_points=5, samples=samples, n_gp_samples=5,
                                       random_state=11)
    assert fb["path"] == "device" and sorted(fb["dims"]) == [1, 3] and list(fb["pairs"]) == [(3, 1)]
    Xg = space.transform(samples)
    g5 = [np.asarray(Space([dm]).transform([[v] for v in bask.utils._pd_grid(dm, 5)[0]]))[:, 0] for dm in dims]
    per_row = [gp.partial_dependence(Xg, g5, [(1, -1), (3, -1), (3, 1)], thetas=r[None, :]) for r in rows]
    for i, key in enumerate([1, 3]):  # (an item's bits do not depend on what shares the build or the call: exact)
        stack = np.stack([p[i][0] for p in per_row])
        np.testing.assert_array_equal(fb["dims"][key][1], stack.mean(axis=0))
        lo, hi = fb["band"][key]
        np.testing.assert_array_equal(lo, np.percentile(stack, 5.0, axis=0))
        np.testing.assert_array_equal(hi, np.percentile(stack, 95.0, axis=0))
    pair_rows = np.stack([p[2][0] for p in per_row])
    np.testing.assert_array_equal(fb["pairs"][(3, 1)][2], pair_rows.mean(axis=0))
    assert _close(pair_rows, _brute(gp, Xg, g5, (3, 1), thetas=rows))
    with pytest.raises(RuntimeError):
        bask.BayesGPR(kernel=bask.construct_default_kernel([0])).partial_dependence(Xg, g5)


def test_the_fallbacks_agree_with_brute_force_and_say_so_once(bask, capfd, monkeypatch):
    import sklearn.gaussian_process.kernels as sk

    from bayes_skopt_amd import _posterior
    from bayes_skopt_amd.space import Space, create_result

    monkeypatch.setattr(_posterior, "_pd_told", [])
    rng = np.random.RandomState(0)
    d, n = 2, 40
    Xt = rng.uniform(size=(n, d))
    y = np.sin(5.0 * Xt[:, 0]) + Xt[:, 1] ** 2 + 0.05 * rng.randn(n)
    space = Space([(-1.0, 1.0), (0.0, 4.0)])
    capfd.readouterr()
    # a generic kernel tree: the host route for the median GP and for chain rows
    gp = bask.BayesGPR(kernel=sk.Matern(length_scale=0.4, nu=2.5) * sk.RBF(length_scale=0.7) + sk.WhiteKernel(0.05),
                       normalize_y=True, random_state=4)
    gp.fit(Xt, y, n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
    assert not gp._post.canonical
    res = create_result(space.inverse_transform(Xt), list(y), space, models=[gp])
    out = bask.utils.partial_dependence(res, n_samples=11, n_points=5, random_state=2)
    assert out["path"] == "host"
    Xs = space.rvs_transformed(11, random_state=np.random.RandomState(2))
    grids = [np.linspace(0.0, 1.0, 5)] * d
    for k in range(d):
        assert _close(out["dims"][k][1], _brute(gp, Xs, grids, (k, -1)))
    assert _close(out["pairs"][(0, 1)][2], _brute(gp, Xs, grids, (0, 1)))
    hyp = bask.utils.partial_dependence(res, dims=[1], pairs=None, n_samples=11, n_points=5, n_gp_samples=2, random_state=2)
    r1 = np.random.RandomState(2)
    Xs1 = space.rvs_transformed(11, random_state=r1)
    rows1 = np.asarray(gp.chain_)[r1.randint(0, len(gp.chain_), size=2)]
    assert hyp["path"] == "host" and not hyp["pairs"]
    want, t = _brute(gp, Xs1, grids, (1, -1), thetas=rows1)
    assert _close(hyp["dims"][1][1], (want.mean(axis=0), t))
    # warp_inputs: the median GP stays on the device (context-level warp); chain rows carry their own warps and go by predict
    gw = bask.BayesGPR(kernel=bask.construct_default_kernel([0, 1]), random_state=1, warp_inputs=True, normalize_y=True)
    gw.fit(Xt, y, n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
    resw = create_result(space.inverse_transform(Xt), list(y), space, models=[gw])
    med = bask.utils.partial_dependence(resw, n_samples=11, n_points=5, random_state=2)
    assert med["path"] == "device"
    assert _close(med["pairs"][(0, 1)][2], _brute(gw, Xs, grids, (0, 1)))
    hyp = bask.utils.partial_dependence(resw, n_samples=11, n_points=5, n_gp_samples=3, random_state=2)
    assert hyp["path"] == "host" and set(hyp["band"]) == {0, 1}
    r2 = np.random.RandomState(2)
    Xs2 = space.rvs_transformed(11, random_state=r2)
    rows = np.asarray(gw.chain_)[r2.randint(0, len(gw.chain_), size=3)]
    want, t = _brute(gw, Xs2, grids, (0, 1), thetas=rows)
    assert _close(hyp["pairs"][(0, 1)][2], (want.mean(axis=0), t))
    err = capfd.readouterr().err
    assert err.count("partial_dependence: through predict on synthesised rows") == 1, err
