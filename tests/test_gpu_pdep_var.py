"""Posterior variance of the partial dependence on the device (``bgp_partial_dependence_var``, bgp_pdvar.hip; DESIGN.md section
30), driven through ``_lib.Context`` on the cases of tests/_pdvarref.py: variance and cell covariance against the long-double
reference on the synthesised rows at ``tol("var", kappa, n)`` on the prior variance's scale, the mean by section 16's metric at
``tol("mean", kappa, n)`` (tests/test_cpu_pdep_var_reference.py qualifies both); bit-for-bit invariants; a context-level warp; the
refusals; and the Python layer on a small ``Optimizer``.  Lines printed with ``pytest -s`` start with ``PRECISION``."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import _pdref as R
import _pdvarref as V
import _precision as P

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

ERR_INVALID, ERR_STATE = 1, 4  # include/bgp.h


@pytest.fixture(scope="module")
def lib():
    import bayes_skopt_amd  # noqa: F401
    from bayes_skopt_amd import _lib

    assert _lib.device_count() >= 1
    return _lib


@contextlib.contextmanager
def _context(lib, X, y, alpha, H, st, fm, warp=None):
    ctx = lib.Context(X, y, alpha, form=fm, stationary=st, max_batch=len(H))
    try:
        if warp is not None:
            ctx.set_warp(warp)
        assert np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)
        yield ctx
    finally:
        ctx.close()


def _curves_first(got, ref_v):
    covs = iter(got[2])
    return [(v, next(covs) if r[1] is not None else None) for v, r in zip(got[1], ref_v)]


@pytest.mark.parametrize("cid", [c["id"] for c in V.CASES])
def test_against_the_long_double_reference(lib, cid):
    c = V.ALL[cid]
    X, y, alpha, H, kap, Xs, grids = R.problem(cid)
    with _context(lib, X, y, alpha, H, c["stationary"], c["form"]) as ctx:
        mean, var, cov = ctx.partial_dependence_var(H[: c["Buse"]], Xs, grids, c["panels"], want_cov=True)
    for b in range(c["Buse"]):
        ref_v = V.reference(cid, b)
        got = _curves_first(([g[b] for g in mean], [g[b] for g in var], [g[b] for g in cov]), ref_v)
        tv, tm = P.tol("var", kap[b], c["n"]), P.tol("mean", kap[b], c["n"])
        ev, ec = (e / tv for e in V.errs(got, ref_v, float(hp.prior_var(H[b], c["d"], c["form"], noise=False))))
        em = max(R.errs([g[b] for g in mean], R.reference(cid, b))) / tm
        print("PRECISION pdvar %s item %d kappa %.3g: var %.4f tol, cov %.4f tol, mean %.4f tol" % (cid, b, kap[b], ev, ec, em))
        assert max(ev, ec, em) <= 1.0
        # never negative; a curve's covariance exactly symmetric, its diagonal the variance bit for bit
        assert all(np.all(v >= 0.0) and (cv is None or (np.array_equal(cv, cv.T) and np.array_equal(np.diagonal(cv), v))) for v, cv in got)


def _same(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint64), y.view(np.uint64)) for x, y in zip(a, b))


@pytest.mark.parametrize("cid", [V.CASES[5]["id"], V.CASES[6]["id"], V.CASES[7]["id"]])
def test_bitwise_invariants(lib, cid, monkeypatch):
    c = V.ALL[cid]
    X, y, alpha, H, _kap, Xs, grids = R.problem(cid)
    panels, B = c["panels"], c["Buse"]
    with _context(lib, X, y, alpha, H, c["stationary"], c["form"]) as ctx:
        run = lambda rows, pn, **kw: ctx.partial_dependence_var(H[rows], Xs, grids, pn, **kw)
        full = run(slice(0, B), panels, want_cov=True)
        monkeypatch.setenv("BGP_PDVAR_CHUNK", "128")  # (read at every call)
        forced = run(slice(0, B), panels, want_cov=True)
        monkeypatch.delenv("BGP_PDVAR_CHUNK")
        assert all(_same(a, b) for a, b in zip(full, forced))
        monkeypatch.setenv("BGP_ITEM_CHUNK", "1")  # one posterior per chunk: the loop over posterior chunks
        assert all(_same(a, b) for a, b in zip(full, run(slice(0, B), panels, want_cov=True)))
        monkeypatch.delenv("BGP_ITEM_CHUNK")
        one = run(slice(0, 1), panels, want_cov=True)  # B = 1 on row 0
        assert all(_same([g[:1] for g in a], b) for a, b in zip(full, one))
        for i, p in enumerate(panels):  # a panel alone (its covariance: the block of the curves before it in the list)
            m, v, cv = run(slice(0, B), [p], want_cov=True)
            assert _same([full[0][i]], m) and _same([full[1][i]], v)
            assert p[1] >= 0 or _same([full[2][sum(q[1] < 0 for q in panels[:i])]], cv)
        assert _same(full[0], run(slice(0, B), panels, want_var=False)[0])  # whichever outputs are asked for
        assert _same(full[1], run(slice(0, B), panels, want_mean=False)[1])
        assert _same(full[2], run(slice(0, B), panels, want_mean=False, want_var=False, want_cov=True)[2])


def test_context_level_warp(lib):
    """WARP_CASES[0]'s problem and warp, as tests/test_gpu_pdep.py: the references on rows synthesised from the mpmath-warped samples
    and grids, the Beta-CDF budget from the fp64 replica's error with the warped inputs rounded to fp32 (``sens`` over 2^-24)."""
    cid = P.WARP_CASES[0]["id"]
    c = P.ALL[cid]
    st, fm, d = c["stationary"], c["form"], c["d"]
    X, y, alpha, H, _ = P.problem(cid)
    Xw, W, kap = P.warped_problem(cid)
    Xs = np.random.RandomState(c["seed"] + 9).uniform(size=(17, d))
    grids, panels = [np.linspace(0.0, 1.0, 9), np.linspace(0.05, 0.95, 5)], ((0, -1), (1, 0))
    ref_m = R.reference_of(X, y, alpha, H[0], Xs, grids, panels, st, fm, warp=W[0])
    ref_v = V.reference_of(X, y, alpha, H[0], Xs, grids, panels, st, fm, warp=W[0])
    gw = [P.f(hp.warp_inputs(np.column_stack([g] * d), W[0]))[:, k] for k, g in enumerate(grids)]
    r32 = V.replica64(P.to32(P.f(Xw[0])), y, alpha, H[0], P.to32(P.f(hp.warp_inputs(Xs, W[0]))), [P.to32(g) for g in gw], panels, st, fm)
    scale = float(hp.prior_var(H[0], d, fm, noise=False))
    tv = P.tol("var", float(kap[0]), len(X), max(V.errs([g[1:] for g in r32], ref_v, scale)) / P.F32)
    tm = P.tol("mean", float(kap[0]), len(X), max(R.errs([g[0] for g in r32], ref_m)) / P.F32)
    with _context(lib, X, y, alpha, H[:1], st, fm, warp=W[0]) as ctx:
        mean, var, cov = ctx.partial_dependence_var(H[:1], Xs, grids, panels, want_cov=True)
    ev, ec = V.errs(_curves_first(([g[0] for g in mean], [g[0] for g in var], [g[0] for g in cov]), ref_v), ref_v, scale)
    em = max(R.errs([g[0] for g in mean], ref_m))
    print("PRECISION pdvar %s context warp: var %.4f tol, cov %.4f tol (tol %.3g), mean %.4f tol (tol %.3g)"
          % (cid, ev / tv, ec / tv, tv, em / tm, tm))
    assert max(ev, ec) <= tv and em <= tm


def test_refusals_leave_predict_as_it_was(lib):
    rng = np.random.RandomState(5)
    n, d = 12, 3
    X, y = rng.uniform(size=(n, d)), rng.randn(n)
    H = np.column_stack([np.zeros(2), np.full((2, d), -1.0), np.full(2, -4.0)])
    Xq, grid, ng, pan = rng.uniform(size=(4, d)), rng.uniform(size=(5, d)), np.array([5, 3, 1], dtype=np.int32), np.array([0, -1, 2, 1], dtype=np.int32)
    dp, ip, out = C.POINTER(C.c_double), C.POINTER(C.c_int), np.zeros(3 * 64)

    def raw(ctx, B=1, S=4, Xs=Xq, ng=ng, grid=grid, outs=(out, out, None)):
        Hb = np.ascontiguousarray(np.zeros((B, ctx.d + 2)))
        ptr = [o.ctypes.data_as(dp) if o is not None else C.cast(None, dp) for o in outs]
        return ctx._lib.bgp_partial_dependence_var(ctx._h, B, Hb.ctypes.data_as(dp), S, Xs.ctypes.data_as(dp), 5, ng.ctypes.data_as(ip),
                                                   grid.ctypes.data_as(dp), 2, pan.ctypes.data_as(ip), *ptr)

    ctx = lib.Context(X, y, 1e-8, max_batch=2)
    big = lib.Context(rng.uniform(size=(n, 33)), y, 1e-8, max_batch=1)
    try:
        assert np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)
        assert np.all(big.posterior(np.zeros((1, 35)), want_alpha=False)["status"] == 0)
        before, before_big = ctx.predict(H, Xq), big.predict(np.zeros((1, 35)), np.zeros((4, 33)))
        assert raw(ctx) == 0
        for code, kw in [(ERR_INVALID, dict(S=16385, Xs=np.zeros((16385, d)))), (ERR_INVALID, dict(outs=(None, None, None))),
                         (ERR_STATE, dict(B=3))]:
            assert raw(ctx, **kw) == code, kw
            assert all(np.array_equal(a, b) for a, b in zip(before, ctx.predict(H, Xq)))
        assert raw(big, Xs=np.zeros((4, 33)), ng=np.full(33, 5, dtype=np.int32), grid=np.zeros((5, 33))) == ERR_INVALID  # d = 33
        assert all(np.array_equal(a, b) for a, b in zip(before_big, big.predict(np.zeros((1, 35)), np.zeros((4, 33)))))
        assert np.all(ctx.posterior(H, want_alpha=False, warps=np.zeros((2, 2 * d)))["status"] == 0)  # per-row warped posteriors
        assert raw(ctx) == ERR_STATE
        assert np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)
        assert all(np.array_equal(a, b) for a, b in zip(before, ctx.predict(H, Xq)))
    finally:
        ctx.close()
        big.close()


def test_optimizer_partial_dependence_std(lib):
    import bayes_skopt_amd as bask
    from bayes_skopt_amd import _posterior

    opt = bask.Optimizer(dimensions=[(-2.0, 2.0), (0.0, 1.0), (-1.0, 3.0)], n_initial_points=8, random_state=0)
    opt.run(lambda x: float(np.sin(2.0 * x[0]) + x[1] ** 2 + 0.1 * (x[2] - 1.0) ** 2), n_iter=22, n_samples=1, gp_samples=40, gp_burnin=5)
    gp, res, kw = opt.gp, opt._result(), dict(n_samples=9, n_points=5, random_state=3)
    assert set(bask.utils.partial_dependence(res, **kw)) == {"dims", "pairs", "path"}  # today's keys, exactly
    out = opt.partial_dependence(return_std=True, **kw)
    assert out["path"] == "device" and set(out) == {"dims", "pairs", "path", "std"}
    Xs, grids = opt.space.rvs_transformed(9, random_state=np.random.RandomState(3)), [np.linspace(0.0, 1.0, 5)] * 3
    panels = [(k, -1) for k in range(3)] + [(0, 1), (0, 2), (1, 2)]
    _m, hv, _c = _posterior.partial_dependence_var_by_predict(gp, None, Xs, grids, panels, False, "the test's forced host path")
    w = np.linalg.eigvalsh(gp.kernel_(gp.X_train_) + np.diag(np.broadcast_to(gp.alpha, (len(gp.X_train_),))))
    with gp.noise_set_to_zero():
        scale = float(gp.kernel_.diag(gp.X_train_[:1])[0])
    y_std, t = float(np.ravel(gp.y_train_std_)[0]), P.tol("var", float(w[-1] / w[0]), len(w))
    dev = list(out["std"]["dims"].values()) + list(out["std"]["pairs"].values())
    e = max(float(np.abs((g / y_std) ** 2 - h[0]).max()) for g, h in zip(dev, hv)) / scale
    print("PRECISION pdvar optimizer: device vs host path %.4f tol" % (e / t))
    assert e <= t
    fb = opt.partial_dependence(return_std=True, n_gp_samples=4, **kw)
    for part in ("dims", "pairs"):
        for k, tot in fb["std"][part].items():
            np.testing.assert_allclose(tot**2, fb["std_within"][part][k] ** 2 + fb["std_between"][part][k] ** 2, rtol=1e-12)
