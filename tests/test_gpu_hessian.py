"""Posterior of the surrogate's Hessian on the device (``bgp_hess_cov``, bgp_hess.hip), driven through
``_lib.Context`` on the cases of tests/_hessref.py and through ``Optimizer.optimum_curvature``: hmean, hvar and hcov against the
long-double reference at the tolerances tests/test_cpu_hessian_reference.py qualifies, with their structure; bitwise independence of
the company, the batch, the call, the point chunk and the outputs asked for; the limits, which are error codes (PRECISION lines: -s)."""
import functools

import numpy as np
import pytest

import _hessref as R
import _precision as P

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

ALL3 = (True, True, True)
LIMITS = "hs4_n65_d8_m3_matern52_product"


@pytest.fixture(scope="module")
def lib():
    from bayes_skopt_amd import _lib
    assert _lib.device_count() >= 1
    return _lib


def _run(lib, cid, calls, rows=slice(None)):
    """One context and posterior build (rows ``rows`` of H) of the case; ``calls``: (H rows of the call, Xq, wants) per device call."""
    c = R.ALL[cid]
    X, y, alpha, H, _kap, _Xq = R.problem(cid)
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=len(H))
    try:
        assert np.all(ctx.posterior(H[rows], want_alpha=False)["status"] == 0)
        return [ctx.hess_cov(Hc, Xq, *want) for Hc, Xq, want in calls]
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def _cached(lib, cid):  # the case's own call: its first Buse posteriors, every output
    return _run(lib, cid, [(R.problem(cid)[3][: R.ALL[cid]["Buse"]], R.problem(cid)[5], ALL3)])[0]


def _same(got, full, pick=lambda a: a, of=lambda a: a):
    return all(np.array_equal(pick(g), of(f)) for g, f in zip(got, full))


@pytest.mark.parametrize("cid", list(R.ALL))
def test_against_the_long_double_reference(lib, cid):
    c = R.ALL[cid]
    kap = R.problem(cid)[4]
    hm, hv, hc = _cached(lib, cid)
    B, m, d = c["Buse"], c["m"], c["d"]
    k, l = np.tril_indices(d)
    assert hm.shape == hv.shape == (B, m, d, d) and hc.shape == (B, m, len(k), len(k))
    assert all(np.array_equal(a, np.swapaxes(a, 2, 3)) for a in (hm, hv, hc)) and (hv >= 0.0).all()
    assert np.array_equal(hv[:, :, k, l], np.diagonal(hc, axis1=2, axis2=3)) and all(np.isfinite(a).all() for a in (hm, hv, hc))
    for b in range(B):
        ref = R.reference(cid, b)
        t_var, t_mean = P.tol("var", kap[b], c["n"]), P.tol("mean", kap[b], c["n"])
        e = R.errors(hm[b], hv[b], hc[b], ref) / np.array([t_var, t_var, t_mean])
        print("PRECISION hess %s b%d kappa %.3g: device vs long double hcov %.4f hvar %.4f hmean %.4f tol" % ((cid, b, kap[b]) + tuple(e)))
        assert e.max() <= 1.0
        if c["special"]:  # far outside the data the covariance is P0 (the clip has nothing to hide) and Hbar is 0
            assert (np.abs(hc[b, R.FAR] - P.f(ref["P0"])) / (ref["s0"][:, None] * ref["s0"][None, :])).max() <= t_var
            assert (np.abs(hm[b, R.FAR][k, l]) / ref["s0"]).max() <= t_mean * ref["scale_hmean"]
    if c["B"] > 1:  # 2 of 3 resident posteriors: B = 1 and all three against them, and posterior 1 built and used alone
        H, Xq = R.problem(cid)[3], R.problem(cid)[5]
        one, three = _run(lib, cid, [(H[:1], Xq, ALL3), (H, Xq, ALL3)])
        assert _same(one, (hm, hv, hc), lambda a: a[0], lambda a: a[0]) and _same(three, (hm, hv, hc), lambda a: a[:2])
        assert _same(_run(lib, cid, [(H[1:2], Xq, ALL3)], rows=slice(1, 2))[0], (hm, hv, hc), lambda a: a[0], lambda a: a[1])


@pytest.mark.parametrize("cid", ["hs3_n129_d6_m7_matern52_sum", LIMITS, "hs5_n129_d16_m2_rbf_product"])
def test_bits_do_not_depend_on_the_company_the_outputs_asked_for_the_chunk_or_the_call(lib, cid, monkeypatch):
    H, Xq = R.problem(cid)[3], R.problem(cid)[5]
    full = _cached(lib, cid)
    pick = sorted({0, len(Xq) - 1})
    WANTS = [(a, b, c) for a in (True, False) for b in (True, False) for c in (True, False) if a or b or c]
    out = _run(lib, cid, [(H[:1], Xq, ALL3)] + [(H[:1], Xq[s : s + 1], ALL3) for s in pick] + [(H[:1], Xq, w) for w in WANTS])
    assert _same(out[0], full)  # two calls
    for s, one in zip(pick, out[1 : 1 + len(pick)]):  # a point alone: m = 1
        assert _same(one, full, lambda a: a[0, 0], lambda a: a[0, s])
    for w, got in zip(WANTS, out[1 + len(pick) :]):  # NULL outputs
        assert all((g is None) == (not have) and (g is None or np.array_equal(g, f)) for have, g, f in zip(w, got, full))
    monkeypatch.setenv("BGP_HESS_CHUNK", "2")  # (read at every call: m = 7 runs as 2 + 2 + 2 + 1 points, m = 3 as 2 + 1)
    assert _same(_run(lib, cid, [(H[:1], Xq, ALL3)])[0], full)


def test_limits_are_error_codes_and_leave_the_posteriors_usable(lib):
    c = R.ALL[LIMITS]
    X, y, alpha, H, _kap, Xq = R.problem(LIMITS)
    rng = np.random.RandomState(0)
    X17 = rng.uniform(size=(20, 17))
    h17 = np.concatenate([[0.0], np.zeros(17), [-4.0]])[None, :]
    made = {st: lib.Context(X, y, alpha, form=c["form"], stationary=st, max_batch=2) for st in (c["stationary"], "matern32", "matern12")}
    made["big"] = lib.Context(X17, rng.randn(20), 1e-6, max_batch=1)
    ctx = made[c["stationary"]]

    def refused(code, who, *args):
        with pytest.raises(lib.BgpError, match=code):
            who.hess_cov(*args)

    try:
        refused(r"code 4", ctx, H[:1], Xq)  # nothing built
        assert np.all(ctx.posterior(H[:1], want_alpha=False)["status"] == 0)
        before = ctx.predict(H[:1], Xq)
        refused(r"code 4", ctx, np.repeat(H[:1], 2, axis=0), Xq)  # more items than resident posteriors
        refused(r"code 1", ctx, H[:1], Xq, False, False, False)  # no output asked for
        refused(r"code 1.*exceeds", ctx, H[:1], np.zeros(((1 << 22) // 48 + 1, c["d"])), True, False, False)  # m Tp over 2^22
        for st, Hs, Xs, why in (("matern32", H[:1], Xq, "not twice differentiable"), ("matern12", H[:1], Xq, "not twice differentiable"),
                                ("big", h17, X17[:2], "d > 16")):  # refused, never approximated; the posteriors still predict
            assert np.all(made[st].posterior(Hs, want_alpha=False)["status"] == 0)
            refused(r"code 1.*" + why, made[st], Hs, Xs)
            assert np.all(np.isfinite(made[st].predict(Hs, Xs)[0]))
        assert _same(ctx.predict(H[:1], Xq)[:2], before[:2])
        assert _same(ctx.hess_cov(H[:1], Xq, *ALL3), _cached(lib, LIMITS))
        ctx.set_warp(np.zeros(2 * c["d"]))  # a context-level warp: refused as by the gradient entry points
        assert np.all(ctx.posterior(H[:1], want_alpha=False)["status"] == 0)
        refused(r"code 1.*warped inputs", ctx, H[:1], np.clip(Xq, 0.0, 1.0))
        assert np.all(np.isfinite(ctx.predict(H[:1], np.clip(Xq, 0.0, 1.0))[0]))
    finally:
        for v in made.values():
            v.close()


def test_optimizer_curvature_of_a_bowl_with_a_flat_direction(monkeypatch, capfd):
    import bayes_skopt_amd as bask
    from bayes_skopt_amd import _posterior, hesscov
    from bayes_skopt_amd.space import Real

    flat = np.array([1.0, -1.0, 0.0]) / np.sqrt(2.0)  # f does not change along x_0 - x_1
    f = lambda x: float(2.0 * (x[0] + x[1] - 1.0) ** 2 + 3.0 * (x[2] - 0.5) ** 2)  # noqa: E731
    opt = bask.Optimizer(dimensions=[Real(0.0, 1.0)] * 3, n_initial_points=32, random_state=0)
    X0 = opt.space.rvs(32, random_state=1)
    opt.tell(X0, [f(x) for x in X0], gp_samples=40, gp_burnin=5, n_samples=1)
    kw = dict(x=[0.5, 0.5, 0.5], delta=0.01, n_draws=400, random_state=7)
    dev = opt.optimum_curvature(**kw)
    capfd.readouterr()
    monkeypatch.setattr(hesscov, "_told", [])
    monkeypatch.setattr(_posterior.CanonicalPosterior, "hessian_cov_path", "host")
    host = opt.optimum_curvature(**kw)
    monkeypatch.setattr(_posterior.CanonicalPosterior, "hessian_cov_path", "auto")
    assert capfd.readouterr().err.count("Hessian covariance: numpy on the downloaded inverse (forced)") == 1
    assert dev["path"] == "device" and host["path"] == "host" and dev["prob_minimum"] == host["prob_minimum"]
    for out in (dev, host):
        v = out["eigenvectors"][:, 0]
        assert abs(float(v @ flat)) >= 0.99 and v[np.argmax(np.abs(v))] > 0.0
        assert np.all(np.diff(out["eigenvalues"]) >= 0.0) and len(out["interval"]) == 3
    print("PRECISION hess bowl: eigenvalues %s, host %s, prob_minimum %.3f" % (dev["eigenvalues"], host["eigenvalues"], dev["prob_minimum"]))
    rows = opt.optimum_curvature(n_gp_samples=3, **kw)  # chain rows: one batched build, one call
    assert rows["path"] == "device" and rows["hessian"].shape == (3, 3) and abs(float(rows["eigenvectors"][:, 0] @ flat)) >= 0.9
