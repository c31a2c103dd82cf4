"""``bgp_shapley`` (bgp_shapley.hip) through ``_lib.Context`` on the cases of tests/_shapref.py against the long-double
reference at the bounds tests/test_cpu_shapley_reference.py qualifies; bits; a context warp; refusals; Python.  ``pytest -s``: PRECISION."""
import numpy as np
import pytest

import _pdref as PD
import _precision as P
import _shapref as R
from bayes_skopt_amd import _lib as lib
from bayes_skopt_amd._posterior import noise_off, shapley_by_predict

pytestmark = pytest.mark.gpu
hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)


def _run(cid, calls, warp=None):  # one context and build of case cid (R or P); calls: (rows of H, Xp, Z, interactions) each
    c, (X, y, alpha, H) = (R.ALL[cid], R.problem(cid)[:4]) if cid in R.ALL else (P.ALL[cid], P.problem(cid)[:4])
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=len(H))
    try:
        ctx.set_warp(warp)
        assert np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)
        return [ctx.shapley(noise_off(H[rows]), xp, z, it) for rows, xp, z, it in calls]
    finally:
        ctx.close()


def _same(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(np.atleast_1d(a).view(np.uint64), np.atleast_1d(b).view(np.uint64))


def _worst(got, B, ref, t, d):
    e = [R.errs(tuple(None if v is None else v[b] for v in got), ref(b), t(b), d) for b in range(B)]
    return {k: max(x[k] for x in e) for k in e[0]}


@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES])
def test_against_the_long_double_reference(cid):
    c, (kap, Xp, Z) = R.ALL[cid], R.problem(cid)[4:]
    B, d = c["Buse"], c["d"]
    got = _run(cid, [(slice(0, B), Xp, Z, c["inter"])])[0]
    worst = _worst(got, B, lambda b: R.reference(cid, b), lambda b: P.tol("mean", kap[b], c["n"]), d)
    print("PRECISION shapley %s kappa %.3g: of the bounds %s" % (cid, kap[:B].max(), " ".join("%s %.4f" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= 1.0
    if c["inter"]:
        assert _same(got[3], np.swapaxes(got[3], 2, 3)) and np.all(np.diagonal(got[3], axis1=2, axis2=3) == 0.0)


@pytest.mark.parametrize("cid,k", [("sh_B3", 1), ("sh7_n65_d8_N1_P3_matern52_sum", 6), ("sh11_n129_d4_N17_P1_matern52_product", 0)])
def test_bitwise_contracts(cid, k):  # alone and inside P = 3, B = 3; zeros where x_pk is every z_sk (k low; high; 3 chunks, P = B = 1), x_p is z_0
    c, (Xp, Z) = R.ALL[cid], R.problem(cid)[5:]
    every, last = slice(0, c["B"]), c["P"] - 1
    Zk = np.where(np.arange(c["d"]) == k, Xp[last], Z)
    ref, alone, one, flat, twin = _run(cid, [(every, Xp, Z, True), (every, Xp[last:], Z, True), (slice(0, 1), Xp, Z, True),
                                             (every, Xp, Zk, True), (every, Xp[:1], Xp[:1], True)])
    assert all(_same(ref[i][:, last:], alone[i]) for i in (0, 2, 3)) and _same(ref[1], alone[1]) and all(_same(a[:1], b) for a, b in zip(ref, one))
    phi, inter = flat[0][:, last], flat[3][:, last]
    assert np.all(phi[:, k] == 0.0) and np.all(inter[:, k, :] == 0.0) and np.all(inter[:, :, k] == 0.0) and np.all(np.delete(phi, k, axis=1) != 0.0)
    assert np.all(twin[0] == 0.0) and np.all(twin[3] == 0.0) and _same(twin[2][:, 0], twin[1])


def test_context_level_warp():  # against the reference on the mpmath-warped inputs; sens as in test_gpu_sobol.py: the replica's error at fp32 inputs
    c = P.WARP_CASES[0]
    cid, st, fm, d = c["id"], c["stationary"], c["form"], c["d"]
    (X, y, alpha, H, _), (Xw, W, kap) = P.problem(cid), P.warped_problem(cid)
    rng = np.random.RandomState(c["seed"] + 9)
    Xp, Z = rng.uniform(size=(2, d)), rng.uniform(size=(17, d))
    ref = R.reference_of(X, y, alpha, H[0], Xp, Z, st, fm, warp=W[0])
    X32, Xp32, Z32 = (P.to32(P.f(v)) for v in (Xw[0], hp.warp_inputs(Xp, W[0]), hp.warp_inputs(Z, W[0])))
    r32 = R.replica64(X32, PD.alpha64(X32, y, alpha, H[0], st, fm), H[0], Xp32, Z32, st, fm)
    e32 = float(max(np.abs(P.f(r32[1] - ref["base"])), np.abs(P.f(r32[2] - ref["value"])).max()) / ref["scale"])
    t = P.tol("mean", float(kap[0]), len(X), e32 / P.F32)
    e = _worst(_run(cid, [(slice(0, 1), Xp, Z, True)], warp=W[0])[0], 1, lambda b: ref, lambda b: t, d)
    print("PRECISION shapley %s context warp (tol %.3g): of the bounds %s" % (cid, t, " ".join("%s %.4f" % kv for kv in sorted(e.items()))))
    assert max(e.values()) <= 1.0


def test_refusals_leave_the_context_usable():
    rng, n, d = np.random.RandomState(5), 12, 3
    X, y = rng.uniform(size=(n, d)), rng.randn(n)
    H = np.column_stack([np.zeros(2), np.full((2, d), -1.0), np.full(2, -4.0)])
    Xp, Z = rng.uniform(size=(2, d)), rng.uniform(size=(5, d))
    ctx, fresh, big = (lib.Context(v, y, 1e-8, max_batch=2) for v in (X, X, rng.uniform(size=(n, 17))))
    try:
        assert big.posterior(np.zeros((1, 19)), want_alpha=False)["status"][0] == 0 == ctx.posterior(H[:1], want_alpha=False)["status"][0]
        for c, h, xp, z, code in ((big, np.zeros((1, 19)), Z[:1].repeat(6, 1)[:, :17], Z.repeat(6, 1)[:, :17], "1.*d > 16"),
                                  (ctx, H, Xp, Z, "4"), (ctx, H[:1], Xp[:0], Z, "1"), (ctx, H[:1], Xp, Z[:0], "1")):
            with pytest.raises(lib.BgpError, match="code " + code):  # d = 17; more than are resident; P < 1; N < 1
                c.shapley(h, xp, z)
        assert np.all(ctx.posterior(H, want_alpha=False, warps=np.zeros((2, 2 * d)))["status"] == 0)
        with pytest.raises(lib.BgpError, match="code 4.*per-row warped"):
            ctx.shapley(H, Xp, Z)
        for c in (ctx, fresh):                             # a plain build and predict afterwards: a fresh context's bits
            assert np.all(c.posterior(H, want_alpha=False)["status"] == 0)
        assert all(_same(a, b) for a, b in zip(ctx.predict(H, Xp) + ctx.shapley(H, Xp, Z, True), fresh.predict(H, Xp) + fresh.shapley(H, Xp, Z, True)))
    finally:
        for c in (ctx, fresh, big):
            c.close()


def test_optimizer_shapley_values_and_the_host_routes(capfd, monkeypatch):
    import bayes_skopt_amd as bask
    import sklearn.gaussian_process.kernels as sk
    from bayes_skopt_amd.space import Real, Space, create_result

    monkeypatch.setattr(bask._posterior, "_shap_told", [])
    opt = bask.Optimizer(dimensions=[Real(-2.0, 2.0, name="a"), Real(0.0, 1.0), Real(-1.0, 1.0, name="c")], n_initial_points=10, random_state=0)
    opt.run(lambda x: float(np.sin(2.0 * x[0]) + 2.0 * x[1] ** 2 + x[0] * x[1]), n_iter=15, n_samples=1, gp_samples=40, gp_burnin=5)
    gp, out = opt.gp, opt.shapley_values(n_samples=40, interactions=True, random_state=3)
    assert out["path"] == "device" and out["names"] == ["a", "X_1", "c"] and sorted(out["interaction"]) == [("X_1", "c"), ("a", "X_1"), ("a", "c")]
    rng = np.random.RandomState(3)
    x = bask.utils.expected_optimum(opt._result(), random_state=rng)[0]
    Xp, Z = opt.space.transform([x]), opt.space.rvs_transformed(40, random_state=rng)
    host = shapley_by_predict(gp, None, Xp, Z, "test", True)
    # device and predict each carry tol("mean", kappa, n) on the means' absolute-sum scale over the coalition rows
    w = np.linalg.eigvalsh(gp.kernel_(gp.X_train_) + gp.alpha * np.eye(len(gp.X_train_)))
    scale = float(np.abs(gp.kernel_(R.coalition_rows(Xp[0], Z, R.coalition_picks(3)), gp.X_train_) * np.ravel(gp.alpha_)).sum(axis=1).max())
    dmu = 2.0 * P.tol("mean", float(w[-1] / w[0]), len(w)) * scale * gp._y_scale()[1]
    phi = np.array([out["phi"][nm] for nm in out["names"]])
    assert out["x"] == list(x) and np.all(np.abs(phi - gp._y_scale()[1] * host[0][0, 0]) <= 2.0 * dmu)
    assert abs(phi.sum() - (out["value"] - out["base"])) <= 4.0 * dmu and abs(out["value"] - float(gp.predict(Xp)[0])) <= dmu
    one = opt.shapley_values(x=x, baseline=[0.0, 0.5, 0.0], n_gp_samples=4, random_state=1)  # baseline Shapley, chain rows
    assert one["path"] == "device" and all(lo <= one["phi"][nm] <= hi for nm, (lo, hi) in one["band"].items())
    r = np.random.RandomState(0)  # a generic kernel tree and 17 dimensions go through predict and say so once
    for kernel, dd in ((sk.Matern(length_scale=0.4, nu=2.5) * sk.RBF(length_scale=0.7) + sk.WhiteKernel(0.05), 2),
                       (bask.construct_default_kernel(list(range(17))), 17)):
        Xt, sp = r.uniform(size=(30, dd)), Space([(0.0, 1.0)] * dd)
        g = bask.BayesGPR(kernel=kernel, normalize_y=True, random_state=4)
        g.fit(Xt, np.sin(5.0 * Xt[:, 0]) + Xt[:, 1] ** 2, n_desired_samples=40, n_burnin=1, n_walkers_per_thread=40, progress=False)
        got = bask.utils.shapley_values(create_result(sp.inverse_transform(Xt), list(g.y_train_), sp, models=[g]), x=list(Xt[0]), baseline=[0.5] * dd)
        assert got["path"] == "host" and abs(sum(got["phi"].values()) - (got["value"] - got["base"])) <= 1e-9 * (1.0 + abs(got["value"]))
    assert capfd.readouterr().err.count("shapley: through predict on synthesised rows") == 1
