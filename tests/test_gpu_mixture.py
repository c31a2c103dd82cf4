"""The hyper-posterior mixture on the device (``bgp_predict_mixture``, ``bgp_predict_mixture_warped``, ``bgp_mixture_values``;
bgp_mix.hip), driven through ``_lib.Context`` on the cases of tests/_mixref.py and through the Python layer
(``BayesGPR.predict_marginal``, ``utils.predict_marginal``, ``Optimizer.predict_marginal``).

* every quantity of every case against the long-double reference at the derived tolerance, the quantiles by back-substitution;
* the exact rules: one row returns its ``mu`` and ``between == 0``, an atom that carries a quantile comes back exactly, every row bad
  gives NaN and ``n_used == 0``, the quantiles rise with p;
* bitwise: a point alone and in a crowd, two identical calls, ``weights=None`` against explicit ones, ``predict_mixture`` against
  ``predict`` + ``mixture_values``, every combination of NULL outputs, the warped entry against ``predict_warped`` + ``mixture_values``;
* the contract: error codes, which posteriors serve which entry, the resident posteriors afterwards.

Lines printed with ``pytest -s`` start with ``PRECISION``."""
import functools
import itertools

import numpy as np
import pytest

import _mixref as R
import _precision as P

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

QUANTS = ("mean", "within", "between", "cdf", "sf", "logpdf")
KEYS = QUANTS + ("quantiles",)


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


@pytest.fixture(scope="module")
def scratch_ctx(lib):
    """A context for ``mixture_values`` (it reads no posterior)."""
    X, y, alpha, _H, _ = P.problem(P.PREDB_CASES[5]["id"])
    ctx = lib.Context(X, y, alpha, max_batch=2)
    yield ctx
    ctx.close()


def _resident_ctx(lib, cid):
    c = R.ALL[cid]
    pc = P.ALL[c["pid"]]
    X, y, alpha, H, _ = P.problem(c["pid"])
    ctx = lib.Context(X, y, alpha, form=pc["form"], stationary=pc["stationary"], max_batch=len(H))
    warps = P.warp_params(c["pid"]) if c["kind"] == "warp" else None
    assert np.all(ctx.posterior(H, want_alpha=False, warps=warps)["status"] == 0)
    return ctx


def _same(a, b, keys=KEYS):
    for k in keys:
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s differs: max |d| %.3e" % (k, np.nanmax(np.abs(a[k] - b[k])))
    assert a["n_used"] == b["n_used"]


@functools.lru_cache(maxsize=None)
def _device(lib, cid):
    """The case's own call, and for a resident case the device's moments behind it: (out, steps, (mean, var) or None)."""
    c = R.ALL[cid]
    inp = R.inputs(cid)
    if c["kind"] == "syn":
        X, y, alpha, _H, _ = P.problem(P.PREDB_CASES[5]["id"])
        ctx = lib.Context(X, y, alpha, max_batch=2)
        try:
            out = ctx.mixture_values(inp["mean"], inp["var"], R.Y_MEAN, R.Y_STD, c["probs"], at=inp["t"], weights=inp["weights"])
            return out, ctx.mixture_stats(), None
        finally:
            ctx.close()
    ctx = _resident_ctx(lib, cid)
    try:
        Hk, Xq, warped = R.h_kernel(cid), P.query(c["pid"]), c["kind"] == "warp"
        out = ctx.predict_mixture(Hk, Xq, R.Y_MEAN, R.Y_STD, c["probs"], at=inp["t"], weights=inp["weights"], warped=warped)
        steps = ctx.mixture_stats()
        mom = ctx.predict_warped(Hk, Xq) if warped else ctx.predict(Hk, Xq)
        return out, steps, mom
    finally:
        ctx.close()


@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES])
def test_against_the_long_double_reference(lib, cid):
    c = R.ALL[cid]
    out, steps, _mom = _device(lib, cid)
    ref = R.reference(cid)
    assert out["n_used"] == ref["n_used"]
    assert ref["keep"].all()  # no point of any case is left out
    for q in QUANTS:
        assert out[q].shape == (c["m"],)
    assert out["quantiles"].shape == (len(c["probs"]), c["m"])
    r = R.ratios(cid, out)
    r["quantile"] = float(R.quantile_ratio(cid, out["quantiles"]).max())
    print("PRECISION mix %s: device vs long double (tol) %s; solver steps <= %d, bracket moves <= %d"
          % (cid, " ".join("%s %.3g" % kv for kv in r.items()), steps[0], steps[1]))
    assert max(r.values()) <= 1.0, r
    assert steps[0] < R.ITMAX


@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES])
def test_the_exact_rules(lib, cid):
    c = R.ALL[cid]
    out, _steps, mom = _device(lib, cid)
    inp = R.inputs(cid)
    if c["special"] == "allbad":
        assert out["n_used"] == 0 and all(np.isnan(out[k]).all() for k in KEYS)
        return
    assert (out["between"] >= 0.0).all() and (out["within"] >= 0.0).all()
    assert (np.diff(out["quantiles"][np.argsort(c["probs"])], axis=0) >= 0.0).all()  # monotone in p
    if c["B"] == 1:
        mean = inp["mean"] if c["kind"] == "syn" else mom[0]
        assert np.array_equal(out["mean"], R.Y_STD * mean[0] + R.Y_MEAN) and (out["between"] == 0.0).all()
    if c["special"] == "identical":
        assert (out["between"] == 0.0).all()
        md = R.model(cid)
        for k, p in enumerate(c["probs"]):
            want = float(R.ref_quantile(md["mu"][:1, 0], md["sd"][:1, 0], np.ones(1), p))
            ulp = np.spacing(abs(want)) + np.spacing(abs(float(md["mu"][0, 0])))
            print("PRECISION mix identical components p = %g: quantile off by %.2g ulp" % (p, abs(out["quantiles"][k, 0] - want) / ulp))
            assert abs(out["quantiles"][k, 0] - want) <= 64.0 * ulp
    if c["special"] == "nanrow":
        assert out["n_used"] == c["B"] - 1
    if c["special"] == "atoms":
        assert (out["logpdf"] == -np.inf).all()
    if c["special"] == "tails":
        assert np.isfinite(out["logpdf"]).all()
    for (k, i), val in R.exact_quantiles(cid).items():
        assert out["quantiles"][k, i] == val, (cid, k, i)


def _big(seed=77, B=129, m=513):
    rng = np.random.RandomState(seed)
    return (rng.randn(m)[None, :] + 0.3 * rng.randn(B, m), 10.0 ** rng.uniform(-3, 0, size=(B, m)), rng.uniform(0.1, 1.0, size=B),
            2.0 * rng.randn(m))


def test_a_point_alone_and_in_a_crowd_two_calls_and_the_weights(scratch_ctx):
    mean, var, w, t = _big()
    crowd = scratch_ctx.mixture_values(mean, var, R.Y_MEAN, R.Y_STD, R.PROBS5, at=t, weights=w)
    assert crowd["n_used"] == 129
    _same(crowd, scratch_ctx.mixture_values(mean, var, R.Y_MEAN, R.Y_STD, R.PROBS5, at=t, weights=w))
    for i in (0, 255, 256, 512):
        alone = scratch_ctx.mixture_values(mean[:, i:i + 1], var[:, i:i + 1], R.Y_MEAN, R.Y_STD, R.PROBS5, at=t[i:i + 1], weights=w)
        for k in KEYS:
            assert np.array_equal(alone[k][..., 0], crowd[k][..., i]), (k, i)
    ones = scratch_ctx.mixture_values(mean, var, R.Y_MEAN, R.Y_STD, R.PROBS5, at=t, weights=np.ones(129))
    _same(ones, scratch_ctx.mixture_values(mean, var, R.Y_MEAN, R.Y_STD, R.PROBS5, at=t))
    assert not np.array_equal(ones["mean"], crowd["mean"])


def test_every_combination_of_null_outputs(scratch_ctx):
    mean, var, w, t = _big(m=257, B=5)
    full = scratch_ctx.mixture_values(mean, var, R.Y_MEAN, R.Y_STD, R.PROBS3, at=t, weights=w)
    parts = {"moments": ("mean", "within", "between"), "quantiles": ("quantiles",), "at": ("cdf", "sf", "logpdf")}
    for n in range(0, 4):
        for want in itertools.combinations(parts, n):
            got = scratch_ctx.mixture_values(mean, var, R.Y_MEAN, R.Y_STD, R.PROBS3, at=t, weights=w, want=want)
            assert got["n_used"] == 5
            for part, keys in parts.items():
                for k in keys:
                    assert (k in got) == (part in want)
                    if part in want:
                        assert np.array_equal(got[k], full[k]), (want, k)


@pytest.mark.parametrize("cid", [R.RES[0], R.RES[3], R.RES[-1]] + R.WARP)
def test_the_resident_entry_is_predict_followed_by_mixture_values(lib, scratch_ctx, cid):
    c = R.ALL[cid]
    out, _steps, (mean, var) = _device(lib, cid)
    inp = R.inputs(cid)
    _same(out, scratch_ctx.mixture_values(mean, var, R.Y_MEAN, R.Y_STD, c["probs"], at=inp["t"], weights=inp["weights"]))


def test_the_contract(lib):
    cid = R.RES[0]
    c = R.ALL[cid]
    pc = P.ALL[c["pid"]]
    X, y, alpha, H, _ = P.problem(c["pid"])
    Hk, Xq, inp = R.h_kernel(cid), P.query(c["pid"]), R.inputs(cid)
    ctx = lib.Context(X, y, alpha, form=pc["form"], stationary=pc["stationary"], max_batch=len(H))
    try:
        args = (Hk, Xq, R.Y_MEAN, R.Y_STD, c["probs"])
        with pytest.raises(lib.BgpError, match=r"bgp_predict_mixture failed \(code 4\).*bgp_predict_mixture: no resident"):
            ctx.predict_mixture(*args)
        with pytest.raises(lib.BgpError, match=r"bgp_predict_mixture_warped failed \(code 4\)"):
            ctx.predict_mixture(*args, warped=True)
        assert np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)
        before = ctx.predict(Hk, Xq)
        good = ctx.predict_mixture(*args, at=inp["t"], weights=inp["weights"])
        for bad in ((0.0,), (1.0,), (0.5, float("nan")), (-0.1,), tuple(np.linspace(0.1, 0.9, R.QMAX + 1))):
            with pytest.raises(lib.BgpError, match=r"code 1"):
                ctx.predict_mixture(Hk, Xq, R.Y_MEAN, R.Y_STD, bad)
            with pytest.raises(lib.BgpError, match=r"code 1"):
                ctx.mixture_values(before[0], before[1], R.Y_MEAN, R.Y_STD, bad)
        for w in ([1.0, -1.0, 1.0], [1.0, float("inf"), 1.0], [float("nan"), 1.0, 1.0]):
            with pytest.raises(lib.BgpError, match=r"code 1"):
                ctx.predict_mixture(*args, weights=w)
        with pytest.raises(lib.BgpError, match=r"code 4.*per-row warped"):  # a plain build does not serve the warped entry
            ctx.predict_mixture(*args, warped=True)
        # the refusals launched nothing and left the posteriors alone: the same bits as before, from both entries
        _same(good, ctx.predict_mixture(*args, at=inp["t"], weights=inp["weights"]))
        after = ctx.predict(Hk, Xq)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        # fewer rows than are resident: the first two
        two = ctx.predict_mixture(Hk[:2], Xq, R.Y_MEAN, R.Y_STD, c["probs"])
        _same(two, ctx.mixture_values(before[0][:2], before[1][:2], R.Y_MEAN, R.Y_STD, c["probs"]), keys=("mean", "within", "between", "quantiles"))
        with pytest.raises(lib.BgpError, match=r"code 4.*needs 4 posteriors, 3 resident"):
            ctx.predict_mixture(np.vstack([Hk, Hk[:1]]), Xq, R.Y_MEAN, R.Y_STD, c["probs"])
    finally:
        ctx.close()
    wid = R.WARP[0]
    wctx = _resident_ctx(lib, wid)
    try:
        wc = R.ALL[wid]
        with pytest.raises(lib.BgpError, match=r"bgp_predict_mixture failed \(code 4\).*per-row warped"):  # ... and the reverse
            wctx.predict_mixture(R.h_kernel(wid), P.query(wc["pid"]), R.Y_MEAN, R.Y_STD, wc["probs"])
    finally:
        wctx.close()


# ------------------------------------------------------------------------------------------------------------------------------
# the Python layer: n = 40, d = 2, 200 points, 8 rows
# ------------------------------------------------------------------------------------------------------------------------------
FIT = dict(n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
LAYER = ("mean", "std", "std_within", "std_between", "quantiles", "cdf", "sf", "logpdf")


def _layer_data():
    rng = np.random.RandomState(0)
    Xt = rng.uniform(size=(40, 2))
    y = np.sin(5.0 * Xt[:, 0]) + Xt[:, 1] ** 2 + 0.05 * rng.randn(40)
    return Xt, y, rng.uniform(size=(200, 2))


def _layer_t(gp, Xq):
    """A value per point within a few standard deviations of the median GP's prediction (|z| stays far below the 38 of the tails
    case: the reference's Phi is asked for nothing it was not qualified on)."""
    mean, std = gp.predict(Xq, return_std=True)
    return mean + R.T_OFF[np.arange(len(Xq)) % len(R.T_OFF)] * std


@pytest.fixture(scope="module")
def fitted(bask):
    Xt, y, _Xq = _layer_data()
    gp = bask.BayesGPR(kernel=bask.construct_default_kernel([0, 1]), normalize_y=True, random_state=3)
    gp.fit(Xt, y, **FIT)
    return gp


def _rows_mixture(gp, rows, Xq, t, noise=False, weights=None):
    """``mixture_values`` on ``_predict_hyper_samples``' moments (y units: y_mean = 0, y_std = 1) in the layer's names."""
    mu, sd = gp._predict_hyper_samples(rows, Xq, noise_zero=not noise)
    out = gp._ctx.mixture_values(mu, sd * sd, 0.0, 1.0, R.PROBS3, at=t, weights=weights)
    out.update(std=np.sqrt(out["within"] + out["between"]), std_within=np.sqrt(out["within"]), std_between=np.sqrt(out["between"]))
    return out, mu, sd


def _layer_against_reference(name, out, mu, sd, t, weights=None):
    """Every fourth point against the long-double mixture of the rows' own fp64 moments (exact inputs)."""
    sl = slice(None, None, 4)
    cid = R.register("layer_" + name, mu[:, sl], (sd * sd)[:, sl], weights, R.PROBS3, t[sl])
    got = dict(mean=out["mean"][sl], within=out["std_within"][sl] ** 2, between=out["std_between"][sl] ** 2, cdf=out["cdf"][sl],
               sf=out["sf"][sl], logpdf=out["logpdf"][sl])
    ref = R.reference(cid)
    # (the layer returns the roots of within / between: squaring them back costs 2 eps of each)
    r = {}
    for q in QUANTS:
        val, tol = ref[q]
        extra = 4.0 * P.EPS * np.abs(P.f(val)) if q in ("within", "between") else 0.0
        err = np.abs(P.f(got[q].astype(val.dtype) - val))
        assert np.isfinite(err).all(), q
        r[q] = float(np.where(err == 0.0, 0.0, err / (tol + extra)).max())
    r["quantile"] = float(R.quantile_ratio(cid, out["quantiles"][:, sl]).max())
    print("PRECISION mix layer %s: predict_marginal vs long double on the rows' moments (tol) %s" % (name, " ".join("%s %.3g" % kv for kv in r.items())))
    assert max(r.values()) <= 1.0, r


def test_predict_marginal_is_the_pass_on_the_rows_moments(bask, fitted):
    gp = fitted
    _Xt, _y, Xq = _layer_data()
    t = _layer_t(gp, Xq)
    rows = np.asarray(gp.chain_)[:8]
    w = np.linspace(0.5, 1.5, 8)
    out, path = gp.predict_marginal(Xq, thetas=rows, at=t, weights=w, return_path=True)
    assert path == "device" and out["n_used"] == 8 and np.array_equal(out["rows"], rows) and np.array_equal(out["probs"], R.PROBS3)
    want, mu, sd = _rows_mixture(gp, rows, Xq, t, weights=w)
    for k in LAYER:
        assert np.array_equal(out[k], want[k]), k
    assert out["quantiles"].shape == (3, 200) and (np.diff(out["quantiles"], axis=0) > 0.0).all()
    _layer_against_reference("canonical", out, mu, sd, t, weights=w)
    # rows drawn as evaluate_acquisitions draws them; fewer if the chain is shorter
    from sklearn.utils import check_random_state

    drawn = gp.predict_marginal(Xq[:5], n_samples=8, random_state=5)
    assert np.array_equal(drawn["rows"], np.asarray(gp.chain_)[check_random_state(5).choice(len(gp.chain_), replace=False, size=8)])
    assert "cdf" not in drawn
    assert len(gp.predict_marginal(Xq[:5], n_samples=10**6, random_state=5)["rows"]) == len(gp.chain_)
    # noise=True keeps every row's own white level: the within-part grows by exactly their weighted average (y units)
    lat, obs = gp.predict_marginal(Xq, thetas=rows), gp.predict_marginal(Xq, thetas=rows, noise=True)
    y_std = float(np.ravel(gp.y_train_std_)[0])
    white = np.mean(np.exp(gp._canonical(rows)[:, -1])) * y_std**2
    np.testing.assert_allclose(obs["std_within"] ** 2 - lat["std_within"] ** 2, white, rtol=1e-9)
    assert np.array_equal(obs["mean"], lat["mean"]) and np.array_equal(obs["std_between"], lat["std_between"])
    # more rows than the context holds: moments in chunks, the same mixture (nine copies of the eight rows)
    many, path = gp.predict_marginal(Xq[:7], thetas=np.tile(rows, (gp._ctx.max_batch // 8 + 1, 1)), at=t[:7], return_path=True)
    few = gp.predict_marginal(Xq[:7], thetas=rows, at=t[:7])
    assert path == "chunks" and many["n_used"] == 8 * (gp._ctx.max_batch // 8 + 1)
    for k in LAYER:
        np.testing.assert_allclose(many[k], few[k], rtol=1e-9, atol=1e-12, err_msg=k)
    # the median GP still predicts afterwards (its posterior is rebuilt on demand)
    assert np.all(np.isfinite(gp.predict(Xq[:3])))
    fresh = bask.BayesGPR(kernel=bask.construct_default_kernel([0, 1]), normalize_y=True, random_state=3)
    with pytest.raises(RuntimeError, match="predict before fit"):
        fresh.predict_marginal(Xq[:3])


def test_the_warped_route(bask):
    Xt, y, Xq = _layer_data()
    gw = bask.BayesGPR(kernel=bask.construct_default_kernel([0, 1]), random_state=1, warp_inputs=True, normalize_y=True)
    gw.fit(Xt, y, **FIT)
    t = _layer_t(gw, Xq)
    rows = np.asarray(gw.chain_)[:8]
    assert rows.shape[1] == len(gw.kernel_.theta) + 4  # the rows carry their warps
    out, path = gw.predict_marginal(Xq, thetas=rows, at=t, return_path=True)
    want, mu, sd = _rows_mixture(gw, rows, Xq, t)
    assert path == "device"
    for k in LAYER:
        assert np.array_equal(out[k], want[k]), k  # bgp_predict_mixture_warped against predict_warped + mixture_values
    _layer_against_reference("warp_inputs", out, mu, sd, t)


def test_the_generic_route_says_so_once(bask, capfd, monkeypatch):
    from sklearn.gaussian_process import kernels as sk

    from bayes_skopt_amd import bayesgpr

    Xt, y, Xq = _layer_data()
    gp = bask.BayesGPR(kernel=sk.Matern(length_scale=0.4, nu=2.5) * sk.RBF(length_scale=0.7) + sk.WhiteKernel(0.05), normalize_y=True,
                       random_state=4)
    gp.fit(Xt, y, **FIT)
    assert not gp._post.canonical
    t = _layer_t(gp, Xq)
    monkeypatch.setattr(bayesgpr, "_marginal_told", [])
    capfd.readouterr()
    rows = np.asarray(gp.chain_)[:8]
    out, path = gp.predict_marginal(Xq, thetas=rows, at=t, return_path=True)
    again = gp.predict_marginal(Xq, thetas=rows, at=t)
    err = capfd.readouterr().err
    assert path == "chunks" and err.count("predict_marginal: the rows' moments chunk by chunk") == 1 and "generic kernel tree" in err
    want, mu, sd = _rows_mixture(gp, rows, Xq, t)
    for k in LAYER:
        assert np.array_equal(out[k], want[k]) and np.array_equal(out[k], again[k]), k
    _layer_against_reference("generic", out, mu, sd, t)


def test_optimizer_and_utils_take_original_space_points(bask):
    from bayes_skopt_amd.space import Real

    opt = bask.Optimizer(dimensions=[Real(-2.0, 2.0), Real(0.0, 1.0)], n_initial_points=8, random_state=0)
    opt.run(lambda x: float(np.sin(2.0 * x[0]) + x[1] ** 2), n_iter=10, n_samples=1, gp_samples=40, gp_burnin=5)
    pts = [[-1.5, 0.2], [0.0, 0.5], [1.9, 0.99]]
    before = opt.rng.get_state()
    a = opt.predict_marginal(pts, n_samples=8, random_state=2, at=0.3)
    after = opt.rng.get_state()
    assert before[0] == after[0] and np.array_equal(before[1], after[1]) and before[2:] == after[2:]
    b = bask.utils.predict_marginal(opt._result(), pts, n_samples=8, random_state=2, at=0.3)
    c = opt.gp.predict_marginal(opt.space.transform(pts), n_samples=8, random_state=2, at=0.3)
    for k in LAYER:
        assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]), k
    assert a["mean"].shape == (3,) and a["n_used"] == 8 and np.all(a["std"] > 0.0)
    np.testing.assert_allclose(a["std"] ** 2, a["std_within"] ** 2 + a["std_between"] ** 2, rtol=1e-12)
    np.testing.assert_allclose(a["cdf"] + a["sf"], 1.0, rtol=1e-12)
