"""Hyper-posterior rows under input warping in one batched device pass: ``Context.posterior(H, warps=W)`` builds row b from the
training inputs through ITS OWN Beta-CDF warp and keeps them resident, ``predict_warped`` shows row b the queries through the
same warp (bgp_posterior_batch_warped / bgp_predict_batch_warped).

* precision -- alpha, mean and var of every row against the long-double reference of tests/_warprows.py at ``_precision.tol``
  (qualified without a GPU in tests/test_cpu_warp_rows_reference.py); lines start with ``PRECISION`` (``pytest -s``);
* bits -- every row equals, bit for bit, the per-row form it replaces: context-level warp, one-row build, one-row predict;
* state -- per-row-warped posteriors are read by ``predict_warped`` alone, everything else refuses and the context stays usable;
* ``BayesGPR._predict_hyper_samples`` takes the batched path and returns the bits of the row-by-row loop."""
import numpy as np
import pytest

import _precision as P
import _warprows as WR

pytestmark = pytest.mark.gpu

CIDS = [c["id"] for c in P.WARP_CASES]


@pytest.fixture(scope="module")
def lib():
    import bayes_skopt_amd  # noqa: F401
    from bayes_skopt_amd import _lib

    assert _lib.device_count() >= 1
    return _lib


def _noise_off(H):
    Hk = H.copy()
    Hk[:, -1] = -np.inf
    return Hk


def _per_row(ctx, H, Hk, W, Xq, rows=None):
    """The form the batched pass replaces, row by row: context-level warp, one-row build, one-row predict."""
    out = {k: [] for k in ("lml", "alpha", "K_inv", "mean", "var", "status")}
    for b in (range(len(H)) if rows is None else rows):
        ctx.set_warp(W[b])
        res = ctx.posterior(H[b:b + 1], want_alpha=True, want_K_inv=True)
        out["status"].append(res["status"][0])
        if res["status"][0] == 0:
            mean, var = ctx.predict(Hk[b:b + 1], Xq)
        else:
            mean = var = np.full((1, len(Xq)), np.nan)
        for k, v in (("lml", res["lml"]), ("alpha", res["alpha"]), ("K_inv", res["K_inv"]), ("mean", mean), ("var", var)):
            out[k].append(v[0])
    ctx.set_warp(None)
    return {k: np.array(v) for k, v in out.items()}


def _batched(ctx, H, Hk, W, Xq, B_predict=None):
    res = ctx.posterior(H, want_alpha=True, want_K_inv=True, warps=W)
    assert ctx.resident_H is None
    Bp = len(H) if B_predict is None else B_predict
    mean, var = ctx.predict_warped(Hk[:Bp], Xq)
    return {"lml": res["lml"], "alpha": res["alpha"], "K_inv": res["K_inv"], "mean": mean, "var": var, "status": res["status"]}


def _assert_same_bits(got, want, rows=None, keys=("lml", "alpha", "K_inv", "mean", "var")):
    for k in keys:
        g = got[k] if rows is None else got[k][rows]
        assert g.shape == want[k].shape, (k, g.shape, want[k].shape)
        assert np.array_equal(g, want[k]), "%s differs from the per-row form: max |d| %.3e" % (k, np.abs(g - want[k]).max())


def _shape_problem(n, d, m, B, stationary="matern52", form="product", seed=0, vec_alpha=False):
    X, y, alpha, H = P._problem(n, d, 4000 + seed, stationary, form, B, vec_alpha)
    rng = np.random.RandomState(4100 + seed)
    return X, y, alpha, H, rng.uniform(-0.7, 0.7, size=(B, 2 * d)), rng.uniform(size=(m, d))


# ------------------------------------------------------------------------------------------------------------------------------
# precision
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CIDS)
def test_every_row_meets_the_long_double_reference(lib, cid):
    hp = pytest.importorskip("oracle.hp_oracle")
    if not hp.available():
        pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference")
    c = P.ALL[cid]
    X, y, alpha, H, _ = P.problem(cid)
    W = P.warp_params(cid)
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=len(H))
    got = _batched(ctx, H, H, W, P.query(cid))
    ctx.close()
    assert np.all(got["status"] == 0)
    for b in range(len(H)):
        errs = WR.row_errs(cid, b, {q: got[q][b] for q in WR.QUANTITIES})
        for q, (e, t) in errs.items():
            print("PRECISION %-40s %-9s %-7s %-6s err/tol %.3e" % ("%s_row%d" % (cid, b), c["stationary"], c["form"], q, e / t))
        for q, (e, t) in errs.items():
            assert e <= t, "%s row %d %s: error %.3e > tol %.3e (%.1fx)" % (cid, b, q, e, t, e / t)


# ------------------------------------------------------------------------------------------------------------------------------
# bit for bit against the per-row form
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CIDS)
@pytest.mark.parametrize("noise_zero", [False, True])
def test_bits_of_the_per_row_form_warp_cases(lib, cid, noise_zero):
    c = P.ALL[cid]
    X, y, alpha, H, _ = P.problem(cid)
    W, Xq = P.warp_params(cid), P.query(cid)
    Hk = _noise_off(H) if noise_zero else H
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=len(H))
    got = _batched(ctx, H, Hk, W, Xq)
    again = _batched(ctx, H, Hk, W, Xq)  # two identical calls
    want = _per_row(ctx, H, Hk, W, Xq)
    ctx.close()
    assert np.all(got["status"] == 0) and np.all(want["status"] == 0)
    _assert_same_bits(got, want)
    _assert_same_bits(again, want)


SHAPES = [  # n, d, m: one point; the 128 tile and the 16-dimension staging at size + 1; every cross tile interior
    (1, 1, 1), (129, 17, 129), (128, 2, 128)]


@pytest.mark.parametrize("n,d,m", SHAPES)
def test_bits_of_the_per_row_form_tile_edges(lib, n, d, m):
    X, y, alpha, H, W, Xq = _shape_problem(n, d, m, 3, seed=n)
    ctx = lib.Context(X, y, alpha, max_batch=3)
    got = _batched(ctx, H, _noise_off(H), W, Xq)
    want = _per_row(ctx, H, _noise_off(H), W, Xq)
    ctx.close()
    assert np.all(got["status"] == 0)
    _assert_same_bits(got, want)


@pytest.mark.parametrize("stationary,form", P.FAMILIES)
def test_bits_of_the_per_row_form_every_family(lib, stationary, form):
    X, y, alpha, H, W, Xq = _shape_problem(65, 3, 33, 3, stationary, form, seed=7, vec_alpha=True)
    ctx = lib.Context(X, y, alpha, form=form, stationary=stationary, max_batch=3)
    got = _batched(ctx, H, H, W, Xq)
    want = _per_row(ctx, H, H, W, Xq)
    ctx.close()
    assert np.all(got["status"] == 0)
    _assert_same_bits(got, want)


def test_bits_with_two_build_chunks_and_fewer_predicted_than_resident(lib):
    X, y, alpha, H, W, Xq = _shape_problem(140, 2, 50, 3, seed=11)
    ctx = lib.Context(X, y, alpha, max_batch=2)  # the build runs as chunks of 2 + 1
    got = _batched(ctx, H, H, W, Xq)
    first2 = ctx.predict_warped(H[:2], Xq)  # 3 resident, 2 predicted
    want = _per_row(ctx, H, H, W, Xq)
    ctx.close()
    _assert_same_bits(got, want)
    assert np.array_equal(first2[0], want["mean"][:2]) and np.array_equal(first2[1], want["var"][:2])


def test_predict_chunk_boundary(lib):
    """CHUNK_CASE's shape with per-row warps: 1025 items at m = 8192 run as predict chunks of 1008 + 17 (and the warp of the queries
    as one launch over all 1025 parameter sets).  The items on both sides of the cut, the first and the last two equal their own
    single-row context-warp result bit for bit."""
    c = P.CHUNK_CASE
    X, y, alpha, H, _ = P.problem(c["id"])
    Xq = np.random.RandomState(c["seed"] + 2).uniform(size=(c["m"], c["d"]))  # (the Beta CDF is defined on [0, 1])
    W = np.random.RandomState(c["seed"] + 1).uniform(-0.7, 0.7, size=(c["B"], 2 * c["d"]))
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=c["B"])
    assert np.all(ctx.posterior(H, want_alpha=False, warps=W)["status"] == 0)
    mean, var = ctx.predict_warped(H, Xq)
    want = _per_row(ctx, H, H, W, Xq, rows=c["items"])
    ctx.close()
    assert np.array_equal(mean[c["items"]], want["mean"]) and np.array_equal(var[c["items"]], want["var"])


# ------------------------------------------------------------------------------------------------------------------------------
# state
# ------------------------------------------------------------------------------------------------------------------------------
def _refused_calls(lib, ctx, H, Xq):
    n, d = ctx.n, ctx.d
    kinds, params = [lib.ACQ_EI, lib.ACQ_LCB], [float("nan"), 1.96]
    z = np.zeros((1, len(Xq)))
    return {
        "bgp_predict_batch": lambda: ctx.predict(H, Xq),
        "bgp_acq_batch": lambda: ctx.acq(H, Xq, 0.0, 1.0, kinds, params, len(H)),
        "bgp_sample_y": lambda: ctx.sample_y(0, H[:1], Xq, z, 1e-8),
        "bgp_sample_y_batch": lambda: ctx.sample_y_batch([0], H[:1], Xq, z, 1e-8),
        "bgp_pvrs": lambda: ctx.pvrs(H[:1], Xq, Xq[:2]),
        "bgp_fantasy_begin": lambda: ctx.fantasy_begin(_noise_off(H), np.exp(H[:, -1]), Xq, 0.0, 1.0, kinds, params, len(H), 2),
        "bgp_predict_grad_batch": lambda: ctx.predict_grad(H, Xq),
        "bgp_minimize_starts": lambda: ctx.minimize_starts(0, H, 0.0, 1.0, 1.96, Xq[:2], 0.0, 1.0),
        "bgp_paths_begin": lambda: ctx.paths_begin([0], _noise_off(H[:1]), H[:1, -1], np.ones((1, 4, d)), np.zeros((1, 4)),
                                                   np.zeros((1, 5)), np.zeros((1, n))),
        "bgp_partial_dependence": lambda: ctx.partial_dependence(H, Xq[:4], [np.linspace(0.0, 1.0, 3)] * d, [(0,)]),
    }


def test_per_row_warped_posteriors_refuse_every_shared_input_consumer(lib):
    X, y, alpha, H, W, Xq = _shape_problem(70, 2, 9, 3, seed=21)
    fresh = lib.Context(X, y, alpha, max_batch=3)
    fresh.posterior(H)
    want = (fresh.posterior(H, want_K_inv=True), fresh.predict(H, Xq))
    fresh.close()
    ctx = lib.Context(X, y, alpha, max_batch=3)
    assert np.all(ctx.posterior(H, warps=W)["status"] == 0)
    for name, call in _refused_calls(lib, ctx, H, Xq).items():
        with pytest.raises(lib.BgpError, match=r"%s failed \(code 4\).*per-row warped" % name):
            call()
    ctx.predict_warped(H, Xq)  # (still served)
    got = (ctx.posterior(H, want_K_inv=True), ctx.predict(H, Xq))  # a plain build ends the state
    for k in ("lml", "alpha", "K_inv"):
        assert np.array_equal(got[0][k], want[0][k]), k
    assert np.array_equal(got[1][0], want[1][0]) and np.array_equal(got[1][1], want[1][1])
    with pytest.raises(lib.BgpError, match=r"bgp_predict_batch_warped failed \(code 4\)"):
        ctx.predict_warped(H, Xq)  # plainly built posteriors
    # ... and so do a context-level warp, new data and pvrs_prepare
    for end in (lambda: ctx.set_warp(W[0]), lambda: ctx.update_data(X, y, alpha), lambda: ctx.pvrs_prepare(H[:1], False)):
        ctx.set_warp(None)
        ctx.posterior(H, warps=W)
        end()
        with pytest.raises(lib.BgpError, match=r"bgp_predict_batch_warped failed \(code 4\)"):
            ctx.predict_warped(H[:1], Xq)
    ctx.set_warp(None)
    ctx.posterior(H, warps=W)
    with pytest.raises(lib.BgpError, match=r"bgp_predict_batch_warped failed \(code 4\)"):
        ctx.predict_warped(np.vstack([H, H[:1]]), Xq)  # more than resident
    ctx.close()


def test_a_context_level_warp_is_replaced_not_composed(lib):
    X, y, alpha, H, W, Xq = _shape_problem(70, 2, 9, 3, seed=22)
    ctx = lib.Context(X, y, alpha, max_batch=3)
    want = _batched(ctx, H, H, W, Xq)
    ctx.set_warp(W[2])
    got = _batched(ctx, H, H, W, Xq)
    ctx.close()
    _assert_same_bits(got, want)


def test_a_warped_lml_batch_between_build_and_predict_changes_no_bit(lib):
    X, y, alpha, H, W, Xq = _shape_problem(140, 2, 50, 3, seed=23)
    ctx = lib.Context(X, y, alpha, max_batch=3)
    want = _batched(ctx, H, H, W, Xq)
    ctx.posterior(H, warps=W)
    ctx.lml_warped(H[::-1], W[::-1] + 0.1)  # overwrites the LML batch's own per-walker inputs and parameters
    mean, var = ctx.predict_warped(H, Xq)
    ctx.close()
    assert np.array_equal(mean, want["mean"]) and np.array_equal(var, want["var"])


def test_a_row_that_is_not_positive_definite_fails_alone(lib):
    """The rows of tests/test_gpu_edge.py::test_mixed_failures_across_chunks: a duplicated training point (still duplicated behind
    any warp), no jitter, and no white noise on the bad rows."""
    from conftest import synth

    n, d = 140, 2
    X, y = synth(n, d, 66)
    X = np.clip(X, 0.0, 1.0)
    X[1] = X[0]
    good, bad = np.array([0.0, -1.0, -1.1, -3.0]), np.array([0.0, -1.0, -1.1, -np.inf])
    H = np.array([good, bad, good + 0.1, bad, bad, good - 0.1, good, bad, good + 0.2])
    isbad = np.array([0, 1, 0, 1, 1, 0, 0, 1, 0], dtype=bool)
    W = np.random.RandomState(67).uniform(-0.7, 0.7, size=(len(H), 2 * d))
    Xq = np.random.RandomState(68).uniform(size=(20, d))
    ctx = lib.Context(X, y, np.zeros(n), max_batch=4)
    got = _batched(ctx, H, H, W, Xq)
    rows = list(np.flatnonzero(~isbad))
    want = _per_row(ctx, H, H, W, Xq, rows=rows)
    ctx.close()
    assert np.all(got["status"][isbad] == 2) and np.all(got["status"][~isbad] == 0)
    assert np.all(want["status"] == 0)
    _assert_same_bits(got, want, rows=rows)


# ------------------------------------------------------------------------------------------------------------------------------
# BayesGPR / evaluate_acquisitions / Optimizer
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bask(lib):
    import bayes_skopt_amd as bask

    return bask


def _data(n, d, seed):
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(n, d))
    y = np.sin(9.0 * X[:, 0] ** 2) + X[:, -1] + 0.05 * rng.randn(n)
    return X, (y - y.mean()) / y.std()


@pytest.fixture(scope="module")
def warped_gp(bask):
    X, y = _data(40, 2, 31)
    gp = bask.BayesGPR(kernel=bask.construct_default_kernel([0, 1]), random_state=5, warp_inputs=True, normalize_y=True)
    gp.fit(X, y, n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
    assert gp.chain_.shape == (40, 4 + 4) and gp._post.canonical
    return gp


def _count_set_warp(gp):
    calls = []
    real = gp._ctx.set_warp

    def spy(w):
        calls.append(w)
        return real(w)

    gp._ctx.set_warp = spy
    return calls, lambda: setattr(gp._ctx, "set_warp", real)


@pytest.mark.parametrize("noise_zero", [True, False])
def test_predict_hyper_samples_takes_the_batched_path_with_the_loops_bits(bask, warped_gp, noise_zero):
    gp = warped_gp
    Xq = np.random.RandomState(32).uniform(size=(30, 2))
    rows = gp.chain_
    assert bask.BayesGPR._warp_rows_path == "auto"
    warpers = (gp.warp_alphas_.copy(), gp.warp_betas_.copy())
    before = gp.predict(Xq, return_std=True)
    calls, restore = _count_set_warp(gp)
    try:
        mus, stds = gp._predict_hyper_samples(rows, Xq, noise_zero=noise_zero)
        assert len(calls) == 0  # neither the estimator's warpers nor the context-level warp are touched
        assert np.array_equal(gp.warp_alphas_, warpers[0]) and np.array_equal(gp.warp_betas_, warpers[1])
        after = gp.predict(Xq, return_std=True)
        gp._warp_rows_path = "loop"
        mus_l, stds_l = gp._predict_hyper_samples(rows, Xq, noise_zero=noise_zero)
        assert len(calls) == len(rows) + 1  # every row's warp, then the estimator's own again
    finally:
        restore()
        del gp._warp_rows_path
    after_loop = gp.predict(Xq, return_std=True)  # (the loop keeps the median GP's posterior: DESIGN.md section 28)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(before[0], after_loop[0]) and np.array_equal(before[1], after_loop[1])
    assert mus.shape == (len(rows), len(Xq)) and np.all(np.isfinite(mus)) and np.all(stds > 0)
    assert np.array_equal(mus, mus_l) and np.array_equal(stds, stds_l)
    assert np.array_equal(gp.warp_alphas_, warpers[0]) and np.array_equal(gp.warp_betas_, warpers[1])


def test_acquisitions_keep_their_bits(bask, warped_gp):
    gp = warped_gp
    Xq = np.random.RandomState(33).uniform(size=(25, 2))
    acqs = [bask.acquisition.ExpectedImprovement(), bask.acquisition.LCB()]
    before = gp.predict(Xq, return_std=True)
    vals = bask.acquisition.evaluate_acquisitions(Xq, gp, acqs, n_samples=6, random_state=0)
    gp._warp_rows_path = "loop"
    try:
        vals_l = bask.acquisition.evaluate_acquisitions(Xq, gp, acqs, n_samples=6, random_state=0)
    finally:
        del gp._warp_rows_path
    after_loop = gp.predict(Xq, return_std=True)
    assert vals.shape == (2, 25) and np.all(np.isfinite(vals))
    assert np.array_equal(vals, vals_l)
    assert np.array_equal(before[0], after_loop[0]) and np.array_equal(before[1], after_loop[1])


def test_optimizer_proposes_the_same_points_on_both_paths(bask, monkeypatch):
    def run():
        rng = np.random.RandomState(0)
        opt = bask.Optimizer(dimensions=[(0.0, 1.0)] * 2, n_points=100, n_initial_points=4, init_strategy="r2",
                             gp_kwargs=dict(warp_inputs=True), acq_func="ei", random_state=0)
        asked, vals = [], []
        for _ in range(6):
            x = opt.ask()
            asked.append(x)
            opt.tell(x, float(np.sin(5 * x[0] ** 2) + x[1] + 0.01 * rng.randn()), n_samples=4, gp_samples=40, gp_burnin=2)
            if opt._last_acq_values is not None:
                vals.append(np.array(opt._last_acq_values))
        assert len(vals) == 3  # the averaged acquisition over the candidates of the tells that had a surrogate
        return np.array(asked + [opt.ask()]), np.array(vals)

    asked, vals = run()
    monkeypatch.setattr(bask.BayesGPR, "_warp_rows_path", "loop")
    asked_l, vals_l = run()
    assert np.array_equal(asked, asked_l) and np.array_equal(vals, vals_l)


@pytest.fixture(scope="module")
def generic_gp(bask):
    from sklearn.gaussian_process import kernels as sk

    X, y = _data(30, 1, 34)
    kernel = sk.Matern(length_scale=0.4, nu=2.5) + sk.Matern(length_scale=1.5, nu=1.5)
    gp = bask.BayesGPR(kernel=kernel, random_state=2, warp_inputs=True)
    gp.fit(X, y, n_desired_samples=20, n_burnin=2, n_walkers_per_thread=10, progress=False)
    assert gp._generic and not gp._post.canonical and gp.chain_.shape == (20, 3 + 2)
    return gp


def test_a_generic_kernel_tree_keeps_the_loop(generic_gp):
    gp = generic_gp
    rows = gp.chain_[:3]
    calls, restore = _count_set_warp(gp)
    try:
        mus, stds = gp._predict_hyper_samples(rows, np.linspace(0.05, 0.95, 7)[:, None])
    finally:
        restore()
    assert len(calls) == len(rows) + 1
    assert mus.shape == (3, 7) and np.all(np.isfinite(mus)) and np.all(stds > 0)


# ------------------------------------------------------------------------------------------------------------------------------
# the median GP's posterior survives every walk over chain rows under their own warps
# ------------------------------------------------------------------------------------------------------------------------------
def _median_state(gp, Xq):
    assert gp._post_theta is not None
    return {"post_theta": gp._post_theta.copy(), "alpha_": gp.alpha_.copy(), "warp_alphas_": gp.warp_alphas_.copy(),
            "warp_betas_": gp.warp_betas_.copy(), **dict(zip(("mean", "std"), gp.predict(Xq, return_std=True)))}


def _assert_median_state(gp, Xq, before):
    after = _median_state(gp, Xq)
    for k in before:
        assert np.array_equal(before[k], after[k]), k


def _on_the_loop(gp, call):
    gp._warp_rows_path = "loop"
    try:
        return call()
    finally:
        del gp._warp_rows_path


def _acqs(bask, gp, Xq):
    acqs = [bask.acquisition.ExpectedImprovement(), bask.acquisition.LCB()]
    return bask.acquisition.evaluate_acquisitions(Xq, gp, acqs, n_samples=6, random_state=0)


_GRID = np.linspace(0.1, 0.9, 4)
SURVIVES = {  # name: (fixture, the call on (bask, gp, Xq))
    "canonical-predict_hyper_samples-loop": ("warped_gp", lambda bask, gp, Xq: _on_the_loop(
        gp, lambda: gp._predict_hyper_samples(gp.chain_, Xq))),
    "canonical-evaluate_acquisitions-loop": ("warped_gp", lambda bask, gp, Xq: _on_the_loop(gp, lambda: _acqs(bask, gp, Xq))),
    "canonical-partial_dependence": ("warped_gp", lambda bask, gp, Xq: gp.partial_dependence(
        Xq[:5], [_GRID] * 2, thetas=gp.chain_[:3])),
    "canonical-sensitivity": ("warped_gp", lambda bask, gp, Xq: gp.sensitivity(Xq[:8], Xq[8:16], thetas=gp.chain_[:3])),
    "canonical-sample_y-reference": ("warped_gp", lambda bask, gp, Xq: gp.sample_y(
        Xq, sample_mean=False, n_samples=3, random_state=0, mvn="reference")),
    "canonical-sample_y-cholesky": ("warped_gp", lambda bask, gp, Xq: gp.sample_y(
        Xq, sample_mean=False, n_samples=3, random_state=0, mvn="cholesky")),
    "canonical-kg-host": ("warped_gp", lambda bask, gp, Xq: bask.acquisition.KnowledgeGradient()(
        Xq, gp, n_reference=5, n_gp_samples=3, random_state=0, return_path=True)),
    "generic-predict_hyper_samples": ("generic_gp", lambda bask, gp, Xq: gp._predict_hyper_samples(gp.chain_, Xq)),
    "generic-cross_validate": ("generic_gp", lambda bask, gp, Xq: gp.cross_validate(thetas=gp.chain_, n_folds=3, random_state=0)),
    "generic-partial_dependence": ("generic_gp", lambda bask, gp, Xq: gp.partial_dependence(Xq[:5], [_GRID], thetas=gp.chain_)),
    "generic-evaluate_acquisitions": ("generic_gp", _acqs),
}


@pytest.mark.parametrize("case", list(SURVIVES))
def test_the_median_posterior_survives(bask, request, case):
    fixture, call = SURVIVES[case]
    gp = request.getfixturevalue(fixture)
    Xq = np.random.RandomState(35).uniform(0.02, 0.98, size=(16, gp._X_train_.shape[1]))
    before = _median_state(gp, Xq)
    calls, restore = _count_set_warp(gp)
    try:
        out = call(bask, gp, Xq)  # (raises nothing)
    finally:
        restore()
    assert len(calls) >= 2  # the case did walk rows under their own warps: at least one row's, then the estimator's own again
    assert case != "canonical-kg-host" or out[1] == "host"
    _assert_median_state(gp, Xq, before)


def test_an_exception_inside_the_row_walk_leaves_the_estimator_as_it_was(warped_gp):
    gp = warped_gp
    Xq = np.random.RandomState(36).uniform(size=(9, 2))
    before = _median_state(gp, Xq)
    with pytest.raises(ZeroDivisionError):
        with gp._row_warps() as install:
            install(gp.chain_[0])
            assert gp._post_theta is None and not np.array_equal(gp.warp_alphas_, before["warp_alphas_"])
            1 / 0
    _assert_median_state(gp, Xq, before)
