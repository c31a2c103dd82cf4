"""The minimiser of a pathwise posterior draw on the device (bgp_paths_minimize, PosteriorPaths.minimize,
Optimizer.optimum_samples, optimum_intervals(method="pathwise")): the whole-workgroup evaluator against the
long-double reference of tests/_pathref.py at its tolerance class, the search on the inputs tests/test_cpu_paths_minimize_reference.py
qualifies, bitwise determinism and independence of a (path, start), the caps, the errors, the Python layers.
Lines start with ``PRECISION`` / ``PATHMIN``.

Measured on the device: evaluator, ten cases: worst err / tol 4.3e-5 (value), 2.6e-4 (gradient).  Search, seven cases: 48 of 52
pairs converged (4 of the d = 32 RBF case stop at max_iter), evaluations per pair mean 170, max 2 067; worst projected gradient at
a converged end point 9.9e-6; end points against the long-double path at most 3.1e-5 tol (value), 2.0e-4 tol (gradient)."""
import functools

import numpy as np
import pytest

import _pathmin as M
import _pathref as R
from conftest import synth

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)


@pytest.fixture(scope="module")
def bask():
    import bayes_skopt_amd as bask

    assert bask._lib.device_count() >= 1
    return bask


def _check(tag, quantity, err, t):
    print("PRECISION %-52s %-6s err/tol %.3e" % (tag, quantity, err / t))
    assert err <= t, "%s %s: error %.3e > tol %.3e (%.1fx)" % (tag, quantity, err, t, err / t)


def _begin(bask, cid):
    """A context with the case's posteriors resident and its paths begun; returns (ctx, problem dict)."""
    from bayes_skopt_amd._posterior import noise_off

    c, pr = R.ALL[cid], R.problem(cid)
    ctx = bask._lib.Context(pr["X"], pr["y"], pr["alpha"], form=c["form"], stationary=c["stationary"], max_batch=2)
    assert np.all(ctx.posterior(pr["H"])["status"] == 0)
    Hp = pr["H"][pr["pidx"]]
    ctx.paths_begin(pr["pidx"], noise_off(Hp), Hp[:, -1], pr["omega"], pr["phase"], pr["w"], pr["eps"])
    return ctx, pr


# ---- 1. the evaluator against the extended-precision reference -------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES])
def test_evaluator_against_the_extended_precision_reference(bask, cid):
    """max_iter = 0: every query row of the case is a start of every path, nothing is clipped, nothing moves."""
    c = R.ALL[cid]
    ctx, pr = _begin(bask, cid)
    X0 = np.ascontiguousarray(np.broadcast_to(pr["Xq"][None], (c["P"], c["m"], c["d"])))
    out = ctx.paths_minimize(X0, -0.5, 1.5, max_iter=0, want_grad=True)
    ctx.close()
    np.testing.assert_array_equal(out["x"], X0)
    assert np.all(out["iters"] == 0) and np.all(out["evals"] == 1)
    assert out["fun"].shape == (c["P"], c["m"]) and out["grad"].shape == (c["P"], c["m"], c["d"])
    assert np.all(np.isfinite(out["fun"])) and np.all(np.isfinite(out["grad"]))
    ev, eg = R.err(out["fun"], out["grad"], R.ref_paths(cid))
    _check(cid, "f", ev, R.case_tol(cid))
    _check(cid, "df", eg, R.case_tol(cid))


# ---- 2. the search ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _search(cid):
    """The search of one case from the qualified starts, computed once: (start evaluation, search result, the gradient of
    ``bgp_paths_eval`` at every end point (P, S, d))."""
    import bayes_skopt_amd as bask

    c = R.ALL[cid]
    ctx, _pr = _begin(bask, cid)
    X0 = M.starts(cid)
    start = ctx.paths_minimize(X0, M.LO, M.HI, max_iter=0, want_grad=True)
    out = ctx.paths_minimize(X0, M.LO, M.HI, gtol=M.GTOL, max_iter=M.MAX_ITER, want_grad=True)
    witness = np.empty_like(out["x"])
    for p in range(c["P"]):
        witness[p] = ctx.paths_eval(out["x"][p], want_grad=True)[1][p]
    ctx.close()
    return start, out, witness


@pytest.mark.parametrize("cid", M.SEARCH_CASES)
def test_search_from_the_qualified_starts(bask, cid):
    c = R.ALL[cid]
    start, out, witness = _search(cid)
    x, f, st = out["x"], out["fun"], out["status"]
    assert x.shape == (c["P"], M.N_STARTS, c["d"]) and np.all(x >= M.LO) and np.all(x <= M.HI)
    assert set(np.unique(st)) <= {0, 1, 2}
    np.testing.assert_array_equal(start["x"], M.starts(cid))
    # Armijo in the evaluator's own arithmetic: never above the start, strictly below wherever the start is not stationary
    pg0 = M.projected_gradient(start["x"], start["grad"])
    assert np.all(f <= start["fun"]), (f - start["fun"]).max()
    assert np.all(f[pg0 > M.GTOL] < start["fun"][pg0 > M.GTOL])
    # converged pairs: the projected gradient from bgp_paths_eval's gradient there (the other kernels are the witness)
    pgw = M.projected_gradient(x, witness)
    worst = float(pgw[st == 0].max()) if np.any(st == 0) else 0.0
    print("PATHMIN %-48s converged %d / %d  status %s  iters max %d  evals mean %.1f max %d  worst |pg| %.2e  decrease min %.2e"
          % (cid, int(np.sum(st == 0)), st.size, np.bincount(st.ravel(), minlength=3).tolist(), out["iters"].max(),
             out["evals"].mean(), out["evals"].max(), worst, (start["fun"] - f).min()))
    assert worst <= 2 * M.GTOL
    # the end points' values and gradients against the long-double path
    t = R.case_tol(cid)
    for p in range(c["P"]):
        rf, rdf, s, sg = M.path_at(cid, p, hp.LD, R._solve_ld, x[p])
        ref = {"f": rf, "df": rdf, "s": np.asarray(s, dtype=np.float64), "sg": np.asarray(sg, dtype=np.float64)}
        ev, eg = R.err(f[p], out["grad"][p], ref)
        _check("%s path %d end points" % (cid, p), "f", ev, t)
        _check("%s path %d end points" % (cid, p), "df", eg, t)


def test_at_most_five_pairs_do_not_converge(bask):
    """The fp64 reference (scipy L-BFGS-B, tests/test_cpu_paths_minimize_reference.py) converges from all 52 pairs."""
    status = np.concatenate([_search(cid)[1]["status"].ravel() for cid in M.SEARCH_CASES])
    evals = np.concatenate([_search(cid)[1]["evals"].ravel() for cid in M.SEARCH_CASES])
    print("PATHMIN all cases: status %s of %d pairs, evals mean %.1f max %d"
          % (np.bincount(status, minlength=3).tolist(), status.size, evals.mean(), evals.max()))
    assert status.size == M.N_PAIRS
    assert int(np.sum(status != 0)) <= 5, status


# ---- 3. bits ----------------------------------------------------------------------------------------------------------------
def test_determinism_and_independence_of_a_pair(bask):
    cid = R.CASES[4]["id"]  # three paths on two posteriors, F = 200, n = 130
    ctx, _pr = _begin(bask, cid)
    X0 = M.starts(cid)
    kw = dict(gtol=M.GTOL, max_iter=M.MAX_ITER, want_grad=True)
    a = ctx.paths_minimize(X0, M.LO, M.HI, **kw)
    b = ctx.paths_minimize(X0, M.LO, M.HI, **kw)
    first = ctx.paths_minimize(X0[:, :2], M.LO, M.HI, **kw)
    ctx.close()
    for key in ("x", "fun", "grad", "iters", "evals", "status"):
        np.testing.assert_array_equal(a[key], b[key])
        np.testing.assert_array_equal(a[key][:, :2], first[key])
    assert np.any(a["iters"] > 0)


# ---- 4. caps ----------------------------------------------------------------------------------------------------------------
def test_every_loop_is_capped(bask):
    cid = R.CASES[9]["id"]
    ctx, _pr = _begin(bask, cid)
    out = ctx.paths_minimize(M.starts(cid), M.LO, M.HI, gtol=M.GTOL, max_iter=3)
    ctx.close()
    assert np.all(out["iters"] <= 3) and np.all(out["evals"] <= 2 + 3 * 30)
    assert np.all(out["iters"][out["status"] == 1] == 3)
    assert np.all(out["x"] >= M.LO) and np.all(out["x"] <= M.HI) and out["grad"] is None


# ---- 5. errors ----------------------------------------------------------------------------------------------------------------
def test_states_and_arguments_are_errors_not_crashes(bask):
    lib = bask._lib
    X, y = synth(40, 2, 3)
    h = np.array([0.0, np.log(0.4), np.log(0.4), np.log(1e-2)])
    hk = np.array([0.0, np.log(0.4), np.log(0.4), -np.inf])
    om, ph, w, eps = R.draw_variates(np.random.RandomState(1), 1, 8, 2, 40, "matern52")
    X0 = np.random.RandomState(2).uniform(size=(1, 3, 2))
    ctx = lib.Context(X, y, 1e-8, max_batch=1)
    with pytest.raises(lib.BgpError, match=r"code 4.*bgp_paths_begin first"):
        ctx.paths_minimize(X0, 0.0, 1.0)
    ctx.posterior(h[None])
    ctx.paths_begin([0], hk[None], h[-1:], om, ph, w, eps)
    with pytest.raises(lib.BgpError, match=r"code 1.*S >= 1"):
        ctx.paths_minimize(np.empty((1, 0, 2)), 0.0, 1.0)
    with pytest.raises(lib.BgpError, match=r"code 1.*max_iter >= 0"):
        ctx.paths_minimize(X0, 0.0, 1.0, max_iter=-1)
    with pytest.raises(lib.BgpError, match=r"code 1.*empty box"):
        ctx.paths_minimize(X0, 1.0, 0.0)
    a = ctx.paths_minimize(X0, 0.0, 1.0, want_grad=True)
    assert np.all(a["x"] >= 0.0) and np.all(a["x"] <= 1.0) and np.all(a["fun"] <= ctx.paths_minimize(X0, 0.0, 1.0, max_iter=0)["fun"])
    ctx.posterior(h[None] + 0.05)  # the paths do not read the resident posteriors
    b = ctx.paths_minimize(X0, 0.0, 1.0, want_grad=True)
    for key in ("x", "fun", "grad", "iters", "evals", "status"):
        np.testing.assert_array_equal(a[key], b[key])
    assert ctx.paths_stats() == {"begins": 1, "evals": 0}
    ctx.paths_end()
    with pytest.raises(lib.BgpError, match="code 4"):
        ctx._paths_P = 1
        ctx.paths_minimize(X0, 0.0, 1.0)
    ctx.close()


# ---- 6. Python ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def surrogate(bask):
    """(gp, space) of the n = 60, d = 3 surrogate of tests/test_gpu_optimum.py, on a box that is not the unit box."""
    from bayes_skopt_amd.space import Space

    n, d = 60, 3
    rng = np.random.RandomState(100 + n)
    space = Space([(-2.0, 3.0)] * d)
    Xt = rng.uniform(size=(n, d))
    y = np.sin(3.0 * Xt.sum(axis=1)) + np.sum((Xt - 0.4) ** 2, axis=1) + 0.5 * np.cos(7.0 * Xt[:, 0]) + 0.05 * rng.randn(n)
    gp = bask.BayesGPR(kernel=bask.construct_default_kernel(list(range(d))), normalize_y=True, random_state=1)
    gp.fit(Xt, y, n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
    return gp, space


def test_posterior_paths_minimize(bask, surrogate):
    gp, _space = surrogate
    kw = dict(n_candidates=300, n_starts=4, random_state=5)
    with gp.sample_paths(n_paths=6, n_features=128, random_state=11) as paths:
        out = paths.minimize(**kw)
        again = paths.minimize(**kw)
        cand = np.random.RandomState(5).uniform(size=(300, 3))  # (the documented consumption: one uniform call)
        rows = paths(cand)
        raw = paths._ctx.paths_minimize(out["x_all"], 0.0, 1.0, max_iter=0)
        given = paths.minimize(X0=cand[:4])
        boxed = paths.minimize(bounds=(np.full(3, 0.25), [0.5, 0.75, 0.3]), **kw)
    assert out["x"].shape == (6, 3) and out["fun"].shape == (6,) and out["x_all"].shape == (6, 4, 3)
    assert all(out[k].shape == (6, 4) for k in ("fun_all", "status", "iters", "evals")) and out["best"].shape == (6,)
    assert np.all(out["x_all"] >= 0.0) and np.all(out["x_all"] <= 1.0)
    # better than the argmin over the rows, for every path
    assert np.all(out["fun"] <= rows.min(axis=0)), (out["fun"] - rows.min(axis=0)).max()
    print("PATHMIN minimize: below the lowest of 300 rows by %.3e .. %.3e (y units)"
          % ((rows.min(axis=0) - out["fun"]).min(), (rows.min(axis=0) - out["fun"]).max()))
    # y units, and the best start
    ym, ys = float(np.ravel(gp.y_train_mean_)[0]), float(np.ravel(gp.y_train_std_)[0])
    np.testing.assert_array_equal(out["fun_all"], ys * raw["fun"] + ym)
    np.testing.assert_array_equal(raw["x"], out["x_all"])
    np.testing.assert_array_equal(out["best"], np.argmin(out["fun_all"], axis=1))
    np.testing.assert_array_equal(out["fun"], out["fun_all"].min(axis=1))
    np.testing.assert_array_equal(out["x"], out["x_all"][np.arange(6), out["best"]])
    for key in out:
        np.testing.assert_array_equal(out[key], again[key])
    assert given["x_all"].shape == (6, 4, 3) and np.all(given["status"] <= 2)
    assert np.all(boxed["x_all"] >= 0.25) and np.all(boxed["x_all"] <= np.array([0.5, 0.75, 0.3]))
    with pytest.raises(RuntimeError):
        paths.minimize()


@pytest.fixture(scope="module")
def optimizer(bask):
    opt = bask.Optimizer(dimensions=[(-2.0, 2.0), (0, 10)], n_initial_points=6, random_state=0)
    opt.run(lambda x: float(np.sin(2.0 * x[0]) + 0.05 * (x[1] - 4) ** 2), n_iter=12, n_samples=1, gp_samples=40, gp_burnin=5)
    return opt


def test_optimizer_optimum_samples_and_pathwise_intervals(bask, optimizer):
    from bayes_skopt_amd.utils import hdi

    opt = optimizer
    kw = dict(n_samples=20, n_features=128, n_candidates=200, n_starts=4)
    X_opt, values = opt.optimum_samples(random_state=3, **kw)
    X2, v2 = opt.optimum_samples(random_state=3, **kw)
    assert X_opt.shape == (20, 2) and values.shape == (20,) and np.all(np.isfinite(values))
    assert np.all(X_opt[:, 0] >= -2.0) and np.all(X_opt[:, 0] <= 2.0) and np.all(X_opt[:, 1] >= 0.0) and np.all(X_opt[:, 1] <= 10.0)
    assert np.any(X_opt[:, 1] != np.round(X_opt[:, 1]))  # (un-rounded, as expected_optimum's point)
    np.testing.assert_array_equal(X_opt, X2)
    np.testing.assert_array_equal(values, v2)
    Xc, _ = opt.optimum_samples(only_mean=False, random_state=3, **kw)
    assert Xc.shape == (20, 2) and not np.array_equal(Xc, X_opt)
    iv = opt.optimum_intervals(opt_samples=20, space_samples=200, random_state=3, method="pathwise")
    assert len(iv) == 2
    for (low, high), ivd in zip([(-2.0, 2.0), (0.0, 10.0)], iv):
        ivd = np.atleast_2d(np.asarray(ivd, dtype=np.float64))
        assert ivd.shape[1] == 2 and np.all(ivd >= low) and np.all(ivd <= high) and np.all(ivd[:, 0] <= ivd[:, 1])
    # the default is the positional call of before: the reference's samples, restated here, with the same seed
    X = opt.space.transform(opt.space.rvs(n_samples=100, random_state=3))
    draws = opt.gp.sample_y(X, sample_mean=True, n_samples=30, random_state=3)
    want = [opt.space.dimensions[i].inverse_transform(hdi(col, hdi_prob=0.9, multimodal=True))
            for i, col in enumerate(X[np.argmin(draws, axis=0)].T)]
    for got in (opt.optimum_intervals(0.9, True, 30, 100, True, 3),
                opt.optimum_intervals(hdi_prob=0.9, opt_samples=30, space_samples=100, random_state=3, method="argmin")):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(np.asarray(g), np.asarray(w))
    with pytest.raises(ValueError, match="method"):
        opt.optimum_intervals(method="paths")
    cat = bask.Optimizer(dimensions=[(0.0, 1.0), ["a", "b"]], n_initial_points=3, random_state=0)
    with pytest.raises(ValueError, match="categorical"):
        cat.optimum_samples()


def test_pathwise_intervals_fall_back_with_one_line(bask, capfd, monkeypatch):
    from bayes_skopt_amd import optimizer as O

    monkeypatch.setattr(O, "_intervals_told", [])
    opt = bask.Optimizer(dimensions=[(-1.0, 1.0)], n_initial_points=5, random_state=0,
                         gp_kwargs=dict(warp_inputs=True, normalize_y=True))
    opt.run(lambda x: float(np.sin(3.0 * x[0])), n_iter=8, n_samples=1, gp_samples=40, gp_burnin=2)
    capfd.readouterr()
    kw = dict(opt_samples=20, space_samples=50, random_state=2)
    a = opt.optimum_intervals(method="pathwise", **kw)
    b = opt.optimum_intervals(method="pathwise", **kw)
    c = opt.optimum_intervals(method="argmin", **kw)
    err = capfd.readouterr().err
    assert err.count("optimum_intervals(method='pathwise'): not available for warped inputs") == 1, err
    for x, y in ((a, c), (b, c)):
        assert len(x) == len(y) == 1
        np.testing.assert_array_equal(np.asarray(x[0]), np.asarray(y[0]))
    with pytest.raises(ValueError, match="warped inputs"):
        opt.optimum_samples(n_samples=2)
