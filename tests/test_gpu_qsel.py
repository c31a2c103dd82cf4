"""Joint batch selection on pathwise draws on the device (``bgp_paths_select``, ``PosteriorPaths.select_batch``,
``Optimizer.ask(strategy="joint_ei" | "thompson", pending=...)``).

The C-ABI is driven through ``_lib.Context`` on the cases of tests/_qselref.py -- m = 1, 2, either side of 64 (the values kernel's
workgroup) and of 256 (the evaluator's), 513; P = 1, 2, either side of 64 and of 256 (the LDS tile of incumbents); n = 1, 65; d = 1,
8, 32; RBF and Matern 5/2 in both forms; duplicate candidate rows, a candidate that is a training point -- and held BIT FOR BIT to
the host restatement ``_qselref.select`` fed with the same state's ``paths_eval`` at the candidates and at the training inputs:
picks, step values and incumbents, with forced picks at index 0 and m - 1 and q = m - n_forced (the last pick is the only
candidate left), for both kinds and both incumbents.  Then the independence of a value from what shares its call, the state left
untouched, the error codes, and the Python layer."""
import ctypes

import numpy as np
import pytest

import _qselref as Q

pytestmark = pytest.mark.gpu

CIDS = [c["id"] for c in Q.CASES]


@pytest.fixture(scope="module")
def bask():
    import bayes_skopt_amd as bask

    assert bask._lib.device_count() >= 1
    return bask


def _begin(bask, cid):
    """A context with the case's posterior resident and its P paths begun; (ctx, problem)."""
    c, pr = Q.ALL[cid], Q.problem(cid)
    ctx = bask._lib.Context(pr["X"], pr["y"], pr["alpha"], form=c["form"], stationary=c["stationary"], max_batch=1)
    assert np.all(ctx.posterior(pr["h"][None])["status"] == 0)
    hk = pr["h"].copy()
    hk[-1] = -np.inf
    P = c["P"]
    ctx.paths_begin(np.zeros(P, dtype=np.int32), np.tile(hk, (P, 1)), np.full(P, pr["h"][-1]), pr["omega"], pr["phase"], pr["w"],
                    pr["eps"])
    return ctx, pr


def _forced(m):
    return [0, m - 1] if m >= 3 else []


# ---- 1. bit for bit against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CIDS)
def test_picks_values_and_incumbents_are_the_restatement_bit_for_bit(bask, cid):
    c = Q.ALL[cid]
    ctx, pr = _begin(bask, cid)
    m, P = c["m"], c["P"]
    try:
        F, _ = ctx.paths_eval(pr["Xc"])
        FX, _ = ctx.paths_eval(pr["X"])
        inc_ref = FX.min(axis=1)
        forced = _forced(m)
        q = m - len(forced)  # every candidate is chosen in the end: the last pick is the only one left
        for kind in ("improvement", "thompson"):  # (Thompson with q > P wherever m - n_forced > P: the path index wraps)
            picks, values, inc = ctx.paths_select(pr["Xc"], q, kind=kind, forced=forced)
            rp, rv = Q.select(F, inc_ref, forced, q, kind)
            assert np.array_equal(inc, inc_ref), kind
            assert np.array_equal(picks, rp), kind
            assert np.array_equal(values, rv), kind
            assert sorted(list(picks) + forced) == list(range(m))
            again = ctx.paths_select(pr["Xc"], q, kind=kind, forced=forced)  # two identical calls agree
            assert all(np.array_equal(a, b) for a, b in zip(again, (picks, values, inc)))
            bare, none_v, none_i = ctx.paths_select(pr["Xc"], q, kind=kind, forced=forced, want_values=False, want_incumbents=False)
            assert none_v is None and none_i is None and np.array_equal(bare, picks)  # NULL outputs change no pick
        # a scalar incumbent inside the range of the draws, no forced picks, a short batch
        y_opt = float(np.median(F))
        q2 = min(3, m)
        picks, values, inc = ctx.paths_select(pr["Xc"], q2, incumbent=y_opt)
        rp, rv = Q.select(F, np.full(P, y_opt), [], q2, "improvement")
        assert np.all(inc == y_opt) and np.array_equal(picks, rp) and np.array_equal(values, rv)
        # ... and one below every value: all values exactly 0, the picks are the lowest unchosen indices in order
        picks, values, _ = ctx.paths_select(pr["Xc"], q, incumbent=float(F.min()) - 1.0, forced=forced)
        assert np.all(values == 0.0) and list(picks) == [i for i in range(m) if i not in forced]
        # the state is as it was
        F2, _ = ctx.paths_eval(pr["Xc"])
        assert np.array_equal(F2, F)
    finally:
        ctx.close()


def test_chosen_rows_twins_and_monotone_values_on_the_device(bask):
    """Exact zeros and exact monotonicity hold for the device's own numbers (case 2: duplicate rows 2 = 5 = m - 1)."""
    cid = CIDS[2]
    ctx, pr = _begin(bask, cid)
    try:
        picks, values, _ = ctx.paths_select(pr["Xc"], 12, forced=[2])
    finally:
        ctx.close()
    m = Q.ALL[cid]["m"]
    assert np.all(values[:, [2, 5, m - 1]] == 0.0)
    assert np.all(values >= 0.0) and np.all(values[1:] <= values[:-1])
    for j, p in enumerate(picks):
        assert np.all(values[j + 1 :, p] == 0.0)
    assert values[0].max() > 0.0


# ---- 2. a value depends on its own column alone ------------------------------------------------------------------------------
def test_a_step_0_value_is_the_same_alone_and_in_a_crowd_and_under_a_permutation(bask):
    cid = CIDS[4]  # m = 257, P = 65, n = 65
    ctx, pr = _begin(bask, cid)
    try:
        Xc = pr["Xc"]
        _, values, inc = ctx.paths_select(Xc, 1)
        for i in (0, 63, 64, 255, 256):
            _, alone, inc1 = ctx.paths_select(Xc[i : i + 1], 1)
            assert alone[0, 0] == values[0, i] and np.array_equal(inc1, inc)
        perm = np.random.RandomState(0).permutation(len(Xc))
        _, vperm, _ = ctx.paths_select(Xc[perm], 1)
        assert np.array_equal(vperm[0], values[0][perm])
    finally:
        ctx.close()


# ---- 3. the estimator's context is left alone ----------------------------------------------------------------------------------
def test_select_batch_leaves_the_estimator_as_it_was(bask):
    from bayes_skopt_amd.kernels import ConstantKernel, Matern

    rng = np.random.RandomState(3)
    X = rng.uniform(size=(30, 2))
    y = 5.0 + 3.0 * (np.sin(3.0 * X.sum(axis=1)) + 0.05 * rng.randn(30))
    gp = bask.BayesGPR(kernel=ConstantKernel(1.0, (0.1, 2.0)) * Matern([0.4, 0.3], (0.2, 0.8), nu=2.5), random_state=0,
                       normalize_y=True)
    gp.fit(X, y, n_desired_samples=20, n_burnin=3, n_walkers_per_thread=10, progress=False)
    Xq = rng.uniform(size=(40, 2))
    before = gp.predict(Xq, return_std=True)
    with gp.sample_paths(n_paths=5, n_features=32, random_state=1) as paths:
        f = paths(Xq)
        out = paths.select_batch(Xq, 4, return_values=True)
        lean = paths.select_batch(Xq, 4)
        ts = paths.select_batch(Xq, 7, kind="thompson", return_values=True)
        fixed = paths.select_batch(Xq, 2, incumbent=float(np.median(y)), return_values=True)
        fX = paths(X)
        Fn, _ = paths._ctx.paths_eval(Xq)  # (normalised-y units: the bits the device selects on)
        FXn, _ = paths._ctx.paths_eval(gp._X_train_)
        assert np.array_equal(paths(Xq), f)
        with pytest.raises(ValueError, match="kind"):
            paths.select_batch(Xq, 2, kind="ucb")
        with pytest.raises(ValueError, match="incumbent"):
            paths.select_batch(Xq, 2, incumbent="best")
    after = gp.predict(Xq, return_std=True)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    ym, ys = float(np.ravel(gp.y_train_mean_)[0]), float(np.ravel(gp.y_train_std_)[0])
    assert lean["values"] is None and np.array_equal(lean["picks"], out["picks"])
    assert out["values"].shape == (4, 40) and out["incumbents"].shape == (5,) and len(set(out["picks"])) == 4
    # y units: the incumbents are the paths' minima over the training inputs, the Thompson values are minus the paths
    np.testing.assert_allclose(out["incumbents"], fX.min(axis=0), rtol=1e-13)
    np.testing.assert_allclose(ts["values"][6], -f[:, 6 % 5], rtol=1e-13)
    rp, rv = Q.select(Fn, FXn.min(axis=1), [], 4, "improvement")
    assert np.array_equal(rp, out["picks"]) and np.array_equal(out["values"], ys * rv)
    assert np.array_equal(out["incumbents"], ys * FXn.min(axis=1) + ym)
    assert np.all(np.abs(fixed["incumbents"] - np.median(y)) <= 1e-12 * abs(np.median(y)))
    for j in range(7):  # pick j is path j's argmin among the rows not yet chosen
        left = [i for i in range(40) if i not in list(ts["picks"][:j])]
        assert ts["picks"][j] == left[int(np.argmin(f[left, j % 5]))]


# ---- 4. states and limits are error codes ---------------------------------------------------------------------------------------
def test_states_and_limits_are_errors_not_crashes(bask, monkeypatch):
    lib = bask._lib
    cid = CIDS[1]  # m = 2, P = 2
    pr = Q.problem(cid)
    ctx = lib.Context(pr["X"], pr["y"], pr["alpha"], form="sum", stationary="rbf", max_batch=1)
    with pytest.raises(lib.BgpError, match=r"code 4.*bgp_paths_begin first"):
        ctx.paths_select(pr["Xc"], 1)
    ctx.close()
    ctx, pr = _begin(bask, CIDS[2])  # m = 255, P = 63
    try:
        Xc, m = pr["Xc"], 255
        good = ctx.paths_select(Xc, 3, forced=[4])
        for kw in (dict(q=0), dict(q=-1), dict(q=m + 1), dict(q=m, forced=[1]), dict(q=2, forced=[m]), dict(q=2, forced=[-1]),
                   dict(q=2, forced=[7, 7]), dict(q=2, kind=2), dict(q=2, kind=-1), dict(q=2, incumbent=float("nan")),
                   dict(q=2, incumbent=float("inf"))):
            with pytest.raises(lib.BgpError, match="code 1"):
                ctx.paths_select(Xc, **kw)
        # incumbent out of range and m < 1 cannot be said through the binding: the C entry point itself
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
        picks = np.zeros(2, dtype=np.int32)
        Xd = np.ascontiguousarray(Xc)

        def raw(m_, kind, incumbent, q):
            return ctx._lib.bgp_paths_select(ctx._h, m_, Xd.ctypes.data_as(dp), kind, incumbent, 0.0, 0, ctypes.cast(None, ip), q,
                                             picks.ctypes.data_as(ip), ctypes.cast(None, dp), ctypes.cast(None, dp))

        assert raw(m, 0, 2, 2) == 1 and raw(m, 0, -1, 2) == 1 and raw(0, 0, 1, 1) == 1 and raw(-3, 0, 1, 1) == 1
        assert raw(m, 0, 1, 2) == 0
        # the size limit of the resident draw matrix, at the binding: a real small array, a patched limit
        monkeypatch.setattr(lib, "SELECT_MAX_DOUBLES", 63 * 256 - 1)
        with pytest.raises(ValueError, match="resident draw matrix"):
            ctx.paths_select(Xc, 1)
        monkeypatch.setattr(lib, "SELECT_MAX_DOUBLES", 63 * 256)
        ctx.paths_select(Xc, 1)
        monkeypatch.undo()
        # the context is usable afterwards, with the same results
        again = ctx.paths_select(Xc, 3, forced=[4])
        assert all(np.array_equal(a, b) for a, b in zip(again, good))
        ctx.paths_end()
        with pytest.raises(lib.BgpError, match="code 4"):
            ctx._paths_P = 63
            ctx.paths_select(Xc, 1)
    finally:
        ctx.close()


# ---- 5. the optimiser -------------------------------------------------------------------------------------------------------------
def branin_like(x):
    return float(np.sin(3.0 * x[0]) + (x[1] - 0.3) ** 2 + 0.5 * np.cos(2.0 * x[0] * x[1]))


def _told(bask, acq, n=30, m=250, seed=0, **okw):
    """An optimizer past its initial design: n random points told at once (one MCMC fit + one proposal)."""
    opt = bask.Optimizer(dimensions=[(-1.0, 1.0)] * 2, n_points=m, n_initial_points=n, init_strategy="r2", acq_func=acq,
                         random_state=seed, **okw)
    rng = np.random.RandomState(seed)
    X = rng.uniform(-1.0, 1.0, size=(n, 2)).tolist()
    y = [branin_like(x) + 0.01 * rng.randn() for x in X]
    opt.tell(X, y, n_samples=4, gp_samples=40, gp_burnin=2)
    return opt


NP, NF = 24, 48  # paths and features of the optimiser tests


@pytest.fixture(scope="module")
def opt_ei(bask):
    return _told(bask, "ei")


def _restated(opt, cand, forced, q, kind):
    """The batch restated on the paths at ``cand`` (normalised-y units, the device's bits), the paths rebuilt from a clone of the
    optimiser's generator; (picks, F)."""
    clone = np.random.RandomState()
    clone.set_state(opt.rng.get_state())
    with opt.gp.sample_paths(n_paths=NP, sample_mean=False, n_features=NF, random_state=clone) as paths:
        F, _ = paths._ctx.paths_eval(cand)
        FX, _ = paths._ctx.paths_eval(opt.gp._X_train_)
    return Q.select(F, FX.min(axis=1), forced, q, kind)[0], F


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def test_joint_ei_batch(bask, opt_ei):
    opt = opt_ei
    single, state = opt.ask(), opt.rng.get_state()
    batch = opt.ask(4, "joint_ei", n_paths=NP, n_features=NF)
    assert list(batch[0]) == list(single)
    assert len(batch) == 4 and len({tuple(p) for p in batch}) == 4
    assert all(dim.low <= v <= dim.high for p in batch for v, dim in zip(p, opt.space.dimensions))
    info = opt._last_batch_info
    assert info["path"] == "pathwise" and info["values"].shape == (3, 250) and info["incumbents"].shape == (NP,)
    assert opt.ask(4, "joint_ei", n_paths=NP, n_features=NF) == batch
    assert _same_state(opt.rng.get_state(), state)
    first = int(np.argmax(opt._last_acq_values))
    want, _ = _restated(opt, opt._last_candidates, [first], 3, "improvement")
    assert info["picks"] == [first] + [int(i) for i in want]
    assert list(opt.ask(1, "joint_ei")) == list(single)  # (one point, nothing pending: ask() itself)


def test_telling_the_first_point_continues_as_without_the_batch(bask):
    a, b = _told(bask, "ei", seed=4), _told(bask, "ei", seed=4)
    batch = a.ask(3, "joint_ei", n_paths=NP, n_features=NF)
    x = b.ask()
    assert list(batch[0]) == list(x)
    for opt in (a, b):
        opt.tell(list(x), branin_like(x), n_samples=4, gp_samples=40, gp_burnin=2)
    assert list(a.ask()) == list(b.ask())
    assert np.array_equal(a._last_acq_values, b._last_acq_values)


def test_thompson_batches_make_sample_acquisitions_batchable(bask):
    opt = _told(bask, "ts", seed=2)
    with pytest.raises(NotImplementedError, match="Thompson"):
        opt.ask(3)
    single = opt.ask()
    batch = opt.ask(3, "thompson", n_paths=NP, n_features=NF)
    assert list(batch[0]) == list(single) and len({tuple(p) for p in batch}) == 3
    first = int(np.argmax(opt._last_acq_values))
    want, F = _restated(opt, opt._last_candidates, [first], 2, "thompson")
    picks = opt._last_batch_info["picks"]
    assert picks == [first] + [int(i) for i in want]
    for j in range(2):  # pick j is path j's argmin among the candidates not yet chosen
        left = [i for i in range(F.shape[1]) if i not in picks[: j + 1]]
        assert picks[j + 1] == left[int(np.argmin(F[j, left]))]


def test_pending_points_are_forced_and_never_returned(bask, opt_ei):
    opt = opt_ei
    cand = opt._last_candidates
    best = int(np.argmax(opt._last_acq_values))
    x_best = opt.ask()
    state = opt.rng.get_state()
    batch = opt.ask(3, "joint_ei", pending=[x_best], n_paths=NP, n_features=NF)
    assert len(batch) == 3 and all(list(p) != list(x_best) for p in batch)
    want, _ = _restated(opt, cand, [best], 3, "improvement")
    assert opt._last_batch_info["picks"] == [int(i) for i in want]
    one = opt.ask(1, "joint_ei", pending=[x_best], n_paths=NP, n_features=NF)
    assert list(one) == list(batch[0])  # a single point, the first greedy pick
    # an off-candidate pending point is appended to the candidates and forced there
    off = [0.123, -0.456]
    assert not np.any(np.all(cand == opt.space.transform([off]), axis=1))
    batch = opt.ask(2, "joint_ei", pending=[x_best, off], n_paths=NP, n_features=NF)
    info = opt._last_batch_info
    assert info["forced"] == [best, len(cand)] and len(info["candidates"]) == len(cand) + 1
    want, _ = _restated(opt, info["candidates"], [best, len(cand)], 2, "improvement")
    assert info["picks"] == [int(i) for i in want] and len(cand) not in info["picks"]
    assert all(list(p) not in (list(x_best), off) for p in batch)
    assert _same_state(opt.rng.get_state(), state)
    for strategy in ("cl_min", "kb"):
        with pytest.raises(ValueError, match="pending"):
            opt.ask(2, strategy, pending=[x_best])
    with pytest.raises(ValueError, match="strategy"):
        opt.ask(2, "joint")


def test_obstacles_of_sample_paths_pass_through(bask):
    import sklearn.gaussian_process.kernels as sk

    opt = _told(bask, "ei", n=20, m=200, seed=1, gp_kwargs=dict(warp_inputs=True))
    with pytest.raises(ValueError, match="warped inputs"):
        opt.ask(3, "joint_ei", n_paths=NP, n_features=NF)
    opt = _told(bask, "lcb", n=20, m=200, seed=2,
                gp_kernel=sk.ConstantKernel(1.0, (0.1, 10.0)) * sk.Matern(0.5, (0.05, 5.0), nu=2.5) * sk.RBF(1.0, (0.05, 5.0)))
    with pytest.raises(ValueError, match="generic kernel tree"):
        opt.ask(3, "thompson", n_paths=NP, n_features=NF)
