"""Profile curves and maps on the device (bgp_profile_dependence: pf_line_kernel / pf_reduce_kernel of bgp_profile.hip; DESIGN.md
section 35) driven from ``_lib.Context`` with no fit, on the cases of tests/_profref.py: structure, the replay by sequential
``minimize_starts`` calls (bit for bit), the long-double mean at every minimiser, the minimum itself against a plain reference, bits
(repeat, panels, posteriors, chains, chunks), edges, refusals, and one fitted Optimizer end to end.  Lines start with ``PROFREF``."""
import functools

import numpy as np
import pytest

import _optref as R
import _profref as F

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

OUT = ("val", "x", "best_chain", "n_converged", "chain_val", "chain_x", "chain_status")


def _context(key, rows=None):
    import bayes_skopt_amd as bask

    c, pr = F.meta(key), F.problem(key)
    H = pr["H"] if rows is None else pr["H"][rows]
    ctx = bask._lib.Context(pr["X"], pr["y"], pr["alpha"], form=c["form"], stationary=c["stationary"], max_batch=len(H))
    assert np.all(ctx.posterior(H)["status"] == 0)
    return ctx, H


def _profile(ctx, key, H, X0=None, panels=None, grids=None, lo=None, hi=None, **kw):
    c, pr = F.meta(key), F.problem(key)
    kw = {"gtol": R.GTOL, "max_iter": R.MAX_ITER, "per_chain": True, **kw}
    return ctx.profile_dependence(H, c["y_mean"], c["y_std"], F.starts(key) if X0 is None else X0, pr["lo"] if lo is None else lo,
                                  pr["hi"] if hi is None else hi, F.grids(key) if grids is None else grids,
                                  F.CASES[key]["panels"] if panels is None else panels, **kw)


def _replay(ctx, key, H, X0, **kw):
    """chain_val / chain_x / chain_status of every panel by sequential ``minimize_starts`` calls in the degenerate box, each cell's
    start the previous cell's end point: per panel (B, cells, S[, d]) arrays."""
    from bayes_skopt_amd.profile import sweep_order

    c, pr = F.meta(key), F.problem(key)
    g, d, S = F.grids(key), len(pr["lo"]), len(X0)
    kw = {"gtol": R.GTOL, "max_iter": R.MAX_ITER, **kw}
    out = []
    for k1, k2 in F.CASES[key]["panels"]:
        kf, ks = (-1, k1) if k2 < 0 else (k1, k2)
        nf, ns = (len(g[kf]) if kf >= 0 else 1), len(g[ks])
        cv, cx, cs = np.empty((len(H), nf, ns, S)), np.empty((len(H), nf, ns, S, d)), np.empty((len(H), nf, ns, S), dtype=np.int32)
        for b, jf, s in np.ndindex(len(H), nf, S):
            lo, hi = pr["lo"].copy(), pr["hi"].copy()
            x = np.minimum(np.maximum(X0[s], lo), hi)
            if kf >= 0:
                lo[kf] = hi[kf] = x[kf] = g[kf][jf]
            order, restart = sweep_order(g[ks], x[ks])
            for pos, cell in enumerate(order):
                if pos == restart:
                    x = cx[b, jf, order[0], s]
                lo[ks] = hi[ks] = g[ks][cell]
                r = ctx.minimize_starts(b, H, c["y_mean"], c["y_std"], 0.0, x[None, :], lo, hi, **kw)
                x = r["x"][0]
                cv[b, jf, cell, s], cx[b, jf, cell, s], cs[b, jf, cell, s] = r["mean"][0], x, r["status"][0]
        out.append([a.reshape((len(H), nf * ns) + a.shape[3:]) for a in (cv, cx, cs)])
    return out


@functools.lru_cache(maxsize=None)
def _run(key):
    """One context per case: the call, its repeat and -- the cases with a few chains -- the replay."""
    ctx, H = _context(key)
    got, again = _profile(ctx, key, H), _profile(ctx, key, H)
    stats = ctx.chunk_stats()
    replay = _replay(ctx, key, H, F.starts(key)) if key in F.REPLAY_CASES else None
    ctx.close()
    return got, again, replay, stats


def _flat(a, trailing=0):
    return a.reshape((a.shape[0], -1) + a.shape[a.ndim - trailing:])


def _same(a, b):
    for k in OUT:
        for u, v in zip(a[k], b[k]):
            np.testing.assert_array_equal(u, v, err_msg=k)


@pytest.mark.parametrize("key", F.REPLAY_CASES)
def test_structure_replay_and_reduction(key):
    from bayes_skopt_amd.profile import reduce_chains

    pr = F.problem(key)
    got, again, replay, stats = _run(key)
    _same(got, again)
    assert stats == {"items": 1, "rows": 1}
    for p, (dims, mesh) in enumerate(F.cells(key)):
        x = _flat(got["x"][p], 1)
        assert np.all(x[:, :, dims] == mesh[None]) and np.all(x >= pr["lo"]) and np.all(x <= pr["hi"])
        cv, cx, cs = (_flat(got[k][p], t) for k, t in (("chain_val", 1), ("chain_x", 2), ("chain_status", 1)))
        for name, a, r in zip(("chain_val", "chain_x", "chain_status"), (cv, cx, cs), replay[p]):
            np.testing.assert_array_equal(a, r, err_msg="%s panel %d %s" % (key, p, name))
        val, xb, best, nc = reduce_chains(cv, cx, cs)
        for a, r in ((got["val"][p], val), (got["x"][p], xb), (got["best_chain"][p], best), (got["n_converged"][p], nc)):
            np.testing.assert_array_equal(_flat(a, a.ndim - got["val"][p].ndim), r)
    assert np.all(got["evals"] >= sum(v[0].size for v in got["chain_val"]))


@pytest.mark.parametrize("key", list(F.CASES))
def test_value_is_the_high_precision_mean_at_the_minimiser(key):
    got = _run(key)[0]
    for p in range(len(got["val"])):
        for b in range(got["val"][p].shape[0]):
            err, tol = F.mean_error(key, b, _flat(got["x"][p], 1)[b], _flat(got["val"][p])[b])
            print("PROFREF %-14s panel %d b %d mean err/tol %.3e" % (key, p, b, err / tol))
            assert err <= tol, (key, p, b, err, tol)


@pytest.mark.parametrize("key", F.MINIMUM_CASES)
def test_the_minimum_itself(key):
    c, got = F.meta(key), _run(key)[0]
    above = cells = 0
    for b in range(c["B"]):
        for v, ref in zip(got["val"], F.reference_profile(key, b)):
            diff = (c["y_mean"] + c["y_std"] * _flat(v)[b]) - ref
            print("PROFREF %-14s b %d above %.2e below %.2e margin %.2e" % (key, b, diff.max(), -diff.min(), F.margin(key)))
            assert np.all(diff >= -F.margin(key)), diff.min()
            above, cells = above + int((diff > F.margin(key)).sum()), cells + diff.size
    assert above <= (0 if key == F.SINGLE_BASIN else F.MISS_CAP * cells), (above, cells)


def test_bits_panels_posteriors_chains_chunks(monkeypatch):
    key = F.BITS_CASE
    got, panels, X0 = _run(key)[0], F.CASES[key]["panels"], F.starts(key)
    ctx, H = _context(key)
    perm = [2, 0, 1]
    other = _profile(ctx, key, H, panels=[panels[i] for i in perm])
    alone = _profile(ctx, key, H, panels=[panels[1]])
    for k in OUT:
        for j, i in enumerate(perm):
            np.testing.assert_array_equal(other[k][j], got[k][i])
        np.testing.assert_array_equal(alone[k][0], got[k][1])
    # S = 3 against the reduction of three S = 1 calls
    from bayes_skopt_amd.profile import reduce_chains

    ones = [_profile(ctx, key, H, X0=X0[s:s + 1]) for s in range(len(X0))]
    for p in range(len(panels)):
        cv, cx, cs = (np.stack([o[k][p] for o in ones], axis=-1 - t) for k, t in (("val", 0), ("x", 1), ("n_converged", 0)))
        for a, r in zip((got["val"][p], got["x"][p], got["best_chain"][p], got["n_converged"][p]), reduce_chains(cv, cx, 1 - cs)):
            np.testing.assert_array_equal(a, r)
    # one line per chunk: a curve, the map's ng[2] lines, a curve
    monkeypatch.setenv("BGP_ROW_CHUNK", "1")
    forced = _profile(ctx, key, H)
    assert ctx.chunk_stats() == {"items": 1, "rows": 1 + F.CASES[key]["ng"][2] + 1}
    monkeypatch.delenv("BGP_ROW_CHUNK")
    _same(forced, got)
    np.testing.assert_array_equal(forced["evals"], got["evals"])
    ctx.close()
    # B = 2 against two B = 1 calls
    ctx2, H2 = _context(key, rows=[1, 2])
    two = _profile(ctx2, key, H2)
    ctx2.close()
    for j, b in enumerate((1, 2)):
        ctx1, H1 = _context(key, rows=[b])
        one = _profile(ctx1, key, H1)
        ctx1.close()
        for k in OUT:
            for u, v, w in zip(one[k], two[k], got[k]):
                np.testing.assert_array_equal(u[0], v[j])
                np.testing.assert_array_equal(u[0], w[b])


def test_edges_pure_evaluation_gtol_zero_and_a_nan_start():
    key = F.BITS_CASE
    pr, panels = F.problem(key), F.CASES[key]["panels"]
    ctx, H = _context(key)
    ev = _profile(ctx, key, H, max_iter=0)
    X0 = np.minimum(np.maximum(F.starts(key), pr["lo"]), pr["hi"])
    for p, (dims, mesh) in enumerate(F.cells(key)):
        pts = np.repeat(X0[None], len(mesh), axis=0)  # (cells, S, d): the clipped starts with the panel overwritten
        pts[:, :, dims] = mesh[:, None, :]
        np.testing.assert_array_equal(_flat(ev["chain_x"][p], 2)[0], pts)
        mean = ctx.predict_grad(H, pts.reshape(-1, pts.shape[-1]), want_dvar=False)[0]
        np.testing.assert_array_equal(_flat(ev["chain_val"][p], 1), mean.reshape(len(H), len(mesh), len(X0)))
    z = _profile(ctx, key, H, gtol=0.0)
    assert all(np.all(np.isfinite(v)) for v in z["val"]) and all(set(np.unique(s)) <= {0, 1, 2} for s in z["chain_status"])
    got, d = _run(key)[0], len(pr["lo"])
    # a NaN in a free coordinate of chain 1: status 2 at every cell, never the best, the other chains' bits unchanged
    for p, pnl in enumerate(panels):
        t = [t for t in range(d) if t not in pnl][0]
        b2 = F.starts(key).copy()
        b2[1, t] = np.nan
        r = _profile(ctx, key, H, X0=b2, panels=[pnl])
        assert np.all(r["chain_status"][0][..., 1] == 2) and np.all(r["best_chain"][0] != 1)
        np.testing.assert_array_equal(r["chain_val"][0][..., [0, 2]], got["chain_val"][p][..., [0, 2]])
    ctx.close()


def _refusals(key):
    pr = F.problem(key)
    g, lo, hi = F.grids(key), pr["lo"], pr["hi"]
    up = hi.copy()
    up[0] = lo[0] - 1.0
    return {"S < 1": dict(X0=np.empty((0, len(lo)))), "P < 1": dict(panels=[]), "max_iter < 0": dict(max_iter=-1),
            "gtol < 0": dict(gtol=-1e-3), "gmax > 256": dict(grids=[np.linspace(lo[0], hi[0], 257)] + g[1:]),
            "panel index": dict(panels=[(0, len(lo))]), "k1 == k2": dict(panels=[(1, 1)]), "lo > hi": dict(hi=up),
            "grid outside": dict(grids=[g[0] + 0.5] + g[1:]), "2^24 cells": dict(
                grids=[np.linspace(lo[t], hi[t], 256) for t in range(len(lo))], panels=[(0, 1)] * 257, per_chain=False)}


@pytest.mark.parametrize("what", list(_refusals(F.BITS_CASE)))
def test_refusals_name_the_entry_and_leave_the_context_usable(what):
    import bayes_skopt_amd as bask

    key = F.BITS_CASE
    ctx, H = _context(key)
    with pytest.raises(bask._lib.BgpError, match=r"\(code 1\): bgp_profile_dependence"):
        _profile(ctx, key, H, **_refusals(key)[what])
    _same(_profile(ctx, key, H), _run(key)[0])
    ctx.close()


def test_refusals_of_the_context_state():
    import bayes_skopt_amd as bask

    key = F.BITS_CASE
    c, pr = F.meta(key), F.problem(key)
    ctx = bask._lib.Context(pr["X"], pr["y"], pr["alpha"], form=c["form"], stationary=c["stationary"], max_batch=3)
    with pytest.raises(bask._lib.BgpError, match=r"\(code 4\): bgp_profile_dependence"):
        _profile(ctx, key, pr["H"])
    ctx.set_warp(np.zeros(2 * c["d"]))
    ctx.posterior(pr["H"])
    with pytest.raises(bask._lib.BgpError, match=r"\(code 1\): bgp_profile_dependence: warped inputs"):
        _profile(ctx, key, pr["H"])
    ctx.close()
    X = np.random.RandomState(0).uniform(size=(40, 33))
    ctx = bask._lib.Context(X, np.sin(X.sum(axis=1)), 1e-8, form="product", stationary="rbf", max_batch=1)
    H = np.concatenate([[0.0], np.full(33, 0.5), [np.log(1e-2)]])[None]
    ctx.posterior(H)
    with pytest.raises(bask._lib.BgpError, match=r"\(code 1\): bgp_profile_dependence: d > 32"):
        ctx.profile_dependence(H, 0.0, 1.0, X[:1], 0.0, 1.0, [np.array([0.5])] * 33, [(0, -1)])
    ctx.close()


def test_end_to_end_on_a_fitted_optimizer(capfd):
    import bayes_skopt_amd as bask

    def f(x):
        return (x[0] - 0.3) ** 2 + 0.5 * (x[1] + 0.2) ** 2 + 0.3 * np.sin(3.0 * x[2])

    def fitted(**gp_kwargs):
        opt = bask.Optimizer([(-1.0, 1.0), (-1.0, 1.0), (0.0, 2.0)], n_initial_points=12, random_state=3, gp_kwargs=gp_kwargs)
        rng = np.random.RandomState(3)
        X = [[rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0, 2)] for _ in range(24)]
        opt.tell(X, [f(x) for x in X], gp_burnin=20, gp_samples=20, n_samples=0, progress=False)
        return opt

    opt = fitted()
    res = opt.profile_dependence(pairs=None, n_points=9)
    assert res["path"] == "device"
    _x, best, info = opt.expected_optimum(n_random_starts=20, random_state=0)
    margin = 1e-6 * float(np.ptp(opt._result().func_vals))
    for k in range(3):
        grid, vals = res["dims"][k]
        arg = res["argmin"][k]
        assert vals.shape == grid.shape and arg.shape == grid.shape + (3,)
        assert np.all(arg >= np.array([-1.0, -1.0, 0.0]) - 1e-12) and np.all(arg <= np.array([1.0, 1.0, 2.0]) + 1e-12)
        assert vals.min() >= best - margin  # (the grid need not hold the optimum's coordinate: never below it)
    # grids that hold the optimum's coordinates, chains from the observed points as utils.profile_dependence takes them: the walk
    # has to reach the optimum, and the minimum of every curve IS the expected optimum
    xt, r = info["x_transformed"][info["best"]], opt._result()
    X0 = opt.space.transform([r.x_iters[i] for i in np.argsort(r.func_vals, kind="stable")[:4]])
    curves = opt.gp.profile_dependence([np.union1d(np.linspace(0.0, 1.0, 5), xt[k:k + 1]) for k in range(3)],
                                       [(k, -1) for k in range(3)], X0=X0)
    for v in curves["val"]:
        assert abs(v.min() - best) <= margin, (v.min(), best)
    capfd.readouterr()
    warped = fitted(warp_inputs=True)
    assert warped.profile_dependence(dims=[0], pairs=None, n_points=3, n_starts=1)["path"] == "host"
    assert warped.profile_dependence(dims=[1], pairs=None, n_points=3, n_starts=1)["path"] == "host"
    assert capfd.readouterr().err.count("profile_dependence: searched on the host") == 1
