"""The device optimum search (bgp_minimize_starts: pg_min_kernel of bgp_predgrad.hip on the projected BFGS of bgp_bfgs.h; DESIGN.md
section 13) driven from ``_lib.Context`` with no fit, on the cases of tests/_optref.py, against references that no device kernel
has a part in: the long-double objective of ``_optref.objective_ld`` (fp64 numpy / LAPACK at n = 3100, at twice the tolerance
class) and scipy's L-BFGS-B on its fp64 restatement, which tests/test_cpu_optimum_reference.py qualifies.  The evaluator at
``max_iter = 0``, the search from every start, the cap on starts that do not converge, bits, caps and edges, arguments.
Lines start with ``OPTREF``.

Measured on the device: moments at the clipped starts and at the end points against long double at most 0.015 tol (mean: the
n = 1 case, on the floor; 1.4e-3 tol otherwise) and 0.014 tol (variance); n = 3100 against fp64 4.5e-5 and 0.49 of twice the class.
Status of the 58 smooth starts [58, 0, 0]; Matern 1/2 [6, 0, 0] (n = 257) and [0, 0, 6] (n = 2: every start ends on the kink at a
training point, as scipy does).  Worst long-double projected gradient at a converged end point 9.94e-6, most evaluations 263,
best value minus the reference's at most 2.9e-9 (n = 3100, kappa 1.96; 1e-6 ptp(y) = 9.2e-6).  Three deliberate breaks, each
red: the b * npad offset of alpha dropped (test_evaluator_at_the_clipped_starts and every b > 0 test), lo / hi swapped in the
trial point's clip (test_search_from_every_start on the tight box, the convergence cap), pg_rows indexed by 0
(test_search_from_every_start and test_the_scratch_row_case_repeats_bit_for_bit at n = 3100, no other case)."""
import functools

import numpy as np
import pytest

import _optref as R
import _precision as P
from conftest import synth

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

KEYS = ("x", "mean", "var", "iters", "evals", "status")
BITS_CASE = "opt3_n128_d3_matern52_product_B3"
KINK_CASE = "opt5_n257_d4_matern12_sum_B1"


@pytest.fixture(scope="module")
def bask():
    import bayes_skopt_amd as bask

    assert bask._lib.device_count() >= 1
    return bask


def _check(tag, quantity, err, t):
    print("OPTREF %-52s %-5s err/tol %.3e" % (tag, quantity, err / t))
    assert err <= t, "%s %s: error %.3e > tol %.3e (%.1fx)" % (tag, quantity, err, t, err / t)


def _context(cid, rows=None):
    """A context with the case's posteriors (or only ``rows`` of its H) resident."""
    import bayes_skopt_amd as bask

    c, pr = R.ALL[cid], R.problem(cid)
    H = pr["H"] if rows is None else pr["H"][rows]
    ctx = bask._lib.Context(pr["X"], pr["y"], pr["alpha"], form=c["form"], stationary=c["stationary"], max_batch=len(H))
    assert np.all(ctx.posterior(H)["status"] == 0)
    return ctx


def _minimize(ctx, cid, j, X0, H=None, b=None, lo=None, hi=None, **kw):
    c, pr = R.ALL[cid], R.problem(cid)
    bb, kappa = c["searches"][j]
    return ctx.minimize_starts(bb if b is None else b, pr["H"] if H is None else H, c["y_mean"], c["y_std"], kappa, X0,
                               pr["lo"] if lo is None else lo, pr["hi"] if hi is None else hi, **kw)


def _objective(cid, j, mean, var):
    """f in y units from the returned moments, in the operation order of the kernel."""
    c = R.ALL[cid]
    return c["y_mean"] + c["y_std"] * mean + c["searches"][j][1] * (c["y_std"] * np.sqrt(var))


@functools.lru_cache(maxsize=None)
def _run(cid):
    """One context and one posterior build per case; per search the evaluator call (``max_iter = 0``), ``predict_grad`` at its
    points and the search (twice at n = 3100)."""
    c, pr = R.ALL[cid], R.problem(cid)
    ctx = _context(cid)
    out = []
    for j, (b, _kappa) in enumerate(c["searches"]):
        X0 = R.starts(cid, j)
        ev = _minimize(ctx, cid, j, X0, gtol=R.GTOL, max_iter=0)
        pg = ctx.predict_grad(pr["H"], ev["x"])
        res = _minimize(ctx, cid, j, X0, gtol=R.GTOL, max_iter=R.MAX_ITER)
        again = _minimize(ctx, cid, j, X0, gtol=R.GTOL, max_iter=R.MAX_ITER) if c.get("big") else None
        out.append({"ev": ev, "pg_mean": pg[0][b], "pg_var": pg[1][b], "res": res, "again": again})
    ctx.close()
    return out


def _reference(cid, j, Xq):
    """(reference objective dict, tolerance factor): long double, or fp64 at twice the class beyond its reach."""
    b, kappa = R.ALL[cid]["searches"][j]
    if R.ALL[cid].get("big"):
        return R.objective64(cid, b, kappa, Xq), 2.0
    return R.objective_ld(cid, b, kappa, Xq), 1.0


def _moments(tag, cid, j, got, Xq):
    """mean / var of ``got`` at the rows ``Xq`` against the reference there, at the classes of _precision; returns the reference."""
    c = R.ALL[cid]
    k = R.kappa_of(cid, c["searches"][j][0])
    ref, fac = _reference(cid, j, Xq)
    _check(tag, "mean", P.err_rel_max(got["mean"], ref["mean"], ref["mean_scale"]), fac * P.tol("mean", k, c["n"]))
    _check(tag, "var", P.err_rel_max(got["var"], ref["var"], ref["prior_var"]), fac * P.tol("var", k, c["n"]))
    return ref


# ---- 1. the evaluator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,j", R.SEARCHES)
def test_evaluator_at_the_clipped_starts(bask, cid, j):
    """max_iter = 0: nothing moves.  The outside start is its clipped image, the moments are predict_grad's bits and meet the
    reference."""
    r = _run(cid)[j]
    ev, X0 = r["ev"], R.starts(cid, j)
    np.testing.assert_array_equal(ev["x"], R.clip(cid, X0))
    assert np.all(ev["iters"] == 0)
    np.testing.assert_array_equal(ev["mean"], r["pg_mean"])
    np.testing.assert_array_equal(ev["var"], r["pg_var"])
    _moments("%s search %d starts" % (cid, j), cid, j, ev, ev["x"])


# ---- 2. the search ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,j", R.SEARCHES)
def test_search_from_every_start(bask, cid, j):
    c, pr = R.ALL[cid], R.problem(cid)
    lo, hi = pr["lo"], pr["hi"]
    r = _run(cid)[j]
    ev, res = r["ev"], r["res"]
    x, st = res["x"], res["status"]
    assert x.shape == R.starts(cid, j).shape and np.all(x >= lo) and np.all(x <= hi)
    assert np.all(x[:, lo == hi] == lo[lo == hi])
    assert set(np.unique(st)) <= {0, 1, 2}
    assert np.all(res["iters"] <= R.MAX_ITER) and np.all(res["evals"] <= 2 + R.MAX_ITER * 30)
    # never above the start; strictly below where the start is not stationary by the reference's gradient
    f0, f = _objective(cid, j, ev["mean"], ev["var"]), _objective(cid, j, res["mean"], res["var"])
    ref0, _fac = _reference(cid, j, ev["x"])
    pg0 = R.projected_gradient(ev["x"], ref0["df"], lo, hi)
    assert np.all(f <= f0), (f - f0).max()
    assert np.all(f[pg0 > R.GTOL] < f0[pg0 > R.GTOL])
    # the end points: a fresh accuracy check of pg_eval, and the stationarity witness
    ref = _moments("%s search %d end points" % (cid, j), cid, j, res, x)
    pg = R.projected_gradient(x, ref["df"], lo, hi)
    worst = float(pg[st == 0].max()) if np.any(st == 0) else 0.0
    # the best value against the CPU search
    best_ref = min(q["f"] for q in R.reference_search(cid, j))
    print("OPTREF %-40s search %d  status %s  iters max %d  evals mean %.1f max %d  worst |pg| %.2e  decrease min %.2e  "
          "best %.12g  reference %.12g  diff %.2e" % (cid, j, np.bincount(st, minlength=3).tolist(), res["iters"].max(),
                                                      res["evals"].mean(), res["evals"].max(), worst, (f0 - f).min(), f.min(),
                                                      best_ref, f.min() - best_ref))
    assert worst <= 2 * R.GTOL
    assert f.min() <= best_ref + 1e-6 * R.y_ptp(cid)


# ---- 3. the convergence cap ---------------------------------------------------------------------------------------------------
def test_at_most_a_tenth_of_the_smooth_starts_do_not_converge(bask):
    """The fp64 reference (scipy L-BFGS-B, tests/test_cpu_optimum_reference.py) converges from all of them.  Matern 1/2 is left
    out: kinks at the training points, fac(0) = 0."""
    status = []
    for cid, j in R.SEARCHES:
        st = _run(cid)[j]["res"]["status"]
        print("OPTREF %-40s search %d  status %s%s" % (cid, j, np.bincount(st, minlength=3).tolist(),
                                                      "" if R.is_smooth(cid) else "  (not counted)"))
        if R.is_smooth(cid):
            status.append(st)
    status = np.concatenate(status)
    print("OPTREF smooth cases: status %s of %d starts" % (np.bincount(status, minlength=3).tolist(), status.size))
    assert status.size == 58
    assert int(np.sum(status != 0)) <= 0.1 * status.size, status


# ---- 4. bits ------------------------------------------------------------------------------------------------------------------
def _same(a, b, rows_a=slice(None), rows_b=slice(None)):
    for key in KEYS:
        np.testing.assert_array_equal(a[key][rows_a], b[key][rows_b], err_msg=key)


def test_a_start_does_not_depend_on_its_call(bask):
    cid = BITS_CASE
    pr = R.problem(cid)
    X0 = R.starts(cid, 0)  # (posterior b = 1 of three)
    kw = dict(gtol=R.GTOL, max_iter=R.MAX_ITER)
    ctx = _context(cid)
    a = _minimize(ctx, cid, 0, X0, **kw)
    _same(a, _run(cid)[0]["res"])
    _same(a, _minimize(ctx, cid, 0, X0, **kw))
    _same(a, _minimize(ctx, cid, 0, X0[:3], **kw), slice(0, 3))
    _same(a, _minimize(ctx, cid, 0, X0[2:3], **kw), slice(2, 3))
    perm = np.array([4, 0, 5, 2, 1, 3])
    _same(a, _minimize(ctx, cid, 0, X0[perm], **kw), perm)
    # the start outside the box is its clipped image
    _same(a, _minimize(ctx, cid, 0, R.clip(cid, X0[-1:]), **kw), slice(5, 6))
    # the full H block or just row b
    _same(a, _minimize(ctx, cid, 0, X0, H=pr["H"][1:2], **kw))
    assert np.any(a["iters"] > 0)
    ctx.close()
    # posterior 1 alone, resident as posterior 0
    alone = _context(cid, rows=slice(1, 2))
    _same(a, _minimize(alone, cid, 0, X0, H=pr["H"][1:2], b=0, **kw))
    alone.close()


def test_the_scratch_row_case_repeats_bit_for_bit(bask):
    for r in _run(R.BIG_CASE):
        _same(r["res"], r["again"])
        assert np.any(r["res"]["iters"] > 0)


# ---- 5. caps and edges --------------------------------------------------------------------------------------------------------
def test_caps_and_a_box_without_room(bask):
    cid = BITS_CASE
    pr = R.problem(cid)
    X0 = R.starts(cid, 1)
    ctx = _context(cid)
    ev = _minimize(ctx, cid, 1, X0, max_iter=0)
    f0 = _objective(cid, 1, ev["mean"], ev["var"])
    capped = _minimize(ctx, cid, 1, X0, gtol=R.GTOL, max_iter=3)
    assert np.all(capped["iters"] <= 3) and np.all(capped["evals"] <= 2 + 3 * 30)
    assert np.all(capped["iters"][capped["status"] == 1] == 3)
    # gtol = 0: only an exactly zero projected gradient (the corner start's) is convergence; everything else ends by the caps
    z = _minimize(ctx, cid, 1, X0, gtol=0.0, max_iter=R.MAX_ITER)
    assert set(np.unique(z["status"])) <= {0, 1, 2} and np.all(z["iters"] <= R.MAX_ITER) and np.all(z["evals"] <= 2 + R.MAX_ITER * 30)
    for out in (capped, z):
        assert all(np.all(np.isfinite(out[k])) for k in ("x", "mean", "var"))
        assert np.all(out["x"] >= pr["lo"]) and np.all(out["x"] <= pr["hi"])
        assert np.all(_objective(cid, 1, out["mean"], out["var"]) <= f0)
    print("OPTREF gtol = 0: status %s  iters max %d  evals max %d" % (np.bincount(z["status"], minlength=3).tolist(),
                                                                    z["iters"].max(), z["evals"].max()))
    # lo == hi in every dimension: the point itself, converged, without an iteration
    p = np.array([0.3, 0.45, 1.0])
    pt = _minimize(ctx, cid, 1, X0, lo=p, hi=p, gtol=R.GTOL, max_iter=R.MAX_ITER)
    assert np.all(pt["x"] == p) and np.all(pt["status"] == 0) and np.all(pt["iters"] == 0)
    np.testing.assert_array_equal(pt["mean"], np.full(len(X0), ctx.predict_grad(pr["H"], p[None])[0][2, 0]))
    ctx.close()


def test_start_on_a_training_point_of_a_near_noise_free_posterior(bask):
    """White term 1e-10, kappa = 1.96, y_std so small that y_std sqrt(var) <= 1e-8 ON the training point and not off it: the
    search leaves through the branch of pg_gradient that drops the std term and comes back to it."""
    X, y = synth(40, 2, 3)
    h = np.array([[0.0, np.log(0.4), np.log(0.4), np.log(1e-10)]])
    ym, ys, kappa = 0.7, 5e-5, 1.96
    X0 = np.vstack([X[7], X[20], X[7] + 0.05])
    ctx = bask._lib.Context(X, y, 1e-8, max_batch=1)
    assert np.all(ctx.posterior(h)["status"] == 0)
    ev = ctx.minimize_starts(0, h, ym, ys, kappa, X0, R.LO, R.HI, max_iter=0)
    sd0 = ys * np.sqrt(ev["var"])
    assert np.all(sd0[:2] <= R.SD_ZERO) and sd0[2] > R.SD_ZERO, sd0
    for gtol in (R.GTOL, 0.0):
        out = ctx.minimize_starts(0, h, ym, ys, kappa, X0, R.LO, R.HI, gtol=gtol, max_iter=R.MAX_ITER)
        assert all(np.all(np.isfinite(out[k])) for k in ("x", "mean", "var"))
        assert np.all(out["x"] >= R.LO) and np.all(out["x"] <= R.HI) and set(np.unique(out["status"])) <= {0, 1, 2}
        f0 = ym + ys * ev["mean"] + kappa * (ys * np.sqrt(ev["var"]))
        f = ym + ys * out["mean"] + kappa * (ys * np.sqrt(out["var"]))
        assert np.all(f <= f0), (f - f0).max()
        print("OPTREF near-noise-free gtol %.0e: sd at the starts %s  status %s  iters %s  moved %s"
              % (gtol, sd0.tolist(), out["status"].tolist(), out["iters"].tolist(), np.abs(out["x"] - X0).max(axis=1).tolist()))
    assert np.all(out["iters"] > 0)  # (gtol = 0: the starts on the training points did leave them)
    ctx.close()


def test_a_non_finite_start_is_not_reported_as_converged(bask):
    """A NaN coordinate passes the clip, and ``fmax`` in the convergence test drops a NaN gradient: the start used to come back
    with status 0.  It ends with status 2 without an iteration, and the starts that share its call keep their bits."""
    cid = BITS_CASE
    X0 = np.array(R.starts(cid, 0))
    kw = dict(gtol=R.GTOL, max_iter=R.MAX_ITER)
    ctx = _context(cid)
    good = _minimize(ctx, cid, 0, X0, **kw)
    X0[1, 2] = np.nan
    out = _minimize(ctx, cid, 0, X0, **kw)
    ctx.close()
    assert out["status"][1] == 2 and out["iters"][1] == 0
    np.testing.assert_array_equal(out["x"][1], X0[1])
    keep = np.array([0, 2, 3, 4, 5])
    _same(good, out, keep, keep)


def test_matern12_start_on_a_training_point(bask):
    """r = 0 at the start: fac(0) = 0 keeps every gradient finite; the search ends inside the box, not above its start."""
    cid = KINK_CASE
    pr = R.problem(cid)
    X0 = pr["X"][[7, 100, 256]]
    ctx = _context(cid)
    ev = _minimize(ctx, cid, 0, X0, max_iter=0)
    out = _minimize(ctx, cid, 0, X0, gtol=R.GTOL, max_iter=R.MAX_ITER)
    ctx.close()
    np.testing.assert_array_equal(ev["x"], X0)
    assert all(np.all(np.isfinite(out[k])) for k in ("x", "mean", "var"))
    assert np.all(out["x"] >= pr["lo"]) and np.all(out["x"] <= pr["hi"]) and set(np.unique(out["status"])) <= {0, 1, 2}
    assert np.all(_objective(cid, 0, out["mean"], out["var"]) <= _objective(cid, 0, ev["mean"], ev["var"]))
    _moments("%s from training points, end points" % cid, cid, 0, out, out["x"])


# ---- 6. arguments -------------------------------------------------------------------------------------------------------------
def test_arguments_are_errors_and_the_context_answers_afterwards(bask):
    """Each call is refused on the host, before any launch; the next correct call gives the bits of the first."""
    lib = bask._lib
    cid = BITS_CASE
    c, pr = R.ALL[cid], R.problem(cid)
    X0 = R.starts(cid, 0)
    d = c["d"]
    kw = dict(gtol=R.GTOL, max_iter=R.MAX_ITER)
    ctx = _context(cid)
    good = _minimize(ctx, cid, 0, X0, **kw)
    bad_lo = pr["lo"].copy()
    bad_lo[1] = pr["hi"][1] + 0.5
    refused = [
        ("code 1", dict(X0=np.empty((0, d)))),
        ("code 1", dict(X0=np.zeros((65536, d)))),
        (r"code 1.*empty box in dimension 1", dict(X0=X0, lo=bad_lo)),
        ("code 4", dict(X0=X0, b=c["B"], H=pr["H"][1:2])),
        ("code 1", dict(X0=X0, max_iter=-1)),
        ("code 1", dict(X0=X0, gtol=float("nan"))),
    ]
    for match, args in refused:
        with pytest.raises(lib.BgpError, match=match):
            _minimize(ctx, cid, 0, **{**kw, **args})
        _same(good, _minimize(ctx, cid, 0, X0, **kw))
    ctx.close()
