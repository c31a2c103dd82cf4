"""Fantasy conditioning on the device (``bgp_fantasy_*``, bgp_fantasy.hip) driven directly through
``_lib.Context`` -- no Optimizer, no MCMC -- on the cases of tests/_precision.py::FANTASY_CASES: every kernel family, the
64-point LDS tile, the 256-candidate workgroup and its padding, d = 32, B < resident posteriors, forced pick sequences.

* the conditioned latent means / variances after every step against ``oracle/hp_oracle.py::fantasy`` (long double, every
  prefix refactorised, no rank-1 identity) at ``tol("fant_mean" / "fant_var", kappa of the augmented matrix, n + j)``, which
  tests/test_cpu_precision.py qualifies (reachable with a 10x margin; fp32 inputs, a dropped sum over the earlier steps and a
  noise without base_alpha each miss by 10x);
* the start state, the step values (closed forms with scipy on the device's own moments of that step, under the reference's
  averaging rules), the argmax, bitwise invariants, and the limits, which are error codes.

Lines printed with ``pytest -s`` start with ``PRECISION``."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
from scipy.special import ndtr

import _precision as P

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

ERR_INVALID, ERR_STATE = 1, 4  # include/bgp.h
Y_MEAN, Y_STD, Y_OPT = 0.3, 1.7, 0.1  # the y normalisation the closed forms undo, and a given EI target (raw units)
CIDS = [c["id"] for c in P.FANTASY_CASES]


@pytest.fixture(scope="module")
def lib():
    import bayes_skopt_amd  # noqa: F401
    from bayes_skopt_amd import _lib

    assert _lib.device_count() >= 1
    return _lib


def _acqs(lib):
    """EI over the draw's lowest mean and over a given target, LCB, mean, std: all five in one begin."""
    return [lib.ACQ_EI, lib.ACQ_EI, lib.ACQ_LCB, lib.ACQ_MEAN, lib.ACQ_STD], [np.nan, Y_OPT, 1.96, 0.0, 0.0]


def _noise_off(H):
    Hk = np.array(H, dtype=np.float64, copy=True)
    Hk[:, -1] = -np.inf
    return Hk


def _run(lib, c, X, y, alpha, H, Bf, Xc, picks, lies, noise=None, acqs=None, qmax=None, n_samples=None):
    """posterior(H), fantasy_begin on its first Bf rows, the forced steps, the moments after each.  ``lies`` None (kriging
    believer) or one value per step."""
    kinds, params = acqs or _acqs(lib)
    ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=len(H))
    try:
        assert np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)
        Hk = _noise_off(H[:Bf])
        out = {"predict": ctx.predict(Hk, Xc), "n_samples": Bf + 2 if n_samples is None else n_samples, "steps": []}
        ctx.fantasy_begin(Hk, c["base_alpha"] + np.exp(H[:Bf, -1]) if noise is None else noise, Xc, Y_MEAN, Y_STD, kinds,
                          params, out["n_samples"], len(picks) if qmax is None else qmax)
        out["begin"] = ctx.fantasy_moments()
        for j, p in enumerate(picks):
            nxt, vals = ctx.fantasy_step(p, None if lies is None else lies[j], want_values=True)
            mean, var = ctx.fantasy_moments()
            out["steps"].append({"next": nxt, "values": vals, "mean": mean, "var": var})
        ctx.fantasy_end()
    finally:
        ctx.close()
    return out


def _case_run(lib, cid, **kw):
    c = P.ALL[cid]
    X, y, alpha, H, _ = P.problem(cid)
    Xc, picks, lies = P.fantasy_inputs(cid)
    kw.setdefault("lies", lies)
    return _run(lib, c, X, y, alpha, kw.pop("H", H), kw.pop("Bf", c["Bf"]), kw.pop("Xc", Xc), kw.pop("picks", picks), **kw)


@functools.lru_cache(maxsize=None)
def _cached(lib, cid):
    """One device run per case, shared by the tests that only read it."""
    return _case_run(lib, cid)


def _same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------------------
# conditioned moments against the extended-precision reference
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", CIDS)
def test_conditioned_moments_match_the_reference(lib, cid):
    c = P.ALL[cid]
    n = c["n"]
    run = _cached(lib, cid)
    worst = {"fant_mean": (0.0, None), "fant_var": (0.0, None)}
    for b in range(c["Bf"]):
        ref = P.ref_fantasy(cid, b)
        for j, step in enumerate(run["steps"]):
            errs = P.fantasy_errs(step["mean"][b], step["var"][b], ref, j)
            for q, e in zip(("fant_mean", "fant_var"), errs):
                t = P.tol(q, ref["kappa"][j], n + j)
                if e / t >= worst[q][0]:
                    worst[q] = (e / t, (b, j, e, t))
    for q, (r, where) in worst.items():
        print("PRECISION %-48s %-9s %-7s %-9s err/tol %.3e  (draw %d, step %d: err %.2e, tol %.2e)"
              % ((cid, c["stationary"], c["form"], q, r) + where))
    for q, (r, where) in worst.items():
        assert r <= 1.0, "%s %s: (draw, step, error, tol) = %r, %.1fx" % (cid, q, where, r)


@pytest.mark.parametrize("cid", CIDS)
def test_start_state_is_predict(lib, cid):
    """Straight after fantasy_begin the moments are predict's, bit for bit."""
    run = _cached(lib, cid)
    assert _same(run["begin"][0], run["predict"][0]) and _same(run["begin"][1], run["predict"][1])


# ------------------------------------------------------------------------------------------------------------------------------
# step values and argmax
# ------------------------------------------------------------------------------------------------------------------------------
def _ei(mu, sd, y_opt):
    out = np.zeros_like(mu)
    ok = sd > 0
    with np.errstate(all="ignore"):
        z = (y_opt - mu[ok]) / sd[ok]
        out[ok] = (z * ndtr(z) + np.exp(-z * z / 2.0) / np.sqrt(2.0 * np.pi)) * sd[ok]
    return out


def _closed_forms(lib, mean, var, kinds, params, n_samples):
    """The reference's evaluate_acquisitions on given latent moments: per draw the closed form of the de-normalised mean and
    standard deviation, a draw with a non-finite value contributes nothing, the sum divided by the requested count."""
    out = np.zeros((len(kinds), mean.shape[1]))
    with np.errstate(all="ignore"):
        for b in range(mean.shape[0]):
            mu, sd = Y_STD * mean[b] + Y_MEAN, np.sqrt(var[b] * (Y_STD * Y_STD))
            for k, (kind, par) in enumerate(zip(kinds, params)):
                if kind == lib.ACQ_EI:
                    tmp = _ei(mu, sd, np.min(mu) if np.isnan(par) else par)
                else:
                    tmp = {lib.ACQ_LCB: par * sd - mu, lib.ACQ_MEAN: -mu, lib.ACQ_STD: sd}[kind]
                if np.all(np.isfinite(tmp)):
                    out[k] += tmp / n_samples
    return out


def _check_values(lib, step, kinds, params, n_samples):
    want = _closed_forms(lib, step["mean"], step["var"], kinds, params, n_samples)
    for k, kind in enumerate(kinds):  # (the tolerances of tests/test_gpu_acquisition.py for these kernels)
        if kind == lib.ACQ_EI:
            np.testing.assert_allclose(step["values"][k], want[k], rtol=1e-9, atol=1e-300)
        else:
            np.testing.assert_allclose(step["values"][k], want[k], rtol=1e-13, atol=0)


def _masked_argmax(values, chosen):
    v = np.array(values, dtype=np.float64, copy=True)
    v[list(chosen)] = -np.inf
    return int(np.argmax(v))


@pytest.mark.parametrize("cid", CIDS)
def test_step_values_are_the_closed_forms_of_the_step_moments(lib, cid):
    run = _cached(lib, cid)
    kinds, params = _acqs(lib)
    assert run["n_samples"] != P.ALL[cid]["Bf"]
    for step in run["steps"]:
        assert np.all(np.isfinite(step["values"]))
        _check_values(lib, step, kinds, params, run["n_samples"])


@pytest.mark.parametrize("cid", CIDS)
def test_next_is_the_argmax_over_the_candidates_not_chosen(lib, cid):
    run = _cached(lib, cid)
    picks = P.ALL[cid]["picks"]
    for j, step in enumerate(run["steps"]):
        assert step["next"] == _masked_argmax(step["values"][0], picks[: j + 1]), (cid, j)


def test_two_candidates_one_step(lib):
    cid = CIDS[0]
    c = P.ALL[cid]
    assert c["m"] == 2 and c["picks"] == [1]
    assert _cached(lib, cid)["steps"][0]["next"] == 0


def test_a_draw_with_non_finite_values_is_dropped(lib):
    """A NaN fantasy noise makes draw 1's update NaN: its means are NaN and its variances clip to 0, so its LCB and mean
    values are non-finite (the draw is left out) while its EI (0 where std is not positive) and std stay in the sum."""
    cid = CIDS[3]
    c = P.ALL[cid]
    _X, _y, _a, H, _ = P.problem(cid)
    assert c["Bf"] == 3 and not c["kb"]
    noise = c["base_alpha"] + np.exp(H[:3, -1])
    noise[1] = np.nan
    run = _case_run(lib, cid, noise=noise)
    kinds, params = _acqs(lib)
    for j, step in enumerate(run["steps"]):
        assert np.all(np.isnan(step["mean"][1])) and np.all(step["var"][1] == 0.0)
        assert np.all(np.isfinite(step["mean"][[0, 2]])) and np.all(np.isfinite(step["values"]))
        _check_values(lib, step, kinds, params, run["n_samples"])
        assert step["next"] == _masked_argmax(step["values"][0], c["picks"][: j + 1])


def test_every_draw_dropped_gives_zeros_and_the_lowest_free_index(lib):
    """EI over y_opt = +inf is +inf wherever std > 0: every draw is non-finite, every value 0, the first index not chosen wins."""
    cid = CIDS[3]
    picks = [0, 1, 5]
    run = _case_run(lib, cid, picks=picks, lies=[0.5, -0.5, 0.0], acqs=([lib.ACQ_EI], [np.inf]))
    for step, want in zip(run["steps"], (1, 2, 2)):
        assert np.all(step["var"] > 0) and np.all(step["values"] == 0.0)
        assert step["next"] == want


def test_duplicated_candidates_tie_to_the_lower_index(lib):
    """Candidate rows i and i + 150 are the same point (the pairs straddle the 256-candidate blocks): their moments and values
    are the same bits, and the argmax takes the lower of a tied pair."""
    cid = CIDS[1]
    Xc, _picks, _lies = P.fantasy_inputs(cid)
    half = 150
    Xd = np.vstack([Xc[:half], Xc[:half]])
    picks = [7, half + 20, 3]
    run = _case_run(lib, cid, Xc=Xd, picks=picks, lies=[0.4, -1.0, 0.2])
    for j, step in enumerate(run["steps"]):
        for a in (step["mean"], step["var"], step["values"]):
            assert _same(a[:, :half], a[:, half:])
        nxt = _masked_argmax(step["values"][0], picks[: j + 1])
        assert step["next"] == nxt
        assert nxt < half or nxt - half in picks[: j + 1]


# ------------------------------------------------------------------------------------------------------------------------------
# invariants, bitwise
# ------------------------------------------------------------------------------------------------------------------------------
def test_kriging_believer_keeps_the_means_and_shares_the_variances(lib):
    cid = CIDS[6]
    c = P.ALL[cid]
    assert c["kb"]
    kb = _cached(lib, cid)
    cl = _case_run(lib, cid, lies=np.linspace(-1.5, 1.5, len(c["picks"])))
    moved = False
    for s_kb, s_cl in zip(kb["steps"], cl["steps"]):
        assert _same(s_kb["mean"], kb["begin"][0])
        assert _same(s_kb["var"], s_cl["var"])
        moved |= not _same(s_cl["mean"], cl["begin"][0])
    assert moved


def test_two_identical_runs_agree(lib):
    cid = CIDS[3]
    a, b = _cached(lib, cid), _case_run(lib, cid)
    assert _same(a["begin"][0], b["begin"][0]) and _same(a["begin"][1], b["begin"][1])
    for sa, sb in zip(a["steps"], b["steps"]):
        assert sa["next"] == sb["next"]
        for k in ("values", "mean", "var"):
            assert _same(sa[k], sb[k]), k


def test_a_draw_does_not_depend_on_the_draws_that_share_its_run(lib):
    """Row b of the B = 3 run is the B = 1 run of that row alone (its posterior built alone as well)."""
    cid = CIDS[3]
    c = P.ALL[cid]
    _X, _y, _a, H, _ = P.problem(cid)
    assert c["Bf"] == 3
    full = _cached(lib, cid)
    for b in range(3):
        one = _case_run(lib, cid, H=H[b : b + 1], Bf=1)
        assert _same(one["begin"][0][0], full["begin"][0][b]) and _same(one["begin"][1][0], full["begin"][1][b])
        for s1, s3 in zip(one["steps"], full["steps"]):
            assert _same(s1["mean"][0], s3["mean"][b]) and _same(s1["var"][0], s3["var"][b]), b


def test_fewer_draws_than_resident_posteriors(lib):
    """B = 1 over three resident posteriors is the first of them: the same bits as with that posterior built alone."""
    cid = CIDS[2]
    c = P.ALL[cid]
    _X, _y, _a, H, _ = P.problem(cid)
    assert c["Bf"] == 1 and c["B"] == 3
    a, b = _cached(lib, cid), _case_run(lib, cid, H=H[:1])
    for sa, sb in zip(a["steps"], b["steps"]):
        assert sa["next"] == sb["next"]
        for k in ("values", "mean", "var"):
            assert _same(sa[k], sb[k]), k


def test_the_same_index_twice_is_legal(lib):
    cid = CIDS[3]
    run = _case_run(lib, cid, picks=[5, 5, 9], lies=[0.3, 0.3, -0.2])
    for j, step in enumerate(run["steps"]):
        assert np.all(np.isfinite(step["mean"])) and np.all(np.isfinite(step["var"])) and np.all(step["var"] >= 0.0)
        assert np.all(np.isfinite(step["values"])) and step["next"] not in [5, 5, 9][: j + 1]
    # conditioning twice on one point shrinks its variance again, and no other grows
    assert np.all(run["steps"][1]["var"][:, 5] < run["steps"][0]["var"][:, 5])
    assert np.all(run["steps"][1]["var"] <= run["steps"][0]["var"])


# ------------------------------------------------------------------------------------------------------------------------------
# limits are errors
# ------------------------------------------------------------------------------------------------------------------------------
def _code(lib, call):
    with pytest.raises(lib.BgpError) as e:
        call()
    return int(re.search(r"code (\d+)", str(e.value)).group(1))


def test_limits_are_error_codes(lib):
    rng = np.random.RandomState(0)
    n, d, m = 20, 2, 12
    X, y, Xc = rng.uniform(size=(n, d)), rng.randn(n), rng.uniform(size=(m, d))
    H = np.array([[0.0, -1.0, -1.2, -4.0], [0.1, -1.1, -0.9, -5.0]])
    Hk, noise = _noise_off(H), 1e-8 + np.exp(H[:, -1])
    nul, nxt, buf = C.cast(None, C.POINTER(C.c_double)), np.zeros(1, dtype=np.int32), np.empty((2, m))
    ctx = lib.Context(X, y, 1e-8, max_batch=2)
    try:
        raw = ctx._lib

        def step_rc(p):
            return raw.bgp_fantasy_step(ctx._h, p, lib.BGP_LIE_VALUE, 0.0, nxt.ctypes.data_as(C.POINTER(C.c_int)), nul)

        def moments_rc():
            return raw.bgp_fantasy_moments(ctx._h, buf.ctypes.data_as(C.POINTER(C.c_double)),
                                           buf.ctypes.data_as(C.POINTER(C.c_double)))

        def begin(Hb=Hk[:1], nz=noise[:1], kinds=(lib.ACQ_EI,), qmax=3):
            ctx.fantasy_begin(Hb, nz, Xc, 0.0, 1.0, list(kinds), [np.nan] * len(kinds), 4, qmax)

        # no state yet, no resident posterior yet
        assert step_rc(0) == ERR_STATE and moments_rc() == ERR_STATE
        assert _code(lib, begin) == ERR_STATE
        assert np.all(ctx.posterior(H[:1], want_alpha=False)["status"] == 0)
        assert _code(lib, lambda: begin(Hb=Hk, nz=noise)) == ERR_STATE  # two draws, one resident posterior
        assert _code(lib, lambda: begin(qmax=m)) == ERR_INVALID
        assert _code(lib, lambda: begin(kinds=(lib.ACQ_EI, 9))) == ERR_INVALID
        assert _code(lib, lambda: begin(kinds=(lib.ACQ_EI,) * (lib.ACQ_MAX + 1))) == ERR_INVALID
        assert step_rc(0) == ERR_STATE and moments_rc() == ERR_STATE  # (a refused begin leaves no state)
        begin(qmax=1)
        assert step_rc(-1) == ERR_INVALID and step_rc(m) == ERR_INVALID
        assert raw.bgp_fantasy_step(ctx._h, 0, 7, 0.0, nxt.ctypes.data_as(C.POINTER(C.c_int)), nul) == ERR_INVALID
        assert step_rc(3) == 0 and moments_rc() == 0
        assert step_rc(4) == ERR_INVALID  # past qmax
        begin(qmax=2)
        assert np.all(ctx.posterior(H[:1], want_alpha=False)["status"] == 0)
        assert step_rc(0) == ERR_STATE  # the posteriors the state was built on are gone
        ctx.fantasy_end()
        assert step_rc(0) == ERR_STATE and moments_rc() == ERR_STATE
        ctx.set_warp(np.zeros(2 * d))
        assert _code(lib, begin) == ERR_INVALID  # a warp is set
        ctx.set_warp(None)
    finally:
        ctx.close()
    d = 33
    ctx = lib.Context(rng.uniform(size=(n, d)), y, 1e-8, max_batch=1)
    try:
        h = np.concatenate([[0.0], np.full(d, 0.3), [-np.inf]])[None, :]
        assert _code(lib, lambda: ctx.fantasy_begin(h, [1e-4], rng.uniform(size=(m, d)), 0.0, 1.0, [lib.ACQ_EI], [np.nan], 1,
                                                    2)) == ERR_INVALID
    finally:
        ctx.close()
