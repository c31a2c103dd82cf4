"""The device-resident ensemble sampler against an independent replay of its plan (tests/_mcmcref.py): the fused n <= 128
half-step (``mcmc_small_kernel``) on a ragged block, every kernel family, a vector alpha, fixed canonical entries, every prior
kind, -inf log-probabilities and the smallest ensemble; both sides of ``p, hp <= 64``; both sides of the step kernel's 20 480
doubles; a plan handed over in segments; a context that grows through n = 128; walkers that carry their own input warp
(group W: a ragged block, two block columns, ng != hp, different priors on alphas and betas, warp entries at +-800, both sides
of the 20 480 doubles).

The reference shares nothing with the device library: positions are replayed in fp64 with the device's operation order and have
to be EQUAL; log-probabilities come from ``oracle.hp_oracle`` in long double and have to be within ``_precision.tol("lml")`` on
``lp_scale`` at the stored position -- tests/test_cpu_mcmc_reference.py shows that the fp64 computation reaches a tenth of that
and that every accept test of every case is decided by at least 1000 times it.  Every run has to report the form of the
half-step its case was written for (``bgp_mcmc_form``).  Lines printed with ``pytest -s`` start with ``PRECISION``."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

import _mcmcref as R  # noqa: E402

NAMES = ("chain", "lps", "coords", "logp", "naccepted")


@pytest.fixture(scope="module")
def lib():
    import bayes_skopt_amd  # noqa: F401
    from bayes_skopt_amd import _lib

    assert _lib.device_count() >= 1
    return _lib


def _context(lib, inp):
    return lib.Context(inp["X"], inp["y"], inp["alpha"], form=inp["form"], stationary=inp["stationary"], max_batch=inp["W"] // 2)


def _tables(inp):
    return inp["h_src"], inp["h_fixed"], inp["prior_kind"], inp["prior_par"]


def _run(lib, cid, ctx=None, coords0=None):
    inp = R.inputs(cid)
    own = ctx is None
    ctx = _context(lib, inp) if own else ctx
    try:
        out = ctx.mcmc_run(inp["coords0"] if coords0 is None else coords0, inp["logp0"], inp["plan"], *_tables(inp),
                           nwarp=inp["nwarp"])
        return out, ctx.mcmc_form
    finally:
        if own:
            ctx.close()


def _compare(cid, out, form, tag=""):
    """A device run against the long-double replay of its case."""
    c, ref = R.ALL[cid], R.replay_full(cid)
    chain, lps, coords, logp, nacc, info = out
    tl, to = R.lps_tolerance(cid)
    worst = 0.0
    for got, want, scale, tol in ((lps, ref["lps"], ref["lps_scale"], tl), (logp, ref["logp"], ref["logp_scale"], to)):
        fin = np.isfinite(want)
        if fin.any():
            worst = max(worst, float((np.abs(got[fin] - want[fin]) / scale[fin] / tol[fin]).max()))
    print("PRECISION %-34s %-9s %-7s lp     err/tol %.3e  ran %s (written for %s); accepted %d of %d%s"
          % (cid, c["stationary"], c["form"], worst, form, c["runs"], int(nacc.sum()), ref["accepted"].size, tag))
    assert form == c["runs"], "the case was written for the %s form and ran on %s" % (c["runs"], form)
    assert np.array_equal(chain, ref["chain"]), "max position difference %.3e" % np.nanmax(np.abs(chain - ref["chain"]))
    assert np.array_equal(coords, ref["coords"]) and np.array_equal(nacc, ref["naccepted"])
    for got, want in ((lps, ref["lps"]), (logp, ref["logp"])):  # -inf exactly where the reference has it, finite elsewhere
        assert np.array_equal(np.isneginf(got), np.isneginf(want)) and np.array_equal(np.isfinite(got), np.isfinite(want))
    assert worst <= 1.0, worst
    assert list(info) == [0, 0, -1, 0], info


@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES if c["group"] != "grow"])
def test_device_run_equals_the_replay_of_its_plan(lib, cid):
    """Group W, the warped walkers: the split ng = p - nwarp of ``mcmc_step_kernel``, the pair-wise sum of the warp priors, the
    scatter of a proposal's last 2 d entries into the per-proposal Beta-CDF design matrices and their row stride, against the
    replay's mpmath warp and long-double LML; the tolerance carries the Beta-CDF budget (``sens``) at kappa of the WARPED Gram
    matrix.  A warped ensemble is never fused.
    (W5 at n = 60 sends two proposals whose warp parameter is exp(800) = inf or exp(-800) = 0: ``bgp_betainc`` answers NaN for
    every point, the Gram kernel builds a matrix of NaN, and on the launch schedule a matrix of one block column is ONE
    ``potrf_kernel<0, 0, 0>`` launch with one workgroup per matrix: ``pf_block<0, ..., 0>`` with PRE = 0, ``wrow`` = nullptr and
    no chain arguments factorises it like any other -- its loops run over block indices, its one early exit is the
    workgroup-uniform failure word read behind a barrier, it waits for nothing but its own barriers -- and leaves a non-zero
    status and a non-finite log-likelihood, which the step kernel turns into -inf.  nblk = 1 never takes the launch-free
    path: ``bgp_persist_fits`` asks for two block columns.)
    Measured on the device (err / tol of the stored log-probabilities; every case EQUAL in positions and on its form):
    PRECISION W0_n17_d1_warp                     matern52  product lp     err/tol 2.596e-03  ran step_lds; accepted 26 of 36
    PRECISION W1_n65_d2_rbf_sum_vec_warp         rbf       sum     lp     err/tol 3.551e-03  ran step_lds; accepted 36 of 54
    PRECISION W2_n129_d2_m32_warp                matern32  product lp     err/tol 2.798e-03  ran step_lds; accepted 41 of 54
    PRECISION W3_n60_d3_iso_fixc_warp            matern52  product lp     err/tol 1.576e-03  ran step_lds; accepted 31 of 54
    PRECISION W4_n60_d2_fixnoise_m12_sum_warp_priors matern12 sum     lp     err/tol 1.229e-03  ran step_lds; accepted 24 of 48
    PRECISION W5_n60_d2_edges_warp               matern52  product lp     err/tol 1.505e-03  ran step_lds; accepted 37 of 54
    PRECISION W6_n3_d70_W48_lds_warp             matern52  product lp     err/tol 9.309e-04  ran step_lds; accepted 34 of 48
    PRECISION W7_n3_d70_W50_hbm_warp             matern52  product lp     err/tol 6.841e-04  ran step_hbm; accepted 28 of 50"""
    out, form = _run(lib, cid)
    _compare(cid, out, form)
    if R.ALL[cid]["edges"]:  # the edges by their outcome
        e, inp = R.inputs(cid)["edges"], R.inputs(cid)
        a, b = e["minus_inf_walkers"]
        chain, lps = out[0], out[1]
        assert np.isfinite(lps[0, a]) and np.isneginf(lps[0, b]) and np.isfinite(lps[1, b])
        assert not np.array_equal(chain[0, a], inp["coords0"][a]) and np.array_equal(chain[0, b], inp["coords0"][b])
        m = inp["plan"][0][e["inf_reject"]]
        assert np.array_equal(chain[0, m], inp["coords0"][m]) and lps[0, m] == inp["logp0"][m]


def test_a_plan_handed_over_in_segments_equals_the_one_shot_run(lib):
    cid = R.SEGMENT_CASE
    inp = R.inputs(cid)
    one, form = _run(lib, cid)
    ctx = _context(lib, inp)
    try:
        ctx.mcmc_begin(inp["coords0"], inp["logp0"], inp["steps"], *_tables(inp))
        seg_form = ctx.mcmc_form
        for lo, hi in ((0, 1), (1, 3), (3, 4)):  # steps(1) / steps(2) / steps(1)
            ctx.mcmc_steps(tuple(a[2 * lo : 2 * hi] for a in inp["plan"]))
        seg = ctx.mcmc_end()
    finally:
        ctx.close()
    assert inp["steps"] == 4 and seg_form == form == R.ALL[cid]["runs"]
    for name, a, b in zip(NAMES, one, seg):
        assert np.array_equal(a, b), name
    assert list(seg[5]) == [0, 0, -1, 0]
    _compare(cid, seg, seg_form, tag="; in segments")


def test_one_context_grown_through_n_128_leaves_the_fused_form_when_it_has_to(lib):
    """``update_data`` at n = 127 -> 128 -> 129 on ONE context, a 2-step run after each: two on the fused form, the last one on
    the step kernel, each against the replay on its own rows."""
    forms = []
    first = R.inputs(R.GROW[0])
    ctx = _context(lib, first)
    try:
        for k, cid in enumerate(R.GROW):
            inp = R.inputs(cid)
            if k:
                ctx.update_data(inp["X"], inp["y"], inp["alpha"])
            out, form = _run(lib, cid, ctx=ctx)
            _compare(cid, out, form, tag="; grown to n = %d" % inp["n"])
            forms.append(form)
    finally:
        ctx.close()
    assert [R.inputs(cid)["n"] for cid in R.GROW] == [127, 128, 129] and forms == ["fused", "fused", "step_lds"]


def _first_non_finite(inp, coords0):
    """(half-step, is NaN) of the first proposal with a non-finite coordinate, from the start rows: a walker that holds one
    never moves (its proposals, and those that read it as a partner, have lp = -inf), and the others stay finite."""
    mv, pr, zz = inp["plan"][:3]
    for h in range(mv.shape[0]):
        with np.errstate(all="ignore"):
            q = coords0[pr[h]] - (coords0[pr[h]] - coords0[mv[h]]) * zz[h][:, None]
        if not np.all(np.isfinite(q)):
            assert np.isnan(q).any() != np.isinf(q).any()  # (one kind per half-step: the walker is a mover or a partner in it)
            return h, bool(np.isnan(q).any())
    raise AssertionError("no non-finite proposal")


def test_a_non_finite_proposal_on_the_fused_form_sets_the_info_words(lib):
    """What ``test_a_non_finite_proposal_raises_...`` of tests/test_gpu_resident.py checks on the step kernel, on the fused
    form: one start coordinate infinite or NaN, handed in with its log-probabilities.  ``info[0] == 1``; ``info[2]`` is the
    first half-step in which that walker moves or is a partner; ``info[3]`` tells the two kinds apart -- a mover at +inf
    proposes +inf, a partner at +inf proposes ``inf - inf`` = NaN.
    (``pf_block<1, ...>`` with ``gen`` set factorises a matrix of NaN like any other: its loops run over block indices, its
    one early exit is the workgroup-uniform failure word read behind a barrier, and with PRE = 0 and no ``wrow`` it waits for
    nothing but its own barriers.)"""
    cid = "G0_n60_d2_edges_fused"
    inp = R.inputs(cid)
    mv, pr = inp["plan"][0], inp["plan"][1]
    others = [w for w in range(inp["W"]) if w not in mv[0]]
    walkers = {"moves in half-step 0": int(mv[0, 3]), "partner in half-step 0": int(pr[0, 3])}
    idle = [w for w in others if w not in pr[0]]
    if idle:
        walkers["first seen as a mover of half-step 1"] = idle[0]
    seen = set()
    for what, w in walkers.items():
        for bad in (np.inf, np.nan):
            coords0 = inp["coords0"].copy()
            coords0[w, 1] = bad
            want = _first_non_finite(inp, coords0)
            out, form = _run(lib, cid, coords0=coords0)
            info = [int(v) for v in out[5]]
            print("PRECISION %s: walker %d (%s) at %s: info %s, expected half-step %d, NaN %d" % (cid, w, what, bad, info, want[0], want[1]))
            assert form == "fused"
            assert info[0] == 1 and info[1] == 0 and info[2] == want[0] and info[3] == int(want[1]), (what, bad, info, want)
            assert np.array_equal(out[2][w], coords0[w], equal_nan=True)  # it never moved
            seen.add((want[0], want[1]))
    assert {(0, False), (0, True)} <= seen
