"""The replay of the device-resident ensemble sampler (tests/_mcmcref.py) without a device: what tests/test_cpu_cv_reference.py
does for tests/_cvref.py.

* The fp64 replay -- ``oracle.gp_oracle.lml`` and the host's own prior callables, the computation the device restates -- walks
  the long-double replay's chain bit for bit on every case, and every one of its log-probabilities (the rejected proposals'
  too) is within tol("lml") / 10 of the long-double value on ``lp_scale``.
* The long-double prior formulas agree with the host callables.
* Conditions on the inputs (not measurements: the seeds are chosen so that they hold): every finite accept margin is >= 1000 x
  the LML tolerance on ``lp_scale`` of the two log-probabilities it compares, so no correct fp64 device can decide an accept
  test differently; every case outside groups D and G has accepted and rejected moves and a walker that moves between two
  consecutive steps; no accept test is left out -- the non-finite ones of group G are compared by their outcome.
* Each slip of ``_mcmcref.SLIPS`` changes the chain of a case in group A and of a case in group B or C.  ``fixed_counted``
  is the exception, for a reason and not for a margin: no case of group A has a fixed canonical entry, so there the slip
  changes no bit (asserted); it has to change BOTH cases of group B.
* Group W (warped walkers): the fp64 replay there is ``gp_oracle.lml_warped`` (scipy's Beta CDF) against mpmath + long double,
  within a tenth of ``tol("lml", kappa of the warped matrix, n, warp sensitivity)``; the same three conditions; each slip of
  ``_mcmcref.WARP_SLIPS`` changes the chain of a warped case.

Lines printed with ``pytest -s`` start with ``MCMCREF``."""
import time

import numpy as np
import pytest

import _precision as P

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

import _mcmcref as R  # noqa: E402

MARGIN = 10.0
CIDS = [c["id"] for c in R.CASES]
T0 = time.time()


def test_cases_reach_every_branch_they_were_written_for():
    A = [c for c in R.CASES if c["group"] == "A"]
    assert {c["n"] for c in A} == {1, 2, 17, 64, 65, 127, 128}
    assert {(c["stationary"], c["form"]) for c in A} == set(P.FAMILIES)
    assert {c["d"] for c in A} == {1, 2, 3} and {c["vec_alpha"] for c in A} == {True, False}
    for c in R.CASES:
        inp = R.inputs(c["id"])
        assert R.expected_form(inp["n"], inp["p"], inp["d"] + 2, inp["W"], inp["nwarp"]) == c["runs"], c["id"]
        assert inp["plan"][0].shape == (2 * c["steps"], c["W"] // 2)
    shapes = {c["id"][:2]: (R.inputs(c["id"])["p"], R.inputs(c["id"])["d"] + 2, c["W"]) for c in R.CASES}
    assert shapes["E0"][:2] == (64, 64) and shapes["E1"][:2] == (65, 65) and shapes["E2"][:2] == (2, 65)

    def doubles(p, _hp, W):
        return W * p + W + 3 * (W // 2) + 2 * (W // 2) * p

    assert doubles(*shapes["F0"]) == 20217 and doubles(*shapes["F1"]) == 20510 and R.MCMC_LDS_DOUBLES == 20480
    b0 = R.inputs("B0_n60_d3_fixed_c_shared_ls")
    assert list(b0["h_src"]) == [-1, 0, 0, 0, 1] and b0["p"] == 2
    assert list(R.inputs("B1_n60_d3_fixed_noise")["h_src"]) == [0, 1, 2, 3, -1]
    assert list(R.inputs("C0_n60_d2_normal_priors")["prior_kind"]) == [3, 3, 3, 3]
    assert sorted(set(R.inputs("C1_n60_d2_mixed_priors")["prior_kind"])) == [1, 2, 3]
    assert R.inputs("D0_n17_d1_W2")["W"] == 2
    assert [R.ALL[g]["runs"] for g in R.GROW] == ["fused", "fused", "step_lds"]
    assert R.ALL[R.SEGMENT_CASE]["group"] == "A" and R.ALL[R.SEGMENT_CASE]["steps"] == 4
    # group W: warped walkers, never fused; the layout [kernel entries, alphas of all columns, betas of all columns]
    Wc = {c["id"][:2]: (c, R.inputs(c["id"])) for c in R.CASES if c["group"] == "W"}
    assert sorted(Wc) == ["W%d" % k for k in range(8)]
    for c, inp in Wc.values():
        d, ng = inp["d"], inp["ng"]
        assert inp["nwarp"] == 2 * d and inp["p"] == ng + 2 * d and c["runs"] != "fused" and (inp["h_src"] < ng).all()
        assert inp["roles"][ng:] == ["wa"] * d + ["wb"] * d and inp["coords0"].shape == (c["W"], inp["p"])
        assert c["W"] == 2 * inp["p"] + 2 or c["id"][:2] in ("W6", "W7")
    assert R.expected_form(17, 5, 3, 12, 0) == "fused" and Wc["W0"][0]["runs"] == "step_lds" and Wc["W0"][1]["p"] == 5
    assert [Wc[k][1]["n"] for k in ("W0", "W1", "W2")] == [17, 65, 129] and np.ndim(Wc["W1"][1]["alpha"]) == 1
    w3 = Wc["W3"][1]
    assert (w3["ng"], w3["d"] + 2, w3["p"]) == (2, 5, 8)  # the warp offset is not the canonical vector's length
    w4 = Wc["W4"][1]
    assert list(w4["prior_kind"]) == [1, 2, 2, 3, 3, 3, 2] and list(w4["h_src"]) == [0, 1, 2, -1]
    assert [tuple(v[:2]) for v in w4["prior_par"][3:6]] == [(0.2, 0.3), (0.2, 0.3), (-0.1, 0.5)]
    # (far from the identity warp, and 0.2 wide in the warp entries: a mover's warp is not its proposal's)
    assert abs(w4["coords0"][:, 3:5].mean() - 0.3) < 0.1 and abs(w4["coords0"][:, 5:].mean() + 0.2) < 0.1
    assert w4["coords0"][:, 3:].std(axis=0).min() > 0.1 and w4["coords0"][:, :3].std(axis=0).max() < 0.02
    assert Wc["W5"][1]["n"] <= 128 and Wc["W5"][0]["edges"]
    assert doubles(212, 72, 48) == 20472 and doubles(212, 72, 50) == 21325
    assert [Wc[k][1]["p"] for k in ("W6", "W7")] == [212, 212] and [Wc[k][0]["runs"] for k in ("W6", "W7")] == ["step_lds", "step_hbm"]


def test_long_double_prior_formulas_agree_with_the_host_callables():
    """The three formulas of bgp_mcmc.h in long double from the device's table against the callables the host-driven loop
    evaluates: 1e-13 relative on t in [-12, 6]."""
    import scipy.stats as st
    from bayes_skopt_amd.bayesgpr import _device_prior

    d = R._default_callables()
    grid = np.linspace(-12.0, 6.0, 145)
    for name, fn in (("half-Normal", d["c"]), ("round-flat", d["ls"]), ("Normal", st.norm(loc=-1.0, scale=1.5).logpdf)):
        kind, par = _device_prior(fn)
        ref = R.prior_terms_ld(np.full(len(grid), kind), np.tile(par, (len(grid), 1)), grid)
        got = np.array([float(fn(t)) for t in grid])
        rel = np.abs(got.astype(np.longdouble) - ref) / np.abs(ref)
        print("MCMCREF prior kind %d (%s): worst relative difference host callable vs long double %.3g" % (kind, name, float(rel.max())))
        assert np.all(np.abs(ref) > 0) and float(rel.max()) <= 1e-13, (name, float(rel.max()))


@pytest.mark.parametrize("cid", CIDS)
def test_fp64_replay_walks_the_long_double_chain_and_the_inputs_hold_their_conditions(cid):
    c, inp = R.ALL[cid], R.inputs(cid)
    t0 = time.time()
    ref, got = R.replay_full(cid), R.replay64(cid)
    chain, lps, coords, logp, nacc, margins = R.replay(cid)
    # the fp64 replay: same positions bit for bit, same decisions, log-probabilities within tol / 10
    for key in ("chain", "coords", "naccepted", "accepted"):
        assert np.array_equal(ref[key], got[key]), key
    fin = np.isfinite(ref["lp"])
    assert np.array_equal(fin, np.isfinite(got["lp"])) and np.array_equal(np.isneginf(ref["lps"]), np.isneginf(got["lps"]))
    tol = R.proposal_tolerance(cid)[fin]  # (P.tol("lml", kappa, n, sens) of every proposal; sens = 0 without a warp)
    assert np.all(np.isfinite(tol)) and (c["warp"] or np.array_equal(tol, [P.tol("lml", k, inp["n"]) for k in ref["kappa"][fin]]))
    reach = float((np.abs(got["lp"][fin] - ref["lp"][fin]) / ref["scale"][fin] / tol).max())
    assert reach <= 1.0 / MARGIN, reach
    # condition 1: every finite margin clears 1000 x the tolerance of the two log-probabilities it compares
    bound = R.margin_bounds(cid)
    f = ref["finite"]
    assert np.array_equal(np.sort(margins), np.sort(ref["margin"][f])) and np.all(np.isfinite(bound[f]))
    over = float((ref["margin"][f] / bound[f]).min()) if f.any() else np.inf
    assert over >= 1.0, over
    # condition 3: nothing is left out -- a test is either finite (and has a margin) or one of group G's, compared by its outcome
    assert f.all() or c["edges"]
    acc, rej = int(ref["accepted"].sum()), int((~ref["accepted"]).sum())
    moved = bool(np.any(chain[1:] != chain[:-1]) if c["steps"] > 1 else np.any(chain[0] != inp["coords0"]))  # (one step: from the start)
    print("MCMCREF %s runs %s: accepted %d rejected %d non-finite tests %d; smallest margin / bound %.3g; fp64 replay %.4f tol, "
          "kappa <= %.3g; %.2f s" % (cid, c["runs"], acc, rej, int((~f).sum()), over, reach, float(np.nanmax(ref["kappa"])),
                                      time.time() - t0))
    # condition 2
    if c["group"] not in ("D", "G"):
        assert acc >= 1 and rej >= 1 and moved, (acc, rej, moved)
    assert nacc.sum() == acc and np.array_equal(lps[-1], logp) and np.array_equal(chain[-1], coords)


@pytest.mark.parametrize("cid", [c["id"] for c in R.CASES if c["edges"]])
def test_the_edges_of_group_g_are_what_they_were_built_to_be(cid):
    """(and those of the warped case W5: there the two proposals with lp = -inf have every prior term finite and every kernel
    entry where its partner has it -- a warp ALPHA entry at +800, a warp BETA entry at -800 decide)"""
    inp, ref = R.inputs(cid), R.replay_full(cid)
    if inp["nwarp"]:
        mv, pr, zz = inp["plan"][:3]
        ng, d = inp["ng"], inp["d"]
        for key, col, target in (("nan_reject", ng, 800.0), ("inf_reject", ng + d + 1, -800.0)):
            h, i = inp["edges"][key]
            s, c = inp["coords0"][mv[h, i]], inp["coords0"][pr[h, i]]
            q = c - (c - s) * zz[h, i]
            assert h == 0 and abs(q[col] - target) < 1e-9 and np.array_equal(np.delete(q, col), np.delete(c, col))
            terms = R.prior_terms_ld(inp["prior_kind"], inp["prior_par"], q)
            assert np.all(np.isfinite(terms.astype(np.float64))) and not R._warp_ok(q[ng:]) and R._warp_ok(c[ng:])
            assert abs(q[col]) > 745.0  # exp is 0 or inf in fp64
    e = inp["edges"]
    a, b = e["minus_inf_walkers"]
    assert np.isneginf(inp["logp0"][[a, b]]).all() and np.isfinite(np.delete(inp["logp0"], [a, b])).all()
    for idx in e["first_finite_accept"]:  # accepted whatever logu is: the test's left side is +inf
        assert np.isfinite(ref["lp"][idx]) and ref["accepted"][idx] and not ref["finite"][idx]
    assert inp["plan"][0][e["first_finite_accept"][0]] == a and inp["plan"][0][e["first_finite_accept"][1]] == b
    for key in ("nan_reject", "inf_reject"):  # lp = -inf on a proposal whose coordinates are all finite
        assert np.isneginf(ref["lp"][e[key]]) and not ref["accepted"][e[key]] and not ref["finite"][e[key]]
    assert inp["plan"][0][e["nan_reject"]] == b and np.isneginf(ref["lps"][0, b]) and np.isfinite(ref["lps"][-1, b])
    assert np.isfinite(inp["logp0"][inp["plan"][0][e["inf_reject"]]])
    assert np.isneginf(inp["plan"][4][e["u_zero"]]) and np.isfinite(ref["lp"][e["u_zero"]]) and ref["accepted"][e["u_zero"]]
    assert inp["plan"][4][e["u_one"]] == 0.0 and ref["finite"][e["u_one"]]
    assert int((~ref["finite"]).sum()) == 5  # and no other test is out of the margins
    # every proposal of the run has finite coordinates: the device's info words stay [0, 0, -1, 0]
    assert np.all(np.isfinite(ref["chain"])) and abs(inp["plan"][2][e["nan_reject"]]) < 1e7


def test_every_slip_changes_a_chain():
    groups = {g: [c["id"] for c in R.CASES if c["group"] == g] for g in "ABC"}
    for slip in R.SLIPS:
        bites = {g: [cid for cid in ids if not np.array_equal(R.replay64(cid, slip)["chain"], R.replay64(cid)["chain"])]
                 for g, ids in groups.items()}
        print("MCMCREF slip %-14s changes the chain of %d / %d cases of group A, %d / %d of B, %d / %d of C"
              % (slip, len(bites["A"]), len(groups["A"]), len(bites["B"]), len(groups["B"]), len(bites["C"]), len(groups["C"])))
        if slip == "fixed_counted":  # (no fixed entry in group A: nothing to count)
            assert all((R.inputs(cid)["h_src"] >= 0).all() for cid in groups["A"]) and not bites["A"]
            assert len(bites["B"]) == len(groups["B"])
        else:
            assert bites["A"], slip
            assert bites["B"] or bites["C"], slip


def test_every_warp_slip_changes_a_warped_chain():
    """The mistakes the warped path could make without any other test noticing (``_mcmcref.WARP_SLIPS``): the scatter handing
    betas where alphas belong; warp parameters read from the mover's current row; a zero stride (every proposal of a half-step
    sees proposal 0's warped matrix); the warp entries taken from ``hp`` onward instead of from ``ng`` (neutral where the two are
    equal -- asserted -- and biting on W3, where ng = 2 and hp = 5); the prior summed over the kernel entries only; the LML on
    the unwarped inputs.  Each changes the chain of at least one of W0 .. W5, and every one of them changes W4: different priors
    on alphas and betas, a start far from the identity and 0.2 wide in the warp entries, ng = 3 against hp = 4.  The other
    ensembles are 1e-2 wide, so there a mover's warp is close to its proposal's and ``warp_of_mover`` flips an accept test only
    on W5, where a mover holds a finite warp entry and its proposal has +-800.  A chain changes only where an accept test
    flips; on the device every slip also moves the stored log-probabilities, which are held to the tolerance."""
    ids = [c["id"] for c in R.CASES if c["group"] == "W" and c["id"][:2] not in ("W6", "W7")]
    for slip in R.WARP_SLIPS:
        bites = [cid for cid in ids if not np.array_equal(R.replay64(cid, slip)["chain"], R.replay64(cid)["chain"])]
        print("MCMCREF slip %-19s changes the chain of %d / %d warped cases: %s" % (slip, len(bites), len(ids), " ".join(b[:2] for b in bites)))
        assert bites, slip
        assert any(b.startswith("W4") for b in bites), slip
        if slip == "warp_offset_hp":
            assert any(b.startswith("W3") for b in bites)
            for cid in ids:  # where ng == hp the slip reads the right entries
                inp = R.inputs(cid)
                assert (cid in bites) or inp["ng"] == inp["d"] + 2, cid


def test_run_time():
    print("MCMCREF module run time %.1f s" % (time.time() - T0))
