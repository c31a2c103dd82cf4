"""The reference and the tolerance of the hyper-posterior mixture tests (tests/_mixref.py; ``bgp_predict_mixture`` and its kin,
DESIGN.md section 26), without a device:

* the case list sits on the edges the issue names;
* on every case the fp64 numpy replica of the device's route is within the derived tolerance of the long-double reference for every
  quantity at every point, its quantiles by back-substitution into the reference CDF, and the exact rules hold (one row, identical
  rows, atoms, a dropped row, no row left);
* each of six slips misses the tolerance by >= 10 tol on at least one case: moments rounded to fp32, ``1 - cdf`` for the upper tail,
  ``between`` as ``E[mu^2] - mean^2``, a dropped row without renormalisation, the Gaussian band ``mean + z_p std`` for the quantile, a
  plain unshifted sum for ``logpdf``;
* the closed form itself: the reference CDF against a trapezoid quadrature of the reference density, reference quantiles monotone in p,
  ``cdf + sf = 1``.

Lines printed with ``pytest -s`` start with ``PRECISION``; the worst reach and the bites are recorded in DESIGN.md section 26."""
import numpy as np
import pytest

import _mixref as R
import _precision as P

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

CIDS = [c["id"] for c in R.CASES]
QUANTS = ("mean", "within", "between", "cdf", "sf", "logpdf")


def test_the_cases_sit_on_the_stated_edges():
    syn = [R.ALL[c] for c in R.SYN]
    assert {c["B"] for c in syn} == {1, 2, 63, 64, 65, 129}
    assert {c["m"] for c in syn} == {1, 255, 256, 257, 513}
    assert {len(c["probs"]) for c in syn} == {1, 5, 16} and max(len(c["probs"]) for c in syn) == R.QMAX
    assert any(set(c["probs"]) == {1e-6, 0.05, 0.5, 0.95, 1.0 - 1e-6} for c in syn)
    assert {c["special"] for c in syn} == {None, "offset", "zeros", "identical", "groups", "spread", "atom", "atoms", "tails", "nanrow",
                                           "allbad"}
    assert set(R.TAIL_Z) == {8.0, -8.0, 30.0, -30.0, 38.0, -38.0}
    res = [R.ALL[c] for c in R.RES]
    assert {c["pid"] for c in res} == {P.PREDB_CASES[j]["id"] for j in (0, 1, 3, 5, 6)}
    assert {c["noise"] for c in res} == {False, True}
    assert {c["n"] for c in res} == {1, 127, 129, 256, 577} and {c["m"] for c in res} == {1, 129, 256, 257, 513}
    assert {c["Bres"] for c in res} == {1, 3, 9} and any(c["B"] < c["Bres"] for c in res)
    assert {(P.ALL[c["pid"]]["form"]) for c in res} == {"product", "sum"}
    assert [R.ALL[c]["pid"] for c in R.WARP] == [P.WARP_CASES[0]["id"]]
    # the spread case spans nine decades of sd within its point; the zero-weight case has zeros and unequal weights
    sd = np.sqrt(R.inputs("syn_B65_m1_Q5_spread")["var"][:, 0]) * R.Y_STD
    assert sd.min() <= 1.0001e-6 and sd.max() >= 0.9999e3
    w = R.inputs("syn_B65_m1_Q5_zero_weights")["weights"]
    assert (w == 0.0).sum() == 22 and len(set(w)) > 40


def _run(cid, slip=None):
    c = R.ALL[cid]
    inp = R.inputs(cid)
    mean, var = R.moments64(cid)
    return R.replica64(mean, var, inp["weights"], R.Y_MEAN, R.Y_STD, c["probs"], inp["t"], slip=slip)


def _reach(cid, got):
    r = R.ratios(cid, got)
    qr = R.quantile_ratio(cid, got["quantiles"])
    r["quantile"] = float(qr.max())
    return r


@pytest.fixture(scope="module")
def survey():
    out = {}
    for cid in CIDS:
        got = _run(cid)
        out[cid] = dict(got=got, reach=_reach(cid, got))
        print("PRECISION mix %s: fp64 replica reach (tol) %s; solver steps <= %d"
              % (cid, " ".join("%s %.3g" % (q, v) for q, v in out[cid]["reach"].items()), got["iters"]))
    return out


def test_fp64_reaches_the_tolerance_everywhere(survey):
    worst = {q: max(v["reach"][q] for v in survey.values()) for q in QUANTS + ("quantile",)}
    print("PRECISION mix worst reach of the fp64 replica over all cases and points: %s (project margin 0.1: %s); largest solver step "
          "count %d" % (" ".join("%s %.3g" % kv for kv in worst.items()), "holds" if max(worst.values()) <= 0.1 else "does not hold",
                        max(v["got"]["iters"] for v in survey.values())))
    for cid, v in survey.items():
        assert max(v["reach"].values()) <= 1.0, (cid, v["reach"])
        assert R.reference(cid)["keep"].all(), cid  # no point of any case is left out
        assert v["got"]["n_used"] == R.reference(cid)["n_used"]
        assert v["got"]["iters"] < R.ITMAX


def test_the_exact_rules(survey):
    for cid, v in survey.items():
        c, got = R.ALL[cid], v["got"]
        inp = R.inputs(cid)
        if c["special"] == "allbad":
            assert got["n_used"] == 0 and all(np.isnan(got[q]).all() for q in QUANTS) and np.isnan(got["quantiles"]).all()
            continue
        assert (got["between"] >= 0.0).all()
        assert (np.diff(got["quantiles"][np.argsort(c["probs"])], axis=0) >= 0.0).all(), cid  # monotone in p
        if c["B"] == 1:
            mean = R.moments64(cid)[0]
            assert np.array_equal(got["mean"], R.Y_STD * mean[0] + R.Y_MEAN) and (got["between"] == 0.0).all()
        if c["special"] == "identical":
            assert (got["between"] == 0.0).all()
        if c["special"] == "nanrow":
            assert got["n_used"] == c["B"] - 1
        if c["special"] == "atoms":
            assert (got["logpdf"] == -np.inf).all()
        for (k, i), val in R.exact_quantiles(cid).items():
            assert got["quantiles"][k, i] == val, (cid, k, i)
        if c["special"] == "tails":
            assert np.isfinite(got["logpdf"]).all()
            ref = R.reference(cid)
            assert 0.0 < float(P.f(ref["cdf"][0]).min()) < 1e-300 and 0.0 < float(P.f(ref["sf"][0]).min()) < 1e-300
        if c["special"] == "atom":
            assert inp["var"][0, 0] == 0.0 and got["cdf"][0] >= 0.6  # t on the atom: its step counts


def test_identical_components_are_one_gaussian(survey):
    cid = "syn_B64_m1_Q5_identical"
    md = R.model(cid)
    got = survey[cid]["got"]
    for k, p in enumerate(R.ALL[cid]["probs"]):
        want = float(R.ref_quantile(md["mu"][:1, 0], md["sd"][:1, 0], np.ones(1), p))
        ulp = np.spacing(abs(want)) + np.spacing(abs(float(md["mu"][0, 0])))
        print("PRECISION mix identical components p = %g: quantile off by %.2g ulp" % (p, abs(got["quantiles"][k, 0] - want) / ulp))
        # (the CDF evaluation term E over the density, in ulps of the quantile's terms: a few at p = 0.5, ~z_p^2 more in the tails)
        assert abs(got["quantiles"][k, 0] - want) <= 64.0 * ulp


@pytest.mark.parametrize("slip", R.SLIPS)
def test_every_slip_misses_the_tolerance_by_ten(survey, slip):
    bites = {}
    for cid in R.SYN + R.RES[4:6] + R.WARP:  # (every synthetic case, the single-point resident case, the warped one)
        if R.ALL[cid]["special"] == "allbad":
            continue
        r = _reach(cid, _run(cid, slip))
        bites[cid] = max(r.values())
    best = max(bites, key=bites.get)
    print("PRECISION mix slip '%s': largest miss %.3g tol (%s), bites %d of %d cases" % (slip, bites[best], best,
                                                                                         sum(b > 1.0 for b in bites.values()), len(bites)))
    assert bites[best] >= 10.0


def test_reference_cdf_against_quadrature_of_the_density():
    """The closed form, not the precision: F(t) by the trapezoid rule over the reference's own density on 200 001 points from 12 sd
    below the lowest component (the rule's error is h^2 / 12 max |f'| (b - a), below 1e-9 here; the tail beyond carries < 1e-30)."""
    trap = getattr(np, "trapezoid", None) or np.trapz
    for cid, i in (("syn_B2_m257_Q16", 5), ("syn_B63_m1_Q16", 0), ("syn_B65_m1_Q5_zero_weights", 0)):
        md = R.model(cid)
        mu, sd, wn = P.f(md["mu"][:, i]), P.f(md["sd"][:, i]), P.f(md["wn"])
        t = R.inputs(cid)["t"][i]
        x = np.linspace((mu - 12.0 * sd).min(), t, 200001)
        dens = (wn[:, None] * np.exp(-0.5 * ((x[None, :] - mu[:, None]) / sd[:, None]) ** 2) / (sd[:, None] * np.sqrt(2 * np.pi))).sum(axis=0)
        quad, ref = trap(dens, x), float(R.reference(cid)["cdf"][0][i])
        print("PRECISION mix closed form %s point %d: reference cdf %.12g, quadrature %.12g" % (cid, i, ref, quad))
        assert abs(quad - ref) <= 1e-8
        assert abs(float(R.reference(cid)["logpdf"][0][i]) - np.log(dens[-1])) <= 1e-12 * max(1.0, abs(np.log(dens[-1])))


def test_reference_quantiles_are_monotone_and_invert_the_cdf():
    """One column of the two-row case: the bisected long-double quantiles rise strictly with p and put back into the reference's
    tail sum they return p to the long-double bracket's width (1e-17 of f |q| + tail (1 + z^2): ~100 units of its last place)."""
    cid, i = "syn_B2_m257_Q16", 3
    md = R.model(cid)
    col = dict(mu=md["mu"][:, i:i + 1], sd=md["sd"][:, i:i + 1], wn=md["wn"])
    probs = sorted(R.ALL[cid]["probs"])
    q = [R.ref_quantile(col["mu"][:, 0], col["sd"][:, 0], col["wn"], p) for p in probs]
    assert all(a < b for a, b in zip(q, q[1:]))
    for p, v in zip(probs, q):
        up = p > 0.5
        target = hp.LD(1) - hp.LD(p) if up else hp.LD(p)
        tail, tail_b, fb, z = R._tails(col, np.array([v], dtype=hp.LD), up)
        f = float((col["wn"][:, None] * fb).sum())
        scale = f * abs(float(v)) + float((col["wn"][:, None] * tail_b * (1 + z * z)).sum())
        assert abs(float(tail[0] - target)) <= 1e-17 * scale, (p, float(tail[0] - target), scale)


def test_cdf_plus_sf_is_one_where_neither_is_tiny():
    for cid in CIDS:
        ref = R.reference(cid)
        if ref["n_used"] == 0:
            continue
        F, S = ref["cdf"][0], ref["sf"][0]
        big = (P.f(F) > 1e-3) & (P.f(S) > 1e-3)
        assert np.all(np.abs(P.f(F + S - 1)[big]) <= P.EPS)
