"""The reference and the tolerance of the knowledge-gradient tests (tests/_kgref.py; ``bgp_knowledge_gradient``, DESIGN.md section
23), without a device:

* on every case the fp64 numpy replica of the device's route is within the derived tolerance of the long-double reference for every
  candidate of every row, and each of five slips misses it on at least one case: inputs rounded to fp32, the candidate's own line
  dropped, the fantasy noise without the constructor alpha, the white level left on in the covariances, a maximisation KG;
* the closed form itself: the reference's envelope against a trapezoid quadrature of ``min_j (p_j + q_j z) phi(z)`` on [-12, 12];
* ``acquisition.knowledge_gradient_values`` (the package's host path) on the reference's fp64 lines, within the same tolerance.

Lines printed with ``pytest -s`` start with ``PRECISION``; the worst reach and the smallest bite are recorded in DESIGN.md section 23."""
import numpy as np
import pytest

import _kgref as R
import _precision as P
from bayes_skopt_amd.acquisition import knowledge_gradient_values  # noqa: F401  (the subject: without it nothing here has one)

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

CIDS = [c["id"] for c in R.CASES]
SLIPS = ("fp32 inputs", "self line dropped", "noise without alpha", "white level on", "maximisation")


def test_the_cases_sit_on_the_device_codes_edges():
    assert {(c["stationary"], c["form"]) for c in R.CASES} == set(P.FAMILIES)
    assert {1, 63, 64, 65, 129, 257} <= {c["n"] for c in R.CASES}
    assert {1, 8, 17, 32} <= {c["d"] for c in R.CASES}
    assert {0, 1, 62, 63, 64, 65, R.MMAX} <= {c["M"] for c in R.CASES}
    assert {1, 255, 256, 257} <= {c["m"] for c in R.CASES} and any(c["m"] > 2 * R.CHUNK for c in R.CASES)
    assert any(c["B"] == 3 and c["Buse"] == 2 for c in R.CASES)
    assert {c["special"] for c in R.CASES} == {None, "points", "noisefree"}
    for c in R.CASES:
        assert np.all(R.problem(c["id"])[4] <= P.KAPPA_MAX)


def _slipped(cid, b, slip):
    c = R.ALL[cid]
    X, y, alpha, H, _kap, Xc, A, noise = R.problem(cid)
    st, fm = c["stationary"], c["form"]
    if slip == "fp32 inputs":
        return R.replica64(P.to32(X), y, alpha, H[b], P.to32(Xc), P.to32(A), noise[b], st, fm)[0]
    if slip == "self line dropped":
        return R.replica64(X, y, alpha, H[b], Xc, A, noise[b], st, fm, drop_self=True)[0]
    if slip == "noise without alpha":
        return R.replica64(X, y, alpha, H[b], Xc, A, max(noise[b] - R.BASE_ALPHA, 0.0), st, fm)[0]
    if slip == "white level on":
        return R.replica64(X, y, alpha, H[b], Xc, A, noise[b], st, fm, white_on=True)[0]
    return R.replica64(X, y, alpha, H[b], Xc, A, noise[b], st, fm, maximise=True)[0]


@pytest.fixture(scope="module")
def survey():
    """Per (case, row): the replica's reach and every slip's bite, each the worst ratio over ALL candidates."""
    out = {}
    for cid in CIDS:
        c = R.ALL[cid]
        X, y, alpha, H, kap, Xc, A, noise = R.problem(cid)
        for b in range(c["Buse"]):
            ref = R.reference(cid, b)
            kg, s = R.replica64(X, y, alpha, H[b], Xc, A, noise[b], c["stationary"], c["form"])
            out[cid, b] = dict(reach=R.ratio(kg, ref), kg=kg, s=s, bites={sl: R.ratio(_slipped(cid, b, sl), ref) for sl in SLIPS})
            print("PRECISION kg %s b%d kappa %.3g: fp64 replica reach %.4f tol (largest KG %.3g, smallest finite tol %.3g); slips miss "
                  "by %s tol" % (cid, b, kap[b], out[cid, b]["reach"], float(ref["kg"].max()), float(ref["tol"].min()),
                                 " ".join("%.3g" % out[cid, b]["bites"][sl] for sl in SLIPS)))
    return out


def test_fp64_reaches_the_tolerance_on_every_candidate(survey):
    worst = max(v["reach"] for v in survey.values())
    print("PRECISION kg worst reach of the fp64 replica over all cases, rows and candidates: %.4f tol (project margin 0.1: %s)"
          % (worst, "holds" if worst <= 0.1 else "does not hold"))
    for (cid, b), v in survey.items():
        ref = R.reference(cid, b)
        assert v["reach"] <= 1.0, (cid, b, v["reach"])
        assert (v["kg"] >= 0.0).all() and np.all(np.isfinite(v["kg"]))
        assert np.all(v["kg"][v["s"] <= 0.0] == 0.0)  # the rule where the replica's own s is not positive
        assert np.all(np.isfinite(ref["tol"]) == (P.f(ref["s"]) > 0.0))
        if R.ALL[cid]["M"] == 0:
            assert np.all(v["kg"] == 0.0) and np.all(P.f(ref["kg"]) == 0.0)
    # only the noise-free case has candidates without a finite tolerance, and only its training-point candidate
    for cid in CIDS:
        inf = ~np.isfinite(R.reference(cid, 0)["tol"])
        assert not inf.any() or (R.ALL[cid]["special"] == "noisefree" and inf[1:].sum() == 0)


@pytest.mark.parametrize("slip", SLIPS)
def test_every_slip_misses_the_tolerance_somewhere(survey, slip):
    bites = {k: v["bites"][slip] for k, v in survey.items()}
    best = max(bites, key=bites.get)
    least = min(b for b in bites.values() if b > 1.0) if any(b > 1.0 for b in bites.values()) else float("nan")
    print("PRECISION kg slip '%s': largest miss %.3g tol (%s b%d), smallest miss among the cases it bites %.3g tol, bites %d of %d "
          "(case, row) pairs (project margin 10 on the largest: %s)"
          % (slip, bites[best], best[0], best[1], least, sum(b > 1.0 for b in bites.values()), len(bites),
             "holds" if bites[best] >= 10.0 else "does not hold"))
    assert bites[best] > 1.0


def test_reference_envelope_against_quadrature():
    """The closed form, not the precision: E[min_j (p_j + q_j Z)] by the trapezoid rule on 600 001 points of [-12, 12] (the
    integrand has kinks at the breakpoints: the rule's error there is h^2 / 8 times the jump of the slope times phi, 2e-10 |dq|;
    the tails beyond 12 carry less than 1e-30) against the reference's sorted-breakpoint sum, to 1e-9 of max |q| -- on hand-made
    lines with tied slopes and duplicate lines at M + 1 = 1, 2, 5, 17, 65 and on the reference's own lines of three cases."""
    z = np.linspace(-12.0, 12.0, 600001)
    w = np.exp(-z * z / 2.0) / np.sqrt(2.0 * np.pi)
    trap = getattr(np, "trapezoid", None) or np.trapz

    def check(p, q, what):
        p64, q64 = P.f(p), P.f(q)
        emin = np.full_like(z, np.inf)
        for pj, qj in zip(p64, q64):
            np.minimum(emin, pj + qj * z, out=emin)
        quad = p64.min() - trap(emin * w, z)
        got = float(R.envelope_ld(p, q))
        scale = max(np.abs(q64).max(), 1e-300)
        print("PRECISION kg closed form %s: lines %d, reference %.12g, quadrature %.12g, difference %.2g of max |q|"
              % (what, len(p64), got, quad, abs(got - quad) / scale))
        assert abs(got - quad) <= 1e-9 * scale

    rng = np.random.RandomState(7)
    for L in (1, 2, 5, 17, 65):
        p, q = rng.randn(L), rng.randn(L)
        if L >= 5:
            q[1] = q[0]                    # tied slopes, different intercepts
            p[3], q[3] = p[2], q[2]        # a duplicate line
        check(p.astype(hp.LD), q.astype(hp.LD), "hand-made")
    for cid, i in (("kg3_n65_d32_M63_m5_matern52_product", 0), ("kg4_n129_d1_M64_m256_rbf_sum", 17), ("kg_special_n129_d3", R.SAME_REF)):
        ref = R.reference(cid, 0)
        check(ref["p"][i], ref["q"][i], cid)


@pytest.fixture(scope="module")
def bask():
    import bayes_skopt_amd as bask

    return bask


@pytest.mark.parametrize("cid", CIDS)
def test_knowledge_gradient_values_on_the_fp64_image_of_the_reference_lines(bask, cid):
    c = R.ALL[cid]
    for b in range(c["Buse"]):
        ref = R.reference(cid, b)
        vals = bask.acquisition.knowledge_gradient_values(P.f(ref["p"]), P.f(ref["q"]))
        assert vals.shape == (c["m"],) and (vals >= 0.0).all()
        vals = np.where(P.f(ref["s"]) > 0.0, vals, 0.0)
        r = R.ratio(vals, ref)
        print("PRECISION kg %s b%d: knowledge_gradient_values on the fp64 lines of the reference %.4f tol" % (cid, b, r))
        assert r <= 1.0


def test_knowledge_gradient_values_shapes_and_ties(bask):
    f = bask.acquisition.knowledge_gradient_values
    assert f(np.zeros((3, 1)), np.ones((3, 1))).tolist() == [0.0, 0.0, 0.0]
    assert f(np.zeros((0, 4)), np.zeros((0, 4))).shape == (0,)
    assert f(np.zeros((2, 3, 5)), np.zeros((2, 3, 5))).shape == (2, 3)
    p, q = np.array([0.3, -0.2, 0.3, 1.0]), np.array([0.5, -1.0, 0.5, -1.0])  # a duplicate line and a dominated parallel one
    assert f(p, q) == f(p[:2], q[:2])
    # two lines: E[min(p0 + q0 Z, p1 + q1 Z)] in closed form (Clark 1961)
    from scipy.special import ndtr

    t, dlt = abs(q[0] - q[1]), p[1] - p[0]
    want = min(p[0], p[1]) - (p[0] * ndtr(dlt / t) + p[1] * ndtr(-dlt / t) - t * np.exp(-0.5 * (dlt / t) ** 2) / np.sqrt(2 * np.pi))
    assert abs(f(p[:2], q[:2]) - want) <= 1e-15
