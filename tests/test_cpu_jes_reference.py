"""The reference and the tolerance of the joint-entropy-search tests (tests/_jesref.py; ``bgp_joint_entropy``),
without a device:

* F, the variance factor of the lower-truncated normal: the definition with erfcx, the continued fraction and the switched function
  against mpmath on z in [-40, 40] (step 0.05) and 1e2 .. 1e8; the switched function stays within the bound ``_jesref.E_F_REL``
  that the tolerance uses;
* the closed form itself: F against an mpmath quadrature of the truncated density;
* on every case the fp64 numpy replica of the device's route is within 0.1 of the derived tolerance of the long-double reference
  for every candidate of every row, and each of seven slips misses it by >= 10 tol on most (case, row) pairs it can touch;
* ``acquisition.joint_entropy_values`` (the package's host path) on the fp64 image of the reference's moments, within 0.1 tol;
* ``0 <= gain <= 1/2 log1p(v / nu)`` on the reference.

Lines printed with ``pytest -s`` start with ``PRECISION``; the worst reach and the bites are recorded in DESIGN.md section 25."""
import numpy as np
import pytest

import _jesref as R
import _precision as P
from bayes_skopt_amd.acquisition import joint_entropy_values  # noqa: F401  (the subject: without it nothing here has one)

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)
mpmath = pytest.importorskip("mpmath")

CIDS = [c["id"] for c in R.CASES]
SLIPS = ("wrong side", "conditioning dropped", "truncation dropped", "shared optimum set", "noise without alpha", "white level on",
         "fp32 inputs")


def test_the_cases_sit_on_the_device_codes_edges():
    assert {(c["stationary"], c["form"]) for c in R.CASES} == set(P.FAMILIES)
    assert {1, 5, 63, 64, 65, 129, 257} <= {c["n"] for c in R.CASES}
    assert {1, 2, 3, 8, 17, 32} <= {c["d"] for c in R.CASES}
    assert {1, 2, 5, 62, 63, 64, 65, R.RMAX} <= {c["R"] for c in R.CASES}
    assert {1, 255, 256, 257, 300} <= {c["m"] for c in R.CASES} and any(c["m"] > 2 * R.CHUNK for c in R.CASES)
    assert any(c["B"] == 3 and c["Buse"] == 2 for c in R.CASES)
    assert {c["special"] for c in R.CASES} == {None, "points", "noisefree"}
    for c in R.CASES:
        X, y, alpha, H, kap, Xc, A, f, noise, tau = R.problem(c["id"])
        assert np.all(kap <= P.KAPPA_MAX) and np.all(noise > 0.0) and np.all(np.isfinite(f))
        assert A.shape == (c["B"], c["R"], c["d"]) and f.shape == (c["B"], c["R"])
        if c["B"] > 1:
            assert not np.array_equal(A[0], A[1])  # every posterior has its OWN optimum points
    # both branches of F are reached, and z ~ 1e3 once
    zs = np.concatenate([P.f(R.reference(cid, 0)["z"]).ravel() for cid in CIDS])
    assert (zs < R.F_SWITCH).any() and (zs >= R.F_SWITCH).any()
    zb = P.f(R.reference("jes_special_n129_d3", 0)["z"])[:, R.BIG_Z]
    print("PRECISION jes z of the large-z sample over the candidates of the points case: %s" % " ".join("%.3g" % v for v in zb))
    assert (zb > 300.0).any()
    X, _y, _al, _H, _k, Xc, A = R.problem("jes_special_n129_d3")[:7]
    assert np.array_equal(Xc[R.SAME_OPT], A[0, 0]) and np.array_equal(Xc[R.TRAIN], X[0]) and np.array_equal(A[0, 1], A[0, 2])
    assert np.array_equal(R.problem("jes_noisefree_n5_d2")[6][0, 0], R.problem("jes_noisefree_n5_d2")[0][0])


def test_F_direct_continued_fraction_and_switched_against_mpmath():
    grid = np.concatenate([np.round(np.arange(-40.0, 40.0 + 1e-9, 0.05), 2), [1e2, 1e3, 1e4, 1e6, 1e8]])
    want = np.array([float(R.F_mp(mpmath.mpf(float(z)))[0]) for z in grid])
    rel = {form: np.abs(R.F64(grid, form) - want) / want for form in ("direct", "cf", "switched")}
    lo = grid < R.F_SWITCH
    for name, sel in (("z < 4", lo), ("4 <= z <= 40", ~lo & (grid <= 40.0)), ("z >= 1e2", grid >= 1e2)):
        k = {form: int(np.nanargmax(np.where(sel, rel[form], -1.0))) for form in rel}
        print("PRECISION jes F on %s: worst relative error direct %.3g (z = %g), continued fraction depth %d %s, switched %.3g (z = %g)"
              % (name, rel["direct"][k["direct"]], grid[k["direct"]], R.F_DEPTH,
                 "not usable" if name == "z < 4" else "%.3g (z = %g)" % (rel["cf"][k["cf"]], grid[k["cf"]]),
                 rel["switched"][k["switched"]], grid[k["switched"]]))
    # where each form is good: the definition up to the switch point, the continued fraction from it on
    first = grid[(grid > 0) & (rel["cf"] <= 5e-16)].min()
    print("PRECISION jes F: the continued fraction (depth %d) is within 5e-16 from z = %g on; the definition exceeds 1e-13 from z = %g on"
          % (R.F_DEPTH, first, grid[(grid > 0) & (rel["direct"] > 1e-13)].min()))
    bound = R.E_F_REL(grid)
    worst = float((rel["switched"] / bound).max())
    print("PRECISION jes F: switched function against its exported bound E_F_REL: worst %.3f of it" % worst)
    assert np.all(rel["switched"] <= bound)
    assert np.all(rel["cf"][~lo] <= 4.0 * P.EPS)
    assert np.all((want > 0.0) & (want <= 1.0))
    # the package's own F (acquisition._jes_F) is the same function
    from bayes_skopt_amd import acquisition

    assert (acquisition.JES_F_SWITCH, acquisition.JES_F_DEPTH) == (R.F_SWITCH, R.F_DEPTH)
    assert np.all(np.abs(acquisition._jes_F(grid) - want) <= bound * want)


def test_truncated_variance_closed_form_against_quadrature():
    """Var[Z | Z >= z] of a standard normal by mpmath quadrature of the truncated density against 1 - lam (lam - z)."""
    with mpmath.workdps(40):
        for z in (-8.0, -1.5, 0.0, 0.7, 3.0, 6.0, 12.0):
            zz = mpmath.mpf(z)
            cuts = [zz + k for k in (0, 0.25, 0.5, 1, 2, 4, 8, 16)] + [mpmath.inf]
            dens = lambda t: mpmath.exp((zz * zz - t * t) / 2)  # noqa: E731  (phi(t) / phi(z): the quadrature's tolerance is absolute)
            mass = mpmath.quad(dens, cuts)
            m1 = mpmath.quad(lambda t: t * dens(t), cuts) / mass
            m2 = mpmath.quad(lambda t: (t - m1) ** 2 * dens(t), cuts) / mass
            F, _Fp, lam = R.F_mp(zz)
            print("PRECISION jes closed form z = %g: quadrature %.15g, 1 - lam (lam - z) %.15g, mean %.15g vs lam %.15g"
                  % (z, float(m2), float(F), float(m1), float(lam)))
            assert abs(m2 - F) <= mpmath.mpf(10) ** -20 * F and abs(m1 - lam) <= mpmath.mpf(10) ** -20 * max(abs(lam), 1)
            # F' by a central difference of the definition
            hh = mpmath.mpf(10) ** -12
            fd = (R.F_mp(zz + hh)[0] - R.F_mp(zz - hh)[0]) / (2 * hh)
            assert abs(fd - _Fp) <= mpmath.mpf(10) ** -15 * max(abs(_Fp), mpmath.mpf(10) ** -10)


def _slipped(cid, b, slip):
    c = R.ALL[cid]
    X, y, alpha, H, _kap, Xc, A, f, noise, tau = R.problem(cid)
    st, fm = c["stationary"], c["form"]
    if slip == "fp32 inputs":
        return R.replica64(P.to32(X), y, alpha, H, P.to32(Xc), P.to32(A), f, noise, tau, b, st, fm)
    if slip == "noise without alpha":
        return R.replica64(X, y, alpha, H, Xc, A, f, noise - R.BASE_ALPHA, tau, b, st, fm)
    kw = {"wrong side": "wrong_side", "conditioning dropped": "no_condition", "truncation dropped": "no_truncation",
          "shared optimum set": "shared_set", "white level on": "white_on"}[slip]
    return R.replica64(X, y, alpha, H, Xc, A, f, noise, tau, b, st, fm, **{kw: True})


def _can_touch(cid, b, slip):
    """A slip changes nothing by construction on some pairs: the shared set is posterior 0's own, the near-noise-free case's nu
    holds no alpha."""
    if slip == "shared optimum set":
        return b > 0
    if slip == "noise without alpha":
        return R.ALL[cid]["special"] != "noisefree"
    return True


@pytest.fixture(scope="module")
def survey():
    """Per (case, row): the replica's reach and every slip's bite, each the worst ratio over ALL candidates."""
    out = {}
    for cid in CIDS:
        c = R.ALL[cid]
        X, y, alpha, H, kap, Xc, A, f, noise, tau = R.problem(cid)
        for b in range(c["Buse"]):
            ref = R.reference(cid, b)
            rep = R.replica64(X, y, alpha, H, Xc, A, f, noise, tau, b, c["stationary"], c["form"])
            bites = {sl: (R.ratio(_slipped(cid, b, sl)["gain"], ref) if _can_touch(cid, b, sl) else float("nan")) for sl in SLIPS}
            out[cid, b] = dict(reach=R.ratio(rep["gain"], ref), rep=rep, bites=bites)
            fin = ref["tol"][np.isfinite(ref["tol"])]
            print("PRECISION jes %s b%d kappa %.3g: fp64 replica reach %.4f tol (largest gain %.3g, smallest finite tol %.3g, rule "
                  "entries %d); slips miss by %s tol" % (cid, b, kap[b], out[cid, b]["reach"], float(ref["gain"].max()),
                                                         float(fin.min()) if fin.size else float("nan"), int(ref["rule"].sum()),
                                                         " ".join("%.3g" % bites[sl] for sl in SLIPS)))
    return out


def test_fp64_reaches_a_tenth_of_the_tolerance_on_every_candidate(survey):
    worst = max(v["reach"] for v in survey.values())
    print("PRECISION jes worst reach of the fp64 replica over all cases, rows and candidates: %.4f tol (project margin 0.1)" % worst)
    n_rule = 0
    for (cid, b), v in survey.items():
        ref, rep = R.reference(cid, b), v["rep"]
        assert v["reach"] <= 0.1, (cid, b, v["reach"])
        assert np.all(np.isfinite(rep["gain"])) and (rep["gain"] >= 0.0).all()
        assert np.all(rep["vt"][rep["vs"] <= 0.0] == 0.0)  # the rule where the replica's own v_s is not positive
        nu = R.problem(cid)[8][b]
        assert np.all(rep["gain"] <= 0.5 * np.log1p(rep["v"] / nu) * (1.0 + 8 * P.EPS) + 8 * P.EPS)
        rule = np.flatnonzero(ref["rule"])
        assert set(rule.tolist()) <= R.designated(cid), (cid, b, rule)
        n_rule += len(rule)
    # the rule entries: counted.  tau > 0 keeps every candidate of the "points" case regular (v_s >= tau v / (v + tau) > 0 even at
    # the candidate that IS an optimum point); in the near-noise-free case w_0 = v_0 at a training point with tau = 0 is the long
    # double's own rounding of 0 for all four candidates
    print("PRECISION jes rule entries over all cases: %d" % n_rule)
    assert n_rule == RULE_ENTRIES


RULE_ENTRIES = 4


@pytest.mark.parametrize("slip", SLIPS)
def test_every_slip_misses_the_tolerance_on_most_pairs(survey, slip):
    bites = {k: v["bites"][slip] for k, v in survey.items() if _can_touch(k[0], k[1], slip)}
    best = max(bites, key=bites.get)
    hit = [b for b in bites.values() if b >= 10.0]
    print("PRECISION jes slip '%s': largest miss %.3g tol (%s b%d), smallest miss among the pairs it bites %.3g tol, bites %d of %d "
          "(case, row) pairs it can touch" % (slip, bites[best], best[0], best[1], min(hit) if hit else float("nan"), len(hit), len(bites)))
    assert bites[best] >= 10.0
    assert 2 * len(hit) > len(bites)


@pytest.fixture(scope="module")
def bask():
    import bayes_skopt_amd as bask

    return bask


@pytest.mark.parametrize("cid", CIDS)
def test_joint_entropy_values_on_the_fp64_image_of_the_reference_moments(bask, cid):
    c = R.ALL[cid]
    f, noise, tau = R.problem(cid)[7], R.problem(cid)[8], R.problem(cid)[9]
    for b in range(c["Buse"]):
        ref = R.reference(cid, b)
        vals = bask.acquisition.joint_entropy_values(P.f(ref["mu"]), np.maximum(P.f(ref["v"]), 0.0), P.f(ref["mur"]), P.f(ref["vr"]),
                                                     P.f(ref["cov"]), f[b], noise[b], tau)
        assert vals.shape == (c["m"],) and (vals >= 0.0).all() and np.all(np.isfinite(vals))
        r = R.ratio(vals, ref)
        print("PRECISION jes %s b%d: joint_entropy_values on the fp64 moments of the reference %.4f tol" % (cid, b, r))
        assert r <= 0.1


def test_joint_entropy_values_shapes_and_rules(bask):
    jv = bask.acquisition.joint_entropy_values
    rng = np.random.RandomState(0)
    mu, var = rng.randn(2, 7), rng.uniform(0.1, 1.0, (2, 7))
    mo, vo, fo = rng.randn(2, 3), rng.uniform(0.1, 1.0, (2, 3)), rng.randn(2, 3)
    cov = 0.1 * rng.randn(2, 7, 3)
    out = jv(mu, var, mo, vo, cov, fo, np.array([1e-3, 2e-3]), 1e-6)
    assert out.shape == (2, 7) and (out >= 0.0).all()
    assert np.array_equal(out[1], jv(mu[1], var[1], mo[1], vo[1], cov[1], fo[1], 2e-3, 1e-6))
    # w <= 0: the sample conditions nothing -- the value is that of zero cross-covariance; v_s <= 0: v_t = 0, the cap itself
    a = jv(mu[0], var[0], mo[0], np.zeros(3), cov[0], fo[0], 1e-3, 0.0)
    assert np.array_equal(a, jv(mu[0], var[0], mo[0], vo[0], np.zeros((7, 3)), fo[0], 1e-3, 0.0))
    full = jv(np.zeros(1), np.array([0.5]), np.zeros(1), np.array([0.5]), np.array([[0.5]]), np.zeros(1), 1e-3, 0.0)
    assert full[0] == 0.5 * (np.log(0.5 + 1e-3) - np.log(1e-3))


@pytest.mark.parametrize("cid", CIDS)
def test_invariants_on_the_reference(cid):
    for b in range(R.ALL[cid]["Buse"]):
        ref = R.reference(cid, b)
        assert np.all(ref["gain"] >= 0) and np.all(ref["gain"] <= ref["cap"])
        assert np.all(ref["vt"] >= 0) and np.all(ref["vt"] <= ref["vs"])
