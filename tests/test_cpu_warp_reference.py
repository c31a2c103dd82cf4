"""The edge grid of the Beta-CDF warp (tests/_warpref.py) without a device: the fp64 restatement of ``bgp_betainc`` against
mpmath at 50 digits, the tolerance it fixes, and the domain in which the continued fraction converges within the kernel's cap.

* On the whole grid the restatement is within a QUARTER of ``_warpref.tol`` (K = 8: the smallest power of two for which that
  holds -- asserted: K / 2 does not), exact at x = 0 and x = 1.
* The relative budget ``_precision.CDF_REL`` holds on the part of the grid with |w| <= 2 and fails at |w| = 6: the reason the
  edge grid is held to an absolute tolerance.
* Monotone across the switch point and symmetric, ``I_x(a, b) + I_{1-x}(b, a) = 1``, within 2 tol: what the device is asked.
* The domain: ``DOMAIN_W`` is the largest integer |w| at which no point of the x grid reaches the cap of 1000 iterations; at
  (20, 20), x = 0.5 the unconverged fraction is 0.48 where the answer is 0.5, which the restatement -- and since this test the
  kernel -- reports as NaN; parameters whose ``exp`` is 0 or inf are NaN at every x.

Lines printed with ``pytest -s`` start with ``WARPREF``."""
import math

import numpy as np
import pytest

import _precision as P

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)
pytest.importorskip("mpmath")

import _warpref as R  # noqa: E402


def _errs():
    ref = R.reference()
    got, its = R.restated()
    return np.abs(got.astype(np.longdouble) - ref).astype(np.float64), ref.astype(np.float64), got, its


def test_grid_is_the_one_described():
    X, T, A, B = R.grid()
    assert X.shape == T.shape == (121, R.N_X) and R.N_X == 20 and len(set(R.PAIRS)) == 121
    assert {abs(w) for w in R.W_GRID} == {0.0, 0.3, 1.0, 2.0, 4.0, 6.0}
    assert np.all(X[:, 0] == 0.0) and np.all(X[:, 1] == 1.0) and np.all(X[:, 2] == np.finfo(np.float64).tiny)
    assert np.all(X[:, 15] == 1.0 - 2.0 ** -53) and np.all(X[:, 15] < 1.0)
    s = X[:, R.SWITCH]
    assert np.array_equal(s[:, 1], (A + 1.0) / (A + B + 2.0)) and np.all(np.diff(s, axis=1) > 0)
    assert np.array_equal(np.nextafter(s[:, 1], 0.0), s[:, 0]) and np.array_equal(np.nextafter(s[:, 1], 1.0), s[:, 2])
    assert np.all((X >= 0.0) & (X <= 1.0)) and np.all(T[:, 2:] > 0.0) and np.all(T[:, :2] == 0.0)


def test_restatement_is_within_a_quarter_of_the_tolerance():
    err, ref, got, its = _errs()
    X, T, _A, _B = R.grid()
    wmax = np.array([max(abs(wa), abs(wb)) for wa, wb in R.PAIRS])
    inner = T > 0.0
    for lim in (1.0, 2.0, 4.0, 6.0):
        m = wmax <= lim
        rel = np.where(ref[m] > 0.0, err[m] / np.where(ref[m] > 0.0, ref[m], 1.0), 0.0)
        ratio1 = np.where(inner[m], err[m] / np.where(inner[m], T[m] / R.K, 1.0), 0.0)
        print("WARPREF |w| <= %g: worst relative error %.2e, worst absolute error %.2e, most iterations %d, worst err / tol at "
              "K = 1 %.3g" % (lim, float(rel.max()), float(err[m].max()), int(its[m].max()), float(ratio1.max())))
    assert np.all(got[:, 0] == 0.0) and np.all(got[:, 1] == 1.0) and np.all(err[~inner] == 0.0)
    ratio = float((err[inner] / T[inner]).max())
    print("WARPREF K = %g: worst err / tol %.3f" % (R.K, ratio))
    assert ratio <= 0.25, ratio
    assert 2.0 * ratio > 0.25 and math.log2(R.K) == int(math.log2(R.K))  # the smallest power of two
    # the relative budget of _precision.py holds near the prior's centre and not at the edge of the grid
    rel = np.where(ref > 0.0, err / np.where(ref > 0.0, ref, 1.0), 0.0)
    assert float(rel[wmax <= 2.0].max()) <= P.CDF_REL / 5.0 and float(rel[wmax <= 6.0].max()) > P.CDF_REL


def test_restatement_is_monotone_across_the_switch_and_symmetric():
    X, T, A, B = R.grid()
    got, _its = R.restated()
    s, t = got[:, R.SWITCH], T[:, R.SWITCH]
    assert np.all(s[:, 1] - s[:, 0] >= -2.0 * np.maximum(t[:, 0], t[:, 1]))
    assert np.all(s[:, 2] - s[:, 1] >= -2.0 * np.maximum(t[:, 1], t[:, 2]))
    worst = 0.0
    for j, (wa, wb) in enumerate(R.PAIRS):
        for i, x in enumerate(X[j]):
            x = float(x)
            if 0.0 < x < 1.0 and (1.0 - (1.0 - x)) == x:  # 1 - x is exact
                mirror = R.betainc64(B[j], A[j], 1.0 - x)[0]
                lim = 2.0 * max(T[j, i], R.tol(B[j], A[j], 1.0 - x))
                worst = max(worst, abs(got[j, i] + mirror - 1.0) / lim)
    print("WARPREF symmetry: worst |I_x(a, b) + I_{1-x}(b, a) - 1| / (2 tol) %.3f" % worst)
    assert worst <= 1.0


def test_domain_of_the_continued_fraction():
    out = {w: R.most_iterations(float(w)) for w in range(6, 21)}
    for w, (it, ok) in out.items():
        print("WARPREF |w| = %2d: most iterations %4d%s" % (w, it, "" if ok else "  (cap reached)"))
    inside = [w for w, (_it, ok) in out.items() if ok]
    assert inside == list(range(6, R.DOMAIN_W + 1)) and R.DOMAIN_W == 15
    assert out[R.DOMAIN_W][0] < R.CF_CAP and not out[R.DOMAIN_W + 1][1]
    # outside: an unconverged fraction is a wrong number without a sign of it -- reported as NaN
    a = math.exp(20.0)
    h, it, ok = R.betacf64(a, a, 0.5)
    assert not ok and it == R.CF_CAP and math.isnan(R.betainc64(a, a, 0.5)[0])
    lg = math.lgamma(2.0 * a) - 2.0 * math.lgamma(a) + a * math.log(0.5) + a * math.log1p(-0.5)
    silent = 1.0 - math.exp(lg) * h / a  # (x = 0.5 is not below the switch point 0.5: the complement branch)
    print("WARPREF w = (20, 20), x = 0.5: the unconverged fraction gives %.4f" % silent)
    assert abs(silent - 0.5) > 0.01
    for w in (700.0, 800.0, -800.0):  # exp(700) is finite and far outside the domain; exp(+-800) is inf / 0
        for x in (0.0, 0.3, 0.9, 1.0):
            e = R._exp(w)
            v = [R.betainc64(e, 1.0, x)[0], R.betainc64(1.0, e, x)[0]]
            if e in (0.0, math.inf):
                assert all(math.isnan(u) for u in v), (w, x, v)
            else:
                assert all(math.isnan(u) or 0.0 <= u <= 1.0 for u in v), (w, x, v)
