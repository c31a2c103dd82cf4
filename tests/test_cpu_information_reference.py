"""An fp64 replica of bgp_info.hip's recurrences against the long-double reference over the GPU test's cases stays within tol / 8
(K = 8 x its worst ratio); in fp32, and without the max pass, it misses tol.  Means 40 sd apart at unit scale do NOT break the
single-pass sum in fp64 (measured err / tol 3e-4: a node's own exponent -t^2 >= -110 never underflows); the max pass protects the
scale (-log sd in the exponents): the same pair at sd = 1e300 underflows every exponential and the plain sum returns -inf."""
import numpy as np
import pytest

import _inforef as R


def _ratios(fn, content, B, Q, m):
    mu, sd, wn = R.columns(*R.moments(content, B, m))
    t, om = R.rule(Q)
    worst = 0.0
    for i in range(m):
        ref = R.reference(mu[:, i], sd[:, i], wn, t, om)
        if not np.isfinite(ref[1]):  # (the atom's point: no number to hold)
            continue
        got = fn(mu[:, i], sd[:, i], wn, t, om)
        unit = R.tolerance(sd[:, i], wn, t, k=1.0)
        worst = max(worst, abs(float(got[0] - ref[0])) / unit, abs(float(got[1] - ref[1])) / unit)
    return worst


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: "%s-B%d-Q%d-m%d" % c)
def test_the_fp64_replica_holds_an_eighth_of_the_tolerance_and_fp32_misses_it(case):
    r64 = _ratios(R.replica, *case)
    print("PRECISION info %s: fp64 replica vs long double %.3g eps-units (K = %g)" % (case, r64, R.K))
    assert r64 <= R.K / 8.0
    if case[1] > 1:  # (one row: the information is exactly 0 in any format)
        assert _ratios(lambda *a: R.replica(*a, dtype=np.float32), *case) > R.K


def test_without_the_max_pass_the_sum_underflows():
    t, om = R.rule(64)
    mu, sd, w = np.array([0.0, 40.0e300]), np.array([1e300, 1e300]), np.array([0.5, 0.5])
    ref = R.reference(mu, sd, w, t, om)
    tol = R.tolerance(sd, w, t)
    two, one = R.replica(mu, sd, w, t, om), R.replica(mu, sd, w, t, om, two_pass=False)
    assert abs(float(two[0] - ref[0])) <= tol / 8.0 and abs(float(two[1] - ref[1])) <= tol / 8.0
    assert abs(float(ref[0]) - np.log(2.0)) <= tol
    assert not abs(float(one[1] - ref[1])) <= tol and not abs(float(one[0] - ref[0])) <= tol
