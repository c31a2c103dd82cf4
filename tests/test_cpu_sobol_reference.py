"""The tolerance of the Sobol' sensitivity tests (tests/test_gpu_sobol.py) is qualified here the way tests/test_cpu_precision.py
qualifies the others, without a device: on every case of tests/_sobolref.py

* the fp64 numpy replica of the device's route (distances as sums of squares in x / l, the estimator in chunks of 256 samples) is
  within tol / 10 of the long-double reference on f0, V and every term's C and J, on every item;
* the same computation with the training inputs and both sample matrices rounded to fp32 misses by >= 10 tol on its worst quantity;
* on the near-twin Matern-1/2 case the replica whose distances are formed by subtraction misses the tolerance while the sum of
  squares holds (``test_distance_by_subtraction``).

Also here, because they need no device: the argument checks of the Python layer, and the numpy estimator on a function whose
indices are known in closed form.

Lines printed with ``pytest -s`` start with ``PRECISION``."""
import numpy as np
import pytest

import _pdref as PD
import _precision as P
import _sobolref as R

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

MARGIN = 10.0
CIDS = [c["id"] for c in R.CASES]


def test_cases_sit_on_the_kernel_s_edges():
    ns, ds, Ns = ({c[k] for c in R.CASES} for k in ("n", "d", "N"))
    assert ns >= {1, 31, 32, 33, 65, 129, 257} | {R.TJ - 1, R.TJ, R.TJ + 1}
    assert ds >= {1, 3, 8, 17, 32} | {9, 16}
    assert Ns >= {R.RC - 1, R.RC, R.RC + 1} and max(Ns) > 2 * R.RC and min(Ns) == 1
    assert {(c["stationary"], c["form"]) for c in R.CASES} == set(P.FAMILIES)
    assert any(len(c["terms"]) == 1 for c in R.CASES) and any(c["terms"] == R._singles(c["d"]) for c in R.CASES)
    assert any(c["d"] == 4 and len(c["terms"]) == 4 + 6 for c in R.CASES)
    mixed = R.ALL["sb_mixed_B3"]
    m = R.masks_of(mixed["terms"])
    assert 0 in m and (1 << mixed["d"]) - 1 in m and mixed["Buse"] < mixed["B"]
    assert any(m[i] == m[i + 2] and m[i] != m[i + 1] for i in range(len(m) - 2))   # a repeated term
    assert any(m.count(v) == 2 and m.index(v) + 1 < len(m) - m[::-1].index(v) - 1 for v in m)  # twice, apart
    twin = R.ALL["sb_twin_matern12"]
    X, A, Bm = R.problem(twin["id"])[0], *R.problem(twin["id"])[5:]
    assert np.array_equal(A[0], X[0]) and np.abs(A[1, 1:] - X[0, 1:]).max() <= 2e-8 and abs(A[1, 0] - X[0, 0]) > 0.4
    assert np.abs(Bm[1] - X[0]).max() <= 2e-8


def _both(cid, b):
    c = R.ALL[cid]
    st, fm, masks = c["stationary"], c["form"], R.masks_of(c["terms"])
    X, y, alpha, H, kap, A, Bm = R.problem(cid)
    t = P.tol("mean", kap[b], c["n"])
    return c, st, fm, masks, X, y, alpha, H[b], A, Bm, t


@pytest.mark.parametrize("cid", CIDS)
def test_fp64_reaches_the_tolerance_and_fp32_inputs_miss_it(cid):
    reach = bite = None
    for b in range(R.ALL[cid]["Buse"]):
        c, st, fm, masks, X, y, alpha, h, A, Bm, t = _both(cid, b)
        ref = R.reference(cid, b)
        e64 = R.worst(R.replica64(X, PD.alpha64(X, y, alpha, h, st, fm), h, A, Bm, masks, st, fm), ref, t)
        X32, A32, B32 = P.to32(X), P.to32(A), P.to32(Bm)
        e32 = R.worst(R.replica64(X32, PD.alpha64(X32, y, alpha, h, st, fm), h, A32, B32, masks, st, fm), ref, t)
        reach, bite = max(reach or 0.0, e64), min(bite if bite is not None else e32, e32)
    kap = R.problem(cid)[4]
    print("PRECISION sobol %s kappa %.3g: fp64 replica %.4f tol, fp32 inputs %.4g tol" % (cid, kap[: c["Buse"]].max(), reach, bite))
    assert reach <= 1.0 / MARGIN
    assert bite >= MARGIN


def test_distance_by_subtraction():
    """Matern-1/2 has unbounded slope in r^2 at r = 0.  The term {0} of sample 1 of the near-twin case lands 1e-8 from a training
    point: as "the distance of A_1 minus the swapped term plus the new one" its r^2 ~ 1e-16 / l^2 is what is left of terms ~ 1 / l^2."""
    cid = "sb_twin_matern12"
    worst = 0.0
    for b in range(R.ALL[cid]["Buse"]):
        c, st, fm, masks, X, y, alpha, h, A, Bm, t = _both(cid, b)
        a = PD.alpha64(X, y, alpha, h, st, fm)
        ref = R.reference(cid, b)
        good = R.worst(R.replica64(X, a, h, A, Bm, masks, st, fm), ref, t)
        with np.errstate(invalid="ignore"):  # (the residue can be negative: sqrt gives NaN, an infinite error)
            bad = R.worst(R.replica64(X, a, h, A, Bm, masks, st, fm, minus=True), ref, t)
        print("PRECISION sobol %s item %d: sum of squares %.4f tol, by subtraction %.4g tol" % (cid, b, good, bad))
        worst = max(worst, bad)
        assert good <= 1.0 / MARGIN
    assert worst >= MARGIN


def test_the_replica_keeps_the_kernel_s_exact_identities():
    """What bgp_sobol.hip promises bit for bit holds in the replica's arithmetic too: the empty term IS fA, the full one IS fB, and
    A == Bm gives exact zeros."""
    cid = "sb_mixed_B3"
    c, st, fm, masks, X, y, alpha, h, A, Bm, _t = _both(cid, 0)
    a = PD.alpha64(X, y, alpha, h, st, fm)
    F = R.means64(X, a, h, A, Bm, masks, st, fm)
    assert np.array_equal(F[2 + masks.index(0)], F[0]) and np.array_equal(F[2 + masks.index(7)], F[1])
    _f0, _V, C, J = R.replica64(X, a, h, A, A, masks, st, fm)
    assert np.all(C == 0.0) and np.all(J == 0.0)


# ------------------------------------------------------------------------------------------------------------------------------
# the Python layer, without a device
# ------------------------------------------------------------------------------------------------------------------------------
def test_terms_are_checked_before_anything_else():
    from bayes_skopt_amd._posterior import sobol_masks, sobol_rows

    assert sobol_masks([(0,), 2, (1, 2), (), (2, 1, 2)], 3) == [1, 4, 6, 0, 6]
    assert sobol_masks([(39,)], 40) == [1 << 39]  # (past 32 bits: the host route's masks are Python ints)
    for bad in ([(3,)], [(0, -1)], [(0,), (1, 7)]):
        with pytest.raises(ValueError, match="outside"):
            sobol_masks(bad, 3)
    with pytest.raises(ValueError, match="at least one term"):
        sobol_masks([], 3)
    A, Bm = np.zeros((2, 3)), np.ones((2, 3))
    assert np.array_equal(sobol_rows(A, Bm, 5), [[1.0, 0.0, 1.0]] * 2)
    assert np.array_equal(sobol_rows(A, Bm, 0), A) and np.array_equal(sobol_rows(A, Bm, 7), Bm)


def test_the_estimator_on_a_function_with_known_indices():
    """f(x) = a1 x1 + a2 x2 + a3 x3 + c x1 x2 on the unit cube.  With z = x - 1/2: f = const + (a1 + c/2) z1 + (a2 + c/2) z2 + a3 z3
    + c z1 z2, so V1 = (a1 + c/2)^2 / 12, V2 = (a2 + c/2)^2 / 12, V3 = a3^2 / 12, V12 = c^2 / 144 and V is their sum; the closed
    effect of {k} is Vk, of {1, 2} V1 + V2 + V12; the total effect of 1 is V1 + V12, of 3 V3.
    Monte-Carlo bound: each estimate is a mean of N independent summands (up to f0, whose own error enters at order 1 / N), so its
    standard error is the summands' standard deviation / sqrt(N), taken from the sample; 5 of them are allowed (a normal deviate
    beyond 5 sigma has probability 6e-7, and the seed is fixed)."""
    from bayes_skopt_amd._posterior import sobol_estimator, sobol_masks, sobol_rows

    a1, a2, a3, c = 1.0, -2.0, 0.5, 3.0
    f = lambda X: a1 * X[:, 0] + a2 * X[:, 1] + a3 * X[:, 2] + c * X[:, 0] * X[:, 1]
    N = 20000
    rng = np.random.RandomState(0)
    A, Bm = rng.uniform(size=(N, 3)), rng.uniform(size=(N, 3))
    terms = [(0,), (1,), (2,), (0, 1), (), (0, 1, 2)]
    fA, fB = f(A), f(Bm)
    fT = np.stack([f(sobol_rows(A, Bm, m)) for m in sobol_masks(terms, 3)])
    f0, V, C, J = sobol_estimator(fA, fB, fT)
    V1, V2, V3, V12 = (a1 + c / 2) ** 2 / 12, (a2 + c / 2) ** 2 / 12, a3 ** 2 / 12, c ** 2 / 144
    Vt = V1 + V2 + V3 + V12
    se = lambda g: 5.0 * float(np.std(g)) / np.sqrt(len(g))
    assert abs(f0 - ((a1 + a2 + a3) / 2 + c / 4)) <= se(np.concatenate([fA, fB]))
    assert abs(V - Vt) <= se((np.concatenate([fA, fB]) - f0) ** 2)
    want_C = [V1, V2, V3, V1 + V2 + V12, 0.0, Vt]
    want_J = [V1 + V12, V2 + V12, V3, V1 + V2 + V12, 0.0, Vt]
    for t in range(len(terms)):
        assert abs(C[t] - want_C[t]) <= se((fB - f0) * (fT[t] - fA)), terms[t]
        assert abs(J[t] - want_J[t]) <= se(0.5 * (fA - fT[t]) ** 2), terms[t]
    assert C[4] == 0.0 and J[4] == 0.0
    # a leading axis (hyper-posterior rows) is carried through
    f0b, Vb, Cb, Jb = sobol_estimator(np.stack([fA, 2 * fA]), np.stack([fB, 2 * fB]), np.stack([fT, 2 * fT]))
    assert f0b.shape == Vb.shape == (2,) and Cb.shape == Jb.shape == (2, len(terms))
    np.testing.assert_allclose(Cb[1], 4.0 * C, rtol=1e-12)
    np.testing.assert_array_equal(Cb[0], C)
