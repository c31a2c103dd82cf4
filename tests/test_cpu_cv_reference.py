"""Cross-validation from the resident inverses without a device.

* The tolerance of tests/test_gpu_cv.py is qualified the way tests/test_cpu_precision.py qualifies the others: on every case of
  tests/_cvref.py, row and fold the fp64 numpy replica of the device's recurrences is within tol / 10 of the long-double refit on
  the remaining points, for the mean, the variance and the fold's log density; and per case, row and quantity each of the two
  single-precision slips -- the training inputs rounded to fp32 before the Gram build, A_FF rounded to fp32 before its
  factorisation -- misses by >= 10 tol on its worst fold.  One exemption, for a reason and not for a margin: at n = 1 the Gram
  matrix does not read the inputs at all (K = k(0) + s2 + alpha), so rounding them changes no bit.
* The rules that combine hyper-posterior rows (``crossval.fold_weights`` / ``combine_rows``) against direct evaluation.
* The fold splitter.

Lines printed with ``pytest -s`` start with ``PRECISION``."""
import numpy as np
import pytest

import _cvref as R
import _precision as P

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

MARGIN = 10.0
CIDS = [c["id"] for c in R.CASES]


def test_cases_sit_on_the_kernels_edges():
    sizes = {len(f) for c in R.CASES for f in c["folds"]}
    assert sizes >= {1, 2, 63, 64, 65, 127, 128} and max(sizes) == R.SMAX
    assert {c["n"] for c in R.CASES} == {1, 2, 65, 129, 257, 385}
    assert {(c["stationary"], c["form"]) for c in R.CASES} == set(P.FAMILIES)
    assert {c["vec_alpha"] for c in R.CASES} == {True, False}
    assert {(c["B"], c["Buse"]) for c in R.CASES} == {(1, 1), (3, 2)}
    part = unc = mixed = loo = False
    for c in R.CASES:
        flat = np.concatenate(c["folds"])
        assert len(np.unique(flat)) == len(flat) and flat.min() >= 0 and flat.max() < c["n"]
        part |= len(flat) == c["n"] and len(c["folds"]) > 1
        unc |= len(flat) < c["n"]
        mixed |= len({len(f) for f in c["folds"]}) > 2
        loo |= len(c["folds"]) > 2 and all(len(f) == 1 for f in c["folds"])
    assert part and unc and mixed and loo
    # contiguous folds across the row-block edges of the padded inverse, and shuffled (non-contiguous, unsorted) ones
    assert any(f.min() < 128 <= f.max() and np.all(np.diff(f) == 1) for c in R.CASES for f in c["folds"])
    assert any(f.min() < 256 <= f.max() and np.all(np.diff(f) == 1) for c in R.CASES for f in c["folds"])
    assert any(len(f) > 2 and np.any(np.diff(f) < 0) for c in R.CASES for f in c["folds"])
    assert len(R.LOO_PAIR) == 2 and not set(R.LOO_PAIR) & set(np.concatenate(R.ALL[R.LOO_CASE]["folds"]))


@pytest.mark.parametrize("cid", CIDS)
def test_fp64_reaches_the_tolerance_and_single_precision_slips_miss_it(cid):
    c = R.ALL[cid]
    st, fm, folds, n = c["stationary"], c["form"], c["folds"], c["n"]
    X, y, alpha, H, kap = R.problem(cid)
    reach = {q: 0.0 for q in R.QUANTITIES}
    bite = {slip: {q: np.inf for q in R.QUANTITIES} for slip in ("inputs32", "block32")}
    for b in range(c["Buse"]):
        ref = R.reference(cid, b)
        t = [{q: R.tol(q, kap[b], n, amp=r["amp"]) for q in R.QUANTITIES} for r in ref]
        e64 = [R.errs(g, r) for g, r in zip(R.replica64(X, y, alpha, H[b], folds, st, fm), ref)]
        for q in R.QUANTITIES:
            reach[q] = max(reach[q], max(e[q] / tk[q] for e, tk in zip(e64, t)))
        for slip in bite:
            e32 = [R.errs(g, r) for g, r in zip(R.replica64(X, y, alpha, H[b], folds, st, fm, **{slip: True}), ref)]
            for q in R.QUANTITIES:
                bite[slip][q] = min(bite[slip][q], max(e[q] / tk[q] for e, tk in zip(e32, t)))
    print("PRECISION cv %s kappa %.3g: fp64 replica %s tol; fp32 inputs %s tol; fp32 A_FF %s tol"
          % (cid, kap[: c["Buse"]].max(), " / ".join("%.4f" % reach[q] for q in R.QUANTITIES),
             " / ".join("%.4g" % bite["inputs32"][q] for q in R.QUANTITIES),
             " / ".join("%.4g" % bite["block32"][q] for q in R.QUANTITIES)))
    for q in R.QUANTITIES:
        assert reach[q] <= 1.0 / MARGIN, (q, reach[q])
        assert bite["block32"][q] >= MARGIN, (q, bite["block32"][q])
        if n > 1:  # (n = 1: K = k(0) + s2 + alpha reads no input)
            assert bite["inputs32"][q] >= MARGIN, (q, bite["inputs32"][q])


def test_identity_needs_no_input_at_n_1():
    """The exemption above is what it says: with one training point the rounded inputs give the same bits."""
    cid = R.CASES[0]["id"]
    c = R.ALL[cid]
    X, y, alpha, H, _ = R.problem(cid)
    a = R.replica64(X, y, alpha, H[0], c["folds"], c["stationary"], c["form"])
    b = R.replica64(X, y, alpha, H[0], c["folds"], c["stationary"], c["form"], inputs32=True)
    assert c["n"] == 1 and all(np.array_equal(u, v) for fa, fb in zip(a, b) for u, v in zip(fa, fb))


# ------------------------------------------------------------------------------------------------------------------------------
# combining rows
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cv():
    from bayes_skopt_amd import crossval

    return crossval


LPD = np.array([[-3.0, 0.5, -700.0], [-1.0, 0.25, -705.0], [-2.5, 0.75, -690.0], [-40.0, 0.5, -701.0]])  # (B = 4, K = 3)


def test_fold_weight_formulas_against_direct_evaluation(cv):
    B = LPD.shape[0]
    w, lpd, ess = cv.fold_weights(LPD[:, :2], "is")  # (the third column under- and overflows a direct evaluation)
    direct = 1.0 / np.exp(LPD[:, :2])
    np.testing.assert_allclose(w, direct / direct.sum(axis=0), rtol=1e-13)
    np.testing.assert_allclose(lpd, -np.log(direct.mean(axis=0)), rtol=1e-13)
    np.testing.assert_allclose(ess, direct.sum(axis=0) ** 2 / (direct**2).sum(axis=0), rtol=1e-13)
    w, lpd, ess = cv.fold_weights(LPD[:, :2], "equal")
    np.testing.assert_array_equal(w, np.full((B, 2), 0.25))
    np.testing.assert_allclose(lpd, np.log(np.exp(LPD[:, :2]).mean(axis=0)), rtol=1e-13)
    np.testing.assert_allclose(ess, B, rtol=1e-15)
    # log-sum-exp: densities of e^-700 neither underflow nor overflow
    for kind in ("is", "equal"):
        w, lpd, ess = cv.fold_weights(LPD, kind)
        assert np.all(np.isfinite(lpd)) and np.all(np.isfinite(w)) and np.allclose(w.sum(axis=0), 1.0)
        assert -705.0 <= lpd[2] <= -690.0
    with pytest.raises(ValueError):
        cv.fold_weights(LPD, "uniform")


def test_harmonic_mean_is_below_arithmetic_mean_and_ess_in_range(cv):
    rng = np.random.RandomState(0)
    lpd = rng.normal(scale=3.0, size=(7, 11))
    w_is, f_is, e_is = cv.fold_weights(lpd, "is")
    w_eq, f_eq, e_eq = cv.fold_weights(lpd, "equal")
    assert np.all(f_is <= f_eq + 1e-12)
    assert np.all(e_is >= 1.0 - 1e-12) and np.all(e_is <= 7.0 + 1e-12) and np.allclose(e_eq, 7.0)
    # one row: the two coincide, with weight 1
    a, b = cv.fold_weights(lpd[:1], "is"), cv.fold_weights(lpd[:1], "equal")
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)
    np.testing.assert_array_equal(a[1], lpd[0])
    np.testing.assert_array_equal(a[2], np.ones(11))


def test_mixture_moments(cv):
    rng = np.random.RandomState(1)
    B, n = 5, 9
    folds = [np.array([4, 0, 7]), np.array([2]), np.array([8, 1])]  # 3, 5, 6 uncovered
    y = rng.normal(size=n)
    m, v, lpd = rng.normal(size=(B, n)), rng.uniform(0.1, 2.0, size=(B, n)), rng.normal(size=(B, 3))
    for kind in ("is", "equal"):
        out = cv.combine_rows(m, v, lpd, folds, y, kind)
        w = cv.fold_weights(lpd, kind)[0]
        for k, f in enumerate(folds):
            wk = w[:, k][:, None]
            mean = (wk * m[:, f]).sum(axis=0)
            np.testing.assert_allclose(out["mean"][f], mean, rtol=1e-13)
            np.testing.assert_allclose(out["std"][f] ** 2, (wk * (v[:, f] + m[:, f] ** 2)).sum(axis=0) - mean**2, rtol=1e-10)
            assert np.all(out["std"][f] ** 2 >= (wk * v[:, f]).sum(axis=0) * (1 - 1e-14))
            dens = (wk * np.exp(-0.5 * (y[f] - m[:, f]) ** 2 / v[:, f]) / np.sqrt(2 * np.pi * v[:, f])).sum(axis=0)
            np.testing.assert_allclose(out["point_lpd"][f], np.log(dens), rtol=1e-12)
        unc = [3, 5, 6]
        assert all(np.all(np.isnan(out[key][unc])) for key in ("mean", "std", "point_lpd", "z"))
        cov = np.concatenate(folds)
        np.testing.assert_allclose(out["z"][cov], (y[cov] - out["mean"][cov]) / out["std"][cov], rtol=1e-15)
        assert out["elpd"] == out["fold_lpd"].sum() and out["ess"].shape == (3,)
    one = cv.combine_rows(m[:1], v[:1], lpd[:1], folds, y, "is")
    cov = np.concatenate(folds)
    np.testing.assert_allclose(one["mean"][cov], m[0, cov], rtol=1e-15)
    np.testing.assert_allclose(one["std"][cov], np.sqrt(v[0, cov]), rtol=1e-15)
    np.testing.assert_array_equal(one["fold_lpd"], lpd[0])


# ------------------------------------------------------------------------------------------------------------------------------
# the splitter and the fold checks
# ------------------------------------------------------------------------------------------------------------------------------
def test_split_folds(cv):
    for n, K in [(974, 10), (10, 10), (11, 3), (5, 1)]:
        a, b = cv.split_folds(n, K, random_state=3), cv.split_folds(n, K, random_state=3)
        assert len(a) == K and all(np.array_equal(u, v) for u, v in zip(a, b))
        flat = np.concatenate(a)
        assert sorted(flat) == list(range(n))
        sizes = [len(f) for f in a]
        assert max(sizes) - min(sizes) <= 1
    assert any(not np.array_equal(u, v) for u, v in zip(cv.split_folds(50, 5, random_state=3), cv.split_folds(50, 5, random_state=4)))
    with pytest.raises(ValueError):
        cv.split_folds(4, 5)
    with pytest.raises(ValueError):
        cv.split_folds(4, 0)


def test_check_folds_names_the_fault(cv):
    ok = cv.check_folds([[3, 1], np.array([0])], 4)
    assert [f.tolist() for f in ok] == [[3, 1], [0]]
    for bad, word in [([], "at least one"), ([[0], []], "empty"), ([list(range(129))], "128"), ([[0, 4]], "outside"),
                      ([[-1]], "outside"), ([[0, 1], [1]], "repeats"), ([[2, 2]], "repeats")]:
        with pytest.raises(ValueError, match=word):
            cv.check_folds(bad, 200 if word == "128" else 4)
