"""The reference and the tolerances of the gradient-covariance tests (tests/_gcovref.py; ``bgp_grad_cov``),
without a device:

* on every case the fp64 numpy replica is within tol / 10 of the long-double reference and the same computation on inputs rounded
  to fp32 misses by >= 10 tol -- for ``cov`` on ``tol("var")``, for ``dmean`` on ``tol("mean")`` and for both sums on their
  first-order image: the project's two margins, with no new constant;
* the reference itself against an independent route: second differences of the long-double predictive covariance;
* the host path of the package (``gradcov.gradient_cov_host``) equals the replica;
* the assembly of ``utils.active_subspace`` on hand-made matrices.

Lines printed with ``pytest -s`` start with ``PRECISION``."""
import numpy as np
import pytest

import _gcovref as R
import _precision as P

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

CIDS = [c["id"] for c in R.CASES]


def test_the_cases_sit_on_the_device_codes_edges():
    fams = {(c["stationary"], c["form"]) for c in R.CASES}
    assert fams == set(R.DIFFERENTIABLE)
    assert {1, R.TJ - 1, R.TJ, R.TJ + 1, 129, 257} <= {c["n"] for c in R.CASES}
    assert {1, 3, 8, 9, 16, 17, 32} <= {c["d"] for c in R.CASES}
    assert {(8, 15), (8, 16), (8, 17), (32, 4), (32, 5)} <= {(c["d"], c["m"]) for c in R.CASES}
    assert {R.RC - 1, R.RC, R.RC + 1, 600} <= {c["m"] for c in R.CASES if c["d"] <= 3}
    assert any(c["B"] == 3 and c["Buse"] == 2 for c in R.CASES) and any(c["special"] for c in R.CASES)


@pytest.mark.parametrize("cid", CIDS)
def test_fp64_reaches_the_tolerances_and_fp32_inputs_miss_them(cid):
    c = R.ALL[cid]
    X, y, alpha, H, kap, Xq = R.problem(cid)
    st, fm = c["stationary"], c["form"]
    for b in range(c["Buse"]):
        ref = R.reference(cid, b)
        t_var, t_mean = P.tol("var", kap[b], c["n"]), P.tol("mean", kap[b], c["n"])
        dm, cv = R.replica64(X, y, alpha, H[b], Xq, st, fm)
        dm32, cv32 = R.replica64(P.to32(X), y, alpha, H[b], P.to32(Xq), st, fm)
        reach = (R.err_cov(cv, ref) / t_var, R.err_dmean(dm, ref) / t_mean) + R.csum_ratio(*R.sums_in_order(dm, cv), ref, t_mean, t_var)
        bite = (R.err_cov(cv32, ref) / t_var, R.err_dmean(dm32, ref) / t_mean) + R.csum_ratio(*R.sums_in_order(dm32, cv32), ref, t_mean,
                                                                                            t_var)
        eig = R.min_eig_scaled(ref["cov"], ref)
        print("PRECISION gcov %s b%d kappa %.3g: fp64 reach cov %.4f dmean %.4f C_mean %.4f C_cov %.4f tol; fp32 inputs miss by "
              "%.0f %.0f %.0f %.0f tol; smallest eigenvalue of Sigma / scale %.4g" % ((cid, b, kap[b]) + reach + bite + (eig,)))
        assert max(reach) <= 0.1, reach
        assert min(bite) >= 10.0, bite
        assert eig > 0.0  # (the reference covariance is positive definite: the device's bound -d tol is not vacuous)


@pytest.mark.parametrize("cid", ["gc1_n63_d3_m255_matern32_product", "gc10_n129_d3_m256_matern52_sum", "gc3_n65_d8_m16_rbf_sum",
                                 "gc_special_n129_d3"])
def test_reference_against_second_differences_of_the_predictive_covariance(cid):
    """Sigma_kl(x) is the limit of Cov[f(x + h e_k) - f(x), f(x + h e_l) - f(x)] / h^2, which the long-double ``predict(...,
    return_cov=True)`` gives without any derivative of the kernel.  The quotient is the average of the mixed derivative of the
    posterior covariance over the square [0, h]^2, so it differs from Sigma(x) at first order in h: for the prior part the series
    of S gives 2 (1 - S(r)) / r^2 = phi (1 - (2 / sqrt 3) r + ...) for Matern 3/2 and O(r^2) for the others, and the data part
    varies on the length scale.  Bound used: 4 h / l_min on the sqrt(H0_kk H0_ll) scale, at h = 1e-4 l_min (rounding of the
    long-double covariance, kappa 2^-64 / h^2 ~ 1e-7 of it, is far below); and halving h halves the discrepancy, which shows that
    the truncation, not an error of the reference, is what is left."""
    c = R.ALL[cid]
    X, y, alpha, H, _kap, Xq = R.problem(cid)
    d = c["d"]
    lmin = float(np.exp(H[0][1 : d + 1]).min())
    pts = Xq[:4]
    ref = R.reference_at(cid, 0, pts)
    sc = R.h0_scale(ref)
    worst = []
    for hrel in (1e-4, 5e-5):
        h = hp.LD(hrel * lmin)
        w = 0.0
        for s, x in enumerate(pts):
            Q = hp._ld(x) + np.vstack([np.zeros((1, d), dtype=hp.LD), h * np.eye(d, dtype=hp.LD)])
            Cq = hp.predict(X, y, alpha, H[0], Q, c["stationary"], c["form"], noise_zero=True, return_cov=True, post=R._post(cid, 0))["cov"]
            D = (Cq[1:, 1:] - Cq[1:, :1] - Cq[:1, 1:] + Cq[0, 0]) / (h * h)
            w = max(w, float((np.abs(P.f(D - ref["cov"][s])) / sc).max()))
        worst.append(w)
    print("PRECISION gcov %s: second differences vs reference %.3g (h = 1e-4 l_min), %.3g (h = 5e-5 l_min)" % (cid, *worst))
    assert worst[0] <= 4.0 * 1e-4
    assert 1.9 <= worst[0] / worst[1] <= 2.1


@pytest.fixture(scope="module")
def bask():
    import bayes_skopt_amd as bask

    return bask


@pytest.mark.parametrize("cid", ["gc1_n63_d3_m255_matern32_product", "gc5_n257_d9_m20_matern52_sum", "gc9_n63_d32_m5_rbf_sum",
                                 "gc_special_n129_d3"])
def test_host_path_equals_the_replica(bask, cid):
    from oracle import gp_oracle as O
    from scipy.linalg import cho_solve, cholesky

    c = R.ALL[cid]
    X, y, alpha, H, kap, Xq = R.problem(cid)
    st, fm = c["stationary"], c["form"]
    L = cholesky(O.gram_with_jitter(X, np.broadcast_to(alpha, (len(X),)), H[0], st, fm), lower=True)
    Ki = cho_solve((L, True), np.eye(len(X)))
    dm, cv = bask.gradcov.gradient_cov_host(H[0], X, cho_solve((L, True), y), 0.5 * (Ki + Ki.T), Xq, st, fm)
    rdm, rcv = R.replica64(X, y, alpha, H[0], Xq, st, fm)
    ref = R.reference(cid, 0)
    t_var, t_mean = P.tol("var", kap[0], c["n"]), P.tol("mean", kap[0], c["n"])
    # the same closed forms on the same inverse: the two differ by the order of fp64 operations, i.e. by no more than either's
    # own distance from the reference (<= tol / 10)
    assert float((np.abs(cv - rcv) / R.h0_scale(ref)[None]).max()) <= 0.1 * t_var
    assert float(np.abs(dm - rdm).max() / ref["scale_dmean"]) <= 0.1 * t_mean
    assert R.err_cov(cv, ref) <= 0.1 * t_var and R.err_dmean(dm, ref) <= 0.1 * t_mean
    assert np.array_equal(cv, np.swapaxes(cv, 1, 2)) and (cv[:, np.arange(c["d"]), np.arange(c["d"])] >= 0.0).all()
    cm, cc = bask.gradcov.subspace_sums(dm, cv)
    assert max(R.csum_ratio(cm, cc, ref, t_mean, t_var)) <= 0.1


def test_host_path_refuses_matern12(bask):
    with pytest.raises(ValueError, match="not differentiable"):
        bask.gradcov.gradient_cov_host(np.zeros(4), np.zeros((3, 2)), np.zeros(3), np.eye(3), np.zeros((1, 2)), "matern12", "product")


def test_assembly_of_the_active_subspace_result(bask):
    A = bask.gradcov.assemble
    v1, v2, v3 = np.array([1.0, 1.0, 0.0]) / np.sqrt(2.0), np.array([-1.0, 1.0, 0.0]) / np.sqrt(2.0), np.array([0.0, 0.0, -1.0])
    C_mean = 5.0 * np.outer(v1, v1) + 0.5 * np.outer(v3, v3)
    C_cov = 1.0 * np.outer(v2, v2) + 1.5 * np.outer(v3, v3)
    out = A(C_mean, C_cov, "device")
    assert set(out) == {"C", "C_mean", "C_cov", "eigenvalues", "eigenvectors", "explained", "diag_share", "path"}
    np.testing.assert_allclose(out["C"], C_mean + C_cov, rtol=0, atol=0)
    np.testing.assert_allclose(out["eigenvalues"], [5.0, 2.0, 1.0], rtol=1e-14)
    V = out["eigenvectors"]
    np.testing.assert_allclose(V[:, 0], v1, atol=1e-14)           # largest component positive already
    np.testing.assert_allclose(V[:, 1], [0.0, 0.0, 1.0], atol=1e-14)  # -e_3 flipped
    np.testing.assert_allclose(np.abs(V[:, 2]), np.abs(v2), atol=1e-14)
    assert V[np.argmax(np.abs(V[:, 2])), 2] > 0.0
    np.testing.assert_allclose(out["explained"], [5.0 / 8.0, 7.0 / 8.0, 1.0], rtol=1e-14)
    np.testing.assert_allclose([out["diag_share"][k] for k in range(3)], np.diag(C_mean + C_cov) / 8.0, rtol=1e-14)
    assert out["path"] == "device" and "band" not in out
    # chain rows: matrices averaged, the band from the per-row ranked eigenvalues
    scales = np.array([1.0, 2.0, 4.0])
    rows = A(scales[:, None, None] * C_mean, scales[:, None, None] * C_cov, "host")
    np.testing.assert_allclose(rows["C"], scales.mean() * (C_mean + C_cov), rtol=1e-14)
    np.testing.assert_allclose(rows["eigenvalues"], scales.mean() * np.array([5.0, 2.0, 1.0]), rtol=1e-13)
    per = scales[:, None] * np.array([5.0, 2.0, 1.0])[None, :]
    lo, hi = rows["band"]
    np.testing.assert_allclose(lo, np.percentile(per, 5.0, axis=0), rtol=1e-13)
    np.testing.assert_allclose(hi, np.percentile(per, 95.0, axis=0), rtol=1e-13)
    assert "active_subspace" in bask.utils.__all__ and bask.Optimizer.active_subspace is not None
