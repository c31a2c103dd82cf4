"""The reference, the tolerances and the host path of the Hessian-posterior tests (tests/_hessref.py; ``bgp_hess_cov``, DESIGN.md
section 32), without a device: the package's fp64 host path against the long-double reference (and the same path on fp32 inputs);
its closed forms against second differences of the long-double ``predict``; ``utils.optimum_curvature``'s assembly (PRECISION: -s)."""
import numpy as np
import pytest

import _hessref as R
import _precision as P

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)
bask = pytest.importorskip("bayes_skopt_amd")


def _host(cid, b, Xq=None, round32=False):
    from oracle import gp_oracle as O
    from scipy.linalg import cho_solve, cholesky

    c = R.ALL[cid]
    X, y, alpha, H, _kap, Xq = R.problem(cid)[:5] + (R.problem(cid)[5] if Xq is None else Xq,)
    if round32:
        X, Xq = P.to32(X), P.to32(Xq)
    L = cholesky(O.gram_with_jitter(X, np.broadcast_to(alpha, (len(X),)), H[b], c["stationary"], c["form"]), lower=True)
    Ki = cho_solve((L, True), np.eye(len(X)))
    return bask.hesscov.hessian_cov_host(H[b], X, cho_solve((L, True), y), 0.5 * (Ki + Ki.T), Xq, c["stationary"], c["form"])


@pytest.mark.parametrize("cid", list(R.ALL))
def test_host_path_reaches_the_tolerances_and_fp32_inputs_miss_them(cid):
    c = R.ALL[cid]
    kap = R.problem(cid)[4]
    for b in range(c["Buse"]):
        ref = R.reference(cid, b)
        tols = np.array([P.tol("var", kap[b], c["n"])] * 2 + [P.tol("mean", kap[b], c["n"])])
        reach, bite = R.errors(*_host(cid, b), ref) / tols, R.errors(*_host(cid, b, round32=True), ref) / tols
        print("PRECISION hess %s b%d kappa %.3g: fp64 host path reach hcov %.4f hvar %.4f hmean %.4f tol; fp32 inputs miss by %.0f "
              "%.0f %.0f tol" % ((cid, b, kap[b]) + tuple(reach) + tuple(bite)))
        assert reach.max() <= 1.0 and bite.min() > 1.0


@pytest.mark.parametrize("cid", list(R.ALL))
def test_host_path_against_second_differences_of_predict(cid):
    """``D_t f = sum_i w_i f(x + h o_i) / (4 h^2)`` (k != l: offsets +-e_k +- e_l, weights +1 -1 -1 +1; k == l: +-2 e_k and 0, weights
    1 -2 1) from the long-double ``predict`` needs no derivative of the kernel.  Its mean and covariance differ from the package's
    ``hess_mean`` / ``hess_cov`` by the truncation bounds derived in DESIGN.md section 32 (second order in h; first order for the
    Matern 5/2 covariance), and halving h shrinks the gap by that order: an error of the closed forms would not shrink."""
    c = R.ALL[cid]
    X, y, alpha, H, _kap, Xq = R.problem(cid)
    d, rbf = c["d"], c["stationary"] == "rbf"
    e, x = np.eye(d), Xq[-1:]  # (the last query: a generic point in every case)
    terms = [[(2 * e[k], 1), (0 * e[k], -2), (-2 * e[k], 1)] if k == l else [(a * e[k] + b * e[l], a * b) for a in (1, -1) for b in (1, -1)]
             for k, l in zip(*np.tril_indices(d))]
    offs = hp._ld(np.array([o for tt in terms for o, _w in tt]))
    W = np.zeros((len(terms), len(offs)), dtype=hp.LD)
    W[np.repeat(np.arange(len(terms)), [len(tt) for tt in terms]), np.arange(len(offs))] = [w for tt in terms for _o, w in tt]
    hm, _hv, hc = _host(cid, 0, Xq=x)
    k, l = np.tril_indices(d)
    pst, s0 = R.post(cid, 0), R.reference(cid, 0, last=True)["s0"]
    asum, lmin = float(np.abs(P.f(pst["alpha"])).sum()), float(np.exp(H[0][1 : d + 1]).min())
    gaps = []
    for hrel in (1e-2, 5e-3):
        h = hp.LD(hrel * lmin)
        pr = hp.predict(X, y, alpha, H[0], hp._ld(x) + h * offs, c["stationary"], c["form"], noise_zero=True, return_cov=True, post=pst)
        Dm, Dc = P.f(W @ pr["mean"] / (4 * h * h)), P.f(W @ pr["cov"] @ W.T / (16 * h * h * h * h))
        gaps.append((float((np.abs(Dm - hm[0][k, l]) / s0).max()), float((np.abs(Dc - hc[0]) / (s0[:, None] * s0[None, :])).max())))
        assert gaps[-1][0] <= 2.0 * float(h) ** 2 * s0.max() * asum
        assert gaps[-1][1] <= (480.0 * hrel**2 if rbf else 34.0 * hrel + 240.0 * hrel**2)
    (m1, c1), (m2, c2) = gaps
    print("PRECISION hess %s: second differences vs host path, mean %.3g -> %.3g (ratio %.3f), covariance %.3g -> %.3g (ratio %.3f) at "
          "h = 1e-2, 5e-3 l_min" % (cid, m1, m2, m1 / m2, c1, c2, c1 / c2))
    assert 3.8 <= m1 / m2 <= 4.2
    assert (3.8 <= c1 / c2 <= 4.2) if rbf else (1.9 <= c1 / c2 <= 2.1)


def _quadratic_posterior(A, Xt, x0, noise=1e-8):
    """Host-path Hessian posterior at ``x0`` of an RBF GP (c = 100, l = 2) on (x - x0)^T A (x - x0) observed at ``Xt`` with ``noise``."""
    hk = np.concatenate([[np.log(100.0)], np.full(Xt.shape[1], np.log(2.0)), [np.log(noise)]])
    y = np.einsum("ik,kl,il->i", Xt - x0, A, Xt - x0)
    Ki = np.linalg.inv(100.0 * np.exp(-0.5 * ((Xt[:, None, :] - Xt[None, :, :]) ** 2).sum(axis=2) / 4.0) + noise * np.eye(len(Xt)))
    return tuple(v[0] for v in bask.hesscov.hessian_cov_host(hk, Xt, Ki @ y, 0.5 * (Ki + Ki.T), x0[None, :], "rbf", "product"))


def test_assembly_of_the_optimum_curvature_result_and_the_refusals():
    HC = bask.hesscov
    x0, delta = np.array([0.5, 0.5]), 0.01
    V = np.array([[1.0, 1.0], [-1.0, 1.0]]) / np.sqrt(2.0)  # columns: (1, -1) / sqrt2 and (1, 1) / sqrt2
    A = V @ np.diag([0.5, 4.0]) @ V.T
    hm, hv, hc = _quadratic_posterior(A, np.random.RandomState(3).uniform(size=(80, 2)), x0)
    out = HC.assemble_curvature(x0, hm, hv, hc, delta, 1000, np.random.RandomState(0), "host")
    # the Hessian of x^T A x is 2 A; an RBF surrogate with l = 2 is a quadratic on the unit box up to 1e-3 of the curvature (measured)
    np.testing.assert_allclose(out["eigenvalues"], [1.0, 8.0], rtol=5e-3)
    np.testing.assert_allclose(np.abs(out["eigenvectors"].T @ V), np.eye(2), atol=5e-3)
    assert (out["eigenvectors"][np.argmax(np.abs(out["eigenvectors"]), axis=0), np.arange(2)] > 0.0).all()
    want = np.sqrt(2.0 * delta / (2.0 * np.diag(A)))
    lo, hi = out["band"]["tolerance_conditional"]
    assert np.all(lo <= want) and np.all(want <= hi) and np.all(hi - lo <= 0.05 * want)
    np.testing.assert_allclose(out["tolerance_marginal"], np.sqrt(2.0 * delta * np.diag(np.linalg.inv(2.0 * A))), rtol=5e-3)
    assert out["prob_minimum"] == 1.0
    # a saddle observed only along its descending direction: the curvature across is the prior's, centred near 0
    line = np.column_stack([np.linspace(0.0, 1.0, 40), np.full(40, 0.5)])
    sad = HC.assemble_curvature(x0, *_quadratic_posterior(np.diag([-2.0, 3.0]), line, x0), delta, 1000, np.random.RandomState(0), "host")
    assert sad["prob_minimum"] < 0.5 and sad["eigenvalues"][0] < 0.0 and np.isnan(sad["tolerance_marginal"]).all()
    assert "optimum_curvature" in bask.utils.__all__ and bask.Optimizer.optimum_curvature is not None
    for st in ("matern32", "matern12"):
        with pytest.raises(ValueError, match="not twice differentiable"):
            HC.hessian_cov_host(np.zeros(4), np.zeros((3, 2)), np.zeros(3), np.eye(3), np.zeros((1, 2)), st, "product")
