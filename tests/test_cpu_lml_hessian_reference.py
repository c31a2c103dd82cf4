"""The reference, the tolerance and the host path of the LML-Hessian tests (tests/_lmlhessref.py; ``bgp_lml_hess_batch``, DESIGN.md
section 33), without a device:
(a) the long-double analytic Hessian against Richardson-extrapolated central differences of ``hp_oracle.lml_and_grad``; (b) the numpy
host path against the reference, which fixes ``C_HESS``; (c) three deliberate slips miss the tolerance; (d) ``hyper_laplace`` (host path
on a stub context) with ONE free parameter: the log evidence against quadrature.  ``pytest -s``: lines that start with ``PRECISION``."""
import numpy as np
import pytest

import _lmlhessref as R
import _precision as P

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)
from oracle import gp_oracle as O  # noqa: E402


@pytest.mark.parametrize("st,fm", P.FAMILIES)
def test_analytic_hessian_against_richardson_differences_of_the_gradient(st, fm):
    X, y, alpha, H = P._problem(14, 2, 3400, st, fm, 1, True, dup=True)
    H, kap = P._fit_noise(X, alpha, H, st, fm)
    h = H[0]
    ref = R.hessian(X, y, alpha, h, st, fm)

    def diff(step):  # central difference of the long-double gradient, column l
        out = np.empty((4, 4), dtype=hp.LD)
        for l in range(4):
            e = np.zeros(4)
            e[l] = step
            out[:, l] = (hp.lml_and_grad(X, y, alpha, h + e, st, fm)["grad"] - hp.lml_and_grad(X, y, alpha, h - e, st, fm)["grad"]) / (2 * hp.LD(step))
        return out

    d = [diff(2.0 ** -s) for s in (6, 7, 8)]  # (steps exact in fp64: h + e is the number meant)
    r1 = [(4 * d[i + 1] - d[i]) / 3 for i in range(2)]  # the h^2 term removed, then the h^4 term: the remainder is O(h^6) = 4e-15 x
    rich = R.err((16 * r1[1] - r1[0]) / 15, ref)         # a derivative ratio, beside the gradient's own kappa 2^-63 n / h of rounding
    g1, g2 = R.err(d[0], ref), R.err(d[1], ref)
    print("PRECISION lmlhess %s/%s kappa %.2g: gap %.2e, ratio on halving the step %.3f, Richardson gap %.2e = %.2e tol"
          % (st, fm, kap[0], g1, g1 / g2, rich, rich / R.tol(kap[0], 14)))
    assert 3.9 < g1 / g2 < 4.1 and rich <= R.tol(kap[0], 14) / 100.0


def _host(cid, b):
    from bayes_skopt_amd import lmlhess

    c = R.ALL[cid]
    X, y, alpha, H, _ = R.problem(cid)
    _L, Ki, a = O.posterior(X, y, np.broadcast_to(alpha, (len(X),)), H[b], c["stationary"], c["form"])
    return lmlhess.lml_hess_host(X, H[b], Ki, a, c["stationary"], c["form"])


def test_host_path_against_the_reference_fixes_the_constant():
    worst = 0.0
    for cid, c in R.ALL.items():
        kap = R.problem(cid)[4]
        for b in range(c["B"]):
            e = R.err(_host(cid, b), R.reference(cid, b))
            unit = kap[b] ** 2 * P.EPS
            print("PRECISION lmlhess %s b%d kappa %.3g: host vs long double %.3e = %.3e kappa^2 eps = %.4f tol"
                  % (cid, b, kap[b], e, e / unit, e / R.tol(kap[b], c["n"])))
            assert e <= R.tol(kap[b], c["n"]) / 8.0
            if unit >= P.FLOOR["grad"]:  # (the rows at which the condition term can reach the floor)
                worst = max(worst, e / unit)
    print("PRECISION lmlhess worst host ratio: %.3e kappa^2 eps (C_HESS = %.1e)" % (worst, R.C_HESS))
    assert 8.0 * worst <= R.C_HESS <= 16.0 * worst  # (the margin of 8, rounded up to one digit)


@pytest.mark.parametrize("slip,cid", [("delta", R.CASES[3]["id"]), ("transpose", R.CASES[3]["id"]), ("constant", R.CASES[4]["id"]),
                                      ("delta", R.CASES[6]["id"]), ("transpose", R.CASES[9]["id"]), ("constant", R.CASES[9]["id"])])
def test_deliberate_slips_miss_the_tolerance(slip, cid):
    ref, bad = R.reference(cid, 0), R.reference(cid, 0, slip)
    e = R.err(bad["hess"], ref) / R.tol(R.problem(cid)[4][0], R.ALL[cid]["n"])
    print("PRECISION lmlhess %s slip %s: %.3g tol" % (cid, slip, e))
    assert e >= 100.0


def test_hyper_laplace_log_evidence_against_quadrature_on_one_free_parameter():
    """ConstantKernel and WhiteKernel fixed, ONE isotropic length scale free, enough data for a near-quadratic log posterior."""
    import scipy.integrate
    import scipy.optimize

    import bayes_skopt_amd as bask
    from bayes_skopt_amd._posterior import CanonicalPosterior
    from bayes_skopt_amd.kernels import RBF, ConstantKernel, WhiteKernel, analyse_kernel

    rng = np.random.RandomState(5)
    X = rng.uniform(size=(60, 2))
    y = np.sin(4.0 * X[:, 0]) + np.cos(3.0 * X[:, 1]) + 0.05 * rng.randn(60)
    y = (y - y.mean()) / y.std()
    ad = np.full(60, 1e-8)

    class Ctx:  # what the host path asks of a context, from the fp64 oracle
        def posterior(self, H, want_alpha=True, want_K_inv=False):
            _L, Ki, a = O.posterior(X, y, ad, H[0], "rbf", "product")
            return {"lml": np.array([O.lml(X, y, ad, H[0], "rbf", "product")]), "status": np.zeros(1, dtype=np.int32),
                    "K_inv": Ki[None], "alpha": a[None]}

        def lml_grad(self, H):
            v, g = O.lml_and_grad(X, y, ad, H[0], "rbf", "product")
            return np.array([v]), g[None], np.zeros(1, dtype=np.int32)

    gp = bask.BayesGPR(kernel=ConstantKernel(1.0, "fixed") * RBF(0.3) + WhiteKernel(0.01, "fixed"), optimizer=None)
    gp.kernel_ = gp.kernel
    gp._X_train_, gp.y_train_ = X, y
    gp._plan, gp._ctx_obj, gp._backend = analyse_kernel(gp.kernel_), Ctx(), CanonicalPosterior()
    gp._backend.lml_hess_path = "host"
    prior = lambda t: -0.5 * (t + 1.0) ** 2  # noqa: E731
    logpost = lambda t: O.lml(X, y, ad, gp._canonical(np.array([t]))[0], "rbf", "product") + prior(t)  # noqa: E731
    mode = scipy.optimize.minimize_scalar(lambda t: -logpost(t), bounds=(-3.0, 1.0), method="bounded", options={"xatol": 1e-10}).x
    gp._post_theta = np.array([mode])
    out = gp.hyper_laplace(priors=[prior], n_samples=500, random_state=1)
    top = logpost(mode)
    Z = scipy.integrate.quad(lambda t: np.exp(logpost(t) - top), mode - 12 * out["sd"][0], mode + 12 * out["sd"][0], epsabs=0, epsrel=1e-10)[0]
    print("PRECISION lmlhess laplace: log evidence %.6f, quadrature %.6f, sd %.4f" % (out["log_evidence"], top + np.log(Z), out["sd"][0]))
    assert out["path"] == "host" and out["negative_definite"] and out["mode"].shape == (1,) and out["corr"][0, 0] == 1.0
    # the Laplace error is the posterior's non-Gaussianity: third and fourth cumulants over n = 60 points, O(1 / n)
    assert abs(out["log_evidence"] - (top + np.log(Z))) < 0.05
    h = 1e-3  # the curvature itself: second difference of the log posterior (truncation h^2 f'''' / 12)
    curv = (logpost(mode + h) - 2 * top + logpost(mode - h)) / h**2
    assert abs(out["hessian"][0, 0] - curv) <= 1e-4 * abs(curv)
    lo, hi = gp.kernel_.bounds[0]
    assert out["samples"].shape == (500, 1) and (out["samples"] >= lo).all() and (out["samples"] <= hi).all()
    assert abs(out["samples"].std() - out["sd"][0]) < 0.15 * out["sd"][0]
    flat = gp.hyper_laplace(theta=np.array([2.0]), priors=[lambda t: 0.0 * t + 300.0 * t * t])  # a prior that makes the point a MINIMUM
    assert not flat["negative_definite"] and np.isnan(flat["log_evidence"]) and np.isnan(flat["cov"]).all()
    gp.warp_inputs = True
    with pytest.raises(NotImplementedError):
        gp.hyper_laplace()
