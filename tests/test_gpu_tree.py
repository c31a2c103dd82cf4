"""Generic kernel trees evaluated on the device (csrc/bgp_tree.hip) against the long-double restatement of
tests/_treeref.py, and the LML / posterior / predict calls behind the kernel program against their host-matrix siblings fed the
reference matrices rounded to fp64 (tolerances: tests/_precision.py)."""
import numpy as np
import pytest
from sklearn.gaussian_process import kernels as sk

import _precision as P
from _treeref import tree_ref

pytestmark = pytest.mark.gpu
EPS = P.EPS


@pytest.fixture(scope="module")
def bask():
    import bayes_skopt_amd as bask

    assert bask._lib.device_count() >= 1
    return bask


def _deep():
    k = sk.RBF(0.9)
    for ell in (0.5, 0.6, 0.7, 1.1, 1.3, 1.7, 1.9):  # right-nested: the value stack reaches depth 8; four metrics
        k = sk.Sum(sk.Matern(ell, nu=1.5) if ell < 1 else sk.ConstantKernel(ell), k)
    return k


def _trees(d):
    ard = np.linspace(0.4, 1.6, d)
    return {
        "constant": sk.ConstantKernel(1.7) + sk.RBF(0.8),  # (a constant alone has no pair to evaluate: beside an RBF)
        "white": sk.WhiteKernel(0.3) + sk.RBF(0.8),
        "rbf_ard": sk.RBF(ard) * sk.ConstantKernel(0.9),
        "matern12": sk.Matern(0.7, nu=0.5) + sk.ConstantKernel(0.1),
        "matern32_ard": sk.Matern(ard, nu=1.5) + sk.ConstantKernel(0.1),
        "matern52": sk.Matern(0.6, nu=2.5) + sk.ConstantKernel(0.1),
        "rq": sk.RationalQuadratic(0.6, alpha=1.3),
        "ess": sk.ExpSineSquared(0.9, periodicity=0.7),
        "dot": sk.DotProduct(0.6),
        "m52_rbf_white": sk.Matern(0.4, nu=2.5) * sk.RBF(0.7) + sk.WhiteKernel(0.05),
        "m52_m32": sk.Matern(0.3, nu=2.5) + sk.Matern(1.1, nu=1.5),
        "c_rq_white": sk.ConstantKernel(0.8) * sk.RationalQuadratic(0.5, alpha=1.3) + sk.WhiteKernel(0.03),
        "rbf2_dot": sk.Exponentiation(sk.RBF(0.8), 2) * sk.DotProduct(0.5),
        "deep": _deep(),
        "white_in_product": sk.WhiteKernel(0.4) * sk.RBF(0.5) + sk.Matern(0.9, nu=1.5),
        "shared_ard": sk.Matern(ard, "fixed", nu=2.5) * sk.RBF(ard, "fixed") + sk.WhiteKernel(0.02),
    }


def _exp_args(k, X, Y):
    """Entry-wise bound on the largest exponent argument of the leaves of ``k`` (fp64 is enough for a bound): 1 + 2 |log K_leaf|
    covers t of exp(-t) poly(t) for RBF / Matern and alpha log(base) of RQ; ExpSineSquared adds the response of 2 sin^2 / l^2 to its
    sine's argument; Exponentiation scales its child's bound by |e| and adds |e log K_child|."""
    if isinstance(k, (sk.Sum, sk.Product)):
        return np.maximum(_exp_args(k.k1, X, Y), _exp_args(k.k2, X, Y))
    if isinstance(k, sk.Exponentiation):
        return abs(k.exponent) * (_exp_args(k.kernel, X, Y) + np.abs(np.log(k.kernel(X, Y))))
    if isinstance(k, (sk.ConstantKernel, sk.WhiteKernel, sk.DotProduct)):
        return np.zeros((len(X), len(X if Y is None else Y)))
    with np.errstate(divide="ignore"):
        A = 1.0 + 2.0 * np.abs(np.log(np.maximum(k(X, Y), 1e-300)))
    if isinstance(k, sk.ExpSineSquared):
        Z = X if Y is None else Y
        r = np.sqrt(((X[:, None, :] - Z[None, :, :]) ** 2).sum(axis=2))
        A = A + 4.0 * np.pi * r / (k.periodicity * k.length_scale**2)
    return A


def _tolerance(k, prog, X, Y, ref, d):
    """Per entry, derived from the program, never from the device's answer.  Relative part eps (R + G (1 + A)): R = 4 n_ins roundings
    on the path (a leaf's polynomial and its <= 1 ulp exp / pow / sin: at most 4; a Sum / Product: 1); G = d + 2 Lmax + 10 is the
    relative error of an exponent argument in eps -- d fma accumulations of squares that each carry the roundings of (x - y), of the
    product with 1 / l and of the square (4), the round trip l -> log l -> exp(-log l) of a parameter twice (2 (Lmax + 2), Lmax the
    largest |log parameter|), the square root and the leaf's scale factor (2) --; A the entry's largest exponent argument
    (``_exp_args``), which is what turns a relative error of the argument into one of the value.  Absolute floor: eps max |K|, for
    entries that are exact zeros or sums of terms of either sign."""
    with np.errstate(divide="ignore"):
        Lmax = np.abs(prog._fixed[np.isfinite(prog._fixed)]).max()
    R, G = 4 * int(prog.ops[1]), d + 2.0 * Lmax + 10.0
    return EPS * (R + G * (1.0 + _exp_args(k, X, Y))) * np.abs(ref) + EPS * np.abs(ref).max()


SHAPES = [(1, 3, 5), (65, 1, 67), (130, 3, 67), (65, 32, 5)]  # (n, d, m): one row; a partial tile beside a full one; two npad
#                                                                blocks and a mirrored off-diagonal tile; d = 1 and d = 32


@pytest.mark.parametrize("n,d,m", SHAPES)
def test_device_tree_matrices_against_the_long_double_reference(bask, n, d, m):
    rng = np.random.RandomState(100 + n + d)
    X = rng.uniform(size=(n, d))
    if n > 1:
        X[n // 2] = X[0]  # a duplicated row: r = 0 off the diagonal (Matern 1/2 and ExpSineSquared at the origin)
    Xq = rng.uniform(size=(m, d))
    Xq[0] = X[0]
    ctx = bask._lib.Context(X, np.zeros(n), np.full(n, 1e-10), max_batch=4)
    worst = {}
    for name, k in _trees(d).items():
        prog = bask.kernels.compile_tree(k, d)
        assert prog is not None, name
        with np.errstate(divide="ignore"):
            T = k.theta + 0.15 * rng.randn(3, len(k.theta))  # B = 3 with distinct parameters
            ks = [k.clone_with_theta(t) for t in T]
        Pm = prog.params(T)
        Ks = ctx.tree_gram(prog, Pm)
        Kc = ctx.tree_gram(prog, Pm, Xq)
        for b, kb in enumerate(ks):
            np.testing.assert_array_equal(Ks[b], Ks[b].T, err_msg=name)  # exactly symmetric
            np.testing.assert_array_equal(ctx.tree_gram(prog, Pm[b])[0], Ks[b], err_msg=name)  # a B = 1 call: the same bits
            np.testing.assert_array_equal(ctx.tree_gram(prog, Pm[b], Xq)[0], Kc[b], err_msg=name)
            for got, Y in ((Ks[b], None), (Kc[b], X)):
                A = X if Y is None else Xq
                ref = tree_ref(kb, A, Y)
                tol = _tolerance(kb, prog, A, Y, ref.astype(np.float64), d)
                dev = float((np.abs(got - ref).astype(np.float64) / tol).max())
                skl = float((np.abs(kb(A, Y) - ref).astype(np.float64) / tol).max())  # scikit-learn's own fp64 error, same scale
                worst[name] = max(worst.get(name, 0.0), dev)
                print("%-18s n=%d d=%d %s: device %.3f tol, scikit-learn %.3f tol" % (name, n, d, "self" if Y is None else "cross", dev, skl))
                assert dev <= 1.0, (name, b, dev)
    print("worst device error / tolerance:", max(worst.values()))
    ctx.close()


def _lml_err(y, got, ref_lml, a, L):
    return abs(got - ref_lml) / (0.5 * abs(y @ a) + np.abs(np.log(np.diag(L))).sum() + len(y) / 2 * np.log(2 * np.pi))


def _check(errs, kappa, n, what):
    for q, v in errs.items():
        t = P.tol(q.split("/")[0], kappa, n)
        print("%s %-10s %.3e (tol %.3e)" % (what, q, v, t))
        assert v <= t, (what, q, v, t)


@pytest.mark.parametrize("vec_alpha", [False, True])
def test_lml_posterior_predict_behind_the_program_match_the_host_matrix_calls(bask, vec_alpha):
    n, d, B, m = 130, 3, 3, 37
    rng = np.random.RandomState(7)
    X, y, Xq = rng.uniform(size=(n, d)), rng.randn(n), rng.uniform(size=(m, d))
    ad = 1e-10 + (0.01 * rng.uniform(size=n) if vec_alpha else np.zeros(n))
    k = sk.Matern(0.4, nu=2.5) * sk.RBF(0.7) + sk.WhiteKernel(0.05)
    T = k.theta + 0.2 * rng.randn(B, len(k.theta))
    ks = [k.clone_with_theta(t) for t in T]
    prog = bask.kernels.compile_tree(k, d)
    Pm = prog.params(T)
    K, Ks, Kss = (np.stack([tree_ref(kb, *a).astype(np.float64) for kb in ks]) for a in ((X,), (Xq, X), (Xq,)))
    ctx = bask._lib.Context(X, y, ad, max_batch=4)
    wl = ctx.lml_gram(K)
    gl = ctx.lml_tree(prog, Pm)
    want = ctx.posterior_gram(K, want_K_inv=True)
    wmean, wvar, wcov = ctx.predict_gram(Ks, np.stack([np.diag(c) for c in Kss]), Kss)
    got = ctx.posterior_tree(prog, Pm, want_K_inv=True)
    mean, var, cov = ctx.predict_tree(prog, Pm, Xq, return_cov=True)
    for b in range(B):
        Kb = K[b] + np.diag(ad)
        a, L = want["alpha"][b], np.linalg.cholesky(Kb)
        _check({"lml": _lml_err(y, got["lml"][b], want["lml"][b], a, L), "lml/batch": _lml_err(y, gl[b], wl[b], a, L),
                "alpha": P.err_rel_max(got["alpha"][b], a), "K_inv": P.err_K_inv(got["K_inv"][b], want["K_inv"][b]),
                "mean": P.err_rel_max(mean[b], wmean[b], np.abs(Ks[b] * a[None, :]).sum(axis=1).max()),
                "var": P.err_rel_max(var[b], wvar[b], Kss[b].max()), "var/cov": P.err_rel_max(cov[b], wcov[b], Kss[b].max())},
               np.linalg.cond(Kb), n, "item %d" % b)
    # an item that is not positive definite (both length scales e^40, no white level, no alpha: a matrix of exact ones): -inf and
    # the failing pivot as the host-matrix call reports them, the neighbours' bits untouched
    bad = Pm.copy()
    bad[1] = prog.params(np.array([40.0, 40.0, -np.inf]))[0]
    lb, sb = ctx.lml_tree(prog, bad, use_alpha=False, return_status=True)
    Kbad = K.copy()
    Kbad[1] = 1.0
    lw, sw = ctx.lml_gram(Kbad, use_alpha=False, return_status=True)
    ok = ctx.lml_tree(prog, Pm, use_alpha=False)
    assert lb[1] == -np.inf and sb[1] == sw[1] != 0 and sb[0] == sb[2] == 0 and lb[0] == ok[0] and lb[2] == ok[2]
    ctx.close()


def test_per_walker_warps_behind_the_program(bask):
    n, d, B = 65, 2, 3
    rng = np.random.RandomState(11)
    X, y = rng.uniform(size=(n, d)), rng.randn(n)
    ad = np.full(n, 1e-10)
    k = sk.Matern(0.3, nu=2.5) + sk.Matern(1.1, nu=1.5) + sk.WhiteKernel(0.02)
    T = k.theta + 0.2 * rng.randn(B, len(k.theta))
    W = rng.uniform(-0.7, 0.7, size=(B, 2 * d))
    prog = bask.kernels.compile_tree(k, d)
    ctx = bask._lib.Context(X, y, ad, max_batch=4)
    K = np.stack([tree_ref(k.clone_with_theta(t), ctx.beta_cdf(X, w)).astype(np.float64) for t, w in zip(T, W)])
    want, got = ctx.lml_gram(K), ctx.lml_tree(prog, prog.params(T), warp=W)
    for b in range(B):
        Kb = K[b] + np.diag(ad)
        L = np.linalg.cholesky(Kb)
        a = np.linalg.solve(Kb, y)
        _check({"lml": _lml_err(y, got[b], want[b], a, L)}, np.linalg.cond(Kb), n, "walker %d" % b)
    ctx.close()


def test_routing_of_a_generic_tree_through_the_program(bask):
    n, d = 60, 2
    rng = np.random.RandomState(5)
    X = rng.uniform(size=(n, d))
    y = np.sin(4 * X[:, 0]) + X[:, 1] ** 2 + 0.05 * rng.randn(n)
    Xq = rng.uniform(size=(19, d))
    gp = bask.BayesGPR(kernel=sk.Matern(nu=2.5) * sk.RBF() + sk.WhiteKernel(), normalize_y=False, random_state=4)
    assert gp.tree_path == "auto"
    gp.fit(X, y, n_desired_samples=40, n_burnin=2, n_walkers_per_thread=20, progress=False)
    assert gp._generic and gp._plan.program is not None
    rows = gp.chain_[::9]
    out = {}
    for path in ("auto", "host"):
        gp.tree_path = path
        gp.theta = gp.theta  # (the posterior rebuilt through this path)
        out[path] = (gp.log_marginal_likelihood(rows), *gp.predict(Xq, return_std=True))
    gp.tree_path = "auto"
    gp.theta = gp.theta
    Kb = gp.kernel_(X) + 1e-10 * np.eye(n)
    kap, L, a = np.linalg.cond(Kb), np.linalg.cholesky(Kb), np.linalg.solve(Kb, y)
    kss = float(gp.kernel_.diag(Xq).max())
    for b in range(len(rows)):
        Kr = gp._kernel_at(rows[b])(X) + 1e-10 * np.eye(n)
        _check({"lml": _lml_err(y, out["auto"][0][b], out["host"][0][b], np.linalg.solve(Kr, y), np.linalg.cholesky(Kr))},
               np.linalg.cond(Kr), n, "row %d" % b)
    _check({"mean": P.err_rel_max(out["auto"][1], out["host"][1], np.abs(gp.kernel_(Xq, X) * a[None, :]).sum(axis=1).max()),
            "var": P.err_rel_max(out["auto"][2] ** 2, out["host"][2] ** 2, kss)}, kap, n, "median GP")
    # the median GP's predict and a one-row hyper_predict of the same theta: the same bits
    m1, v1, _ = gp._post.predict(gp, Xq, False)
    m2, v2 = gp._post.hyper_predict(gp, gp.theta[None, :], Xq, False)
    np.testing.assert_array_equal(m1, m2)
    np.testing.assert_array_equal(v1, v2)
