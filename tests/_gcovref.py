"""Posterior covariance of the surrogate's gradient and the active-subspace sums (``bgp_grad_cov``, bgp_gcov.hip; DESIGN.md section
22): the cases shared by tests/test_cpu_gcov_reference.py and tests/test_gpu_gcov.py, the long-double reference and an fp64 numpy
replica of the device's route.

With ``G_jk(x) = cf fac(r_j) (x_k - X_jk) / l_k^2`` (tests/_gradref.py), ``H0 = diag(cf phi / l_k^2)``, phi = 1 / 3 / 5/3:
``g = G^T alpha``, ``Sigma = H0 - G^T K^-1 G``, ``C_mean = mean_s g g^T``, ``C_cov = mean_s Sigma``; normalised-y units.

* ``reference``: long double throughout, from ``oracle.hp_oracle`` (``posterior``, ``_r2``, ``_S``, ``_unpack``) and ``_gradref._fac``.
* ``replica64``: the same closed forms in fp64 numpy / LAPACK on an explicit inverse (what the device restates).

Metrics, against the existing tolerance classes of tests/_precision.py (no new constant):
* cov     ``max_kl |d Sigma_kl| / sqrt(H0_kk H0_ll)``  against ``tol("var", kappa, n)``: the prior variance of the two derivatives is
          the scale the cancellation H0 - Q happens on, as the prior variance is for the predictive variance;
* dmean   ``max |d g| / max_{s,k} sum_j |G_sjk alpha_j|``  against ``tol("mean", kappa, n)``  (the ``_gradref`` metric);
* csum    the first-order image of those two through the estimator, on the reference values:
          ``|d C_cov,kl| <= t_var sqrt(H0_kk H0_ll)``  (an average of covariances cannot lose more than one of them does) and, with
          every g moved by at most t_mean scale, ``|d C_mean,kl| <= t_mean scale (1 / m) sum_s (|g_sk| + |g_sl|)``."""
import functools

import numpy as np

import _gradref as GR
import _precision as P

TJ, RC, DMAX = 64, 256, 32  # bgp_gcov.hip: training tile, points per reduction chunk, limit on d
PHI = {"rbf": 1.0, "matern32": 3.0, "matern52": 5.0 / 3.0}
DIFFERENTIABLE = [(s, f) for f in ("product", "sum") for s in ("rbf", "matern32", "matern52")]


def _case(cid, n, d, st, fm, m, seed, B=1, Buse=1, special=False):
    return dict(id=cid, n=n, d=d, stationary=st, form=fm, m=m, seed=seed, B=B, Buse=Buse, special=special)


def _cases():
    # the six differentiable (family, form) pairs; n = 1 and on both sides of the 64-point training tile and of the 128-pad; d = 1
    # and at the padded widths 8 / 16 / 32 and just past them; m so that m d sits at a 128-row tile edge (15 / 16 / 17 at d = 8,
    # 4 / 5 at d = 32) and at the 256-point reduction chunk - 1, exact, + 1 and over several chunks
    rows = [
        (1, 1, "rbf", "product", 1),
        (63, 3, "matern32", "product", RC - 1),
        (64, 8, "matern52", "product", 15),
        (65, 8, "rbf", "sum", 16),
        (129, 8, "matern32", "sum", 17),
        (257, 9, "matern52", "sum", 20),
        (64, 16, "rbf", "product", 8),
        (65, 17, "matern32", "product", 9),
        (129, 32, "matern52", "product", 4),
        (63, 32, "rbf", "sum", 5),
        (129, 3, "matern52", "sum", RC),
        (65, 2, "matern32", "sum", RC + 1),
        (64, 1, "rbf", "product", 600),
        (385, 3, "rbf", "product", 33),
    ]
    out = [_case("gc%d_n%d_d%d_m%d_%s_%s" % (j, n, d, m, st, fm), n, d, st, fm, m, 2300 + j)
           for j, (n, d, st, fm, m) in enumerate(rows)]
    out.append(_case("gc_B3_n65_d3", 65, 3, "matern52", "product", 40, 2330, B=3, Buse=2))
    # three posteriors, all used, over three point chunks of the forced 256: the forced posterior chunks of
    # tests/test_gpu_chunk_loops.py run with both loop indices of gcov_run non-zero
    out.append(_case("gc_B3_n64_d2_m600", 64, 2, "matern52", "product", 600, 2350, B=3, Buse=3))
    # query 0 IS training point 0, query 1 is 1e-8 from it in every coordinate, query 2 lies far outside the data
    out.append(_case("gc_special_n129_d3", 129, 3, "matern32", "product", 6, 2340, special=True))
    return out


CASES = _cases()
ALL = {c["id"]: c for c in CASES}
FAR = 2  # index of the far-away query of the special case


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(X, y, alpha, H, kappas, Xq): the training set and canonical vectors of ``_precision._problem`` with the noise fitted to
    KAPPA_MAX, and the query points (a little outside the unit box too)."""
    c = ALL[cid]
    X, y, alpha, H = P._problem(c["n"], c["d"], c["seed"], c["stationary"], c["form"], c["B"], bool(c["seed"] % 2))
    Xq = np.random.RandomState(c["seed"] + 7).uniform(-0.1, 1.1, size=(c["m"], c["d"]))
    if c["special"]:
        Xq[0] = X[0]
        Xq[1] = X[0] + 1e-8
        Xq[FAR] = 50.0
    H, kap = P._fit_noise(X, alpha, H, c["stationary"], c["form"])
    return X, y, alpha, H, kap, Xq


@functools.lru_cache(maxsize=None)
def _post(cid, b):
    from oracle import hp_oracle as HP

    c = ALL[cid]
    X, y, alpha, H, _kap, _Xq = problem(cid)
    return HP.posterior(X, y, alpha, H[b], c["stationary"], c["form"])


def cross_gradient_ld(X, h, Xq, stationary, form):
    """(G (m, n, d), H0 diagonal (d,)) in long double."""
    from oracle import hp_oracle as HP

    d = np.atleast_2d(X).shape[1]
    cst, ell, _s2 = HP._unpack(h, d)
    r2 = HP._r2(Xq, X, ell)
    S = HP._S(r2, stationary)
    fac = GR._fac(r2, stationary, S, HP.LD)
    cf = cst if form == "product" else HP.LD(1)
    diff = (HP._ld(Xq)[:, None, :] - HP._ld(X)[None, :, :]) / (ell * ell)[None, None, :]
    phi = {"rbf": HP.LD(1), "matern32": HP.LD(3), "matern52": HP.LD(5) / HP.LD(3)}[stationary]
    return cf * fac[:, :, None] * diff, cf * phi / (ell * ell)


def reference_at(cid, b, Xq):
    """Long-double ``dmean`` (m, d), ``cov`` (m, d, d; not clipped), ``H0`` (d,), the scale of dmean and the two sums at ``Xq``."""
    c = ALL[cid]
    X, _y, _alpha, H, _kap, _ = problem(cid)
    post = _post(cid, b)
    G, h0 = cross_gradient_ld(X, H[b], Xq, c["stationary"], c["form"])
    dmean = np.einsum("sjk,j->sk", G, post["alpha"])
    P_ = np.einsum("sjk,ij->sik", G, post["K_inv"])
    cov = -np.einsum("sik,sil->skl", P_, G)
    idx = np.arange(len(h0))
    cov[:, idx, idx] += h0[None, :]
    scale = float(np.abs(G * post["alpha"][None, :, None]).sum(axis=1).max())
    m = len(dmean)
    return {"dmean": dmean, "cov": cov, "H0": h0, "scale_dmean": scale,
            "C_mean": np.einsum("sk,sl->kl", dmean, dmean) / m, "C_cov": cov.sum(axis=0) / m}


@functools.lru_cache(maxsize=None)
def reference(cid, b=0):
    return reference_at(cid, b, problem(cid)[5])


def replica64(X, y, alpha, h, Xq, stationary, form):
    """``(dmean, cov)`` in fp64 numpy / LAPACK: Gram matrix, Cholesky, explicit inverse, the closed forms; cov symmetric by
    construction of the product, diagonal clipped at 0 as the device clips it."""
    from oracle import gp_oracle as O
    from scipy.linalg import cho_solve, cholesky

    X, Xq = np.atleast_2d(np.asarray(X, dtype=np.float64)), np.atleast_2d(np.asarray(Xq, dtype=np.float64))
    n, d = X.shape
    K = O.gram_with_jitter(X, np.broadcast_to(alpha, (n,)), h, stationary, form)
    L = cholesky(K, lower=True, check_finite=False)
    a = cho_solve((L, True), y, check_finite=False)
    Ki = cho_solve((L, True), np.eye(n), check_finite=False)
    Ki = 0.5 * (Ki + Ki.T)
    cst, ell = np.exp(h[0]), np.exp(h[1 : d + 1])
    diff = Xq[:, None, :] - X[None, :, :]
    r2 = np.sum((diff / ell) ** 2, axis=2)
    if stationary == "rbf":
        S = np.exp(-0.5 * r2)
    else:
        S = None  # (fac of the Matern families does not read it)
    fac = GR._fac(r2, stationary, S, np.float64)
    cf = cst if form == "product" else 1.0
    G = cf * fac[:, :, None] * diff / (ell * ell)
    dmean = np.einsum("sjk,j->sk", G, a)
    Q = np.einsum("sik,sil->skl", np.einsum("sjk,ij->sik", G, Ki), G)
    cov = -0.5 * (Q + np.swapaxes(Q, 1, 2))
    idx = np.arange(d)
    cov[:, idx, idx] = np.maximum(cf * PHI[stationary] / (ell * ell) - Q[:, idx, idx], 0.0)
    return dmean, cov


def sums_in_order(dmean, cov, chunk=RC):
    """(C_mean, C_cov) of fp64 per-point values with chunk partials added in ascending order and one division by m."""
    m = len(dmean)
    cm, cc = np.zeros(cov.shape[1:]), np.zeros(cov.shape[1:])
    for i0 in range(0, m, chunk):
        g = dmean[i0 : i0 + chunk]
        cm = cm + np.einsum("sk,sl->kl", g, g)
        cc = cc + cov[i0 : i0 + chunk].sum(axis=0)
    return cm / m, cc / m


def h0_scale(ref):
    h0 = P.f(ref["H0"])
    return np.sqrt(h0[:, None] * h0[None, :])


def err_cov(got, ref):
    """max |d Sigma_kl| / sqrt(H0_kk H0_ll).  The clipped diagonal of ``got`` is compared with the clipped reference."""
    r = P.f(ref["cov"]).copy()
    idx = np.arange(r.shape[1])
    r[:, idx, idx] = np.maximum(r[:, idx, idx], 0.0)
    return float((np.abs(P.f(got) - r) / h0_scale(ref)[None]).max())


def err_dmean(got, ref):
    return P.err_rel_max(got, ref["dmean"], ref["scale_dmean"])


def csum_ratio(got_mean, got_cov, ref, t_mean, t_var):
    """(worst |d C_mean| / bound, worst |d C_cov| / bound); a bound of exactly 0 is met by an error of exactly 0 alone."""
    g = np.abs(P.f(ref["dmean"]))
    gm = g.mean(axis=0)
    b_mean = t_mean * ref["scale_dmean"] * (gm[:, None] + gm[None, :])
    b_cov = t_var * h0_scale(ref)

    def ratio(err, bound):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0.0, 0.0, err / bound)
        return float(r.max())

    return (ratio(np.abs(P.f(got_mean) - P.f(ref["C_mean"])), b_mean), ratio(np.abs(P.f(got_cov) - P.f(ref["C_cov"])), b_cov))


def min_eig_scaled(cov, ref):
    """Smallest eigenvalue over the points of Sigma / sqrt(H0_kk H0_ll)."""
    return float(min(np.linalg.eigvalsh(P.f(S) / h0_scale(ref))[0] for S in P.f(cov)))
