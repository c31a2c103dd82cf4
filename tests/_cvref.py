"""Cross-validation from the resident inverses (``bgp_cross_validate``, bgp_cv.hip): the cases shared by
tests/test_cpu_cv_reference.py and tests/test_gpu_cv.py, the long-double reference, an fp64 numpy replica of the device's
recurrences and the tolerance.

With A = K^-1 (alpha diagonal and white level in K) and a = A y, the device forms for a fold F
``Sigma_F = A_FF^-1, r_F = Sigma_F a_F, mu_F = y_F - r_F, var = diag Sigma_F, lpd_F = -1/2 a_F^T r_F + sum log C_kk - s/2 log 2 pi``.

* ``reference``: no identity at all -- ``oracle.hp_oracle.predict`` on the REMAINING points (``noise_zero=False, return_cov=True``)
  plus ``diag(alpha_F)``, then a long-double Cholesky factor of that covariance for the log density of ``y_F``.
* ``replica64``: the device's route in fp64 numpy: K^-1 from the LAPACK factor, then the fold kernel's recurrences -- A_FF gathered,
  factorised column by column, C^-1 by forward substitution, the two triangular products, ordered sums.  ``inputs32``: the training
  inputs rounded to fp32 before the Gram build; ``block32``: A_FF rounded to fp32 before its factorisation (the two single-precision
  slips the tolerance has to catch).

Errors, each on the scale a correct fp64 computation can lose digits on:

* ``cv_mean``  max |d mu| / max_i sum_j |Sigma_F,ij a_j|
* ``cv_var``   max |d var| / max_i var_i
* ``cv_lpd``   |d lpd| / (1/2 sum |a_i r_i| + sum |log C_kk| + s/2 log 2 pi)

against ``tol(q, kappa, n) = max(FLOOR[q] max(1, sqrt(n / 128)), C[q] kappa eps)`` (the form of ``_precision.tol``; + the Beta-CDF
budget under input warping), kappa = the 2-norm condition number of the full Gram matrix.

The mean's reach grows faster than kappa on the fold's own scale, and that is modelled, not absorbed into a constant: a_F carries
the ABSOLUTE error of the full solve, kappa eps max |a|, so a fold whose own |a| are small -- a leave-one-out point that the others
predict almost exactly -- loses ``amp = max_j |a_j| / max_{j in F} |a_j|`` times more on sum_j |Sigma_F,ij a_j|.  Without the factor
the fp64 replica is off by 8.7 kappa eps on one leave-one-out point of case cv8 while no fold of more than 60 points exceeds 0.05;
``tol("cv_mean", ..., amp=...)`` multiplies its kappa term by ``amp`` (every fold's reference carries it, from the long-double a).

The constants are the smallest one-significant-digit values for which, over every (row, fold) of CASES, the replica stays within
tol / 10 and, per case, row and quantity, both slips miss by at least 10 tol on their worst fold -- the floor first (n = 1, 2), then
C (tests/test_cpu_cv_reference.py asserts both margins and prints them).  Measured with them: worst reach 0.0952 tol (mean, n = 2, on
the floor; 0.0921 on C, the leave-one-out case), 0.0978 tol (variance, n = 2, floor; 0.0905 on C, n = 65 at kappa 5.4e4), 0.0797
tol (lpd, n = 1, floor; 0.0694 on C); worst bite, inputs rounded to fp32: 2975 / 11 630 / 2067 tol (mean / var / lpd), A_FF rounded
to fp32: 1368 / 5879 / 136 tol.  At n = 1 the Gram matrix reads no input (K = k(0) + s2 + alpha): rounding the inputs changes no
bit there, which the test asserts instead of a margin.  No case changed its seed."""
import functools
import math

import numpy as np

import _precision as P

SMAX = 128  # bgp_cv.hip CV_SMAX

C = {"cv_mean": 0.9, "cv_var": 0.8, "cv_lpd": 2.0}
FLOOR = {"cv_mean": 2e-15, "cv_var": 3e-15, "cv_lpd": 2e-15}


def tol(quantity, kappa, n, sens=0.0, amp=1.0):
    """``amp`` (``cv_mean`` only; a fold's reference carries it): max_j |a_j| / max_{j in F} |a_j| >= 1.  a_F inherits the ABSOLUTE
    error of the full solve, kappa eps max |a|, so on the fold's own scale the mean's reach grows with that ratio and not with kappa
    alone: a leave-one-out point that the others predict almost exactly (|a_i| << max |a|) is the extreme."""
    return (max(FLOOR[quantity] * max(1.0, math.sqrt(n / 128.0)), C[quantity] * kappa * P.EPS * (amp if quantity == "cv_mean" else 1.0))
            + P.CDF_REL * sens)


QUANTITIES = ("cv_mean", "cv_var", "cv_lpd")


def _case(j, n, d, family, vec_alpha, B, Buse, folds):
    st, fm = family
    return dict(id="cv%d_n%d_d%d_%s_%s_B%dof%d" % (j, n, d, st, fm, Buse, B), n=n, d=d, stationary=st, form=fm, vec_alpha=vec_alpha,
                B=B, Buse=Buse, seed=1700 + j, folds=[np.asarray(f, dtype=np.int64) for f in folds])


def _perm(n, j):
    return np.random.RandomState(1750 + j).permutation(n)


def _cases():
    F = P.FAMILIES
    out = []
    # the whole training set held out: nothing remains, the predictive is the prior (one point: the one-point kernel)
    out.append(_case(0, 1, 1, F[0], False, 1, 1, [[0]]))
    # leave-one-out at n = 2, listed backwards
    out.append(_case(1, 2, 2, F[1], True, 1, 1, [[1], [0]]))
    # 63 shuffled points and 1 in one call, one point uncovered; 2 of 3 resident rows
    p = _perm(65, 2)
    out.append(_case(2, 65, 3, F[2], False, 3, 2, [p[:63], p[63:64]]))
    # a partition: 64 + 1
    p = _perm(65, 3)
    out.append(_case(3, 65, 2, F[3], True, 1, 1, [p[:64], p[64:]]))
    # a contiguous fold straddling index 128, the rest shuffled into 65 + 35: a partition of mixed sizes
    p = _perm(100, 4)
    out.append(_case(4, 129, 3, F[4], False, 1, 1, [np.arange(100, 129), p[:65], p[65:]]))
    # the largest fold, 128 shuffled points, beside a single point: a partition; 2 of 3 resident rows
    p = _perm(129, 5)
    out.append(_case(5, 129, 5, F[5], True, 3, 2, [p[:128], p[128:]]))
    # a contiguous fold straddling index 256, 127 shuffled points, 2 points; 71 points uncovered
    p = _perm(200, 6)
    out.append(_case(6, 257, 4, F[6], False, 1, 1, [np.arange(200, 257), p[:127], p[127:129]]))
    # a partition of three row blocks of the padded inverse: 128 + 128 + 127 + 2 shuffled points
    p = _perm(385, 7)
    out.append(_case(7, 385, 3, F[7], True, 1, 1, [p[:128], p[128:256], p[256:383], p[383:]]))
    # leave-one-out in shuffled order over 63 of 65 points (the other two: ``LOO_PAIR``); 2 of 3 resident rows
    p = _perm(65, 8)
    out.append(_case(8, 65, 2, F[3], True, 3, 2, [[i] for i in p[:63]]))
    return out


CASES = _cases()
ALL = {c["id"]: c for c in CASES}
LOO_CASE = CASES[8]["id"]
LOO_PAIR = _perm(65, 8)[63:]  # the two points that case leaves out: a two-point fold that sends the call through the fold kernel


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(X, y, alpha (n,), H, kappas) of a case: ``_precision._problem`` with the noise fitted to KAPPA_MAX, as ``_precision.problem``."""
    c = ALL[cid]
    X, y, alpha, H = P._problem(c["n"], c["d"], c["seed"], c["stationary"], c["form"], c["B"], c["vec_alpha"])
    H, kap = P._fit_noise(X, alpha, H, c["stationary"], c["form"])
    return X, y, np.broadcast_to(np.asarray(alpha, dtype=np.float64), (len(X),)).copy(), H, kap


def reference_of(X, y, alpha, h, folds, stationary, form):
    """Long double, per fold a dict: mean, var (s,), lpd and the three scales.  ``X`` may be long double (warped inputs)."""
    from oracle import hp_oracle as HP

    LD = HP.LD
    X = HP._ld(X)
    n = X.shape[0]
    yl = np.asarray(y, dtype=np.float64).astype(LD)
    a_full = HP.lml(X, y, alpha, h, stationary, form)["alpha"]
    out = []
    for F in folds:
        F = np.asarray(F)
        rest = np.setdiff1d(np.arange(n), F)
        s = len(F)
        if len(rest) == 0:
            mean = np.zeros(s, dtype=LD)
            cov = HP.gram(X[F], h, stationary, form, alpha_diag=alpha[F])
        else:
            pr = HP.predict(X[rest], y[rest], alpha[rest], h, X[F], stationary, form, noise_zero=False, return_cov=True)
            mean = pr["mean"]
            cov = pr["cov"] + np.diag(alpha[F].astype(LD))
        L = HP.cholesky(cov)
        r = yl[F] - mean
        z = HP.solve_lower(L, r)
        half_log2pi = HP._log2pi() / 2
        lpd = LD(-0.5) * (z @ z) - np.log(np.diagonal(L)).sum() - s * half_log2pi
        aF = a_full[F]
        Cf = HP.cholesky(HP.inverse_from_factor(L))  # A_FF = C C^T
        out.append({"mean": mean, "var": np.diagonal(cov).copy(), "lpd": lpd, "amp": float(np.abs(a_full).max() / np.abs(aF).max()),
                    "scale": {"cv_mean": float(np.abs(cov * aF[None, :]).sum(axis=1).max()),
                              "cv_var": float(np.diagonal(cov).max()),
                              "cv_lpd": float(LD(0.5) * np.abs(aF * r).sum() + np.abs(np.log(np.diagonal(Cf))).sum()
                                              + s * half_log2pi)}})
    return out


@functools.lru_cache(maxsize=None)
def reference(cid, b):
    c = ALL[cid]
    X, y, alpha, H, _ = problem(cid)
    return reference_of(X, y, alpha, H[b], c["folds"], c["stationary"], c["form"])


def inverse64(X, y, alpha, h, stationary, form):
    """(K^-1, K^-1 y) in fp64 from the LAPACK factor (the resident arrays of a posterior build)."""
    from oracle import gp_oracle as O
    from scipy.linalg import cho_solve, cholesky

    K = O.gram_with_jitter(X, alpha, h, stationary, form)
    L = cholesky(K, lower=True, check_finite=False)
    A = cho_solve((L, True), np.eye(len(y)), check_finite=False)
    return 0.5 * (A + A.T), cho_solve((L, True), y, check_finite=False)


def fold64(A, a, y, F, block32=False):
    """The fold kernel's recurrences in fp64 numpy: (mean (s,), var (s,), lpd) of fold F from the inverse A and a = A y."""
    F = np.asarray(F)
    s = len(F)
    S = A[np.ix_(F, F)].copy()
    if block32:
        S = P.to32(S)
    aF = a[F]
    dd = np.empty(s)
    for j in range(s):  # right-looking, column by column
        dd[j] = math.sqrt(S[j, j])
        S[j + 1:, j] /= dd[j]
        S[j + 1:, j + 1:] -= np.outer(S[j + 1:, j], S[j + 1:, j])
    Cf = np.tril(S)
    np.fill_diagonal(Cf, dd)
    M = np.zeros((s, s))  # C^-1, column by column
    for c in range(s):
        M[c, c] = 1.0 / dd[c]
        for i in range(c + 1, s):
            M[i, c] = -(Cf[i, c:i] @ M[c:i, c]) / dd[i]
    w = M @ aF
    r = M.T @ w
    var = (M * M).sum(axis=0)
    lpd = -0.5 * float(aF @ r) + float(np.log(dd).sum()) - s * 0.5 * math.log(2.0 * math.pi)
    return y[F] - r, var, lpd


def replica64(X, y, alpha, h, folds, stationary, form, inputs32=False, block32=False):
    """Per fold (mean, var, lpd) in fp64; ``inputs32`` / ``block32``: the single-precision slips."""
    A, a = inverse64(P.to32(X) if inputs32 else P.f(X), y, alpha, h, stationary, form)
    return [fold64(A, a, y, F, block32) for F in folds]


def errs(got, ref):
    """{quantity: error} of one fold's (mean, var, lpd) against its reference (a NaN counts as an infinite error)."""
    mean, var, lpd = got
    sc = ref["scale"]
    e = {"cv_mean": np.abs(P.f(mean) - P.f(ref["mean"])).max() / sc["cv_mean"],
         "cv_var": np.abs(P.f(var) - P.f(ref["var"])).max() / sc["cv_var"],
         "cv_lpd": abs(float(lpd) - float(ref["lpd"])) / sc["cv_lpd"]}
    return {q: float(np.nan_to_num(v, nan=np.inf)) for q, v in e.items()}


def device_folds(mean, var, lpd, b, folds):
    """Row b of ``Context.cross_validate``'s arrays as per-fold (mean, var, lpd) tuples."""
    return [(mean[b, F], var[b, F], lpd[b, k]) for k, F in enumerate(folds)]


def covered(folds, n):
    m = np.zeros(n, dtype=bool)
    for F in folds:
        m[np.asarray(F)] = True
    return m


# ------------------------------------------------------------------------------------------------------------------------------
# per-row-warped residents (bgp_posterior_batch_warped): WARP_CASES[1]'s problem, two folds
# ------------------------------------------------------------------------------------------------------------------------------
WARP_CID = P.WARP_CASES[1]["id"]
_WARP_PERM = np.random.RandomState(1790).permutation(300)
WARP_FOLDS = [_WARP_PERM[:128], _WARP_PERM[128:178]]  # 128 and 50 shuffled points, 122 uncovered


@functools.lru_cache(maxsize=None)
def warp_reference(b):
    """Row b of the warped case: the reference on the long-double warped inputs, kappa of the warped Gram matrix and, per fold and
    quantity, the Beta-CDF sensitivity (the replica's error with the warped inputs rounded to fp32, over 2^-24: ``ref_set_warp``'s)."""
    c = P.ALL[WARP_CID]
    X, y, alpha, H, _ = P.problem(WARP_CID)
    alpha = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (len(X),)).copy()
    Xw, W, kap = P.warped_problem(WARP_CID)
    ref = reference_of(Xw[b], y, alpha, H[b], WARP_FOLDS, c["stationary"], c["form"])
    got32 = replica64(P.f(Xw[b]), y, alpha, H[b], WARP_FOLDS, c["stationary"], c["form"], inputs32=True)
    sens = [{q: v / P.F32 for q, v in errs(g, r).items()} for g, r in zip(got32, ref)]
    return ref, float(kap[b]), sens
