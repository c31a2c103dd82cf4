"""Hessian of the log marginal likelihood (``bgp_lml_hess_batch``, bgp_lmlhess.hip): the cases shared by
tests/test_cpu_lml_hessian_reference.py and tests/test_gpu_lml_hessian.py, the analytic Hessian in long double on
``oracle.hp_oracle``'s primitives (the second kernel derivatives are written here), the error metric and the tolerance.

* metric     ``max_kl |d H_kl| / scale_kl``, scale_kl = 1/2 sum |W D_kl| + |v_k|^T |K^-1| |v_l| + 1/2 sum |P_k[i,j] P_l[j,i]|: the
             absolute sums a correct fp64 summation can lose digits on (the ``grad`` metric of tests/_precision.py, term by term)
* tolerance  ``max(FLOOR["grad"] sqrt(n / 128), C_HESS kappa^2 eps)``: ``tol("grad")`` with kappa^2, because K^-1 enters twice.  C_HESS
             = 8 x the fp64 host path's worst ``err / (kappa^2 eps)`` over the rows of CASES with kappa^2 eps >= FLOOR (where the
             condition term can reach the floor at all), rounded up to one digit: 8 x 1.164e-4 (lh2)."""
import functools

import numpy as np

import _precision as P

C_HESS = 1e-3

# n = 1, under / at / over the 128 tile edge, two tile rows with a mirror pair; d = 1, 3, 16; B = 1, 3; the eight families; vector
# alpha_diag; duplicated training points for the r = 0 guards of Matern 1/2 and 3/2
ROWS = [(1, 1, "rbf", "product", 1, False, False), (127, 3, "matern12", "product", 3, True, False),
        (128, 16, "matern32", "product", 1, False, False), (129, 3, "matern52", "product", 3, True, False),
        (257, 3, "rbf", "sum", 1, False, False), (129, 1, "matern12", "sum", 1, True, False),
        (127, 16, "matern32", "sum", 1, False, False), (257, 1, "matern52", "sum", 3, True, False),
        (129, 3, "matern12", "product", 1, False, True), (129, 3, "matern32", "sum", 1, True, True)]
CASES = [dict(id="lh%d_n%d_d%d_%s_%s_B%d%s" % (j, n, d, st, fm, B, "_dup" if dup else ""), n=n, d=d, stationary=st, form=fm, B=B,
              vec_alpha=vec, dup=dup, seed=3300 + j) for j, (n, d, st, fm, B, vec, dup) in enumerate(ROWS)]
ALL = {c["id"]: c for c in CASES}


def tol(kappa, n):
    return max(P.FLOOR["grad"] * max(1.0, (n / 128.0) ** 0.5), C_HESS * kappa * kappa * P.EPS)


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(X, y, alpha, H, kappas) of ``_precision._problem`` with the noise fitted to KAPPA_MAX."""
    c = ALL[cid]
    X, y, alpha, H = P._problem(c["n"], c["d"], c["seed"], c["stationary"], c["form"], c["B"], c["vec_alpha"], c["dup"])
    H, kap = P._fit_noise(X, alpha, H, c["stationary"], c["form"])
    return X, y, alpha, H, kap


def _fr2(r2, stationary, LD):
    """fr2 = -2 dfr / dr^2 of the family (0 where r = 0 makes it singular: it multiplies u_k u_l = 0 there)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if stationary == "rbf":
            return np.exp(LD(-0.5) * r2)
        r = np.sqrt(r2)
        if stationary == "matern12":
            return np.where(r > 0, np.exp(-r) * (1 + r) / (r * r * r), LD(0))
        if stationary == "matern32":
            t = np.sqrt(LD(3)) * r
            return np.where(t > 0, 9 * np.exp(-t) / t, LD(0))
        return LD(25) / 3 * np.exp(-np.sqrt(LD(5)) * r)


def hessian(X, y, alpha_diag, h, stationary, form, slip=None):
    """Long double: {"hess" (p, p), "scale" (p, p), "lml", "grad"}.  ``slip``: a deliberate mistake -- "delta" (the delta_kl term of
    D_kl dropped), "transpose" (P_l[i, j] for P_l[j, i] in the trace), "constant" (the product form's constant row and column
    under whatever form the kernel has)."""
    from oracle import hp_oracle as HP

    LD = HP.LD
    X = HP._ld(X)
    n, d = X.shape
    p = d + 2
    r = HP.lml_and_grad(X, y, alpha_diag, h, stationary, form)
    a, Ki = r["alpha"], HP.inverse_from_factor(r["L"])
    W = np.outer(a, a) - Ki
    cst, ell, _s2 = HP._unpack(h, d)
    product = form == "product" or slip == "constant"
    cf = cst if form == "product" else LD(1)
    D = np.stack([HP.kernel_gradient_k(X, h, k, stationary, form) for k in range(p)])
    if slip == "constant" and form != "product":
        S = HP._S(HP._r2(X, X, ell), stationary)
        np.fill_diagonal(S, LD(1))
        D[0] = cst * S
    Xs = X / ell
    U = np.stack([(Xs[:, k][:, None] - Xs[:, k][None, :]) ** 2 for k in range(d)])
    w2 = cf * _fr2(HP._r2(X, X, ell), stationary, LD)
    np.fill_diagonal(w2, LD(0))
    first, fscale = np.zeros((p, p), dtype=LD), np.zeros((p, p), dtype=LD)
    for k in range(d):
        for l in range(d):
            Dkl = w2 * U[k] * U[l] - (2 * D[1 + k] if k == l and slip != "delta" else 0)
            first[1 + k, 1 + l], fscale[1 + k, 1 + l] = (W * Dkl).sum() / 2, np.abs(W * Dkl).sum() / 2
    for k, l in [(0, 0), (p - 1, p - 1)] + ([(0, 1 + j) for j in range(d)] if product else []):
        first[k, l] = first[l, k] = (W * D[max(k, l)]).sum() / 2
        fscale[k, l] = fscale[l, k] = np.abs(W * D[max(k, l)]).sum() / 2
    Pm = np.stack([D[k] @ Ki for k in range(p)])
    v = D @ a
    q, qscale = v @ Ki @ v.T, np.abs(v) @ np.abs(Ki) @ np.abs(v).T
    Pr = Pm if slip == "transpose" else np.swapaxes(Pm, 1, 2)
    T = np.array([[(Pm[k] * Pr[l]).sum() for l in range(p)] for k in range(p)], dtype=LD)
    Ts = np.array([[np.abs(Pm[k] * Pr[l]).sum() for l in range(p)] for k in range(p)], dtype=LD)
    return {"hess": first - q + T / 2, "scale": fscale + qscale + Ts / 2, "lml": r["lml"], "grad": r["grad"]}


@functools.lru_cache(maxsize=None)
def reference(cid, b=0, slip=None):
    c = ALL[cid]
    X, y, alpha, H, _ = problem(cid)
    return hessian(X, y, alpha, H[b], c["stationary"], c["form"], slip)


def err(got, ref):
    s = P.f(ref["scale"])
    return float((np.abs(P.f(got) - P.f(ref["hess"])) / np.maximum(s, 1e-30 * s.max() + 1e-300)).max())
