"""Extended-precision reference for the pathwise posterior draws (bgp_paths_*), its fp64 numpy restatement,
the case list shared by tests/test_cpu_paths_reference.py and tests/test_gpu_paths.py, and the error metric.

Path p (normalised-y units; h = its posterior's canonical vector, h[-1] = log s2):
  A = sqrt(2 cS / F), cS = c (product form) | 1 (sum form)
  f0(x) = A sum_j w_j cos(phase_j + sum_k (x_k / l_k) omega_jk)  [+ sqrt(c) w_F, sum form]
  r = y - f0(X) - sqrt(alpha_diag + s2) eps ;  v = K^-1 r ;  f(x) = f0(x) + sum_i k(x, X_i) v_i
  df/dx_k = -A sum_j w_j sin(arg_j) omega_jk / l_k + sum_i v_i G_ik        (G as in tests/_gradref.py)

Error metric: |f - f_ref| / s(x), s(x) = A sum_j |w_j| (1 + |phase_j| + sum_k |x_k omega_jk / l_k|) + sum_i |k(x, X_i) v_i| -- the
absolute sum a correct fp64 summation can lose digits on; the argument term is there because the rounding of a large cosine
argument (Matern-1/2 frequencies are Cauchy: they reach 1e4) is legitimate fp64 behaviour.  The gradient's component k is measured
on the derivative of that sum, s_k(x) = A sum_j |w_j omega_jk / l_k| (1 + |phase_j| + sum_k' |x_k' omega_jk' / l_k'|) + sum_i |v_i G_ik|.
Tolerance, in the shape of ``_precision.tol``: ``max(FLOOR sqrt(n / 128), C kappa eps64)`` with the class "path" below.

C and FLOOR are those of the class "K_inv" of tests/_precision.py (4 kappa eps64, floor 2e-12): v is a product with the explicit
resident inverse, so a path cannot be held to more than that inverse is -- and every other step (the feature sum, the generated
GEMV) is a sum of F or n rounded terms, which the floor covers.  They satisfy the project's rule on every case of ``CASES``
(tests/test_cpu_paths_reference.py asserts it): the fp64 numpy restatement ``path64`` -- the device's own method: v by a product
with the explicit inverse -- lies within tol / 10 of the long-double reference, and the same computation with X and Xq rounded to
fp32 misses it by >= 10 tol.  Measured (x86-64, 80-bit long double; worst over the cases, value and gradient together): fp64
restatement err / tol <= 5.2e-4 (bound 0.1); fp32 inputs err / tol >= 44 (bound 10; the one-point case path0, then 70 at
kappa = 1.9e4)."""
import functools
import math

import numpy as np

import _precision as P

C = {"path": 4.0}
FLOOR = {"path": 2e-12}
NU = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}


def tol(kappa, n):
    return max(FLOOR["path"] * max(1.0, math.sqrt(n / 128.0)), C["path"] * kappa * P.EPS)


def _case(j, st, fm, n, d, F, m, Pn, vec_alpha, **kw):
    return dict(id="path%d_%s_%s_n%d_d%d_F%d_m%d_P%d" % (j, st, fm, n, d, F, m, Pn), stationary=st, form=fm, n=n, d=d, F=F, m=m,
                P=Pn, vec_alpha=vec_alpha, seed=1400 + j, **kw)


# the smallest shapes that cross a tile edge (64 features / 64 training points / 256 rows) or degenerate; P = 3: two paths on one
# posterior, one on another
CASES = [
    _case(0, "rbf", "product", 1, 1, 1, 1, 1, False),
    _case(1, "matern12", "product", 63, 3, 63, 255, 3, True, dup_query=True),
    _case(2, "matern32", "product", 64, 17, 64, 257, 1, False),
    _case(3, "matern52", "product", 65, 32, 65, 1, 3, True),
    _case(4, "rbf", "sum", 130, 3, 200, 257, 3, False, no_constant=True),
    _case(5, "matern12", "sum", 65, 1, 200, 255, 1, True),
    _case(6, "matern32", "sum", 130, 17, 63, 1, 3, False, no_white=True),
    _case(7, "matern52", "sum", 64, 32, 1, 257, 1, False),
    _case(8, "rbf", "product", 63, 32, 64, 255, 3, True),
    _case(9, "matern52", "product", 130, 17, 200, 255, 1, False),
]
ALL = {c["id"]: c for c in CASES}


def draw_variates(rng, Pn, F, d, n, stationary):
    """omega (P, F, d), phase (P, F), w (P, F + 1), eps (P, n) in the order ``BayesGPR.sample_paths`` documents."""
    omega, phase = np.empty((Pn, F, d)), np.empty((Pn, F))
    w, eps = np.empty((Pn, F + 1)), np.empty((Pn, n))
    for p in range(Pn):
        z = rng.standard_normal((F, d))
        if stationary in NU:
            z = z * np.sqrt(2.0 * NU[stationary] / rng.chisquare(2.0 * NU[stationary], size=F))[:, None]
        omega[p], phase[p] = z, rng.uniform(0.0, 2.0 * np.pi, size=F)
        w[p], eps[p] = rng.standard_normal(F + 1), rng.standard_normal(n)
    return omega, phase, w, eps


@functools.lru_cache(maxsize=None)
def problem(cid):
    """dict: X, y, alpha, H (B, d + 2; noise fitted so that kappa <= 1e5), kappa (B,), pidx (P,), Xq, omega, phase, w, eps."""
    c = ALL[cid]
    B = 2 if c["P"] > 1 else 1
    X, y, alpha, H = P._problem(c["n"], c["d"], c["seed"], c["stationary"], c["form"], B, c["vec_alpha"])
    if c.get("no_constant"):
        H[:, 0] = -np.inf
    if c.get("no_white"):  # the white level is off: the conditioning comes from alpha alone
        H[:, -1] = -np.inf
        alpha = 1e-4
        while max(P.kappa_of(X, alpha, h, c["stationary"], c["form"]) for h in H) > P.KAPPA_MAX:
            alpha *= 4.0
        kap = np.array([P.kappa_of(X, alpha, h, c["stationary"], c["form"]) for h in H])
    else:
        H, kap = P._fit_noise(X, alpha, H, c["stationary"], c["form"])
    rng = np.random.RandomState(c["seed"] + 5)
    Xq = rng.uniform(-0.1, 1.1, size=(c["m"], c["d"]))
    if c.get("dup_query"):
        Xq[7] = X[11]  # r = 0 between a query row and a training row
    pidx = np.array([0, 1, 0][: c["P"]], dtype=np.int32)
    omega, phase, w, eps = draw_variates(rng, c["P"], c["F"], c["d"], c["n"], c["stationary"])
    return dict(X=X, y=y, alpha=alpha, H=H, kappa=kap, pidx=pidx, Xq=Xq, omega=omega, phase=phase, w=w, eps=eps)


def _stationary_fac(r2, stationary, xp):
    """(S, (dS/dr) / r) from squared scaled distances in the scalar type ``xp``; Matern 1/2: fac = 0 at r = 0."""
    if stationary == "rbf":
        S = np.exp(-r2 / 2)
        return S, -S
    r = np.sqrt(r2)
    if stationary == "matern12":
        S = np.exp(-r)
        with np.errstate(divide="ignore", invalid="ignore"):
            return S, np.where(r > 0, -S / np.where(r > 0, r, xp(1)), xp(0))
    if stationary == "matern32":
        t = np.sqrt(xp(3)) * r
        e = np.exp(-t)
        return (1 + t) * e, -xp(3) * e
    t = np.sqrt(xp(5)) * r
    e = np.exp(-t)
    return (1 + t + t * t / 3) * e, -(xp(5) / xp(3)) * (1 + t) * e


def _path(xp, solve, X, y, alpha, h, omega, phase, w, eps, Xq, stationary, form):
    """One path in the scalar type ``xp``; ``solve(K, r)`` returns K^-1 r.  Returns f (m,), df (m, d), s (m,), sg (m, d)."""
    X, Xq = np.asarray(X, dtype=np.float64).astype(xp), np.atleast_2d(np.asarray(Xq, dtype=np.float64)).astype(xp)
    n, d = X.shape
    F = omega.shape[0]
    with np.errstate(divide="ignore"):
        e = np.exp(np.asarray(h, dtype=np.float64).astype(xp))
    cst, ell, s2 = e[0], e[1 : d + 1], e[d + 1]
    product = form == "product"
    A = np.sqrt(2 * (cst if product else xp(1)) / xp(F))
    oms = omega.astype(xp) / ell[None, :]
    ww, ph = w.astype(xp), phase.astype(xp)
    c0 = xp(0) if product else np.sqrt(cst) * ww[F]

    def feats(Z):
        return ph[None, :] + Z @ oms.T  # (rows, F)

    def kern(Z):
        diff = (Z[:, None, :] - X[None, :, :]) / ell[None, None, :]  # scaled differences (rows, n, d)
        S, fac = _stationary_fac(np.sum(diff * diff, axis=2), stationary, xp)
        return (cst * S if product else cst + S), (cst if product else xp(1)) * fac, diff

    f0X = A * (np.cos(feats(X)) @ ww[:F]) + c0
    S0, _, _ = kern(X)
    K = np.array(S0, copy=True)
    np.fill_diagonal(K, (cst if product else cst + 1) + s2)
    ad = np.broadcast_to(np.asarray(alpha, dtype=np.float64), (n,)).astype(xp)
    K[np.diag_indices(n)] += ad
    r = (y.astype(xp) - f0X) - np.sqrt(ad + s2) * eps.astype(xp)
    v = solve(K, r)
    arg = feats(Xq)
    Ks, gfac, diff = kern(Xq)
    f = A * (np.cos(arg) @ ww[:F]) + c0 + Ks @ v
    G = gfac[:, :, None] * diff / ell[None, None, :]  # (m, n, d)
    df = -A * ((np.sin(arg) * ww[None, :F]) @ oms) + np.einsum("j,ijk->ik", v, G)
    amp = 1 + np.abs(ph)[None, :] + np.abs(Xq) @ np.abs(oms).T  # (m, F)
    s = A * (amp @ np.abs(ww[:F])) + np.abs(Ks * v[None, :]).sum(axis=1)
    sg = A * np.einsum("ij,jk->ik", amp * np.abs(ww[None, :F]), np.abs(oms)) + np.abs(v[None, :, None] * G).sum(axis=1)
    return f, df, s, sg


def _solve_ld(K, r):
    from oracle import hp_oracle as HP

    return HP.cho_solve(HP.cholesky(K), r)


def _solve_inv64(K, r):
    """The device's method: the explicit inverse (from a Cholesky factor), then a matrix-vector product."""
    from scipy.linalg import cho_solve, cholesky

    L = cholesky(K, lower=True, check_finite=False)
    return cho_solve((L, True), np.eye(len(K)), check_finite=False) @ r


def _all_paths(cid, xp, solve, round32=False):
    c, pr = ALL[cid], problem(cid)
    X, Xq = (P.to32(pr["X"]), P.to32(pr["Xq"])) if round32 else (pr["X"], pr["Xq"])
    out = [_path(xp, solve, X, pr["y"], pr["alpha"], pr["H"][pr["pidx"][p]], pr["omega"][p], pr["phase"][p], pr["w"][p],
                 pr["eps"][p], Xq, c["stationary"], c["form"]) for p in range(c["P"])]
    return [np.stack([o[k] for o in out]) for k in range(4)]  # f (P, m), df (P, m, d), s (P, m), sg (P, m, d)


@functools.lru_cache(maxsize=None)
def ref_paths(cid):
    """Long-double f (P, m), df (P, m, d) and the scales s (P, m), sg (P, m, d)."""
    from oracle import hp_oracle as HP

    HP.require()
    f, df, s, sg = _all_paths(cid, HP.LD, _solve_ld)
    return {"f": f, "df": df, "s": P.f(s), "sg": P.f(sg)}


def path64(cid, round32=False):
    """(f, df) of the fp64 numpy restatement; ``round32``: X and Xq rounded to fp32 first."""
    f, df, _s, _sg = _all_paths(cid, np.float64, _solve_inv64, round32)
    return f, df


def err(f, df, ref):
    """(value error, gradient error) on the scales of the module docstring; ``df`` may be None."""
    ev = float((np.abs(P.f(f) - P.f(ref["f"])) / ref["s"]).max())
    if df is None:
        return ev, 0.0
    sg = np.maximum(ref["sg"], 1e-300)
    return ev, float((np.abs(P.f(df) - P.f(ref["df"])) / sg).max())


def case_tol(cid):
    pr = problem(cid)
    return tol(float(pr["kappa"].max()), ALL[cid]["n"])


def moments_restated(X, y, alpha, h, stationary, form, Xq, n_paths, F, seed):
    """``n_paths`` paths of ONE posterior at Xq in fp64 numpy, the variates drawn as ``sample_paths(sample_mean=True)`` draws them
    from ``RandomState(seed)``: (n_paths, m)."""
    rng = np.random.RandomState(seed)
    n, d = X.shape
    omega, phase, w, eps = draw_variates(rng, n_paths, F, d, n, stationary)
    out = np.empty((n_paths, len(Xq)))
    from scipy.linalg import cho_solve, cholesky

    cache = {}

    def solve(K, r):
        if "L" not in cache:
            cache["L"] = cholesky(K, lower=True, check_finite=False)
        return cho_solve((cache["L"], True), r, check_finite=False)

    for p in range(n_paths):
        out[p] = _path(np.float64, solve, X, y, alpha, h, omega[p], phase[p], w[p], eps[p], Xq, stationary, form)[0]
    return out
