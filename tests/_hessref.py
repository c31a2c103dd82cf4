"""Posterior of the surrogate's Hessian (``bgp_hess_cov``, bgp_hess.hip): the cases shared by
tests/test_cpu_hessian_reference.py and tests/test_gpu_hessian.py, the long-double reference (identities of section 32, from
``oracle.hp_oracle``'s ``posterior``, ``_r2``, ``_S``, ``_unpack``; vech order (k, l), k >= l, row-major) and the error metrics,
against the existing tolerance classes of tests/_precision.py (no new constant):
* hcov, hvar  ``max |d Cov[t, u]| / sqrt(P0[t, t] P0[u, u])``  against ``tol("var", kappa, n)``: the prior variance of the two second
              derivatives is the scale the cancellation P0 - Q happens on;
* hmean       every row on its own prior scale, ``max_t (|d Hbar_t| / sqrt(P0[t, t])) / max_{s,t} (sum_j |R_stj alpha_j| / sqrt(P0[t,
              t]))``  against ``tol("mean", kappa, n)``  (the ``_gradref`` metric: the absolute sum a correct summation loses digits on)."""
import functools

import numpy as np

import _gradref as GR
import _precision as P

# (n, d, family, form, m, B, Buse, special): the four (family, form) pairs; n = 1 and on both sides of the 64-point staging tile and of
# the 128-pad; T = 1, 3, 15, 21, 36, 136 (under one MFMA tile, at 15, across the 16-row tile edge, 136 -> Tp = 144); m = 1, 2 and
# m Tp across a 128-row tile edge of the ring (7 x 32, 3 x 48, 2 x 144); 2 of 3 resident posteriors; the special case: query 0 IS
# training point 0, query 1 is 1e-8 from it in every coordinate, query 2 (FAR) lies far outside the data
ROWS = [(1, 1, "rbf", "product", 1, 1, 1, False), (63, 2, "matern52", "product", 2, 1, 1, False), (65, 5, "rbf", "sum", 2, 1, 1, False),
        (129, 6, "matern52", "sum", 7, 1, 1, False), (65, 8, "matern52", "product", 3, 1, 1, False),
        (129, 16, "rbf", "product", 2, 1, 1, False), (63, 16, "matern52", "sum", 1, 1, 1, False), (65, 3, "rbf", "sum", 5, 3, 2, False),
        (129, 3, "matern52", "product", 4, 1, 1, True)]
CASES = [dict(id="hs%d_n%d_d%d_m%d_%s_%s" % (j, n, d, m, st, fm), n=n, d=d, stationary=st, form=fm, m=m, B=B, Buse=Bu, special=sp,
              seed=3200 + (j if j < 7 else 10 * (j - 4))) for j, (n, d, st, fm, m, B, Bu, sp) in enumerate(ROWS)]
ALL, FAR = {c["id"]: c for c in CASES}, 2


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(X, y, alpha, H, kappas, Xq): the training set and canonical vectors of ``_precision._problem`` with the noise fitted to
    KAPPA_MAX, and the query points (a little outside the unit box too)."""
    c = ALL[cid]
    X, y, alpha, H = P._problem(c["n"], c["d"], c["seed"], c["stationary"], c["form"], c["B"], bool(c["seed"] % 2))
    Xq = np.random.RandomState(c["seed"] + 7).uniform(-0.1, 1.1, size=(c["m"], c["d"]))
    if c["special"]:
        Xq[0], Xq[1], Xq[FAR] = X[0], X[0] + 1e-8, 50.0
    H, kap = P._fit_noise(X, alpha, H, c["stationary"], c["form"])
    return X, y, alpha, H, kap, Xq


@functools.lru_cache(maxsize=None)
def post(cid, b):
    from oracle import hp_oracle as HP

    X, y, alpha, H, _kap, _Xq = problem(cid)
    return HP.posterior(X, y, alpha, H[b], ALL[cid]["stationary"], ALL[cid]["form"])


@functools.lru_cache(maxsize=None)
def reference(cid, b=0, last=False):
    """Long-double ``hmean`` (m, T), ``cov`` (m, T, T; not clipped), ``P0`` (T, T), its root diagonal ``s0`` and the scale of hmean at
    the case's queries (``last``: at the last one alone)."""
    from oracle import hp_oracle as HP

    c, LD = ALL[cid], HP.LD
    X, h, Xq, d = problem(cid)[0], problem(cid)[3][b], problem(cid)[5][-1 if last else 0 :], c["d"]
    cst, ell, _s2 = HP._unpack(h, d)
    r2 = HP._r2(Xq, X, ell)
    S = HP._S(r2, c["stationary"])
    fac = GR._fac(r2, c["stationary"], S, LD)
    rbf = c["stationary"] == "rbf"
    fac2 = S if rbf else (LD(25) / LD(3)) * np.exp(-np.sqrt(LD(5)) * np.sqrt(r2))
    psi, cf = LD(1) if rbf else LD(25) / LD(3), cst if c["form"] == "product" else LD(1)
    w = (HP._ld(Xq)[:, None, :] - HP._ld(X)[None, :, :]) / (ell * ell)[None, None, :]  # z_k / l_k
    (k, l), il = np.tril_indices(d), 1 / ell
    R = cf * (fac2[:, None, :] * np.swapaxes(w[:, :, k] * w[:, :, l], 1, 2)
              + np.where(k == l, il[k] * il[l], LD(0))[None, :, None] * fac[:, None, :])
    K, L, Pq, Q = k[:, None], l[:, None], k[None, :], l[None, :]
    cnt = ((K == L) & (Pq == Q)).astype(LD) + ((K == Pq) & (L == Q)) + ((K == Q) & (L == Pq))
    P0 = cf * psi * cnt * (il[K] * il[L]) * (il[Pq] * il[Q])
    pst = post(cid, b)
    s0 = np.sqrt(P.f(np.diagonal(P0)))
    scale = float((P.f(np.abs(R * pst["alpha"][None, None, :]).sum(axis=2)) / s0[None, :]).max())
    return {"hmean": R @ pst["alpha"], "cov": P0[None] - np.einsum("stj,ji,sui->stu", R, pst["K_inv"], R), "P0": P0, "s0": s0,
            "scale_hmean": scale}


def errors(hm, hv, hc, ref):
    """(hcov, hvar, hmean) errors on the metrics above; the clipped diagonal is compared with the clipped reference."""
    (k, l), idx = np.tril_indices(hm.shape[-1]), np.arange(hc.shape[-1])
    r = P.f(ref["cov"]).copy()
    r[:, idx, idx] = np.maximum(r[:, idx, idx], 0.0)
    s0 = ref["s0"]
    return (float((np.abs(P.f(hc) - r) / (s0[:, None] * s0[None, :])[None]).max()),
            float((np.abs(P.f(hv)[:, k, l] - r[:, idx, idx]) / (s0 * s0)[None]).max()),
            float((np.abs(P.f(hm)[:, k, l] - P.f(ref["hmean"])) / s0[None, :]).max() / ref["scale_hmean"]))
