"""Sobol' sensitivity of the surrogate mean (``bgp_sobol_indices``, bgp_sobol.hip): the cases shared by
tests/test_cpu_sobol_reference.py and tests/test_gpu_sobol.py, the long-double reference and an fp64 numpy replica of the device's
route.

For sample matrices A, Bm (N x d) and a term (a set of dimensions, a mask), with fA_i = mu(A_i), fB_i = mu(Bm_i) and fT_i = mu(A_i
with the term's columns taken from Bm_i):
``f0 = mean(fA, fB)``, ``V = (1 / 2N) sum (fA - f0)^2 + (fB - f0)^2``, ``C = (1 / N) sum (fB - f0) (fT - fA)``,
``J = (1 / 2N) sum (fA - fT)^2``, all in normalised-y units.

* ``reference``: ``oracle.hp_oracle.gram`` on the SYNTHESISED rows times the long-double ``alpha`` of ``hp_oracle.lml``, then the
  estimator in long double.
* ``replica64``: what the device computes, in fp64 numpy: every row's squared distance as a sum of squares in x / l over the
  dimensions in ascending order, the kernel, the dot product with the fp64 alpha, the estimator in chunks of 256 samples whose
  partials are added in order, f0 first.  ``minus=True`` forms a term's distance as "the distance of A_i minus the swapped terms
  plus the new ones" instead (what the kernel must not do).

Metric.  The error of f0 is ``|d f0| / scale`` with ``scale = max_rows sum_j |K*_ij alpha_j|`` over every synthetic row of the call
-- the predictive mean's metric of tests/_precision.py -- against ``t = tol("mean", kappa, n)``: an average of means cannot lose
more than one of them does.  V, C and J are held against the FIRST-ORDER IMAGE of that tolerance through the estimator, evaluated
on the reference means (the ``ref_acq`` approach of tests/_precision.py).  With every mean moved by at most dmu = t scale:
  d V = (1 / N) sum (fA - f0) d fA + (fB - f0) d fB          (the term in d f0 carries sum (fA - f0) + (fB - f0) = 0)
        |d V| <= dmu (1 / N) sum |fA - f0| + |fB - f0|
  d C = (1 / N) sum (d fB - d f0) (fT - fA) + (fB - f0) (d fT - d fA)
        |d C| <= dmu (2 / N) sum |fT - fA| + |fB - f0|
  d J = (1 / N) sum (fA - fT) (d fA - d fT)
        |d J| <= dmu (2 / N) sum |fA - fT|
A bound of exactly 0 (the empty term: fT IS fA) is met by an error of exactly 0 alone.  No new constant."""
import functools
import math

import numpy as np

import _pdref as PD
import _precision as P

TJ, RC, DMAX, TMAX = 64, 256, 32, 4096  # bgp_sobol.hip: training tile, samples per reduction chunk (and per workgroup), limits


def _singles(d):
    return [(k,) for k in range(d)]


def _case(cid, n, d, st, fm, N, terms, seed, B=1, Buse=1, twin=False):
    return dict(id=cid, n=n, d=d, stationary=st, form=fm, N=N, terms=[tuple(t) for t in terms], seed=seed, B=B, Buse=Buse,
                twin=twin)


def _cases():
    # every stationary family x both forms; n on both sides of the 64-point training tile and at the sizes the other post-hoc
    # kernels tile by (32, 128, 256); d at 1, at the padded row widths 8 / 16 / 32 and just past them (9, 17); N at the 256-sample
    # chunk - 1, exact, + 1, below it and over several chunks; T = 1, T = d, singletons + all pairs at d = 4
    rows = [
        (1, 1, "rbf", "product", 1, [(0,)]),
        (31, 3, "matern12", "product", RC - 1, _singles(3)),
        (32, 8, "matern32", "sum", RC, [(2, 5)]),
        (33, 17, "matern52", "product", RC + 1, _singles(17)),
        (65, 32, "rbf", "sum", 40, _singles(32)),
        (129, 4, "matern12", "sum", 2 * RC + 88, _singles(4) + [(a, b) for a in range(4) for b in range(a + 1, 4)]),
        (257, 9, "matern32", "product", 64, [(0,), (8,), (0, 8), (1, 2, 3)]),
        (63, 16, "matern52", "sum", 100, [(0,), (15,), (7, 8)]),
        (64, 3, "rbf", "product", 17, _singles(3)),
    ]
    out = [_case("sb%d_n%d_d%d_N%d_T%d_%s_%s" % (j, n, d, N, len(terms), st, fm), n, d, st, fm, N, terms, 2100 + j)
           for j, (n, d, st, fm, N, terms) in enumerate(rows)]
    # the empty and the full mask, a repeated term, a term listed twice in different positions, 2 of 3 resident posteriors
    out.append(_case("sb_mixed_B3", 20, 3, "matern32", "product", 37, [(), (0, 1, 2), (1,), (0, 2), (1,), (2,), (0, 2)], 2130,
                     B=3, Buse=2))
    # r = 0: A_0 IS training point 0; A_1 is within 1e-8 of it in every coordinate but the first, where it is far away, and Bm_1
    # is within 1e-8 of it in every coordinate -- the term {0} (and every term that holds 0) puts a row 1e-8 from a training point
    out.append(_case("sb_twin_matern12", 40, 3, "matern12", "product", 17, _singles(3) + [(0, 1), (0, 2), (1, 2)], 2140, B=3,
                     Buse=3, twin=True))
    return out


CASES = _cases()
ALL = {c["id"]: c for c in CASES}


def masks_of(terms):
    return [sum(1 << k for k in set(t)) for t in terms]


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(X, y, alpha, H, kappas, A, Bm): the training set and canonical vectors of ``_precision._problem`` with the noise fitted to
    KAPPA_MAX, and two sample matrices in the unit box."""
    c = ALL[cid]
    X, y, alpha, H = P._problem(c["n"], c["d"], c["seed"], c["stationary"], c["form"], c["B"], False)
    rng = np.random.RandomState(c["seed"] + 7)
    A, Bm = rng.uniform(size=(c["N"], c["d"])), rng.uniform(size=(c["N"], c["d"]))
    if c["twin"]:
        A[0] = X[0]
        A[1] = X[0] + 1e-8
        A[1, 0] = (X[0, 0] + 0.5) % 1.0
        Bm[1] = X[0] + 1e-8
    H, kap = P._fit_noise(X, alpha, H, c["stationary"], c["form"])
    return X, y, alpha, H, kap, A, Bm


def synth_rows(A, Bm, mask):
    """A with the columns whose bits are set in ``mask`` taken from Bm (the dtype of the inputs is kept)."""
    pick = np.array([(mask >> k) & 1 for k in range(A.shape[1])], dtype=bool)
    return np.where(pick[None, :], Bm, A)


def all_rows(A, Bm, masks):
    """The (T + 2) N rows of a call: A, Bm, then every term's synthetic rows."""
    return np.concatenate([A, Bm] + [synth_rows(A, Bm, m) for m in masks])


def estimator(F, chunk=None):
    """(f0, V, C (T,), J (T,)) from the means F (T + 2, N) in F's own dtype.  ``chunk``: per-chunk partial sums added in ascending
    order, as the device does; None: one sum."""
    N = F.shape[1]

    def total(v):
        if chunk is None:
            return v.sum(axis=-1)
        s = np.zeros(v.shape[:-1], dtype=v.dtype)
        for i0 in range(0, N, chunk):
            s = s + v[..., i0:i0 + chunk].sum(axis=-1)
        return s

    fA, fB, fT = F[0], F[1], F[2:]
    two_n = F.dtype.type(2 * N)
    f0 = total(fA + fB) / two_n
    ca, cb = fA - f0, fB - f0
    V = total(ca * ca + cb * cb) / two_n
    dt = fT - fA[None, :]
    return f0, V, total(cb[None, :] * dt) / F.dtype.type(N), total(dt * dt) / two_n


def reference_of(X, y, alpha, h, A, Bm, masks, stationary, form, warp=None):
    """Long double: dict of the means ``F`` (T + 2, N), their absolute-sum ``scale``, ``f0``, ``V``, ``C``, ``J`` and the first-order
    images ``gV``, ``gC``, ``gJ`` of a unit error of every mean (see the module docstring).  ``warp``: context-level warp
    parameters -- training inputs and both matrices through ``hp_oracle.warp_inputs``."""
    from oracle import hp_oracle as HP

    N = len(A)
    Xt = HP.warp_inputs(X, warp) if warp is not None else X
    a = HP.lml(Xt, y, alpha, h, stationary, form)["alpha"]
    if warp is not None:
        A, Bm = HP.warp_inputs(A, warp), HP.warp_inputs(Bm, warp)
    T = HP.gram(all_rows(A, Bm, masks), h, stationary, form, Y=Xt) * a[None, :]
    F = T.sum(axis=1).reshape(len(masks) + 2, N)
    f0, V, C, J = estimator(F)
    ca, cb, dt = np.abs(P.f(F[0] - f0)), np.abs(P.f(F[1] - f0)), np.abs(P.f(F[2:] - F[0][None, :]))
    return dict(F=F, scale=float(np.abs(T).sum(axis=1).max()), f0=f0, V=V, C=C, J=J, gV=float((ca + cb).sum() / N),
                gC=2.0 * (dt.sum(axis=1) + cb.sum()) / N, gJ=2.0 * dt.sum(axis=1) / N)


@functools.lru_cache(maxsize=None)
def reference(cid, b):
    c = ALL[cid]
    X, y, alpha, H, _kap, A, Bm = problem(cid)
    return reference_of(X, y, alpha, H[b], A, Bm, masks_of(c["terms"]), c["stationary"], c["form"])


def means64(X, a, h, A, Bm, masks, stationary, form, minus=False):
    """The device's means in fp64 numpy, (T + 2, N).  ``a``: the fp64 alpha."""
    n, d = X.shape
    cst, ell = math.exp(h[0]), np.exp(np.asarray(h[1:d + 1], dtype=np.float64))
    U, ua, ub = X / ell, A / ell, Bm / ell

    def sq(u, ks):
        q = np.zeros((len(u), n))
        for k in ks:
            df = u[:, k][:, None] - U[:, k][None, :]
            q = df * df + q
        return q

    out = []
    for m in [0, (1 << d) - 1] + list(masks):
        inside = [k for k in range(d) if (m >> k) & 1]
        if minus:  # the forbidden form: A_i's distance, the swapped columns' terms taken off, the new ones put on
            r2 = sq(ua, range(d)) - sq(ua, inside) + sq(ub, inside)
        else:
            r2 = sq(synth_rows(ua, ub, m), range(d))
        out.append(PD._kernel64(r2, cst, stationary, form) @ a)
    return np.array(out)


def replica64(X, a, h, A, Bm, masks, stationary, form, minus=False):
    """(f0, V, C, J) of the device's route in fp64 numpy."""
    return estimator(means64(X, a, h, A, Bm, masks, stationary, form, minus), chunk=RC)


def _ratio(err, bound):
    err, bound = np.atleast_1d(P.f(err)), np.atleast_1d(P.f(bound))
    err = np.nan_to_num(err, nan=np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err == 0.0, 0.0, err / bound).max())


def errs(got, ref, t):
    """{"f0", "V", "C", "J"}: the worst error of (f0, V, C, J) = ``got`` over its bound at mean tolerance ``t`` (1 = on the bound;
    a NaN, and any error against a bound of 0, counts as infinite)."""
    f0, V, C, J = got
    dmu = t * ref["scale"]
    return {"f0": _ratio(abs(f0 - P.f(ref["f0"])), dmu), "V": _ratio(abs(V - P.f(ref["V"])), dmu * ref["gV"]),
            "C": _ratio(np.abs(C - P.f(ref["C"])), dmu * ref["gC"]), "J": _ratio(np.abs(J - P.f(ref["J"])), dmu * ref["gJ"])}


def worst(got, ref, t):
    return max(errs(got, ref, t).values())
