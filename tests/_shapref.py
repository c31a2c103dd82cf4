"""Shapley attribution of the surrogate mean (``bgp_shapley``, bgp_shapley.hip): the cases of
tests/test_cpu_shapley_reference.py and tests/test_gpu_shapley.py, the long-double reference (``hp_oracle.gram`` on the synthesised
rows times the long-double alpha) and an fp64 numpy replica of the device's route (half tables, r2 = TL + TH).  Both apply the
weights through the package's ``shapley_from_values`` in their own dtype, so neither sees an error in it: the closed-form test
of the CPU file and the device's own weights do.  Bounds: with ``t = tol("mean", kappa, n)`` and ``scale = max_rows sum_j |K*_ij
alpha_j|`` every mean moves by at most t scale, so base and value by t scale, phi (weights that sum to 1 on a difference of two
means) by 2 t scale, inter by 4 t scale and sum_k phi_k - (value - base) by (2 d + 2) t scale.  No new constant."""
import functools

import numpy as np

import _pdref as PD
import _precision as P
from bayes_skopt_amd._posterior import coalition_picks, coalition_rows, shapley_from_values

def _cases():  # n N at the pair tile - 1 / exact / + 1 (128 pairs below d = 8, 64 from there), at the 1024-pair chunk - 1 / exact / + 1 and over
    # three chunks; d = 1 (no high half), 2, 3 (uneven halves), every accumulator count (d = 4, 6, 8), 9, and 15, 16 (8, 16 coalition
    # blocks); N = 1, 2, 17; P = 1, 3; every family and form; inter given and NULL; 2 of 3 resident posteriors
    rows = [(1, 1, "rbf", "product", 1, 1), (63, 2, "matern12", "product", 2, 3), (127, 3, "matern32", "sum", 1, 1),
            (128, 3, "matern52", "product", 1, 1), (129, 3, "rbf", "sum", 1, 1), (63, 8, "matern12", "sum", 1, 1),
            (64, 8, "matern32", "product", 1, 1), (65, 8, "matern52", "sum", 1, 3), (33, 9, "rbf", "product", 31, 1),
            (32, 8, "matern12", "product", 32, 1), (41, 6, "matern32", "sum", 25, 1), (129, 4, "matern52", "product", 17, 1),
            (33, 15, "matern52", "sum", 3, 1), (17, 16, "matern32", "product", 2, 1)]
    out = [dict(id="sh%d_n%d_d%d_N%d_P%d_%s_%s" % (j, n, d, N, Pn, st, fm), n=n, d=d, stationary=st, form=fm, N=N, P=Pn,
                seed=2700 + j, B=1, Buse=1, inter=j % 3 != 1) for j, (n, d, st, fm, N, Pn) in enumerate(rows)]
    out.append(dict(id="sh_B3", n=20, d=3, stationary="matern32", form="product", N=5, P=3, seed=2730, B=3, Buse=2, inter=True))
    return out


CASES = _cases()
ALL = {c["id"]: c for c in CASES}


@functools.lru_cache(maxsize=None)
def problem(cid):  # (X, y, alpha, H, kappas, Xp, Z): _precision._problem with the noise fitted to KAPPA_MAX; points, background
    c = ALL[cid]
    X, y, alpha, H = P._problem(c["n"], c["d"], c["seed"], c["stationary"], c["form"], c["B"], False)
    rng = np.random.RandomState(c["seed"] + 7)
    Xp, Z = rng.uniform(size=(c["P"], c["d"])), rng.uniform(size=(c["N"], c["d"]))
    return (X, y, alpha) + P._fit_noise(X, alpha, H, c["stationary"], c["form"]) + (Xp, Z)


def reference_of(X, y, alpha, h, Xp, Z, stationary, form, warp=None):
    """Long double: dict of ``phi`` (P, d), ``base``, ``value`` (P,), ``inter`` (P, d, d) and the means' absolute-sum ``scale``."""
    from oracle import hp_oracle as HP
    if warp is not None:
        X, Xp, Z = (HP.warp_inputs(v, warp) for v in (X, Xp, Z))
    a = HP.lml(X, y, alpha, h, stationary, form)["alpha"]
    v, scale = [], 0.0
    for x in Xp:
        T = HP.gram(coalition_rows(x, Z, coalition_picks(len(x))), h, stationary, form, Y=X) * a[None, :]
        v.append(T.sum(axis=1).reshape(-1, len(Z)).sum(axis=1) / len(Z))
        scale = max(scale, float(np.abs(T).sum(axis=1).max()))
    v = np.stack(v)
    phi, inter = shapley_from_values(v, Xp.shape[1], True)
    return dict(phi=phi, base=v[0, 0], value=v[:, -1], inter=inter, scale=scale)


@functools.lru_cache(maxsize=None)
def reference(cid, b):
    X, y, alpha, H, _kap, Xp, Z = problem(cid)
    return reference_of(X, y, alpha, H[b], Xp, Z, ALL[cid]["stationary"], ALL[cid]["form"])


def replica64(X, a, h, Xp, Z, stationary, form):
    """The device's route in fp64 numpy: ``(phi, base, value, inter)``.  ``a``: the fp64 alpha."""
    (n, d), dl = X.shape, (X.shape[1] + 1) // 2
    cst, ell = float(np.exp(h[0])), np.exp(np.asarray(h[1:d + 1], dtype=np.float64))
    U = X / ell
    zz = ((Z / ell)[:, None, :] - U[None, :, :]) ** 2  # (N, n, d)

    def table(aa, ks):  # [m] = sum over ks, ascending, of (bit ? a_k : z_k), (2^len(ks), N, n)
        out = np.zeros((1 << len(ks),) + zz.shape[:2])
        for i, k in enumerate(ks):
            bit = ((np.arange(len(out)) >> i) & 1).astype(bool)
            out = out + np.where(bit[:, None, None], aa[None, None, :, k], zz[None, :, :, k])
        return out

    v = []
    for x in Xp:
        aa = (x / ell - U) ** 2
        TL = table(aa, range(dl))
        v.append(np.concatenate([(PD._kernel64(TL + th[None], cst, stationary, form) @ a).sum(axis=1) for th in table(aa, range(dl, d))]) / len(Z))
    v = np.stack(v)
    phi, inter = shapley_from_values(v, d, True)
    return phi, v[0, 0], v[:, -1], inter


def errs(got, ref, t, d):
    """Per quantity the worst error of ``got = (phi, base, value, inter | None)`` over its bound (a NaN is infinite); "sum": efficiency."""
    dmu, BOUND = t * ref["scale"], {"base": 1.0, "value": 1.0, "phi": 2.0, "inter": 4.0}
    named = dict(zip(("phi", "base", "value", "inter"), got))
    out = {k: float(np.nan_to_num(np.abs(P.f(np.asarray(named[k]) - ref[k])), nan=np.inf).max() / (BOUND[k] * dmu))
           for k in BOUND if named[k] is not None}
    gap = np.asarray(named["phi"]).sum(axis=-1) - (np.asarray(named["value"]) - named["base"])
    out["sum"] = float(np.nan_to_num(np.abs(gap), nan=np.inf).max() / ((2 * d + 2) * dmu))
    return out
