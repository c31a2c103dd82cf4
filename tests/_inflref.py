"""Case-deletion influence (``bgp_influence``): cases, reference and tolerances of the two influence tests.
Reference: for a checked observation i a REFIT without it (``hp_oracle.predict`` on the other n - 1 points, long double, latent),
minus the full fit at the same rows; no rank-1 identity; at n = 1 the deleted fit is the prior.  Checked i: all up to n = 65, else
0, 63, 64, 65, 127, 128, n - 1 and three seeded ones.
Tolerances: ``dmu`` / ``dvar`` are products with the explicit inverse, like the fantasy moments: tm = ``tol("fant_mean")`` on the
scale max_x sum_k |K*_xk a_k|, tv = ``tol("fant_var")`` on the latent prior variance (the scales of ``P.fantasy_errs``), kappa of the
full Gram matrix.  The sums carry them to first order, with v = var + s (tv too) and v_i = v + dvar:
    sum_dm2: sum_x 2 |dmu| tm          sum_cook: sum_x (2 |dmu| / v) tm + (dmu^2 / v^2) tv          max_abs: tm
    sum_kl:  sum_x (|dmu| / v_i) tm + 1/2 (|dvar - dmu^2| / v_i^2 + |dvar / v_i^2 - dvar / (v v_i) - dmu^2 / v_i^2|) tv
plus the sum's own rounding, m eps times the sum.  K_DMU: at n = 1 and 2 (kappa ~ 1, the class on its floor of 2e-15) the fp64
restatement of dmu -- three roundings where a fantasy mean has one -- reaches 0.25 ``tol("fant_mean")``, not the tenth the CPU test
asks; 3 is the smallest one-digit factor on tm with which it does on the whole list (reach 0.083 with it, dmu_focus at n = 2; below
0.01 from n = 63 on either way).  dvar needs none (0.045).  ``arg_max`` may differ from the reference's only within tm of its maximum.
The ``v <= 0`` rule: with kappa <= KAPPA_MAX the white level keeps the latent variance at a training point near 1e-4, so the noise-0
twin row below never reaches it; ``zero_variance_problem`` does (n = 1, K = 1 exactly: every operation of the build is exact)."""
import functools

import numpy as np

import _precision as P

K_DMU = 3.0
# n, m, d, family, B resident, B read, vector alpha, n_focus, a query row on a training point, observation noise 0
ROWS = [(1, 1, 1, ("rbf", "product"), 1, 1, False, 1, False, False),
        (2, 64, 17, ("matern12", "product"), 3, 3, True, 64, False, False),
        (63, 65, 32, ("matern32", "product"), 3, 1, False, 1, False, False),
        (64, 128, 1, ("matern52", "product"), 1, 1, False, 0, False, False),
        (65, 129, 17, ("rbf", "sum"), 3, 3, True, 1, True, False),
        (129, 257, 32, ("matern12", "sum"), 1, 1, False, 0, False, False),
        (257, 65, 1, ("matern32", "sum"), 3, 3, False, 1, False, False),
        (257, 257, 17, ("matern52", "sum"), 1, 1, True, 1, True, True),
        (129, 1, 32, ("matern52", "product"), 1, 1, True, 1, False, False)]
ALL = {"infl%d_n%d_m%d_d%d_%s_%s_B%d" % (j, r[0], r[1], r[2], *r[3], r[5]): dict(
    zip(("n", "m", "d", "family", "B", "Bq", "vec_alpha", "n_focus", "twin", "noise0"), r), seed=3400 + j) for j, r in enumerate(ROWS)}
CIDS = list(ALL)


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(X, y, alpha, H with kappa <= KAPPA_MAX, kappas, Xq, noise (B,))."""
    c = ALL[cid]
    X, y, alpha, H = P._problem(c["n"], c["d"], c["seed"], *c["family"], c["B"], c["vec_alpha"])
    H, kap = P._fit_noise(X, alpha, H, *c["family"])
    Xq = np.random.RandomState(c["seed"] + 1).uniform(size=(c["m"], c["d"]))
    if c["twin"]:
        Xq[c["m"] // 2] = X[c["n"] // 2]
    return X, y, alpha, H, kap, Xq, np.zeros(c["B"]) if c["noise0"] else 1e-3 + np.exp(H[:, -1])


def zero_variance_problem():
    """(X, y, alpha, H, Xq): one point, rbf / product with c = 1, no alpha, white level below an ulp: K = P = 1 and the latent
    variance at the point 1 - 1 * 1 * 1 = 0, all exactly.  Query row 0 is the point, row 1 is not."""
    return np.array([[0.5]]), np.array([0.7]), 0.0, np.array([[0.0, np.log(0.3), -80.0]]), np.array([[0.5], [0.9]])


@functools.lru_cache(maxsize=None)
def reference(cid, b):
    """Long double: (checked i, dmu, dvar (checked, m), v = var + s of the full fit (m,), the two error scales)."""
    from oracle import hp_oracle as HP

    c = ALL[cid]
    X, y, alpha, H, _kap, Xq, noise = problem(cid)
    (st, fm), n = c["family"], c["n"]
    av = np.broadcast_to(alpha, (n,))
    fit = lambda keep: HP.predict(X[keep], y[keep], av[keep], H[b], Xq, st, fm, noise_zero=True)  # noqa: E731
    full, pv = fit(slice(None)), HP.prior_var(H[b], c["d"], fm, noise=False)
    idx = list(range(n)) if n <= 65 else sorted(
        {0, 63, 64, 65, 127, 128, n - 1, *np.random.RandomState(c["seed"] + 2).choice(n, 3, False)})
    dmu, dvar = np.zeros((len(idx), c["m"]), dtype=HP.LD), np.zeros((len(idx), c["m"]), dtype=HP.LD)
    for k, i in enumerate(idx):
        r = {"mean": 0, "var": pv} if n == 1 else fit(np.arange(n) != i)
        dmu[k], dvar[k] = r["mean"] - full["mean"], r["var"] - full["var"]
    Ks = HP.gram(Xq, H[b], st, fm, Y=X)
    scale = float(np.max(np.abs(Ks) @ np.abs(HP.lml(X, y, av, H[b], st, fm)["alpha"])))
    return idx, dmu, dvar, full["var"] + HP.LD(noise[b]), scale, float(pv)


def errs_over_tol(cid, b, got, who):
    """{quantity: worst error / tolerance} of one posterior's outputs ``got`` (``influence_values``' dict, or one row of the device
    call's) against the reference; the ``arg_max`` rule is asserted here."""
    idx, dmu, dvar, v, scale, pv = reference(cid, b)
    c, kap = ALL[cid], problem(cid)[4][b]
    m, nf = c["m"], c["n_focus"]
    tm, tv = K_DMU * P.tol("fant_mean", kap, c["n"]) * scale, P.tol("fant_var", kap, c["n"]) * pv
    ok = v > 0
    v = np.where(ok, v, 1)
    vi, a, d2 = v + dvar, np.abs(dmu), dmu * dmu
    cook, kl = np.where(ok, d2 / v, 0), np.where(ok, (v / vi - 1 + np.log(vi / v) + d2 / vi) / 2, 0)
    s_cook = np.where(ok, 2 * a / v * tm + d2 / (v * v) * tv, 0)
    s_kl = np.where(ok, a / vi * tm + (np.abs(dvar - d2) + np.abs(dvar - dvar * vi / v - d2)) / (vi * vi) / 2 * tv, 0)
    out = {}
    if nf:
        out["dmu_focus"] = float(np.max(np.abs(P.f(got["dmu_focus"])[:, idx].T - P.f(dmu[:, :nf])))) / tm
        out["dvar_focus"] = float(np.max(np.abs(P.f(got["dvar_focus"])[:, idx].T - P.f(dvar[:, :nf])))) / tv
    for q, terms, sens in (("sum_dm2", d2, 2 * a * tm), ("sum_cook", cook, s_cook), ("sum_kl", kl, s_kl)):
        want = terms.sum(axis=1)
        out[q] = float(np.max(np.abs(P.f(got[q])[idx] - P.f(want)) / P.f(sens.sum(axis=1) + m * P.EPS * want)))
    out["max_abs"] = float(np.max(np.abs(P.f(got["max_abs"])[idx] - P.f(a.max(axis=1))))) / tm
    for k, i in enumerate(idx):
        assert P.f(a[k])[int(got["arg_max"][i])] >= P.f(a[k]).max() - tm, (cid, b, i)
    print("PRECISION influence %s %s b%d: " % (who, cid, b) + ", ".join("%s %.4f tol" % kv for kv in out.items()))
    return out
