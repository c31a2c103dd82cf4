"""The hyper-posterior mixture (``bgp_predict_mixture``, ``bgp_predict_mixture_warped``, ``bgp_mixture_values``; bgp_mix.hip, DESIGN.md
section 26): the cases shared by tests/test_cpu_mixture_reference.py and tests/test_gpu_mixture.py, the long-double reference, an fp64
numpy replica of the device's route and the derived tolerance.

For rows b with normalised moments ``mean_bi``, ``var_bi``: ``mu = y_std mean + y_mean``, ``sd = sqrt(var y_std^2)``; a row is used iff
its weight is positive and all its moments are finite; ``w^_b = w_b / W`` over the used rows.  ``mean = sum w^ mu``, ``within = sum w^
sd^2``, ``between = sum w^ (mu - mean)^2``; ``cdf = sum w^ Phi(z)``, ``sf = sum w^ Phi(-z)``, ``logpdf = log sum w^ phi(z) / sd`` at
``z = (t - mu) / sd``; ``q_p = inf {t : F(t) >= p}``.  A row with ``sd = 0`` is a step at ``mu``.

* ``reference``: long double throughout, ``Phi`` / ``phi`` from ``oracle.hp_oracle.normal_cdf_pdf`` (mpmath); the resident cases take
  their moments from ``hp_oracle.predict`` (``_precision.ref_predict_b``; the warped case from ``_warprows.ref_row``).
  ``ref_quantile`` bisects that CDF until the long-double bracket stops shrinking.
* ``replica64``: the device's route in fp64 numpy (scipy's ``erfc`` / ``ndtri``): sums over the used rows in ascending b, each tail
  from ``erfc(|z| / sqrt 2) / 2``, the max-shifted density sum, the bracket ``[min, max]`` of ``mu + z_p sd`` moved outwards where a
  sign is wrong, Newton steps aimed a little past the Newton point (further after each one that did not cross) with bisection as the safeguard, until the ends are adjacent doubles;
  the upper end is returned.  Its keyword arguments are the slips the CPU test shows to miss the tolerance.

Tolerance, per point.  A row's moments may be off by ``dmu_b = y_std t_mean mean_scale_b`` and ``dsd_bi = y_std tv_b / (2 sqrt(var_bi))``,
``t_mean = P.tol("mean", kappa_b, n)``, ``tv_b = P.tol("var", kappa_b, n) prior_var_b`` (the warped case: ``_warprows.row_tol`` with its
Beta-CDF budget); caller-supplied moments are exact inputs (both 0).  The evaluator's own rounding of ``mu`` and ``sd`` (a product and a
sum; two products and a root) is added to them: ``2 eps (|y_std mean| + |y_mean|)`` and ``2 eps sd``.  With those

    mean      sum w^ dmu_b + g sum w^ |mu_b|                                             g = (2 n_used + 4) eps: the weights'
    within    sum w^ (2 sd_b dsd_b + dsd_b^2) + g sum w^ sd_b^2                            normalisation and the ordered sum
    between   sum w^ (2 |mu_b - mean| (dmu_b + dmean) + (dmu_b + dmean)^2) + (g + 2 eps) between,  dmean = the mean's bound
    cdf, sf   sum w^ phi(z_b) / sd_b (dmu_b + |z_b| dsd_b) + E,   E = C_TAIL eps sum w^ tail_b (1 + z_b^2) + 2^-1022
    logpdf    sum w^ f_b (|z_b| dmu_b + |z_b^2 - 1| dsd_b) / sd_b / f + C_LOGPDF eps (1 + |logpdf| + sum w^ f_b (z_b^2 + |log sd_b|) / f)
    quantile  back-substitution: |F_ref(t^) - p| (p > 0.5: |S_ref(t^) - (1 - p)|) <= f_ref(t^) (max_b (dmu_b + |z_b| dsd_b) + eps |t^|) + E

``tail_b`` is the summed tail (a tail probability has relative condition ~ z^2), ``f_b = phi(z_b) / sd_b``, ``f = sum w^ f_b``.  The factor
in front of ``f_ref`` bounds the quantile's shift because that shift is a convex combination of the components' shifts; ``eps |t^|`` is the
width of the final bracket.  A column with an atom among its used rows has no back-substitution (F jumps there): its quantiles are
held EXACTLY where an atom carries them (``exact_quantiles``).  Candidates kept: every row's variance >= 100 tv_b, as in
``_precision.ref_acq``; on the resident cases none is left out (asserted by both tests).

``2^-1022`` is the smallest normal double: a tail below it (z = -38: 2.9e-316) is outside the range where fp64 has relative accuracy at
all, and libraries underflow there (cephes' erfc returns 0 once x^2 > 709.78, i.e. beyond z = 37.7).

C_TAIL and C_LOGPDF are the only constants.  Every other term above is a worst-case bound with constant 1 on a handful of roundings, so
the fp64 replica comes close to it by construction (one row: two roundings against a two-rounding bound; a quantile one double off its
root uses up to all of ``f eps |t^|``): the project's margin of 0.1 cannot be asked of those terms and is asked of the term a constant
governs -- each constant is the smallest value, rounded up to one significant digit, with ``error <= derived terms + 0.1 x its term`` for
the fp64 replica at every point of every case.  Measured on the CPU: C_TAIL needs 5.9 (sf, 64 identical rows at z = 6; cdf needs 0.1),
C_LOGPDF needs nothing at all (the derived terms cover the replica's logpdf everywhere) and is 1, one unit of its term.  The replica's
worst reach of the whole tolerance with them is printed by tests/test_cpu_mixture_reference.py and recorded in DESIGN.md section 26."""
import functools

import numpy as np

import _precision as P
import _warprows as WR

EPS = P.EPS
QMAX = 16
TINY = 2.0 ** -1022  # the smallest normal double: below it (Phi(-38) = 2.9e-316) fp64 has no relative accuracy and libraries underflow
C_TAIL = 6.0
C_LOGPDF = 1.0
Y_MEAN, Y_STD = P.ACQ_Y_MEAN, P.ACQ_Y_STD
PROBS1 = (0.5,)
PROBS3 = (0.05, 0.5, 0.95)
PROBS5 = (1e-6, 0.05, 0.5, 0.95, 1.0 - 1e-6)
PROBS16 = (1e-6, 1e-3, 0.01, 0.05, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9, 0.95, 0.99, 0.999, 1.0 - 1e-6, 0.5000001)
TAIL_Z = (8.0, -8.0, 30.0, -30.0, 38.0, -38.0)
T_OFF = np.array([-3.0, -1.0, 0.0, 0.5, 2.0, 6.0])


def _syn(cid, B, m, probs, seed, special=None):
    return dict(id=cid, kind="syn", B=B, m=m, probs=tuple(probs), seed=seed, special=special)


def _res(cid, pid, noise, Buse, warped=False):
    c = P.ALL[pid]
    return dict(id=cid, kind="warp" if warped else "res", pid=pid, noise=noise, B=Buse, Bres=c["B"], m=c.get("m", 40), n=c["n"],
                probs=PROBS3, special=None)


def _cases():
    out = [
        _syn("syn_B1_m513_Q5", 1, 513, PROBS5, 3000),
        _syn("syn_B2_m257_Q16", 2, 257, PROBS16, 3001),
        _syn("syn_B63_m1_Q16", 63, 1, PROBS16, 3002),
        _syn("syn_B2_m255_Q5_offset_weights", 2, 255, PROBS5, 3003, "offset"),   # unequal weights, |mu| ~ 1000 x the spread
        _syn("syn_B1_m256_Q1", 1, 256, PROBS1, 3004),
        _syn("syn_B129_m1_Q5", 129, 1, PROBS5, 3005),
        _syn("syn_B65_m1_Q5_zero_weights", 65, 1, PROBS5, 3006, "zeros"),        # unequal weights, every third one 0
        _syn("syn_B64_m1_Q5_identical", 64, 1, PROBS5, 3007, "identical"),       # ONE Gaussian: between == 0, q = mu + z_p sd
        _syn("syn_B64_m1_Q5_groups", 64, 1, PROBS5, 3008, "groups"),             # 32 + 32 rows 100 sd apart: p = 0.5 on the plateau
        _syn("syn_B65_m1_Q5_spread", 65, 1, PROBS5, 3009, "spread"),             # sd from 1e-6 to 1e3 within the point
        _syn("syn_B2_m1_Q5_atom", 2, 1, PROBS5, 3010, "atom"),                   # an atom of weight 0.6 carries the median
        _syn("syn_B2_m1_Q5_atoms", 2, 1, PROBS5, 3011, "atoms"),                 # every sd = 0: logpdf = -inf
        _syn("syn_B2_m255_Q1_tails", 2, 255, PROBS1, 3012, "tails"),             # t at z = +-8, +-30, +-38 of the nearer component
        _syn("syn_B2_m513_Q1_nanrow", 2, 513, PROBS1, 3013, "nanrow"),           # row 1 has ONE NaN: dropped everywhere
        _syn("syn_B2_m1_Q1_allbad", 2, 1, PROBS1, 3014, "allbad"),               # every row bad: NaN, n_used = 0
    ]
    for j in (0, 1, 3, 5, 6):
        pid = P.PREDB_CASES[j]["id"]
        for noise in (False, True):
            out.append(_res("res_%s_%s" % (pid, "noise" if noise else "latent"), pid, noise, P.PREDB_CASES[j]["B"]))
    pid = P.PREDB_CASES[3]["id"]
    out.append(_res("res_%s_latent_first4" % pid, pid, False, 4))  # fewer rows than are resident
    out.append(_res("res_%s_rowwarp" % P.WARP_CASES[0]["id"], P.WARP_CASES[0]["id"], True, P.WARP_CASES[0]["B"], warped=True))
    return out


CASES = _cases()
ALL = {c["id"]: c for c in CASES}


def register(cid, mean, var, weights, probs, t, y_mean=0.0, y_std=1.0):
    """An ad-hoc case on given fp64 moments (taken as exact inputs, like the synthetic ones), e.g. an estimator's own rows: it is
    looked up like a listed case but is not part of ``CASES``."""
    mean, var = P.f(np.atleast_2d(mean)), P.f(np.atleast_2d(var))
    ALL[cid] = dict(id=cid, kind="syn", B=mean.shape[0], m=mean.shape[1], probs=tuple(probs), seed=None, special=None,
                    y=(float(y_mean), float(y_std)),
                    given=dict(mean=mean, var=var, weights=None if weights is None else P.f(weights), t=P.f(t)))
    return cid


def y_of(cid):
    return ALL[cid].get("y", (Y_MEAN, Y_STD))
SYN = [c["id"] for c in CASES if c["kind"] == "syn"]
RES = [c["id"] for c in CASES if c["kind"] == "res"]
WARP = [c["id"] for c in CASES if c["kind"] == "warp"]


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """What the evaluator is given.  Synthetic: ``mean``, ``var`` (B, m; normalised), ``weights`` (B,) or None, ``t`` (m,).  Resident:
    ``weights`` and ``t`` only (the moments come from the posteriors of ``_precision.problem(pid)``); ``t`` sits T_OFF standard
    deviations of row 0 from its mean, cycling over the points."""
    c = ALL[cid]
    if "given" in c:
        return c["given"]
    B, m, sp = c["B"], c["m"], c["special"]
    if c["kind"] != "syn":
        r0 = _res_moments(cid)
        mu0, sd0 = Y_STD * P.f(r0[0][0]) + Y_MEAN, Y_STD * np.sqrt(P.f(r0[1][0]))
        w = None if c["B"] == 1 else np.random.RandomState(4000 + c["n"]).uniform(0.2, 1.0, size=B)
        return dict(weights=w, t=mu0 + T_OFF[np.arange(m) % len(T_OFF)] * sd0)
    rng = np.random.RandomState(c["seed"])
    mean = 2.0 * rng.randn(m)[None, :] + 0.5 * rng.randn(B, m)
    var = 10.0 ** rng.uniform(-3.0, 0.0, size=(B, m))
    w = None
    k = np.arange(m) % len(T_OFF)
    if sp == "offset":
        mean = 300.0 + 0.3 * rng.randn(B, m)
        w = np.array([0.3, 0.7])
    elif sp == "zeros":
        w = rng.uniform(0.1, 1.0, size=B)
        w[::3] = 0.0
    elif sp == "identical":
        mean, var = np.full((B, m), 0.75), np.full((B, m), 0.0421)  # (mu = 3.75: its multiples k / 64 are exact, so is the mean)
    elif sp == "groups":
        mean = np.where(np.arange(B)[:, None] < B // 2, -5.0, 5.0) + 0.0 * mean
        var = np.full((B, m), 0.01 / Y_STD**2)
    elif sp == "spread":
        var = (10.0 ** np.linspace(-6.0, 3.0, B)[:, None] / Y_STD) ** 2 + 0.0 * var
    elif sp == "atom":
        mean, var, w = np.array([[0.25], [2.0]]), np.array([[0.0], [0.04]]), np.array([0.6, 0.4])
    elif sp == "atoms":
        mean, var, w = np.array([[0.25], [-1.0]]), np.zeros((2, 1)), np.array([0.3, 0.7])
    elif sp == "nanrow":
        mean[1, 300] = np.nan
    elif sp == "allbad":
        mean[0, 0], var[1, 0] = np.nan, np.inf
    mu0, sd0 = Y_STD * mean[0] + Y_MEAN, Y_STD * np.sqrt(var[0])
    with np.errstate(invalid="ignore"):
        t = mu0 + T_OFF[k] * sd0
    if sp == "tails":
        var[1] = var[0]
        mean[1] = mean[0] + 0.5 * np.sqrt(var[0])  # (row 1 half a standard deviation above row 0: it is the nearer one from above)
        zt = np.array(TAIL_Z)[np.arange(m) % len(TAIL_Z)]
        t = np.where(zt > 0.0, Y_STD * mean[1] + Y_MEAN, mu0) + zt * sd0
    if sp == "atom":
        t = np.array([Y_STD * 0.25 + Y_MEAN])  # t ON the atom: the step counts (Phi = 1 where t >= mu)
    return dict(mean=mean, var=var, weights=w, t=t)


@functools.lru_cache(maxsize=None)
def _res_moments(cid):
    """Long-double normalised (mean, var) (B, m) of a resident case, its per-row moment tolerances ``(dmean_b, tv_b)`` in normalised
    units and the ``keep`` mask of ``_precision.ref_acq``."""
    c = ALL[cid]
    pid, B, n = c["pid"], c["B"], c["n"]
    if c["kind"] == "warp":
        rows = [WR.ref_row(pid, b) for b in range(B)]
        mean = np.array([r["ref"]["mean"] for r in rows])
        var = np.array([r["ref"]["var"] for r in rows])
        dmean = np.array([WR.row_tol(pid, b, "mean") * rows[b]["scale"]["mean"] for b in range(B)])
        tv = np.array([WR.row_tol(pid, b, "var") * rows[b]["scale"]["var"] for b in range(B)])
    else:
        nz = not c["noise"]
        kap = P.problem(pid)[4]
        mean = np.array([P.ref_predict_b(pid, b, nz)["mean"] for b in range(B)])
        var = np.array([P.ref_predict_b(pid, b, nz)["var"] for b in range(B)])
        dmean = np.array([P.tol("mean", kap[b], n) * P.mean_scale(pid, b) for b in range(B)])
        tv = np.array([P.tol("var", kap[b], n) * P.prior_var(pid, nz, b) for b in range(B)])
    keep = (P.f(var) >= 100.0 * tv[:, None]).all(axis=0)
    return mean, var, dmean, tv, keep


def h_kernel(cid):
    """The canonical vectors of a resident case as the device takes them: the white level stays (noise) or is -inf (latent)."""
    c = ALL[cid]
    H = P.problem(c["pid"])[3][: c["B"]].copy()
    if not c["noise"]:
        H[:, -1] = -np.inf
    return H


def _phi_ld(z):
    from oracle import hp_oracle as HP

    return HP.normal_cdf_pdf(z)


@functools.lru_cache(maxsize=None)
def model(cid):
    """The long-double mixture components of a case: ``mu``, ``sd`` (rows used only: (Bu, m)), ``wn`` (Bu,), ``n_used`` and the per-row
    perturbation bounds ``dmu`` (Bu, m), ``dsd`` (Bu, m) of the module docstring (fp64), ``keep`` (m,)."""
    from oracle import hp_oracle as HP

    LD = HP.LD
    c = ALL[cid]
    inp = inputs(cid)
    if c["kind"] == "syn":
        mean, var = inp["mean"].astype(LD), inp["var"].astype(LD)
        dmean, tv, keep = np.zeros(c["B"]), np.zeros(c["B"]), np.ones(c["m"], dtype=bool)
    else:
        mean, var, dmean, tv, keep = _res_moments(cid)
    w = np.ones(c["B"]) if inp["weights"] is None else inp["weights"]
    used = (w > 0.0) & np.isfinite(P.f(mean)).all(axis=1) & np.isfinite(P.f(var)).all(axis=1)
    if not used.any():
        return dict(n_used=0)
    mean, var, w, dmean, tv = mean[used], var[used], w[used].astype(LD), dmean[used], tv[used]
    y_mean, y_std = y_of(cid)
    ys, ym = LD(y_std), LD(y_mean)
    mu, sd = ys * mean + ym, np.sqrt(var * (ys * ys))
    wn = w / w.sum()
    v64 = P.f(var)
    with np.errstate(divide="ignore", invalid="ignore"):
        dsd = np.where(tv[:, None] > 0.0, y_std * tv[:, None] / (2.0 * np.sqrt(np.maximum(v64, 100.0 * tv[:, None]))), 0.0)
    dmu = y_std * dmean[:, None] + 2.0 * EPS * (np.abs(y_std * P.f(mean)) + abs(y_mean))
    dsd = dsd + 2.0 * EPS * P.f(sd)
    return dict(n_used=int(used.sum()), mu=mu, sd=sd, wn=wn, dmu=dmu, dsd=dsd, keep=keep)


def _tails(md, t, upper):
    """Long double, at t (m,): the summed tail (m,), per-component tails, phi(z) / sd and z (Bu, m); atoms are steps."""
    from oracle import hp_oracle as HP

    LD = HP.LD
    mu, sd, wn = md["mu"], md["sd"], md["wn"]
    pos = sd > 0
    z = np.zeros(mu.shape, dtype=LD)
    z[pos] = ((np.asarray(t, dtype=LD)[None, :] - mu) / np.where(pos, sd, LD(1)))[pos]
    Phi, phi = _phi_ld(-z if upper else z)
    tb = np.broadcast_to(np.asarray(t, dtype=LD)[None, :], mu.shape)
    step = (tb < mu) if upper else (tb >= mu)
    tail_b = np.where(pos, Phi, step.astype(LD))
    f_b = np.where(pos, phi / np.where(pos, sd, LD(1)), LD(0))
    return (wn[:, None] * tail_b).sum(axis=0), tail_b, f_b, z


@functools.lru_cache(maxsize=None)
def reference(cid):
    """{quantity: (value (m,) long double, tol (m,) fp64)} for mean, within, between, cdf, sf, logpdf, and ``n_used``, ``keep``."""
    from oracle import hp_oracle as HP

    LD = HP.LD
    md = model(cid)
    c = ALL[cid]
    if md["n_used"] == 0:
        nan = np.full(c["m"], np.nan)
        return dict(n_used=0, keep=np.ones(c["m"], dtype=bool), **{q: (nan, nan) for q in ("mean", "within", "between", "cdf", "sf", "logpdf")})
    mu, sd, wn, dmu, dsd = md["mu"], md["sd"], md["wn"], md["dmu"], md["dsd"]
    w64, mu64, sd64 = P.f(wn)[:, None], P.f(mu), P.f(sd)
    g = (2.0 * md["n_used"] + 4.0) * EPS
    mean = (wn[:, None] * mu).sum(axis=0)
    within = (wn[:, None] * sd * sd).sum(axis=0)
    dev = mu - mean[None, :]
    between = (wn[:, None] * dev * dev).sum(axis=0)
    t_mean = (w64 * dmu).sum(axis=0) + g * (w64 * np.abs(mu64)).sum(axis=0)
    t_within = (w64 * (2.0 * sd64 * dsd + dsd * dsd)).sum(axis=0) + g * P.f(within)
    dd = dmu + t_mean[None, :]
    t_between = (w64 * (2.0 * np.abs(P.f(dev)) * dd + dd * dd)).sum(axis=0) + (g + 2.0 * EPS) * P.f(between)
    t = inputs(cid)["t"]
    out = dict(n_used=md["n_used"], keep=md["keep"], mean=(mean, t_mean), within=(within, t_within), between=(between, t_between))
    F, Fb, fb, z = _tails(md, t, False)
    S, Sb, _fb, _z = _tails(md, t, True)
    z64, fb64 = P.f(z), P.f(fb)
    pos = sd64 > 0.0
    sdp = np.where(pos, sd64, 1.0)
    shift = (w64 * fb64 * (dmu + np.abs(z64) * dsd)).sum(axis=0)
    out["cdf"] = (F, shift + C_TAIL * EPS * (w64 * P.f(Fb) * (1.0 + z64 * z64)).sum(axis=0) + TINY)
    out["sf"] = (S, shift + C_TAIL * EPS * (w64 * P.f(Sb) * (1.0 + z64 * z64)).sum(axis=0) + TINY)
    f = (wn[:, None] * fb).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        logpdf = np.where(f > 0, np.log(np.where(f > 0, f, LD(1))), LD(-np.inf))
        rel = P.f(wn[:, None] * fb / np.where(f > 0, f, LD(1))[None, :])  # (each component's share of the density)
        t_log = ((rel * (np.abs(z64) * dmu + np.abs(z64 * z64 - 1.0) * dsd) / sdp).sum(axis=0)
                 + C_LOGPDF * EPS * (1.0 + np.abs(P.f(logpdf)) + (rel * (z64 * z64 + np.abs(np.log(sdp)))).sum(axis=0)))
    out["logpdf"] = (logpdf, np.where(f > 0, t_log, 0.0))  # (-inf is held exactly)
    return out


def ratios(cid, got):
    """{quantity: worst |got - reference| / tol over the kept points} for the moment / at-t quantities present in ``got``; an error of
    exactly 0 (also -inf against -inf, NaN against NaN) counts 0 whatever the tolerance."""
    ref = reference(cid)
    out = {}
    for q in ("mean", "within", "between", "cdf", "sf", "logpdf"):
        if q not in got:
            continue
        val, tol = ref[q]
        g, v = P.f(got[q]), val
        same = (g == P.f(v)) & ~np.isfinite(g) | (np.isnan(g) & np.isnan(P.f(v)))
        with np.errstate(invalid="ignore", divide="ignore"):
            err = np.where(same, 0.0, np.abs(P.f(g.astype(v.dtype) - v)))
            r = np.where(err == 0.0, 0.0, err / tol)
        r = np.where(np.isnan(r), np.inf, r)
        out[q] = float(r[ref["keep"]].max())
    return out


def has_atom(cid):
    md = model(cid)
    return md["n_used"] > 0 and bool((P.f(md["sd"]) == 0.0).any())


def quantile_ratio(cid, tq):
    """The back-substitution of an evaluator's quantiles ``tq`` (Q, m): worst residual / bound per probability (Q,).  Columns with an
    atom are left to ``exact_quantiles``."""
    from oracle import hp_oracle as HP

    LD = HP.LD
    c = ALL[cid]
    md = model(cid)
    tq = P.f(tq)
    if md["n_used"] == 0 or has_atom(cid):
        return np.zeros(len(c["probs"]))
    w64 = P.f(md["wn"])[:, None]
    out = []
    for k, p in enumerate(c["probs"]):
        up = p > 0.5
        target = LD(1) - LD(p) if up else LD(p)
        tail, tail_b, fb, z = _tails(md, tq[k], up)
        z64 = P.f(z)
        fref = P.f((md["wn"][:, None] * fb).sum(axis=0))
        E = C_TAIL * EPS * (w64 * P.f(tail_b) * (1.0 + z64 * z64)).sum(axis=0) + TINY
        bound = fref * ((md["dmu"] + np.abs(z64) * md["dsd"]).max(axis=0) + EPS * np.abs(tq[k])) + E
        res = np.abs(P.f(tail - target))
        with np.errstate(invalid="ignore", divide="ignore"):
            r = np.where(res == 0.0, 0.0, res / bound)
        r = np.where(np.isnan(r), np.inf, r)
        out.append(float(r[md["keep"]].max()))
    return np.array(out)


def exact_quantiles(cid):
    """Where atoms alone decide: {(k, i): value} -- the quantile p_k of point i is carried by an atom and must come back as exactly
    that ``mu`` in fp64 (the device's own ``y_std * mean + y_mean``, contraction off)."""
    c = ALL[cid]
    inp = inputs(cid)
    if c["special"] == "atom":
        mu = Y_STD * inp["mean"][0, 0] + Y_MEAN  # F jumps from ~0 to 0.6 there: every p in (1e-6, 0.6] is carried by the atom
        return {(k, 0): mu for k, p in enumerate(c["probs"]) if 1e-6 <= p <= 0.5}
    if c["special"] == "atoms":
        mus = Y_STD * inp["mean"][:, 0] + Y_MEAN  # weights 0.3 (at mus[0]) and 0.7 (at mus[1] < mus[0])
        return {(k, 0): (mus[1] if p <= 0.7 else mus[0]) for k, p in enumerate(c["probs"])}
    return {}


def ref_quantile(mu, sd, wn, p):
    """``inf {t : F(t) >= p}`` of ONE point by bisection on the long-double CDF (mpmath's Phi) until the bracket stops shrinking;
    ``mu``, ``sd``, ``wn`` (Bu,) long double, every sd > 0."""
    from oracle import hp_oracle as HP

    LD = HP.LD
    mu, sd, wn = (np.asarray(a, dtype=LD) for a in (mu, sd, wn))
    up = p > 0.5
    target = LD(1) - LD(p) if up else LD(p)

    def g(t):
        z = (t - mu) / sd
        Phi, _ = _phi_ld(-z if up else z)
        s = (wn * Phi).sum()
        return target - s if up else s - target

    lo, hi = (mu - 40 * sd).min(), (mu + 40 * sd).max()
    while True:
        mid = lo + (hi - lo) / 2
        if not (lo < mid < hi):
            return hi
        if g(mid) < 0:
            lo = mid
        else:
            hi = mid


# ------------------------------------------------------------------------------------------------------------------------------
# the device's route in fp64 numpy
# ------------------------------------------------------------------------------------------------------------------------------
SLIPS = ("fp32 moments", "1 - cdf", "naive between", "no renormalisation", "gaussian band", "plain logpdf")
ITMAX = 200


def replica64(mean, var, weights, y_mean, y_std, probs, t, slip=None):
    """dict(mean, within, between, cdf, sf, logpdf (m,), quantiles (Q, m), n_used, iters) the way bgp_mix.hip computes them, or with
    one of ``SLIPS``."""
    from scipy.special import erfc, ndtri

    mean, var = P.f(np.atleast_2d(mean)), P.f(np.atleast_2d(var))
    if slip == "fp32 moments":
        mean, var = P.to32(mean), P.to32(var)
    B, m = mean.shape
    w = np.ones(B) if weights is None else P.f(weights)
    good = np.isfinite(mean).all(axis=1) & np.isfinite(var).all(axis=1)
    used = (w > 0.0) & good
    rows = [b for b in range(B) if used[b]]
    Q = len(probs)
    nan = np.full(m, np.nan)
    if not rows:
        return dict(mean=nan, within=nan, between=nan, cdf=nan, sf=nan, logpdf=nan, quantiles=np.full((Q, m), np.nan), n_used=0, iters=0)
    W = 0.0
    for b in range(B):
        if used[b] or (slip == "no renormalisation" and w[b] > 0.0):
            W += w[b]
    wn = np.where(used, w / W, 0.0)
    with np.errstate(invalid="ignore"):
        mu, sd = y_std * mean + y_mean, np.sqrt(var * (y_std * y_std))
    mix = np.zeros(m)
    within, between = np.zeros(m), np.zeros(m)
    for b in rows:
        mix = mix + wn[b] * mu[b]
        within = within + wn[b] * (sd[b] * sd[b])
    for b in rows:
        between = between + wn[b] * ((mu[b] - mix) * (mu[b] - mix))
    if slip == "naive between":
        e2 = np.zeros(m)
        for b in rows:
            e2 = e2 + wn[b] * (mu[b] * mu[b])
        between = e2 - mix * mix
    r2, s2pi = 0.70710678118654752440, 2.5066282746310002

    def tail(tt, up):
        s, f = np.zeros(m), np.zeros(m)
        for b in rows:
            pos = sd[b] > 0.0
            with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
                z = (tt - mu[b]) / np.where(pos, sd[b], 1.0)
                e = 0.5 * erfc(np.abs(z) * r2)
                ph = np.where(z >= 0.0, e, 1.0 - e) if up else np.where(z <= 0.0, e, 1.0 - e)
                step = ((tt < mu[b]) if up else (tt >= mu[b])).astype(np.float64)
                s = s + wn[b] * np.where(pos, ph, step)
                f = f + np.where(pos, wn[b] * (np.exp(-(z * z) / 2.0) / (np.where(pos, sd[b], 1.0) * s2pi)), 0.0)
        return s, f

    t = P.f(t)
    cdf, _f = tail(t, False)
    sf, _f = tail(t, True)
    if slip == "1 - cdf":
        sf = 1.0 - cdf
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        A = np.full(m, -np.inf)
        for b in rows:
            pos = sd[b] > 0.0
            z = (t - mu[b]) / np.where(pos, sd[b], 1.0)
            A = np.where(pos, np.maximum(A, -(z * z) / 2.0 - np.log(np.where(pos, sd[b], 1.0))), A)
        acc, plain = np.zeros(m), np.zeros(m)
        for b in rows:
            pos = sd[b] > 0.0
            z = (t - mu[b]) / np.where(pos, sd[b], 1.0)
            a = -(z * z) / 2.0 - np.log(np.where(pos, sd[b], 1.0))
            acc = acc + np.where(pos, wn[b] * np.exp(a - np.where(np.isfinite(A), A, 0.0)), 0.0)
            plain = plain + np.where(pos, wn[b] * (np.exp(-(z * z) / 2.0) / (np.where(pos, sd[b], 1.0) * s2pi)), 0.0)
        logpdf = np.where(A > -np.inf, (A + np.log(acc)) - 0.91893853320467274178, -np.inf)
        if slip == "plain logpdf":
            logpdf = np.log(plain)
    quant, iters = np.empty((Q, m)), 0
    tiny = 2.2250738585072014e-308
    for k, p in enumerate(probs):
        up = p > 0.5
        target = 1.0 - p if up else p
        zp = -ndtri(target) if up else ndtri(p)
        if slip == "gaussian band":
            quant[k] = mix + ndtri(p) * np.sqrt(within + between)
            continue
        v = np.array([mu[b] + zp * sd[b] for b in rows])
        lo, hi, smax = v.min(axis=0), v.max(axis=0), np.array([sd[b] for b in rows]).max(axis=0)

        def G(tt):
            s, f = tail(tt, up)
            return (target - s if up else s - target), f

        glo, flo = G(lo)
        ghi, fhi = G(hi)
        step, ng = None, 0
        while (glo >= 0.0).any() and ng < 2200:
            mk = glo >= 0.0
            if step is None:
                step = np.maximum(np.maximum(smax, np.abs(lo)) * 2.0 ** -40, tiny)
            new = np.where(mk, lo - step, lo)
            gn, fn = G(new)
            hi, ghi, fhi = np.where(mk, lo, hi), np.where(mk, glo, ghi), np.where(mk, flo, fhi)
            lo, glo, flo = new, np.where(mk, gn, glo), np.where(mk, fn, flo)
            step, ng = np.where(mk, step * 2.0, step), ng + 1
        step = None
        while (ghi < 0.0).any() and ng < 4400:
            mk = ghi < 0.0
            if step is None:
                step = np.maximum(np.maximum(smax, np.abs(hi)) * 2.0 ** -40, tiny)
            new = np.where(mk, hi + step, hi)
            gn, fn = G(new)
            lo, glo, flo = np.where(mk, hi, lo), np.where(mk, ghi, glo), np.where(mk, fhi, flo)
            hi, ghi, fhi = new, np.where(mk, gn, ghi), np.where(mk, fn, fhi)
            step, ng = np.where(mk, step * 2.0, step), ng + 1
        w1, w2, boost = np.full(m, np.inf), np.full(m, np.inf), np.ones(m)
        for it in range(ITMAX):
            wd = hi - lo
            mid = lo + 0.5 * wd
            act = (mid > lo) & (mid < hi)
            if not act.any():
                break
            iters = max(iters, it + 1)
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                from_lo = -glo <= ghi
                tb, dirn = np.where(from_lo, lo, hi), np.where(from_lo, 1.0, -1.0)
                s = -np.where(from_lo, glo, ghi) / np.where(from_lo, flo, fhi)
                over = (np.abs(s) * 0.00390625 + 4.440892098500626e-16 * np.abs(tb)) * boost
                cnd = tb + (s + dirn * over)
            newton = act & ~(wd > 0.5 * w2) & (cnd > lo) & (cnd < hi)
            tn = np.where(newton, cnd, mid)
            w2, w1 = np.where(act, w1, w2), np.where(act, wd, w1)
            gt, ft = G(tn)
            neg, nonneg = act & (gt < 0.0), act & ~(gt < 0.0)
            boost = np.where(newton, np.where(from_lo == (gt < 0.0), boost * 4.0, 1.0), boost)
            lo, glo, flo = np.where(neg, tn, lo), np.where(neg, gt, glo), np.where(neg, ft, flo)
            hi, ghi, fhi = np.where(nonneg, tn, hi), np.where(nonneg, gt, ghi), np.where(nonneg, ft, fhi)
        quant[k] = hi
    return dict(mean=mix, within=within, between=between, cdf=cdf, sf=sf, logpdf=logpdf, quantiles=quant, n_used=len(rows),
                iters=iters)


def moments64(cid):
    """fp64 normalised (mean, var) (B, m) of a case for the replica: the synthetic inputs, or the fp64 oracle's predict of a resident
    case (``gp_oracle.predict``; the warped case: ``_warprows.moments64``)."""
    from oracle import gp_oracle as O

    c = ALL[cid]
    if c["kind"] == "syn":
        inp = inputs(cid)
        return inp["mean"], inp["var"]
    pid = c["pid"]
    pc = P.ALL[pid]
    if c["kind"] == "warp":
        rows = [WR.moments64(pid, b) for b in range(c["B"])]
        return np.array([r["mean"] for r in rows]), np.array([r["var"] for r in rows])
    X, y, alpha, H, _ = P.problem(pid)
    ad = np.broadcast_to(alpha, (len(X),))
    rows = [O.predict(X, y, ad, H[b], P.query(pid), pc["stationary"], pc["form"], noise_zero=not c["noise"]) for b in range(c["B"])]
    return np.array([r[0] for r in rows]), np.array([r[1] ** 2 for r in rows])
