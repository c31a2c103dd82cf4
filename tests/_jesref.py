"""Joint entropy search acquisition (``bgp_joint_entropy``, bgp_jes.hip): the cases shared by
tests/test_cpu_jes_reference.py and tests/test_gpu_jes.py, the long-double reference, an fp64 numpy replica of the device's route and
the derived tolerance.

For posterior b with its OWN optimum samples (a_r, f_r), r < R, a candidate x, ``nu_b`` = BASE_ALPHA + the row's white level and the
jitter ``tau`` (normalised-y units; latent moments mu, v of x and mu_r, v_r of a_r, ``c_r = cov_b(a_r, x)``, ``w_r = v_r + tau``):

    m_r = mu + c_r (f_r - mu_r) / w_r       v_s = max(v - c_r^2 / w_r, 0)       z_r = (f_r - m_r) / sqrt(v_s)
    v_t = clip(v_s F(z_r), 0, v_s)          F(z) = 1 - lam (lam - z),  lam = phi(z) / Phi(-z)
    g_r = max(1/2 [log(v + nu_b) - log(v_t + nu_b)], 0)                          gain_b(x) = (1 / R) sum_r g_r

``w_r <= 0``: the sample conditions nothing; ``v_s <= 0``: ``v_t = 0``.

* ``reference``: ``oracle.hp_oracle.posterior`` and ``predict(..., Xq=[A_b; Xc], noise_zero=True, return_cov=True, post=...)`` for the
  joint moments, the conditioning in long double, then per (candidate, sample) the hazard ``lam``, F, its derivative and the logs
  from mpmath (``_terms_mp``).  Nothing of the device's route and no K^-1.
* ``replica64``: fp64 numpy / LAPACK on an explicit inverse in the device's form -- R_b = k(A_b, X), P_b = R_b K^-1,
  cov = k(A_b, x) - P_b k(X, x), the variances as ``k_** - rowsum((K_* K^-1) o K_*)`` clipped at 0, the two quotients by w_r formed
  once per sample, F switched at 4 between erfcx and the continued fraction.  Its keyword arguments are the slips the CPU test shows
  to miss the tolerance.

Tolerance per (row, candidate), derived -- no new constant: the first-order propagation, with ANALYTIC partials taken at the
reference's own moments, of ``t_mean mean_scale`` on mu and mu_r and of ``t_var pv`` on v, v_r and c_r (``t_mean = P.tol("mean",
kappa_b, n)``, ``t_var = P.tol("var", kappa_b, n)``, ``mean_scale`` the ``mean`` metric's scale at that point, ``pv`` the prior
variance).  With ``G_m = dg/dm = sqrt(v_s) F'(z) / (2 (v_t + nu))``, ``G_s = dg/dv_s = -(F - z F'(z) / 2) / (2 (v_t + nu))``,
``F' = lam [1 - (lam - z)(2 lam - z)]``, ``dl = f_r - mu_r``:

    tol_r = t_mean (|G_m| scale_x + |G_m c / w| scale_r)
          + t_var pv (|1 / (2 (v + nu)) + G_s| + |G_m dl / w - 2 G_s c / w| + |G_s c^2 / w^2 - G_m c dl / w^2|)
          + v_s e_F(z) / (2 (v_t + nu))                                            tol = (1 / R) sum_r tol_r

The last term is the rounding of F itself: ``e_F(z) = 4 E_F_REL(z) F(z)``, ``E_F_REL`` the relative bound that
tests/test_cpu_jes_reference.py measures for the switched function against mpmath over z in [-40, 40] and up to 1e8, and 4 the margin
for the device's erfcx not being scipy's.  Where the reference's own ``v_s`` or ``w_r`` is <= 0, or the bound is not finite, the
entry is a RULE entry: what is asserted there is the rule -- ``v_t`` is exactly 0 where the evaluator's own ``v_s <= 0`` -- and the
invariants ``0 <= gain <= 1/2 log1p(v / nu)``.  Only designated special candidates may be rule entries; the tests count them."""
import functools
import math
import warnings

import numpy as np

import _precision as P

BASE_ALPHA = 1e-3  # the constructor alpha of the observation (the value tests/_precision.py's fantasy cases use)
TAU = 1e-6         # the jitter on the optimum observation (the acquisition's default)
NS = 5             # n_samples of the average (deliberately not the number of rows)
DMAX, RMAX, CHUNK = 32, 255, 128  # bgp_jes.hip: limits on d and R, the forced small candidate chunk
F_SWITCH, F_DEPTH = 4.0, 40       # bgp_jes.hip / acquisition.py: where F changes form, the continued fraction's last numerator


def E_F_REL(z):
    """Relative rounding bound of the switched fp64 F (measured by tests/test_cpu_jes_reference.py, which asserts it on its whole
    grid).  The definition ``1 - lam (lam - z)`` amplifies the rounding of erfcx by ``lam (2 lam - z) / F`` -- 16 at z = 1, growing
    as z^4 --: 16 eps (1 + max(z, 0)^4) covers the grid below the switch point (worst 0.75 of it, 1.15e-13 at z = 3.25); the continued
    fraction stays within 4 eps from the switch point up to z = 1e8 (worst 7.2e-16)."""
    z = np.asarray(z, dtype=np.float64)
    zp = np.minimum(np.maximum(z, 0.0), F_SWITCH)
    return np.where(z < F_SWITCH, 16.0 * P.EPS * (1.0 + zp ** 4), 4.0 * P.EPS)


def _case(cid, n, d, st, fm, R, m, seed, B=1, Buse=1, special=None):
    return dict(id=cid, n=n, d=d, stationary=st, form=fm, R=R, m=m, seed=seed, B=B, Buse=Buse, special=special)


def _cases():
    # the eight (family, form) pairs; n = 1 and on both sides of the 64-column GEMM tile and of the 128-pad; d = 1 .. 32 past the padded
    # widths 16 and 32; R = 1, 2, 5, either side of a 64-lane wave and the limit; m = 1, 255 / 256 / 257 (the gain kernel's
    # four-candidate workgroups, the 128-row tiles) and 300 = three chunks of the forced 128-candidate chunk.  The large R go with a
    # small m: the reference evaluates every (candidate, sample) pair in mpmath.
    rows = [
        (1, 1, "rbf", "product", 1, 1),
        (63, 8, "matern12", "product", 2, 255),
        (64, 17, "matern32", "product", 62, 9),
        (65, 32, "matern52", "product", 63, 5),
        (129, 1, "rbf", "sum", 64, 7),
        (257, 8, "matern12", "sum", 65, 6),
        (65, 3, "matern32", "sum", 255, 4),
        (63, 2, "matern52", "sum", 5, 257),
        (64, 2, "matern52", "product", 3, 300),
        (63, 3, "rbf", "product", 1, 256),
    ]
    out = [_case("jes%d_n%d_d%d_R%d_m%d_%s_%s" % (j, n, d, R, m, st, fm), n, d, st, fm, R, m, 2700 + j)
           for j, (n, d, st, fm, R, m) in enumerate(rows)]
    # three resident posteriors, two used, each with its OWN optimum set
    out.append(_case("jes_B3_n65_d3", 65, 3, "matern52", "product", 10, 40, 2730, B=3, Buse=2))
    # three posteriors, all used, over three candidate chunks of the forced 128: the forced posterior chunks of
    # tests/test_gpu_chunk_loops.py run with both loop indices of bgp_cond_run non-zero
    out.append(_case("jes_B3_n64_d2_R3_m300", 64, 2, "matern52", "product", 3, 300, 2760, B=3, Buse=3))
    # candidate 0 IS optimum point 0, candidate 1 IS training point 0, candidate 2 is 1e-8 from it, candidate 3 lies far outside the
    # data; optimum points 1 and 2 coincide; sample 5 has f_r = mu_r + 1e3 sqrt(v_r): z ~ 1e3
    out.append(_case("jes_special_n129_d3", 129, 3, "matern32", "product", 6, 8, 2740, special="points"))
    # a near-noise-free posterior (alpha 0, white level exp(-80)) of five points, nu = 1e-12, tau = 0: optimum point 0 IS training
    # point 0, so w_0 = v_0 ~ 0
    out.append(_case("jes_noisefree_n5_d2", 5, 2, "matern52", "product", 2, 4, 2750, special="noisefree"))
    return out


CASES = _cases()
ALL = {c["id"]: c for c in CASES}
SAME_OPT, TRAIN, TWIN, FAR = 0, 1, 2, 3  # candidates of the "points" case
BIG_Z = 5                                # its sample with z ~ 1e3


def t_values(cid, b):
    """The standardised optimum values of posterior b: ``f_r = mu_r + t_r sqrt(v_r)``, t spread over [-6, 6] in a shuffled order (both
    branches of F are reached); R = 1: -1."""
    c = ALL[cid]
    R = c["R"]
    t = np.linspace(-6.0, 6.0, R) if R > 1 else np.array([-1.0])
    t = np.random.RandomState(c["seed"] + 11 + b).permutation(t)
    if c["special"] == "points":
        t[BIG_Z] = 1e3
    return t


@functools.lru_cache(maxsize=None)
def _geometry(cid):
    c = ALL[cid]
    X, y, alpha, H = P._problem(c["n"], c["d"], c["seed"], c["stationary"], c["form"], c["B"], bool(c["seed"] % 2))
    rng = np.random.RandomState(c["seed"] + 7)
    Xc = rng.uniform(-0.1, 1.1, size=(c["m"], c["d"]))
    A = rng.uniform(-0.1, 1.1, size=(c["B"], c["R"], c["d"]))
    tau = TAU
    if c["special"] == "points":
        A[0, 2] = A[0, 1]
        Xc[SAME_OPT] = A[0, 0]
        Xc[TRAIN] = X[0]
        Xc[TWIN] = X[0] + 1e-8
        Xc[FAR] = 50.0
    if c["special"] == "noisefree":
        alpha = 0.0
        H[:, -1] = -80.0
        A[0, 0] = X[0]
        tau = 0.0
    H, kap = P._fit_noise(X, alpha, H, c["stationary"], c["form"])
    noise = np.full(c["B"], 1e-12) if c["special"] == "noisefree" else BASE_ALPHA + np.exp(H[:, -1])
    return X, y, alpha, H, kap, Xc, A, noise, tau


@functools.lru_cache(maxsize=None)
def _post(cid, b):
    from oracle import hp_oracle as HP

    c = ALL[cid]
    X, y, alpha, H = _geometry(cid)[:4]
    return HP.posterior(X, y, alpha, H[b], c["stationary"], c["form"])


@functools.lru_cache(maxsize=None)
def _moments(cid, b):
    """Long-double latent joint moments of [A_b; Xc] under posterior b, and the mean metric's scale at those points."""
    from oracle import hp_oracle as HP

    c = ALL[cid]
    X, y, alpha, H, _kap, Xc, A = _geometry(cid)[:7]
    post = _post(cid, b)
    Q = np.vstack([A[b], Xc])
    pr = HP.predict(X, y, alpha, H[b], Q, c["stationary"], c["form"], noise_zero=True, return_cov=True, post=post)
    Ks = HP.gram(Q, H[b], c["stationary"], c["form"], Y=X)
    sc = P.f(np.abs(Ks * post["alpha"][None, :]).sum(axis=1))
    return pr["mean"], pr["cov"], sc


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(X, y, alpha, H, kappas, Xc, A (B, R, d), f (B, R), noise (B,), tau): the training set and canonical vectors of
    ``_precision._problem`` with the noise fitted to KAPPA_MAX, the candidates and every posterior's own optimum points (a little
    outside the unit box too), the optimum values ``f_r = mu_r + t_r sqrt(v_r)`` (fp64, from the reference's moments) and the
    observation noise per row."""
    c = ALL[cid]
    X, y, alpha, H, kap, Xc, A, noise, tau = _geometry(cid)
    R = c["R"]
    f = np.zeros((c["B"], R))
    for b in range(c["B"]):
        mean, cov, _sc = _moments(cid, b)
        vr = np.maximum(P.f(np.diagonal(cov)[:R]), 0.0)
        f[b] = P.f(mean[:R]) + t_values(cid, b) * np.sqrt(vr)
    return X, y, alpha, H, kap, Xc, A, f, noise, tau


def _mp(x):
    import mpmath

    return mpmath.mpf(np.format_float_scientific(x, precision=24, unique=False))


def F_mp(z, dps=None):
    """(F, F', lam) of the lower-truncated normal at z as mpmath numbers, by the DEFINITION at enough digits for its cancellation
    (z^4 at large z: 50 + 4 log10 z digits and a guard)."""
    import mpmath

    z = mpmath.mpf(z)
    if dps is None:
        dps = 50 + (int(4 * math.log10(float(abs(z)))) + 20 if abs(z) > 10 else 0)
    with mpmath.workdps(dps):
        lam = mpmath.npdf(z) / mpmath.ncdf(-z)
        F = 1 - lam * (lam - z)
        Fp = lam * (1 - (lam - z) * (2 * lam - z))
        return +F, +Fp, +lam


def _terms_mp(v, nu, vs, z):
    """Per (candidate, sample), from long-double ``v``, ``nu``, ``v_s`` > 0 and ``z``: g, v_t, F and F' through mpmath (hazard, logs)."""
    import mpmath
    from oracle import hp_oracle as HP

    F, Fp, _lam = F_mp(_mp(z))
    with mpmath.workdps(50), np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # (F' below the long double's range rounds to 0)
        vsm, vm, num = _mp(vs), _mp(v), _mp(nu)
        vt = min(max(vsm * F, mpmath.mpf(0)), vsm)
        g = max((mpmath.log(vm + num) - mpmath.log(vt + num)) / 2, mpmath.mpf(0))
        return HP._mp_to_ld(g), HP._mp_to_ld(vt), HP._mp_to_ld(F), HP._mp_to_ld(Fp)


@functools.lru_cache(maxsize=None)
def reference(cid, b=0):
    """Long double: ``gain`` (m,), per (candidate, sample) ``g``, ``vs``, ``vt``, ``z`` (m, R), the candidates' ``mu``, ``v`` (m,), the
    bound ``cap = 1/2 log1p(v / nu)`` and in fp64 the tolerance ``tol`` (m,; inf at a rule entry) of the module docstring; ``rule`` (m,)
    marks the rule entries."""
    from oracle import hp_oracle as HP

    LD = HP.LD
    c = ALL[cid]
    X, y, alpha, H, kap, Xc, A, f, noise, tau = problem(cid)
    R, m, n, d = c["R"], c["m"], c["n"], c["d"]
    mean, cov, sc = _moments(cid, b)
    mur, vr, mu, v = mean[:R], np.diagonal(cov)[:R], mean[R:], np.diagonal(cov)[R:]
    C = cov[:R, R:].T  # (m, R): cov(a_r, x_i)
    fr = f[b].astype(LD)
    nu = LD(noise[b])
    w = vr + LD(tau)
    on = w > 0
    ws = np.where(on, w, LD(1))
    dl = fr - mur
    mr = mu[:, None] + np.where(on[None, :], C * (dl / ws)[None, :], LD(0))
    vs_raw = v[:, None] - np.where(on[None, :], C * C / ws[None, :], LD(0))
    vs = np.maximum(vs_raw, LD(0))
    pos = vs > 0
    z = (fr[None, :] - mr) / np.sqrt(np.where(pos, vs, LD(1)))
    g, vt = np.zeros((m, R), dtype=LD), np.zeros((m, R), dtype=LD)
    Fv, Fp = np.zeros((m, R), dtype=LD), np.zeros((m, R), dtype=LD)
    for i in range(m):
        for r in range(R):
            if pos[i, r]:
                g[i, r], vt[i, r], Fv[i, r], Fp[i, r] = _terms_mp(v[i], nu, vs[i, r], z[i, r])
            else:
                g[i, r] = np.maximum(np.log1p(v[i] / nu) / 2, LD(0))
    gain = g.sum(axis=1) / LD(R)
    # the tolerance: analytic partials at the reference's own moments, in fp64
    pv = float(HP.prior_var(H[b], d, c["form"], noise=False))
    t_mean, t_var = P.tol("mean", kap[b], n), P.tol("var", kap[b], n)
    tol = tol_from(P.f(v), float(nu), P.f(vs), P.f(vt), P.f(z), P.f(Fv), P.f(Fp), P.f(C), P.f(ws), P.f(dl), on, pos, sc[R:], sc[:R], pv,
                   t_mean, t_var)
    rule = ~np.isfinite(tol)
    cap = np.log1p(v / nu) / 2
    return {"gain": gain, "g": g, "vs": vs, "vt": vt, "z": z, "mu": mu, "v": v, "mur": mur, "vr": vr, "cov": C, "cap": cap,
            "tol": np.where(rule, np.inf, tol), "rule": rule}


def F64(z, form="switched"):
    """fp64 F in the device's two forms (scipy's erfcx): ``form`` "direct", "cf" or "switched" (at F_SWITCH)."""
    from scipy.special import erfcx

    z = np.asarray(z, dtype=np.float64)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        if form != "cf":
            zd = z if form == "direct" else np.where(z < F_SWITCH, z, 0.0)
            lam = 0.79788456080286535588 / erfcx(zd * 0.70710678118654752440)
            direct = 1.0 - lam * (lam - zd)
            if form == "direct":
                return direct
        zc = z if form == "cf" else np.where(z < F_SWITCH, F_SWITCH, z)
        rz = 1.0 / zc
        N, D = np.zeros_like(zc), np.ones_like(zc)
        for k in range(F_DEPTH, 1, -1):
            N, D = (k * rz) * D, D + rz * N
        U = N / D
        T = 1.0 / (zc + U)
        cf = T * (U - T)
    return cf if form == "cf" else np.where(z < F_SWITCH, direct, cf)


def tol_from(v, nu, vs, vt, z, F, Fp, C, w, dl, on, pos, scale_x, scale_r, pv, t_mean, t_var):
    """The tolerance of the module docstring per candidate (m,), in fp64, from the moments of ONE posterior: ``v`` (m,), ``vs``, ``vt``,
    ``z``, ``F``, ``Fp``, ``C`` (m, R), ``w``, ``dl`` (R,), ``on`` = w > 0 (R,), ``pos`` = v_s > 0 (m, R), the mean metric's scales at the
    candidates (m,) and at the optimum points (R,).  inf where a sample of the candidate has ``v_s <= 0`` or ``w <= 0``."""
    v, w, dl, onf = v[:, None], w[None, :], dl[None, :], on[None, :].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Gm = np.sqrt(vs) * Fp / (2.0 * (vt + nu))
        Gs = -(F - z * Fp / 2.0) / (2.0 * (vt + nu))
        t = (t_mean * (np.abs(Gm) * scale_x[:, None] + onf * np.abs(Gm * C / w) * scale_r[None, :])
             + t_var * pv * (np.abs(1.0 / (2.0 * (v + nu)) + Gs) + onf * np.abs(Gm * dl / w - 2.0 * Gs * C / w)
                             + onf * np.abs(Gs * C * C / (w * w) - Gm * C * dl / (w * w)))
             + vs * 4.0 * E_F_REL(z) * F / (2.0 * (vt + nu)))
        t = np.where(pos & on[None, :], t, np.inf)
        return t.sum(axis=1) / t.shape[1]


def tolerance64(mu, v, mur, vr, C, f, nu, tau, scale_x, scale_r, pv, t_mean, t_var):
    """``tol_from`` on fp64 moments alone (the Python-layer tests, where no long-double reference of a fitted model exists): the
    conditioning in fp64, F by ``F64`` and ``F' = lam (F - (lam - z)^2)`` with ``lam - z`` from the form F takes at that z."""
    from scipy.special import erfcx

    w = vr + tau
    on = w > 0.0
    ws = np.where(on, w, 1.0)
    dl = f - mur
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        mr = mu[:, None] + np.where(on[None, :], C * (dl / ws)[None, :], 0.0)
        vs = np.maximum(v[:, None] - np.where(on[None, :], C * C / ws[None, :], 0.0), 0.0)
        pos = vs > 0.0
        z = (f[None, :] - mr) / np.sqrt(np.where(pos, vs, 1.0))
        F = F64(z)
        zl = np.where(z < F_SWITCH, z, 0.0)
        T_direct = 0.79788456080286535588 / erfcx(zl * 0.70710678118654752440) - zl
        zc = np.where(z < F_SWITCH, F_SWITCH, z)
        T_cf = 0.5 * (np.sqrt(zc * zc + 4.0 * (1.0 - F64(zc) )) - zc)  # T (z + T) = 1 - F
        T = np.where(z < F_SWITCH, T_direct, T_cf)
        Fp = (z + T) * (F - T * T)
        vt = np.where(pos, np.clip(vs * F, 0.0, vs), 0.0)
    return tol_from(v, nu, vs, vt, z, F, Fp, C, ws, dl, on, pos, scale_x, scale_r, pv, t_mean, t_var)


def replica64(X, y, alpha, H, Xc, A, f, noise, tau, b, stationary, form, wrong_side=False, no_condition=False, no_truncation=False,
              shared_set=False, white_on=False):
    """``{gain (m,), vs, vt (m, R), v (m,)}`` of posterior b in fp64 numpy / LAPACK on an explicit inverse, in the device's form (module
    docstring).  The slips: ``wrong_side`` truncates f(x) <= f_r, ``no_condition`` drops the conditioning, ``no_truncation`` the
    truncation, ``shared_set`` uses the optimum set of posterior 0 for every posterior, ``white_on`` leaves the white level in the
    variances and in k(a, x) at a == x."""
    from oracle import gp_oracle as O
    from scipy.linalg import cho_solve, cholesky

    X, Xc = np.atleast_2d(np.asarray(X, dtype=np.float64)), np.atleast_2d(np.asarray(Xc, dtype=np.float64))
    n, d = X.shape
    h = H[b]
    Ab, fb = (A[0], f[0]) if shared_set else (A[b], f[b])
    Ab = np.asarray(Ab, dtype=np.float64).reshape(-1, d)
    K = O.gram_with_jitter(X, np.broadcast_to(alpha, (n,)), h, stationary, form)
    L = cholesky(K, lower=True, check_finite=False)
    a = cho_solve((L, True), y, check_finite=False)
    Ki = cho_solve((L, True), np.eye(n), check_finite=False)
    Ki = 0.5 * (Ki + Ki.T)
    hk = np.array(h, dtype=np.float64)
    white = 0.0 if not white_on else float(np.exp(hk[-1]))
    hk[-1] = -np.inf
    prior = float(O.kernel_diag(1, hk, d, form)[0]) + white
    Ks = O.kernel_matrix(Xc, hk, stationary, form, Y=X)
    mu = Ks @ a
    v = np.maximum(prior - np.einsum("ij,ij->i", Ks @ Ki, Ks), 0.0)
    Rm = O.kernel_matrix(Ab, hk, stationary, form, Y=X)
    mur = Rm @ a
    Pm = Rm @ Ki
    vr = np.maximum(prior - np.einsum("ij,ij->i", Pm, Rm), 0.0)
    kAx = O.kernel_matrix(Xc, hk, stationary, form, Y=Ab)
    if white_on:
        kAx = kAx + white * (Xc[:, None, :] == Ab[None, :, :]).all(axis=2)
    C = kAx - Ks @ Pm.T
    nu = float(noise[b])
    w = vr + tau
    on = (w > 0.0) & (not no_condition)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rw = np.where(on, 1.0 / np.where(on, w, 1.0), 0.0)
        sdl = np.where(on, (fb - mur) / np.where(on, w, 1.0), 0.0)
        mr = mu[:, None] + C * sdl[None, :]
        vs = np.maximum(v[:, None] - (C * C) * rw[None, :], 0.0)
        pos = vs > 0.0
        z = (fb[None, :] - mr) / np.sqrt(np.where(pos, vs, 1.0))
        Fz = np.ones_like(z) if no_truncation else F64(-z if wrong_side else z)
        vt = np.where(pos, np.clip(vs * Fz, 0.0, vs), 0.0)
        g = np.maximum(0.5 * (np.log(v[:, None] + nu) - np.log(vt + nu)), 0.0)
    return {"gain": g.sum(axis=1) / g.shape[1], "vs": vs, "vt": vt, "v": v}


def ratio(got, ref):
    """Worst ``|got - reference| / tol`` over the candidates (a rule entry counts 0, a finite tolerance that is 0 is met by an error
    of exactly 0 alone)."""
    err = np.abs(P.f(got) - P.f(ref["gain"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / ref["tol"])
    return float(r.max())


def designated(cid):
    """The candidates that may be rule entries: the candidate that IS an optimum point (tau > 0 keeps even that one regular), the
    training point and its twin of the "points" case; every candidate of the near-noise-free case, whose sample 0 sits on a training
    point with tau = 0 (w_0 = v_0 is the reference's own rounding of 0, for every candidate)."""
    sp = ALL[cid]["special"]
    m = ALL[cid]["m"]
    return set(range(m)) if sp == "noisefree" else {SAME_OPT, TRAIN, TWIN} if sp == "points" else set()
