"""Knowledge-gradient acquisition (``bgp_knowledge_gradient``, bgp_kg.hip): the cases shared by
tests/test_cpu_kg_reference.py and tests/test_gpu_kg.py, the long-double reference and an fp64 numpy replica of the device's route.

For posterior b, reference points A (M, d), a candidate x and ``s = var_b(x) + noise_b`` (latent variance; ``noise_b`` = BASE_ALPHA +
the row's white level, as ``bgp_fantasy_begin`` takes it) the M + 1 lines are ``p_j = mu_b(a_j), q_j = cov_b(a_j, x) / sqrt(s)`` and
``p_M = mu_b(x), q_M = var_b(x) / sqrt(s)``; ``KG_b(x) = min_j p_j - E[min_j (p_j + q_j Z)]``, 0 where ``s <= 0``; normalised-y units.

* ``reference``: ``oracle.hp_oracle.posterior`` and ``predict(..., Xq=[A; Xc], noise_zero=True, return_cov=True, post=...)`` for the
  joint moments, the lines and the sorted-breakpoint envelope in long double, Phi / phi from ``hp_oracle.normal_cdf_pdf`` (mpmath).
  Nothing of the device's route and no K^-1.
* ``replica64``: fp64 numpy / LAPACK on an explicit inverse in the device's form -- R = k(A, X), P = R K^-1, cov = k(A, x) - P k(X, x),
  the variance as ``k_** - rowsum((K_* K^-1) o K_*)`` clipped at 0, the envelope by pairwise interval clipping, the interval terms
  ``(p_j - p*) (Phi(hi) - Phi(lo)) + q_j (phi(lo) - phi(hi))`` with erfc / exp.  Its keyword arguments are the slips the CPU test
  shows to miss the tolerance.

Tolerance per (row, candidate), derived -- no new constant.  ``h(p, q) = E[min_j (p_j + q_j Z)]`` is 1-Lipschitz in max |dp| and
sqrt(2 / pi)-Lipschitz in max |dq|; min p is 1-Lipschitz in max |dp|; with every mean within ``t_mean mean_scale`` and every latent
(co)variance within ``t_var pv`` (``pv`` the prior variance), ``q = c / sqrt(s)`` moves by at most ``t_var pv / sqrt(s) + |q| t_var pv
/ (2 s)`` at first order:

    tol_i = 2 t_mean mean_scale + sqrt(2 / pi) max_j (t_var pv / sqrt(s) + |q_j| t_var pv / (2 s))

``t_mean = P.tol("mean", kappa_b, n)``, ``t_var = P.tol("var", kappa_b, n)``, ``mean_scale`` the ``mean`` metric's scale over [A; x].
The bound grows without limit as s -> 0; where the reference's s is <= 0 (a noise-free posterior at a training point with noise 0:
the true s is 0 and its sign is the reference's own rounding) it is infinite, and what is asserted there is the rule itself: the
value is exactly 0 wherever the evaluator's OWN s is <= 0.

The rounding of Phi / phi themselves (erfc and exp of fp64: a few ulp of values <= 1, times |p_j - p*| and |q_j|) is far inside that
bound on every case: the replica's worst reach is printed by the CPU test (``PRECISION`` lines), no additive term was needed."""
import functools
import math

import numpy as np

import _precision as P

BASE_ALPHA = 1e-3  # the constructor alpha of the fantasy observation (the value tests/_precision.py's fantasy cases use)
Y_STD = 3.0        # the device returns y_std times the normalised value
LMAX, DMAX, MMAX, CHUNK = 256, 32, 255, 128  # bgp_kg.hip: lines per candidate, limits on d and M, the forced small candidate chunk
SQ2PI = math.sqrt(2.0 / math.pi)


def _case(cid, n, d, st, fm, M, m, seed, B=1, Buse=1, special=None):
    return dict(id=cid, n=n, d=d, stationary=st, form=fm, M=M, m=m, seed=seed, B=B, Buse=Buse, special=special)


def _cases():
    # the eight (family, form) pairs; n = 1 and on both sides of the 64-column GEMM tile and of the 128-pad; d = 1, 8 and past the
    # padded widths 16 and 32; M = 0, one line, either side of a 64-lane wave (62 .. 65 reference points + the candidate's own line)
    # and the limit; m = 1, 255 / 256 / 257 (the envelope kernel's four-candidate workgroups, the 128-row tiles) and 300 = three
    # chunks of the forced 128-candidate chunk
    rows = [
        (1, 1, "rbf", "product", 0, 1),
        (63, 8, "matern12", "product", 1, 255),
        (64, 17, "matern32", "product", 62, 9),
        (65, 32, "matern52", "product", 63, 5),
        (129, 1, "rbf", "sum", 64, 256),
        (257, 8, "matern12", "sum", 65, 7),
        (65, 3, "matern32", "sum", 255, 6),
        (63, 2, "matern52", "sum", 5, 257),
        (64, 2, "matern52", "product", 3, 300),
    ]
    out = [_case("kg%d_n%d_d%d_M%d_m%d_%s_%s" % (j, n, d, M, m, st, fm), n, d, st, fm, M, m, 2500 + j)
           for j, (n, d, st, fm, M, m) in enumerate(rows)]
    out.append(_case("kg_B3_n65_d3", 65, 3, "matern52", "product", 10, 40, 2530, B=3, Buse=2))
    # three posteriors, all used, over three candidate chunks of the forced 128: the forced posterior chunks of
    # tests/test_gpu_chunk_loops.py run with both loop indices of bgp_cond_run non-zero
    out.append(_case("kg_B3_n64_d2_M3_m300", 64, 2, "matern52", "product", 3, 300, 2560, B=3, Buse=3))
    # candidate 0 IS reference point 0, candidate 1 IS training point 0, candidate 2 is 1e-8 from it, candidate 3 lies far outside
    # the data; reference points 1 and 2 coincide
    out.append(_case("kg_special_n129_d3", 129, 3, "matern32", "product", 6, 8, 2540, special="points"))
    # a noise-free posterior (alpha 0, white level exp(-80)) of five points, noise 0: candidate 0 IS training point 0
    out.append(_case("kg_noisefree_n5_d2", 5, 2, "matern52", "product", 2, 4, 2550, special="noisefree"))
    return out


CASES = _cases()
ALL = {c["id"]: c for c in CASES}
SAME_REF, TRAIN, TWIN, FAR = 0, 1, 2, 3  # candidates of the "points" case


@functools.lru_cache(maxsize=None)
def problem(cid):
    """(X, y, alpha, H, kappas, Xc, A, noise): the training set and canonical vectors of ``_precision._problem`` with the noise
    fitted to KAPPA_MAX, the candidates and the reference points (a little outside the unit box too) and the fantasy noise per row."""
    c = ALL[cid]
    X, y, alpha, H = P._problem(c["n"], c["d"], c["seed"], c["stationary"], c["form"], c["B"], bool(c["seed"] % 2))
    rng = np.random.RandomState(c["seed"] + 7)
    Xc = rng.uniform(-0.1, 1.1, size=(c["m"], c["d"]))
    A = rng.uniform(-0.1, 1.1, size=(c["M"], c["d"]))
    if c["special"] == "points":
        A[2] = A[1]
        Xc[SAME_REF] = A[0]
        Xc[TRAIN] = X[0]
        Xc[TWIN] = X[0] + 1e-8
        Xc[FAR] = 50.0
    if c["special"] == "noisefree":
        alpha = 0.0
        H[:, -1] = -80.0
        Xc[0] = X[0]
    H, kap = P._fit_noise(X, alpha, H, c["stationary"], c["form"])
    noise = np.zeros(c["B"]) if c["special"] == "noisefree" else BASE_ALPHA + np.exp(H[:, -1])
    return X, y, alpha, H, kap, Xc, A, noise


@functools.lru_cache(maxsize=None)
def _post(cid, b):
    from oracle import hp_oracle as HP

    c = ALL[cid]
    X, y, alpha, H = problem(cid)[:4]
    return HP.posterior(X, y, alpha, H[b], c["stationary"], c["form"])


def envelope_ld(p, q):
    """min p - E[min_j (p_j + q_j Z)] of ONE set of lines in long double: the sorted-breakpoint form.  Lines by descending slope of
    the minimum (ascending -q; equal slopes: the lower intercept, then the lower index), the lower envelope by a stack, then
    ``sum_k (b_(k+1) - b_(k)) f(-|c_k|)`` over the envelope's breakpoints with ``b = -q``, ``f(z) = z Phi(z) + phi(z)``."""
    from oracle import hp_oracle as HP

    a, b = -np.asarray(p, dtype=HP.LD), -np.asarray(q, dtype=HP.LD)
    order = sorted(range(len(a)), key=lambda j: (b[j], -a[j], j))
    keep = [j for k, j in enumerate(order) if k == 0 or b[j] != b[order[k - 1]]]
    stack, cs = [keep[0]], [-np.inf]
    for j in keep[1:]:
        while True:
            t = stack[-1]
            z = (a[t] - a[j]) / (b[j] - b[t])
            if z <= cs[-1]:
                stack.pop()
                cs.pop()
                continue
            stack.append(j)
            cs.append(z)
            break
    if len(stack) == 1:
        return HP.LD(0)
    c = np.array(cs[1:], dtype=HP.LD)
    z = -np.abs(c)
    Phi, phi = HP.normal_cdf_pdf(z)
    db = np.array([b[stack[k + 1]] - b[stack[k]] for k in range(len(stack) - 1)], dtype=HP.LD)
    return (db * (z * Phi + phi)).sum()


@functools.lru_cache(maxsize=None)
def reference(cid, b=0):
    """Long double: ``kg`` (m,; 0 where s <= 0), the lines ``p``, ``q`` (m, M + 1; q is 0 where s <= 0), ``s`` (m,), and in fp64 the
    tolerance ``tol`` (m,; inf where s <= 0) of the module docstring -- all in normalised-y units."""
    from oracle import hp_oracle as HP

    c = ALL[cid]
    X, y, alpha, H, kap, Xc, A, noise = problem(cid)
    M, m, n, d = c["M"], c["m"], c["n"], c["d"]
    post = _post(cid, b)
    Q = np.vstack([A, Xc])
    pr = HP.predict(X, y, alpha, H[b], Q, c["stationary"], c["form"], noise_zero=True, return_cov=True, post=post)
    mean, cov = pr["mean"], pr["cov"]
    var = np.diagonal(cov)[M:]
    s = var + HP.LD(noise[b])
    p = np.concatenate([np.broadcast_to(mean[:M], (m, M)), mean[M:, None]], axis=1)
    cq = np.concatenate([cov[:M, M:].T, var[:, None]], axis=1)
    q = np.zeros_like(cq)
    kg = np.zeros(m, dtype=HP.LD)
    for i in range(m):
        if s[i] > 0:
            q[i] = cq[i] / np.sqrt(s[i])
            kg[i] = envelope_ld(p[i], q[i])
    Ks = HP.gram(Q, H[b], c["stationary"], c["form"], Y=X)
    sc = P.f(np.abs(Ks * post["alpha"][None, :]).sum(axis=1))
    mean_scale = np.maximum(sc[:M].max() if M else 0.0, sc[M:])
    pv = float(HP.prior_var(H[b], d, c["form"], noise=False))
    t_mean, t_var = P.tol("mean", kap[b], n), P.tol("var", kap[b], n)
    sf, qf = P.f(s), np.abs(P.f(q)).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        tol = np.where(sf > 0.0, 2.0 * t_mean * mean_scale + SQ2PI * (t_var * pv / np.sqrt(sf) + qf * t_var * pv / (2.0 * sf)), np.inf)
    return {"kg": kg, "p": p, "q": q, "s": s, "tol": tol}


def envelope64(p, q):
    """The device's form in fp64 numpy for (m, L) line arrays: line j is the minimum on [lo_j, hi_j], the intersection over k of
    ``{z : (q_j - q_k) z <= p_k - p_j}``; equal slopes: the lower intercept wins, exact duplicates: the lower index; a line that owns
    an interval contributes ``(p_j - p*) (Phi(hi) - Phi(lo)) + q_j (phi(lo) - phi(hi))``; the value is minus the sum, clipped at 0."""
    from scipy.special import erfc

    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    L = p.shape[1]
    dq = q[:, :, None] - q[:, None, :]
    dp = p[:, None, :] - p[:, :, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        z = dp / dq
    hi = np.where(dq > 0.0, z, np.inf).min(axis=2)
    lo = np.where(dq < 0.0, z, -np.inf).max(axis=2)
    jj, kk = np.arange(L)[None, :, None], np.arange(L)[None, None, :]
    dead = ((dq == 0.0) & (kk != jj) & ((dp < 0.0) | ((dp == 0.0) & (kk < jj)))).any(axis=2)
    owns = ~dead & (lo < hi)
    r2 = math.sqrt(0.5)
    dPhi = np.where(lo >= 0.0, 0.5 * (erfc(lo * r2) - erfc(hi * r2)), 0.5 * (erfc(-hi * r2) - erfc(-lo * r2)))
    with np.errstate(over="ignore"):
        dphi = (np.exp(-(lo * lo) / 2.0) - np.exp(-(hi * hi) / 2.0)) / math.sqrt(2.0 * math.pi)
    term = (p - p.min(axis=1)[:, None]) * dPhi + q * dphi
    return np.maximum(-np.where(owns, term, 0.0).sum(axis=1), 0.0)


def replica64(X, y, alpha, h, Xc, A, noise, stationary, form, drop_self=False, white_on=False, maximise=False):
    """``(kg (m,), s (m,))`` in fp64 numpy / LAPACK on an explicit inverse, in the device's form (module docstring).  The slips:
    ``drop_self`` leaves the candidate's own line out, ``white_on`` evaluates the variance and k(a, x) at a == x with the white level
    on, ``maximise`` computes E[max_j (p_j + q_j Z)] - max_j p_j."""
    from oracle import gp_oracle as O
    from scipy.linalg import cho_solve, cholesky

    X, Xc = np.atleast_2d(np.asarray(X, dtype=np.float64)), np.atleast_2d(np.asarray(Xc, dtype=np.float64))
    A = np.asarray(A, dtype=np.float64).reshape(-1, X.shape[1])
    n, d = X.shape
    M, m = len(A), len(Xc)
    K = O.gram_with_jitter(X, np.broadcast_to(alpha, (n,)), h, stationary, form)
    L = cholesky(K, lower=True, check_finite=False)
    a = cho_solve((L, True), y, check_finite=False)
    Ki = cho_solve((L, True), np.eye(n), check_finite=False)
    Ki = 0.5 * (Ki + Ki.T)
    hk = np.array(h, dtype=np.float64)
    white = 0.0 if not white_on else float(np.exp(hk[-1]))
    hk[-1] = -np.inf
    Ks = O.kernel_matrix(Xc, hk, stationary, form, Y=X)
    mean = Ks @ a
    prior = float(O.kernel_diag(1, hk, d, form)[0]) + white
    var = np.maximum(prior - np.einsum("ij,ij->i", Ks @ Ki, Ks), 0.0)
    s = var + noise
    if M:
        R = O.kernel_matrix(A, hk, stationary, form, Y=X)
        muA = R @ a
        kAx = O.kernel_matrix(Xc, hk, stationary, form, Y=A)
        if white_on:
            kAx = kAx + white * (Xc[:, None, :] == A[None, :, :]).all(axis=2)
        C = kAx - Ks @ (R @ Ki).T
    else:
        muA, C = np.zeros(0), np.zeros((m, 0))
    ok = s > 0.0
    rs = np.where(ok, 1.0 / np.sqrt(np.where(ok, s, 1.0)), 0.0)
    p = np.concatenate([np.broadcast_to(muA, (m, M)), mean[:, None]], axis=1)
    q = np.concatenate([C, var[:, None]], axis=1) * rs[:, None]
    if drop_self:
        p, q = (p[:, :M], q[:, :M]) if M else (p, 0.0 * q)
    kg = envelope64(-p, -q) if maximise else envelope64(p, q)
    return np.where(ok, kg, 0.0), s


def ratio(got, ref):
    """Worst ``|got - reference| / tol`` over the candidates (an infinite tolerance counts 0, a finite one that is 0 is met by an
    error of exactly 0 alone) -- ``got`` in normalised-y units."""
    err = np.abs(P.f(got) - P.f(ref["kg"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, err / ref["tol"])
    return float(r.max())
