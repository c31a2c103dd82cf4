"""bgp_info.hip's definitions in ``numpy.longdouble`` on the same Gauss-Hermite rule, the tolerance, and an fp64
replica of the device's recurrences for tests/test_cpu_information_reference.py.  No code shared with the product.
Tolerance (absolute, per point): ``K * eps * (1 + t_max^2 + max_b |log sd_b| + max_b |log w^_b|)``, the magnitudes that cancel in g.
K = 8 x the replica's worst ratio (0.88, means 1e3 sd apart with B = 65): the margin for the device's exp / log against libm."""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
K = 7.04


# (content, B, Q, m): B*Q on and around multiples of 64; B = 257: one row past the kernel's 256-row LDS tile; m around 4 per workgroup
CASES = [("random", 1, 32, 1), ("random", 2, 1, 4), ("random", 3, 2, 257), ("random", 63, 31, 5), ("random", 64, 32, 4),
         ("random", 65, 64, 5), ("random", 257, 2, 5), ("identical", 3, 32, 4), ("identical", 64, 31, 1), ("apart", 2, 32, 5),
         ("apart", 65, 2, 4), ("apart", 3, 64, 1), ("ratio", 2, 32, 4), ("ratio", 64, 64, 5), ("dropped", 5, 32, 5),
         ("dropped", 65, 31, 4), ("atom", 3, 32, 5), ("ystd_small", 3, 32, 4), ("ystd_big", 63, 2, 5)]


def moments(content, B, m, seed=0):
    """(mean (B, m), var (B, m), weights (B,) or None, y_mean, y_std) of a case."""
    rng = np.random.RandomState(seed + 1000 * B + m)
    mean, sd = rng.randn(B, m), 10.0 ** rng.uniform(-1.0, 0.5, size=(B, m))
    w, y_mean, y_std = rng.uniform(0.1, 1.0, size=B), 0.25, 1.5
    if content == "identical":
        mean[:], sd[:] = mean[0], sd[0]
    elif content == "apart":  # means 1e3 sd apart, uniform weights: information = log B
        sd[:] = sd[0]
        mean, w = mean[0] + 1e3 * sd * np.arange(B)[:, None], None
    elif content == "ratio":  # sd ratio 1e6 between neighbouring rows
        sd = np.where(np.arange(B)[:, None] % 2 == 0, 1e-3, 1e3) * np.ones((B, m))
    elif content == "dropped":
        w[1], mean[B - 2, m // 2] = 0.0, np.inf
    elif content == "atom":
        sd[1, 0] = 0.0
    elif content == "ystd_small":
        y_std = 1e-3
    elif content == "ystd_big":
        y_std = 1e3
    return mean, sd * sd, w, y_mean, y_std


rule = np.polynomial.hermite.hermgauss


def columns(mean, var, weights, y_mean, y_std):
    """The pass's inputs as the device forms them in fp64 (mix_prep_kernel / mix_norm_kernel's expressions): mu, sd (n_used, m) of the
    used rows -- positive weight, finite moments everywhere -- and their normalised weights."""
    mean, var = np.atleast_2d(np.asarray(mean, dtype=np.float64)), np.atleast_2d(np.asarray(var, dtype=np.float64))
    w = np.ones(len(mean)) if weights is None else np.asarray(weights, dtype=np.float64)
    used = (w > 0.0) & np.isfinite(mean).all(axis=1) & np.isfinite(var).all(axis=1)
    W = 0.0
    for wb in w[used]:
        W += wb
    with np.errstate(invalid="ignore"):
        return y_std * mean[used] + y_mean, np.sqrt(var[used] * (y_std * y_std)), w[used] / W


def reference(mu, sd, w, t, omega):
    """(information, entropy) of ONE point: mu, sd, w (B,) of the used rows (w normalised), the rule (t, omega).  Long double."""
    mu, sd, w, t, omega = (np.asarray(a, dtype=np.float64).astype(LD) for a in (mu, sd, w, t, omega))
    if len(mu) == 0:
        return np.nan, np.nan
    if not np.all(sd > 0):
        return np.nan, -np.inf
    lw, lsd = np.log(w), np.log(sd)
    y = mu[:, None] + np.sqrt(LD(2)) * sd[:, None] * t[None, :]                                  # (b, q)
    a = (lw - lsd)[None, None, :] - ((y[:, :, None] - mu[None, None, :]) / sd[None, None, :]) ** 2 / 2  # (b, q, c)
    A = a.max(axis=2)
    lse = A + np.log(np.exp(a - A[:, :, None]).sum(axis=2))
    g = (lw - lsd)[:, None] - t[None, :] ** 2 - lse
    om = omega / np.sqrt(LD(np.pi))
    kl = ((g - lw[:, None]) * om[None, :]).sum(axis=1)
    return (w * kl).sum(), -(w * (lse * om[None, :]).sum(axis=1)).sum() + np.log(2 * LD(np.pi)) / 2


def tolerance(sd, w, t, k=K):
    with np.errstate(divide="ignore"):
        return k * EPS * (1.0 + float(np.max(np.asarray(t) ** 2)) + float(np.max(np.abs(np.log(sd)))) + float(np.max(np.abs(np.log(w)))))


def replica(mu, sd, w, t, omega, dtype=np.float64, two_pass=True):
    """The device's recurrences for ONE point in ``dtype``: the own component's exponent written out, the max pass, the shifted sum
    over c ascending, the (b, q) terms.  ``two_pass=False``: the log of the plain sum of exponentials."""
    mu, sd, w, t, omega = (np.asarray(a).astype(dtype) for a in (mu, sd, w, t, omega))
    B, f = len(mu), dtype
    with np.errstate(all="ignore"):
        lw, L, rinv = np.log(w), np.log(w) - np.log(sd), f(1) / sd
        y = mu[:, None] + (f(1.4142135623730951) * sd)[:, None] * t[None, :]
        own = L[:, None] - t[None, :] * t[None, :]
        a = [np.where(np.arange(B)[:, None] == c, own, L[c] - ((y - mu[c]) * rinv[c]) ** 2 / f(2)) for c in range(B)]
        A = own.copy() if two_pass else np.zeros_like(own)
        for c in range(B if two_pass else 0):
            A = np.maximum(A, a[c])
        s = np.zeros_like(own)
        for c in range(B):
            s = s + np.exp(a[c] - A)
        lse = A + np.log(s)
        wq = (omega / f(1.7724538509055159))[None, :]
        info = (w[:, None] * (wq * ((own - lse) - lw[:, None]))).sum(dtype=dtype)
        ent = f(0.91893853320467274178) - (w[:, None] * (wq * lse)).sum(dtype=dtype)
    return max(info, f(0)) if info == info else info, ent
