"""The Beta-CDF input warp (``warp_kernel`` / ``bgp_betainc`` / ``bgp_betacf``, bgp_warp.hip) at its edges: the grid shared by
tests/test_cpu_warp_reference.py and tests/test_gpu_warp.py, the mpmath reference, a plain fp64 restatement of the kernel's
arithmetic and the tolerance.

The grid.  Log-space parameters w in ``W_GRID`` = {0, +-0.3, +-1, +-2, +-4, +-6}, all 121 pairs (wa, wb) with a = exp(wa),
b = exp(wb); per pair the points ``xs(a, b)``: 0 and 1; the smallest normal double, 1e-300, 1e-12, 1e-6, 0.01, 0.1, 0.3, 0.5,
0.7, 0.9, 0.99, 1 - 1e-6, 1 - 1e-12, 1 - 2^-53; the mean a / (a + b); the switch point (a + 1) / (a + b + 2) of the two continued
fractions and its two fp64 neighbours.  The reference is ``oracle.hp_oracle.warp_inputs`` at 50 digits (mpmath's
hypergeometric series converges on the whole grid with its default ``maxterms``; beyond |w| = 6 it does not, so the grid
stops there).

``betainc64`` restates ``bgp_betainc`` in fp64 Python with the kernel's operation order, ``math.lgamma`` / ``log`` / ``log1p`` /
``exp`` standing in for the device's, and reports the iterations of the continued fraction and whether it converged within
the kernel's cap of ``CF_CAP`` = 1000 -- HOST arithmetic: what the device does is measured by tests/test_gpu_warp.py.

The tolerance is ABSOLUTE: a warped coordinate lives in [0, 1] and enters the Gram matrix through differences.

    tol(a, b, x) = K eps (1 + |lgamma(a + b)| + |lgamma(a)| + |lgamma(b)| + |a log x| + |b log1p(-x)|)

-- the prefactor is the exponential of a sum of five terms, the absolute rounding error of that exponent (each term carries
a relative error of about eps) is the RELATIVE error of the prefactor, and every result is at most 1.  K was not fixed in
advance: it is the smallest power of two at which the restatement stays within a QUARTER of the tolerance on the whole
grid.  Measured on this grid (tests/test_cpu_warp_reference.py prints the lines, prefix ``WARPREF``):

    largest |w|   worst relative error   worst absolute error   most iterations   worst err / tol at K = 1
    1             7.3e-14                2.0e-15                16                1.95
    2             7.3e-14                3.2e-15                26                1.95
    4             2.1e-12                2.9e-14                50                1.95
    6             1.1e-10                2.2e-13                88                1.95
    (the 1.95 is at wa = -0.3, wb = 0.3, x = the switch point 0.4256: the complement branch returns 0.57 as 1 - 0.43 with an
    error of 6e-16, a few ulps of the result, against a tolerance whose exponent terms all but vanish: 1.4 eps)

    K = 8, the smallest power of two with err / tol <= 0.25: worst err / tol 0.244.

The relative error is NOT bounded by the relative budget ``_precision.CDF_REL`` = 1e-11 at |w| = 6: at a = e^6, b = e^-6 and x
at the switch point the complement branch returns 5.5e-4 as 1 - 0.99945, 1.1e-10 relative, 6e-14 absolute.

The domain.  ``DOMAIN_W`` = 15 is the largest integer |w| at which the restatement's continued fraction converges within
the cap at every point of the x grid for every pair (wa, wb) in {-|w|, 0, +|w|}^2 (most iterations: 570 at |w| = 14, 778 at
|w| = 15, both at wa = wb = |w| and x = 0.5; on a lattice of 0.1 the cap is first reached at |w| = 15.8, 985 iterations
at 15.6; every integer pair with max(|wa|, |wb|) in {14, 15} converges too).  Outside, the kernel returns NaN -- an
unconverged fraction, or a parameter ``exp(w)`` that is not a positive finite number -- and the factorisation's failure path
turns the NaN Gram matrix into ``-inf`` with a non-zero status (include/bgp.h at ``bgp_beta_cdf``).
"""
import functools
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
TINY = float(np.finfo(np.float64).tiny)
W_GRID = (0.0, 0.3, -0.3, 1.0, -1.0, 2.0, -2.0, 4.0, -4.0, 6.0, -6.0)
PAIRS = [(wa, wb) for wa in W_GRID for wb in W_GRID]
X_FIXED = (0.0, 1.0, TINY, 1e-300, 1e-12, 1e-6, 0.01, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 1.0 - 1e-6, 1.0 - 1e-12, 1.0 - 2.0 ** -53)
N_X = len(X_FIXED) + 4
SWITCH = slice(len(X_FIXED) + 1, len(X_FIXED) + 4)  # the switch point's lower neighbour, itself, its upper neighbour
CF_CAP = 1000
K = 8.0          # measured: see the module docstring
DOMAIN_W = 15    # measured: see the module docstring


def switch_point(a, b):
    return (a + 1.0) / (a + b + 2.0)


def xs(a, b):
    """The points of the grid for one parameter pair, ``N_X`` of them, the last three in increasing order."""
    s = switch_point(a, b)
    return np.array(list(X_FIXED) + [a / (a + b), np.nextafter(s, 0.0), s, np.nextafter(s, 1.0)])


def params(wa, wb):
    return math.exp(wa), math.exp(wb)


# ------------------------------------------------------------------------------------------------------------------------------
# bgp_betacf / bgp_betainc restated in fp64
# ------------------------------------------------------------------------------------------------------------------------------
def betacf64(a, b, x, cap=CF_CAP):
    """(h, iterations, converged): the modified Lentz continued fraction with the kernel's operation order."""
    FPMIN, CEPS = 1e-300, 1e-16
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    if abs(d) < FPMIN:
        d = FPMIN
    d = 1.0 / d
    h = d
    for m in range(1, cap + 1):
        m2 = 2.0 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d
        if abs(d) < FPMIN:
            d = FPMIN
        c = 1.0 + aa / c
        if abs(c) < FPMIN:
            c = FPMIN
        d = 1.0 / d
        h *= d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d
        if abs(d) < FPMIN:
            d = FPMIN
        c = 1.0 + aa / c
        if abs(c) < FPMIN:
            c = FPMIN
        d = 1.0 / d
        de = d * c
        h *= de
        if abs(de - 1.0) < CEPS:
            return h, m, True
    return h, cap, False


def _exp(v):
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


def betainc64(a, b, x, cap=CF_CAP):
    """(I_x(a, b), iterations, converged) as ``bgp_betainc`` computes it; NaN where the kernel returns NaN on purpose (a
    parameter that is not a positive finite number, or the cap reached)."""
    if not (0.0 < a < math.inf and 0.0 < b < math.inf):
        return math.nan, 0, False
    if not x > 0.0:
        return 0.0, 0, True
    if x >= 1.0:
        return 1.0, 0, True
    bt = _exp(math.lgamma(a + b) - math.lgamma(a) - math.lgamma(b) + a * math.log(x) + b * math.log1p(-x))
    if x < (a + 1.0) / (a + b + 2.0):
        h, it, ok = betacf64(a, b, x, cap)
        return (bt * h / a if ok else math.nan), it, ok
    h, it, ok = betacf64(b, a, 1.0 - x, cap)
    return (1.0 - bt * h / b if ok else math.nan), it, ok


def most_iterations(wabs, cap=CF_CAP):
    """(most iterations, all converged) of the restatement over the x grid for (wa, wb) in {-wabs, 0, +wabs}^2."""
    worst, allok = 0, True
    for wa in (-wabs, 0.0, wabs):
        for wb in (-wabs, 0.0, wabs):
            a, b = params(wa, wb)
            for x in xs(a, b):
                _v, it, ok = betainc64(a, b, float(x), cap)
                worst, allok = max(worst, it), allok and ok
    return worst, allok


# ------------------------------------------------------------------------------------------------------------------------------
# tolerance and reference
# ------------------------------------------------------------------------------------------------------------------------------
def tol(a, b, x, k=K):
    """The absolute tolerance of one value (module docstring); at x = 0 and x = 1 the value is exact and nothing is allowed."""
    if not 0.0 < x < 1.0:
        return 0.0
    return k * EPS * (1.0 + abs(math.lgamma(a + b)) + abs(math.lgamma(a)) + abs(math.lgamma(b)) + abs(a * math.log(x))
                      + abs(b * math.log1p(-x)))


@functools.lru_cache(maxsize=None)
def grid():
    """X (121, N_X) the points, T (121, N_X) their tolerances, A, B (121,) the parameters of every pair."""
    A = np.array([params(*p)[0] for p in PAIRS])
    B = np.array([params(*p)[1] for p in PAIRS])
    X = np.array([xs(a, b) for a, b in zip(A, B)])
    T = np.array([[tol(a, b, float(x)) for x in row] for a, b, row in zip(A, B, X)])
    return X, T, A, B


@functools.lru_cache(maxsize=None)
def reference():
    """I_x(a, b) on the grid from mpmath at 50 digits, (121, N_X) long double."""
    from oracle import hp_oracle as hp

    X = grid()[0]
    import warnings

    with warnings.catch_warnings():  # (I_x at the smallest normal x and a = e^6 is below the long double's range: 0)
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.array([hp.warp_inputs(X[j][:, None], np.array(PAIRS[j]), dps=50)[:, 0] for j in range(len(PAIRS))])


@functools.lru_cache(maxsize=None)
def restated():
    """(values, iterations) of ``betainc64`` on the grid."""
    X, _T, A, B = grid()
    out = [[betainc64(a, b, float(x)) for x in row] for a, b, row in zip(A, B, X)]
    assert all(o[2] for row in out for o in row)
    return np.array([[o[0] for o in row] for row in out]), np.array([[o[1] for o in row] for row in out])
