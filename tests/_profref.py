"""Cases and references of the profile tests (bgp_profile_dependence), shared by
tests/test_cpu_profile_reference.py and tests/test_gpu_profile.py.  The posteriors, ``y_mean`` / ``y_std`` and boxes are those of
tests/_optref.py (``kappa`` is 0 throughout: the profile is of the mean), plus one single-basin problem of its own -- targets from
a convex bowl -- with its own fp64 and long-double objective (``_bowl_objective``); nothing of ``_optref`` is changed.

A case: the _optref case, its panels, the grid sizes per dimension (``ng``; a dimension's grid is ``linspace(lo, hi, ng)``, the
midpoint for ``ng = 1``) and its chains' starts -- names: ``low0`` the lowest row of ``_optref.starts``, ``hi`` / ``lo`` the box
corners (anchored at the last cell / at cell 0: one sweep is empty), ``out`` the start outside the box; or a number m: the
cell-centred lattice of m values per dimension.

``reference_profile`` is the plain method for the cases with at most two free dimensions: a dense grid over the free coordinates,
then scipy L-BFGS-B on ``objective64`` from its best four points.  It shares nothing with the device."""
import functools
import math

import numpy as np

import _optref as R
import _precision as P

BOWL = "bowl_n129_d3_rbf_product_B1"
_BOWL_META = dict(id=BOWL, n=129, d=3, stationary="rbf", form="product", B=1, y_mean=0.7, y_std=2.5)


@functools.lru_cache(maxsize=None)
def _bowl():
    X = np.random.RandomState(1720).uniform(size=(129, 3))
    y = np.sum((X - np.array([0.4, 0.55, 0.3])) ** 2, axis=1)
    y = (y - y.mean()) / y.std()
    H = np.array([[0.5, math.log(0.9), math.log(0.8), math.log(1.0), math.log(1e-2)]])
    pr = {"X": X, "y": y, "alpha": 1e-8, "H": H, "lo": np.full(3, R.LO), "hi": np.full(3, R.HI)}
    for v in (X, y, H, pr["lo"], pr["hi"]):
        v.setflags(write=False)
    return pr


@functools.lru_cache(maxsize=None)
def _bowl_alpha(ld):
    from oracle import gp_oracle as O
    from oracle import hp_oracle as HP

    pr = _bowl()
    if ld:
        return HP.posterior(pr["X"], pr["y"], pr["alpha"], pr["H"][0], "rbf", "product")["alpha"]
    return np.linalg.solve(O.gram_with_jitter(pr["X"], np.full(129, 1e-8), pr["H"][0], "rbf", "product"), pr["y"])


def _bowl_objective(Xq, ld):
    """mean, mean_scale, f, df of the bowl's posterior (RBF, product form) in fp64 numpy or long double."""
    xp = np.longdouble if ld else np.float64
    pr, a = _bowl(), _bowl_alpha(ld)
    h, X, Xq = pr["H"][0].astype(xp), pr["X"].astype(xp), np.atleast_2d(Xq).astype(xp)
    diff = (Xq[:, None, :] - X[None, :, :]) / np.exp(h[1:4])
    T = np.exp(h[0]) * np.exp(-(diff * diff).sum(axis=2) / 2) * a[None, :]
    mean, dmean = T.sum(axis=1), -(T[:, :, None] * diff / np.exp(h[1:4])).sum(axis=1)
    return {"mean": mean, "mean_scale": float(np.abs(T).sum(axis=1).max()), "f": xp(0.7) + xp(2.5) * mean, "df": xp(2.5) * dmean}


def _lattice(d, m):
    """m cell-centred values per dimension: the starts of the cases whose several basins a few observed points do not reach."""
    return np.stack(np.meshgrid(*[(np.arange(m) + 0.5) / m] * d, indexing="ij"), axis=-1).reshape(-1, d)


_ROWS = [  # tag, _optref case, panels, ng, starts (names, or the lattice's values per dimension)
    ("opt0", "opt0_n1_d1_rbf_product_B1", [(0, -1)], [5], ("low0",)),                                  # no free dimension
    ("opt1", "opt1_n2_d2_matern12_product_B1", [(0, 1), (1, -1)], [3, 4], ("low0", "hi", "out")),       # a 2-D panel in d = 2
    ("opt2", "opt2_n127_d2_matern32_product_B1", [(0, -1), (1, -1), (1, 0)], [7, 1], ("low0", "hi", "lo")),  # a single-cell line
    ("opt3", "opt3_n128_d3_matern52_product_B3", [(0, -1), (2, 1), (1, -1)], [4, 3, 5], ("low0", "hi", "out")),
    ("opt4", "opt4_n129_d5_rbf_sum_B1", [(0, -1), (3, 1), (2, -1)], [5, 3, 1, 4, 2], ("low0",)),        # a degenerate free dimension
    ("opt5", "opt5_n257_d4_matern12_sum_B1", [(1, -1), (0, 3)], [3, 2, 2, 3], ("low0",)),
    ("opt6", "opt6_n385_d3_matern32_sum_B3", [(1, -1), (0, 2)], [3, 4, 3], ("low0",)),
    ("opt7", "opt7_n129_d32_matern52_sum_B1", [(0, -1), (31, 5)], [3] * 32, ("low0",)),
    ("bowl", BOWL, [(0, -1), (1, 2), (2, -1)], [5, 3, 4], ("low0", "lo", "out")),
    ("opt8", R.BIG_CASE, [(0, -1)], [3, 3], ("low0",)),                                                 # the scratch-row branch
    # the multi-modal problems (sin(3 sum x) under length scales near a third of the box: several basins per cell) from a lattice
    # whose spacing is below the length scales; these are held to the minimum, not replayed
    ("opt3", "opt3_n128_d3_matern52_product_B3", [(0, -1), (2, 1), (1, -1)], [4, 3, 5], 3),
    ("opt6", "opt6_n385_d3_matern32_sum_B3", [(1, -1), (0, 2)], [3, 4, 3], 2),
    ("opt8", R.BIG_CASE, [(0, -1)], [3, 3], 3),
]
CASES = {"prof_%s_%s" % (tag, "S%d" % len(st) if isinstance(st, tuple) else "L%d" % st): dict(cid=cid, panels=pan, ng=ng, starts=st)
         for tag, cid, pan, ng, st in _ROWS}
REPLAY_CASES = [k for k, c in CASES.items() if isinstance(c["starts"], tuple)]
BITS_CASE = "prof_opt3_S3"
# The cases whose minimum is held to ``reference_profile``: at most two free dimensions in every panel.  The n = 1 case is not among
# them: ptp(y) = 0 there, so the margin is 0, and with no free dimension the comparison is a pure evaluation, which the long-double
# check of the value covers.  From the three observed-point chains of prof_opt3_S3 and the one of prof_opt6_S1 / prof_opt8_S1 the fp64
# host walk itself misses cells (3 of 24, 1 of 3 at n = 3100): those go through replay and structure, their lattice twins through this.
MINIMUM_CASES = ["prof_opt1_S3", "prof_opt2_S3", "prof_bowl_S3", "prof_opt3_L3", "prof_opt6_L2", "prof_opt8_L3"]
SINGLE_BASIN = "prof_bowl_S3"
MISS_CAP = 0.05  # share of a multi-modal case's cells the device may end above the reference (a condition, not a measurement)


def meta(key):
    cid = CASES[key]["cid"]
    return _BOWL_META if cid == BOWL else R.ALL[cid]


def problem(key):
    cid = CASES[key]["cid"]
    return _bowl() if cid == BOWL else R.problem(cid)


def grids(key):
    c, pr = CASES[key], problem(key)
    return [np.linspace(l, h, g) if g > 1 else np.array([0.5 * (l + h)]) for l, h, g in zip(pr["lo"], pr["hi"], c["ng"])]


@functools.lru_cache(maxsize=None)
def starts(key):
    """(S, d) starts of a case's chains, as handed to the device (not clipped)."""
    c, pr = CASES[key], problem(key)
    if isinstance(c["starts"], tuple):
        X0 = _bowl_starts() if c["cid"] == BOWL else R.starts(c["cid"], 0)
        rows = {"low0": X0[0], "hi": pr["hi"], "lo": pr["lo"], "out": X0[-1]}
        out = np.array([rows[s] for s in c["starts"]])
    else:
        out = _lattice(len(pr["lo"]), c["starts"])
    out.setflags(write=False)
    return out


def cells(key):
    """Per panel: (the panel's dimensions, the (cells, len(dims)) grid values in the order of the panel's block)."""
    g = grids(key)
    out = []
    for k1, k2 in CASES[key]["panels"]:
        dims = [k1] + ([k2] if k2 >= 0 else [])
        mesh = np.stack(np.meshgrid(*[g[k] for k in dims], indexing="ij"), axis=-1).reshape(-1, len(dims))
        out.append((dims, mesh))
    return out


def _bowl_starts():
    """The lowest of 256 seeded rows under the fp64 objective, and that row pushed out of the box through the upper face of x0."""
    Xr = np.random.RandomState(1730).uniform(size=(256, 3))
    low = Xr[int(np.argmin(_bowl_objective(Xr, False)["f"]))]
    return np.array([low, low + np.array([1.7, 0.0, 0.0])])


def _objective(key, b, X, ld):
    cid = CASES[key]["cid"]
    if cid == BOWL:
        return _bowl_objective(X, ld)
    return (R.objective_ld if ld and not meta(key).get("big") else R.objective64)(cid, b, 0.0, X)


def f64(key, b, X):
    """(f, df) of the fp64 objective (y units) at the rows of X."""
    o = _objective(key, b, X, False)
    return o["f"], o["df"]


def margin(key):
    return 1e-6 * float(meta(key)["y_std"] * np.ptp(problem(key)["y"]))


@functools.lru_cache(maxsize=None)
def reference_profile(key, b, dense=41):
    """Per panel the (cells,) profile of posterior b in y units by the plain method."""
    from scipy.optimize import minimize

    pr = problem(key)
    lo, hi, d = pr["lo"], pr["hi"], len(pr["lo"])
    out = []
    for dims, mesh in cells(key):
        free = [t for t in range(d) if t not in dims]
        axes = [np.linspace(lo[t], hi[t], dense) if hi[t] > lo[t] else lo[t:t + 1] for t in free]
        Z = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, len(free)) if free else np.zeros((1, 0))
        vals = np.empty(len(mesh))
        for i, g in enumerate(mesh):
            Xq = np.empty((len(Z), d))
            Xq[:, dims], Xq[:, free] = g, Z

            def fun(z, x=Xq[0].copy()):
                x[free] = z
                f, df = f64(key, b, x[None, :])
                return float(f[0]), np.array(df[0][free], dtype=np.float64)

            f = f64(key, b, Xq)[0]
            best = float(f.min())
            for j in (np.argsort(f, kind="stable")[:4] if free else []):
                r = minimize(fun, Z[j].copy(), jac=True, method="L-BFGS-B", bounds=list(zip(lo[free], hi[free])),
                             options=dict(gtol=R.GTOL, ftol=0.0, maxiter=R.MAX_ITER))
                best = min(best, fun(np.minimum(np.maximum(r.x, lo[free]), hi[free]))[0])
            vals[i] = best
        out.append(vals)
    return out


def mean_error(key, b, x, val):
    """(error of the normalised means ``val`` at the rows ``x`` against the high-precision mean there -- long double; fp64 at twice
    the class at n = 3100 --, relative to the reference's absolute-sum scale; the tolerance of the class the optimum search's end
    points are held to)."""
    c, pr = meta(key), problem(key)
    ref = _objective(key, b, x, True)
    kappa = P.kappa_of(pr["X"], pr["alpha"], pr["H"][b], c["stationary"], c["form"])
    return P.err_rel_max(val, ref["mean"], ref["mean_scale"]), (2.0 if c.get("big") else 1.0) * P.tol("mean", kappa, c["n"])
