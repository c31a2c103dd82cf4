"""Host side of ``BayesGPR.cross_validate``: the fold splitter and the rules that combine the per-row
held-out predictives of ``bgp_cross_validate`` -- numpy on (B, n) and (B, K) arrays, nothing of size n^2."""
import numpy as np

MAX_FOLD = 128  # bgp_cv.hip CV_SMAX: points per fold


def split_folds(n, n_folds, random_state=None):
    """``n_folds`` disjoint index arrays that cover ``range(n)``: a shuffle seeded by ``random_state`` cut into near-equal parts
    (sizes differ by at most 1, the larger ones first)."""
    from sklearn.utils import check_random_state

    n, n_folds = int(n), int(n_folds)
    if not 1 <= n_folds <= n:
        raise ValueError(f"n_folds = {n_folds} must lie in 1 .. n = {n}")
    perm = check_random_state(random_state).permutation(n)
    return [np.sort(part).astype(np.int64) for part in np.array_split(perm, n_folds)]


def check_folds(folds, n):
    """The fold list as int64 arrays; ValueError for what ``bgp_cross_validate`` refuses (named here, before any build)."""
    folds = [np.asarray(f, dtype=np.int64).reshape(-1) for f in folds]
    if not folds:
        raise ValueError("cross_validate needs at least one fold")
    seen = np.zeros(n, dtype=bool)
    for k, f in enumerate(folds):
        if len(f) == 0:
            raise ValueError(f"fold {k} is empty")
        if len(f) > MAX_FOLD:
            raise ValueError(f"fold {k} has {len(f)} points: at most {MAX_FOLD} per fold are supported "
                             f"(use n_folds >= {-(-n // MAX_FOLD)} at n = {n})")
        if f.min() < 0 or f.max() >= n:
            raise ValueError(f"fold {k} holds an index outside [0, {n})")
        if seen[f].any() or len(np.unique(f)) != len(f):
            raise ValueError(f"fold {k} repeats an index (the folds must be disjoint)")
        seen[f] = True
    return folds


def _logsumexp0(a):
    m = np.max(a, axis=0)
    return m + np.log(np.sum(np.exp(a - m[None]), axis=0))


def fold_weights(row_fold_lpd, weights="is"):
    """(normalised weights (B, K), combined fold_lpd (K,), ess (K,)) of B rows.  ``"is"``: the importance weights that carry the
    rows from p(theta | y) to p(theta | y_-F), w_bF ~ 1 / p(y_F | y_-F, theta_b), and the harmonic-mean fold density
    ``-log mean_b exp(-lpd_bF)``; ``"equal"``: the plug-in mixture, ``log mean_b exp(lpd_bF)``."""
    lpd = np.atleast_2d(np.asarray(row_fold_lpd, dtype=np.float64))
    B = lpd.shape[0]
    if weights == "is":
        lse = _logsumexp0(-lpd)
        w = np.exp(-lpd - lse[None])
        combined = -(lse - np.log(B))
    elif weights == "equal":
        w = np.full(lpd.shape, 1.0 / B)
        combined = _logsumexp0(lpd) - np.log(B)
    else:
        raise ValueError(f"weights must be 'is' or 'equal', got {weights!r}")
    return w, combined, 1.0 / np.sum(w * w, axis=0)


def combine_rows(row_mean, row_var, row_fold_lpd, folds, y, weights="is"):
    """The rows' held-out predictives as one: per fold the weights of ``fold_weights``, then per point the mixture's mean and
    variance (``sum_b w_b (var_b + (mean_b - mean)^2)``, never below the weighted mean of the rows' variances) and the mixture's log
    density at ``y``.  Points that no fold covers are NaN.  Returns a dict: mean, std, point_lpd, z (n,), fold_lpd, ess (K,), elpd."""
    row_mean, row_var = np.atleast_2d(row_mean), np.atleast_2d(row_var)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n = row_mean.shape[1]
    w, fold_lpd, ess = fold_weights(row_fold_lpd, weights)
    mean, var, point = (np.full(n, np.nan) for _ in range(3))
    for k, f in enumerate(folds):
        wk = w[:, k][:, None]
        m, v = row_mean[:, f], row_var[:, f]
        mean[f] = np.sum(wk * m, axis=0)
        var[f] = np.sum(wk * (v + (m - mean[f][None]) ** 2), axis=0)
        with np.errstate(divide="ignore"):
            dens = np.log(wk) - 0.5 * ((y[f][None] - m) ** 2 / v + np.log(2.0 * np.pi * v))
        point[f] = _logsumexp0(dens)
    std = np.sqrt(var)
    return {"mean": mean, "std": std, "fold_lpd": fold_lpd, "point_lpd": point, "z": (y - mean) / std, "elpd": float(np.sum(fold_lpd)),
            "ess": ess}
