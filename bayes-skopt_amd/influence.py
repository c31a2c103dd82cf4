"""Case-deletion influence of the observations on the surrogate: which observations is the posterior resting
on?  Deleting observation i -- hyper-parameters, warps and the y normalisation held fixed, as ``cross_validate`` holds them -- moves
the latent posterior at any x by a rank-1 term in the resident ``P = K^-1`` and ``a = alpha``:

    c_i(x)    = [k_*(x)^T P]_i
    dmu_i(x)  = mu_{-i}(x) - mu(x)   = -c_i(x) a_i / P_ii
    dvar_i(x) = var_{-i}(x) - var(x) = +c_i(x)^2 / P_ii
    v = var(x) + s,  v_i = v + dvar_i(x)                        s: the variance of an observation
    kl_i(x)   = 1/2 [v / v_i - 1 + log(v_i / v) + dmu_i(x)^2 / v_i]

This module holds what is not the device call (``bgp_influence``, ``_lib.Context.influence``): the same quantities in numpy from a
downloaded inverse (``influence_values``: the host path, and what the tests restate), the host path's walk over the rows, and the
assembly of the result."""
import sys

import numpy as np

INFL_DMAX = 32   # dimensions the device call serves
INFL_FMAX = 64   # focus rows of one call
HOST_ROWS = 1 << 22  # entries of V (m n) per block of the host path

_told = []


def _tell_once(why):
    """One line on stderr, once per process: the influence computed by numpy on the downloaded inverse."""
    if not _told:
        _told.append(True)
        print("[bayes_skopt_amd] influence: numpy on the downloaded inverse (%s)" % why, file=sys.stderr, flush=True)


def influence_values(Ks, K_inv, alpha, var, noise, n_focus=0):
    """What ``bgp_influence`` returns for ONE posterior, in plain numpy: ``Ks`` (m, n) the latent cross kernel of the query rows,
    ``K_inv`` (n, n) and ``alpha`` (n,) as the posterior build leaves them, ``var`` (m,) the latent variances, ``noise`` the variance
    of an observation.  Returns a dict: ``sum_dm2``, ``sum_cook``, ``sum_kl``, ``max_abs``, ``arg_max`` (n,) over the m rows, and
    the signed ``dmu_focus`` / ``dvar_focus`` (n_focus, n) of the first ``n_focus`` rows.  A row with ``var + noise <= 0`` gives 0
    to ``sum_cook`` and ``sum_kl``.  Normalised-target units."""
    Ks, K_inv = np.atleast_2d(np.asarray(Ks, dtype=np.float64)), np.asarray(K_inv, dtype=np.float64)
    alpha, var = np.asarray(alpha, dtype=np.float64).ravel(), np.asarray(var, dtype=np.float64).ravel()
    m, n = Ks.shape
    pii = np.diag(K_inv).copy()
    ca, cp = alpha / pii, 1.0 / pii
    out = {k: np.zeros(n) for k in ("sum_dm2", "sum_cook", "sum_kl")}
    out["max_abs"], out["arg_max"] = np.full(n, -1.0), np.zeros(n, dtype=np.int32)
    out["dmu_focus"], out["dvar_focus"] = np.empty((n_focus, n)), np.empty((n_focus, n))
    step = max(1, HOST_ROWS // max(1, n))
    for lo in range(0, m, step):
        V = Ks[lo : lo + step] @ K_inv
        dmu, dvar = -(V * ca), (V * V) * cp
        d2 = dmu * dmu
        v = (var[lo : lo + step] + noise)[:, None]
        ok = v > 0.0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            rv = np.where(ok, 1.0 / np.where(ok, v, 1.0), 0.0)
            t = dvar * rv
            ri = 1.0 / (1.0 + t)
            cook = d2 * rv
            kl = np.where(ok, 0.5 * ((np.log1p(t) - t * ri) + cook * ri), 0.0)
        out["sum_dm2"] += d2.sum(axis=0)
        out["sum_cook"] += cook.sum(axis=0)
        out["sum_kl"] += kl.sum(axis=0)
        a = np.abs(dmu)
        top = np.argmax(a, axis=0)  # (the first row that attains the block's maximum)
        best = a[top, np.arange(n)]
        new = best > out["max_abs"]
        out["max_abs"] = np.where(new, best, out["max_abs"])
        out["arg_max"] = np.where(new, lo + top, out["arg_max"]).astype(np.int32)
        f = min(n_focus, lo + len(V)) - lo
        if f > 0:
            out["dmu_focus"][lo : lo + f], out["dvar_focus"][lo : lo + f] = dmu[:f], dvar[:f]
    return out


def stack(rows):
    """The per-posterior dicts of ``influence_values`` as one dict of (B, ...) arrays, with the ``status`` of the device call."""
    out = {k: np.stack([r[k] for r in rows]) for k in rows[0]}
    out["status"] = np.array([0 if all(np.all(np.isfinite(r[k])) for k in ("sum_dm2", "sum_cook", "sum_kl", "max_abs")) else 1
                              for r in rows], dtype=np.int32)
    return out


def concat(parts):
    """Device calls over successive blocks of rows -> one dict."""
    return parts[0] if len(parts) == 1 else {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def host_rows(gp, thetas, X, n_focus, why):
    """The host path for the median GP (``thetas=None``) or a block of chain rows: every posterior's inverse and alpha downloaded,
    the latent cross kernel from the kernel object, ``influence_values``.  Under ``warp_inputs`` the median GP sees ``X`` and the
    training inputs through the current warpers, as ``predict`` does, and a chain row through its own (``_row_warps``)."""
    from ._posterior import _with_white_zeroed
    from .acquisition import _kg_white_level

    _tell_once(why)
    base = gp._fantasy_base_alpha()

    def one(kernel, K_inv, alpha, white):
        Xw = gp.warp(X) if gp.warp_inputs else X
        k = _with_white_zeroed(kernel)
        Ks = k(Xw, gp.X_train_)
        var = np.maximum(k.diag(Xw) - np.einsum("ij,jk,ik->i", Ks, K_inv, Ks), 0.0)
        return influence_values(Ks, K_inv, alpha, var, base + white, n_focus)

    def built(t):
        """(K_inv, alpha) of the posterior at the (1, p) block ``t`` under the warp that is installed."""
        if gp._post.canonical:
            res = gp._ctx.posterior(gp._canonical(t), want_L=False, want_alpha=True, want_K_inv=True)
        else:
            res = gp._post._posterior_gram(gp, gp._gram_stack(t, gp.X_train_), want_alpha=True, want_K_inv=True)
        if res["status"][0] != 0:
            raise np.linalg.LinAlgError("%d-th leading minor of the array is not positive definite" % res["status"][0])
        return res["K_inv"][0], res["alpha"][0]

    if thetas is None:
        return stack([one(gp.kernel_, gp.K_inv_, gp.alpha_, _kg_white_level(gp, gp._post_theta))])
    rows = np.atleast_2d(np.asarray(thetas, dtype=np.float64))
    n_theta = len(gp.kernel_.theta)
    out = []
    with gp._keeping_posterior():
        if gp.warp_inputs:
            with gp._row_warps() as install:
                for r in rows:
                    t = install(r)
                    out.append(one(gp._kernel_at(t[0]), *built(t), _kg_white_level(gp, t[0])))
        else:
            for r in rows:
                t = r[None, :n_theta]
                out.append(one(gp._kernel_at(t[0]), *built(t), _kg_white_level(gp, t[0])))
    return stack(out)


def assemble(raw, m, n_focus, y_std, sd_focus, weights, path):
    """The result of ``BayesGPR.influence`` from the normalised (B, ...) arrays of the device call or the host path: y units
    (``rms``, ``max_abs``, ``dmean_focus`` scale by ``y_std``, ``dstd_focus`` too; ``cook``, ``kl`` and ``focus_z`` have none).
    ``sd_focus`` (B, n_focus): the latent standard deviation at the focus rows, normalised.  One row: (n,) arrays.  More rows
    (``weights`` (B,) or None): their weighted average, and under ``"band"`` {name: (5 %, 95 %)} the per-row band."""
    rows = {"rms": np.sqrt(raw["sum_dm2"] / m) * y_std, "cook": raw["sum_cook"] / m, "kl": raw["sum_kl"] / m,
            "max_abs": raw["max_abs"] * y_std}
    if n_focus:
        sd = np.asarray(sd_focus, dtype=np.float64)[:, :, None]
        rows["dmean_focus"] = raw["dmu_focus"] * y_std
        rows["dstd_focus"] = (np.sqrt(np.maximum(sd * sd + raw["dvar_focus"], 0.0)) - sd) * y_std
        with np.errstate(divide="ignore", invalid="ignore"):
            rows["focus_z"] = raw["dmu_focus"] / sd
    B = len(raw["sum_dm2"])
    out = {"path": path, "status": raw["status"]}
    if B == 1:
        out.update({k: v[0] for k, v in rows.items()})
        out["arg_max"] = raw["arg_max"][0]
        return out
    w = np.ones(B) if weights is None else np.asarray(weights, dtype=np.float64).reshape(B)
    w = w / w.sum()
    out["band"] = {k: tuple(np.percentile(v, [5.0, 95.0], axis=0)) for k, v in rows.items()}
    out.update({k: np.tensordot(w, v, axes=1) for k, v in rows.items()})
    out["arg_max"] = raw["arg_max"][int(np.argmax(w))]  # (a row index has no average: the heaviest row's)
    return out
