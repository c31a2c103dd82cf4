"""The reference and the tolerances of the influence tests (tests/_inflref.py; ``bgp_influence``), without a
device: ``influence.influence_values`` -- the package's host path -- fed fp64 LAPACK ``K_inv`` / ``alpha`` / ``K_*`` is held against
the long-double refit on every case, within a tenth of the tolerance the device is held to; and its ``v <= 0`` rule."""
import numpy as np
import pytest

import _inflref as R
from bayes_skopt_amd.influence import influence_values

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)


def fp64_inputs(X, y, alpha, h, Xq, st, fm):  # (K_*, K_inv, alpha, latent var) from scipy's Cholesky and its explicit inverse
    from oracle import gp_oracle as O
    from scipy.linalg import cho_solve, cholesky

    L = cholesky(O.gram_with_jitter(X, np.broadcast_to(alpha, (len(X),)), h, st, fm), lower=True, check_finite=False)
    Ki, Ks = cho_solve((L, True), np.eye(len(X)), check_finite=False), O.kernel_matrix(Xq, h, st, fm, Y=X)
    prior = np.exp(h[0]) if fm == "product" else np.exp(h[0]) + 1.0
    return Ks, Ki, cho_solve((L, True), y, check_finite=False), np.maximum(prior - ((Ks @ Ki) * Ks).sum(axis=1), 0.0)


@pytest.mark.parametrize("cid", R.CIDS)
def test_influence_values_stay_within_a_tenth_of_the_tolerance(cid):
    c = R.ALL[cid]
    X, y, alpha, H, _kap, Xq, noise = R.problem(cid)
    for b in range(c["Bq"]):
        got = influence_values(*fp64_inputs(X, y, alpha, H[b], Xq, *c["family"]), noise[b], c["n_focus"])
        ratios = R.errs_over_tol(cid, b, got, "fp64")
        assert max(ratios.values()) <= 0.1, ratios


def test_a_row_without_variance_gives_nothing_to_cook_and_kl():
    X, y, alpha, H, Xq = R.zero_variance_problem()
    Ks, Ki, a, var = fp64_inputs(X, y, alpha, H[0], Xq, "rbf", "product")
    assert var[0] == 0.0 and var[1] > 0.0
    both, far = influence_values(Ks, Ki, a, var, 0.0), influence_values(Ks[1:], Ki, a, var[1:], 0.0)
    assert both["sum_cook"][0] == far["sum_cook"][0] > 0.0 and both["sum_kl"][0] == far["sum_kl"][0] > 0.0
    assert both["sum_dm2"][0] > far["sum_dm2"][0] and both["arg_max"][0] == 0
