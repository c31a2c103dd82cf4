"""The tolerance classes of the prediction gradients qualify (the project's rule, tests/test_cpu_precision.py): measured against
the long-double references of tests/_gradref.py on the six posterior cases, fp64 numpy / LAPACK stays within tol / 10 and a
single-precision slip (inputs rounded to fp32) misses by >= 10 tol -- for ``dmean`` with ``tol("mean", kappa, n)`` and for ``dvar``
with ``tol("var", kappa, n)``, on the absolute-sum scales of _gradref."""
import numpy as np
import pytest

import _gradref as G
import _precision as P

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)


@pytest.mark.parametrize("cid", [c["id"] for c in P.POST_CASES])
def test_gradient_tolerances_qualify(cid):
    c = P.ALL[cid]
    X, y, alpha, H, kap = P.problem(cid)
    Xq = P.query(cid)
    ref = G.ref_gradients(cid)
    n = len(X)
    t_mean, t_var = P.tol("mean", kap[0], n), P.tol("var", kap[0], n)
    dm, dv = G.gradients64(X, y, alpha, H[0], Xq, c["stationary"], c["form"])
    dm32, dv32 = G.gradients64(P.to32(X), y, alpha, H[0], P.to32(Xq), c["stationary"], c["form"])
    e = {"dmean": G.err_dmean(dm, ref) / t_mean, "dvar": G.err_dvar(dv, ref) / t_var,
         "dmean32": G.err_dmean(dm32, ref) / t_mean, "dvar32": G.err_dvar(dv32, ref) / t_var}
    print("PRECISION %-28s dmean %.3e tol (fp32 inputs %.3e)  dvar %.3e tol (fp32 inputs %.3e)"
          % (cid, e["dmean"], e["dmean32"], e["dvar"], e["dvar32"]))
    assert e["dmean"] <= 0.1 and e["dvar"] <= 0.1, e
    assert e["dmean32"] >= 10.0 and e["dvar32"] >= 10.0, e


def test_matern12_factor_is_zero_at_coinciding_points():
    """fac(0) = 0 for Matern 1/2 (the rule of CanonicalPosterior.grad_x); finite and as the closed forms elsewhere."""
    r2 = np.array([0.0, 0.25])
    fac = G._fac(r2, "matern12", np.exp(-np.sqrt(r2)), np.float64)
    assert fac[0] == 0.0 and np.isclose(fac[1], -np.exp(-0.5) / 0.5)
