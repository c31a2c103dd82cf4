"""The tolerance of tests/test_gpu_pdep_var.py, qualified without a device as tests/test_cpu_pdep_reference.py does for the mean:
on every case of tests/_pdvarref.py the fp64 numpy replica of the factored recurrences is within tol / 10 of the long-double
reference (variance, cell covariance, mean), and on inputs rounded to fp32 it misses the variance by >= 10 tol.  ``pytest -s``
prints ``PRECISION`` lines."""
import pytest

import _pdref as R
import _pdvarref as V
import _precision as P

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

MARGIN = 10.0


@pytest.mark.parametrize("cid", [c["id"] for c in V.CASES])
def test_fp64_reaches_the_tolerance_and_fp32_inputs_miss_it(cid):
    c = V.ALL[cid]
    st, fm, panels = c["stationary"], c["form"], c["panels"]
    X, y, alpha, H, kap, Xs, grids = R.problem(cid)
    reach, reach_m, bite = 0.0, 0.0, None
    for b in range(c["Buse"]):
        scale = float(hp.prior_var(H[b], c["d"], fm, noise=False))
        tv, tm = P.tol("var", kap[b], c["n"]), P.tol("mean", kap[b], c["n"])
        r64 = V.replica64(X, y, alpha, H[b], Xs, grids, panels, st, fm)
        r32 = V.replica64(P.to32(X), y, alpha, H[b], P.to32(Xs), [P.to32(g) for g in grids], panels, st, fm)
        reach = max(reach, max(V.errs([g[1:] for g in r64], V.reference(cid, b), scale)) / tv)
        reach_m = max(reach_m, max(R.errs([g[0] for g in r64], R.reference(cid, b))) / tm)
        e32 = V.errs([g[1:] for g in r32], V.reference(cid, b), scale)[0] / tv
        bite = e32 if bite is None else min(bite, e32)
    print("PRECISION pdvar %s kappa %.3g: fp64 replica var/cov %.4f tol, mean %.4f tol, fp32 inputs %.4g tol"
          % (cid, kap[: c["Buse"]].max(), reach, reach_m, bite))
    assert reach <= 1.0 / MARGIN and reach_m <= 1.0 / MARGIN
    assert bite >= MARGIN
