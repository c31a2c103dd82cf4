"""The references of the profile tests (tests/_profref.py) held together without a GPU: the fp64 host restatement of the device's
walk (``profile.profile_values``: same lines, anchors and sweep order, scipy L-BFGS-B) against the plain dense-grid reference on the
cases whose minimum the device is held to, the walk's order, the reduction over the chains, and that inputs rounded to fp32 fail the
tolerance the device's values are held to."""
import numpy as np
import pytest

import _optref as R
import _profref as F

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)


def _host(key, b):
    from bayes_skopt_amd.profile import profile_values

    pr = F.problem(key)
    return profile_values(lambda x: tuple(v[0] for v in F.f64(key, b, x[None, :])), F.starts(key), pr["lo"], pr["hi"], F.grids(key),
                          F.CASES[key]["panels"], gtol=R.GTOL, max_iter=R.MAX_ITER)


@pytest.mark.parametrize("key", F.MINIMUM_CASES)
def test_the_host_restatement_misses_at_no_cell(key):
    pr = F.problem(key)
    for b in range(F.meta(key)["B"]):
        got = _host(key, b)
        for (dims, mesh), v, x, ref in zip(F.cells(key), got["val"], got["x"], F.reference_profile(key, b)):
            x = x.reshape(-1, x.shape[-1])
            assert np.all(x[:, dims] == mesh) and np.all(x >= pr["lo"]) and np.all(x <= pr["hi"])
            assert np.all(np.abs(v.reshape(-1) - ref) <= F.margin(key)), (key, b, np.abs(v.reshape(-1) - ref).max())


def test_sweep_order_and_reduction():
    from bayes_skopt_amd.profile import reduce_chains, sweep_order

    g = np.array([0.0, 0.25, 0.5, 1.0])
    assert sweep_order(g, 0.6) == ([2, 3, 1, 0], 2)
    assert sweep_order(g, 0.125) == ([0, 1, 2, 3], 4)        # a tie: the lower index; no backward sweep
    assert sweep_order(g, 7.0) == ([3, 2, 1, 0], 1)          # anchored at the last cell: no forward sweep
    assert sweep_order(g, np.nan) == ([0, 1, 2, 3], 4)
    cv = np.array([[np.nan, 2.0, 2.0], [np.nan, np.inf, np.nan], [1.0, -np.inf, 0.0]])
    cx = np.arange(9.0).reshape(3, 3, 1)
    val, x, best, nc = reduce_chains(cv, cx, np.array([[2, 0, 0], [2, 2, 2], [0, 1, 0]]))
    assert best.tolist() == [1, 0, 2] and nc.tolist() == [2, 0, 2] and x[:, 0].tolist() == [1.0, 3.0, 8.0]
    assert val[0] == 2.0 and np.isnan(val[1]) and val[2] == 0.0


@pytest.mark.parametrize("key", ["prof_opt2_S3", "prof_opt3_S3", "prof_bowl_S3"])
def test_inputs_rounded_to_fp32_fail_the_mean_tolerance(key):
    """The fp64 mean at the host profile's minimisers meets the tolerance of ``mean_error``; at the same points rounded to fp32 it
    does not."""
    c = F.meta(key)
    x = np.concatenate([v.reshape(-1, c["d"]) for v in _host(key, 0)["x"]])
    mean = lambda q: (F.f64(key, 0, q)[0] - c["y_mean"]) / c["y_std"]
    err, tol = F.mean_error(key, 0, x, mean(x))
    err32, _ = F.mean_error(key, 0, x, mean(x.astype(np.float32).astype(np.float64)))
    print("PROFREF %-14s fp64 err/tol %.3e  fp32-rounded inputs err/tol %.3e" % (key, err / tol, err32 / tol))
    assert err <= tol < err32
