"""The tolerance of the partial-dependence tests (tests/test_gpu_pdep.py) is qualified here the way tests/test_cpu_precision.py
qualifies the others, without a device: on every case of tests/_pdref.py

* the fp64 numpy replica of the device's factored recurrence (Q over the dimensions outside the panel, T per axis, k(Q + T),
  chunks of 16 samples) is within tol / 10 of the long-double reference on the synthesised rows, on every panel and item;
* the same computation with the training inputs, samples and grids rounded to fp32 misses by >= 10 tol on its worst panel
  (rounding the inputs of a one-cell, one-point problem still moves the single distance: no case is exempt);
* on the r = 0 case the replica with Q formed as "full squared distance minus the panel's terms" is measured against the same
  tolerance (``test_full_minus_panel_form_of_Q``).

Lines printed with ``pytest -s`` start with ``PRECISION``."""
import numpy as np
import pytest

import _pdref as R
import _precision as P

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

MARGIN = 10.0
CIDS = [c["id"] for c in R.CASES]


def test_cases_sit_on_the_kernel_s_edges():
    by = {c["id"]: c for c in R.CASES}
    for e in (-1, 0, 1):
        c = by["pd_edge%+d" % e]
        assert (c["n"], c["S"], c["ng"][0]) == (R.TJ + e, R.SC + e, R.GT + e)
    assert {(c["n"], c["d"]) for c in R.CASES} >= {(1, 1), (257, 32)}
    rag = by["pd_ragged_B3"]
    assert 1 in rag["ng"] and R.GMAX in rag["ng"] and rag["Buse"] < rag["B"]
    assert any(k2 >= 0 and k1 > k2 for k1, k2 in rag["panels"]) and len(set(rag["panels"])) < len(rag["panels"])
    assert {c["stationary"] for c in R.CASES} == {"rbf", "matern12", "matern32", "matern52"}
    assert {c["form"] for c in R.CASES} == {"product", "sum"}


@pytest.mark.parametrize("cid", CIDS)
def test_fp64_reaches_the_tolerance_and_fp32_inputs_miss_it(cid):
    c = R.ALL[cid]
    st, fm, panels = c["stationary"], c["form"], c["panels"]
    X, y, alpha, H, kap, Xs, grids = R.problem(cid)
    reach = bite = None
    for b in range(c["Buse"]):
        t = P.tol("mean", kap[b], c["n"])
        ref = R.reference(cid, b)
        e64 = max(R.errs(R.replica64(X, R.alpha64(X, y, alpha, H[b], st, fm), H[b], Xs, grids, panels, st, fm), ref)) / t
        X32, Xs32, g32 = P.to32(X), P.to32(Xs), [P.to32(g) for g in grids]
        e32 = max(R.errs(R.replica64(X32, R.alpha64(X32, y, alpha, H[b], st, fm), H[b], Xs32, g32, panels, st, fm), ref)) / t
        reach, bite = max(reach or 0.0, e64), min(bite if bite is not None else e32, e32)
    print("PRECISION pdep %s kappa %.3g: fp64 replica %.4f tol, fp32 inputs %.4g tol" % (cid, kap[: c["Buse"]].max(), reach, bite))
    assert reach <= 1.0 / MARGIN
    assert bite >= MARGIN


def test_full_minus_panel_form_of_Q():
    """Matern-1/2 has unbounded slope in r^2 at r = 0.  Where a sample EQUALS a training point outside the panel, every cancelled
    term is an exact 0 and "full squared distance minus the panel's terms" is exact too (measured: it reaches the tolerance there, as
    the factored form does).  Its neighbour shows the loss: sample 1 of the case is within 1e-8 of training point 0 in every
    coordinate but the first, where it is far away, so that for the panels on dimension 0 the full distance carries a panel term
    ~1e15 times the Q that is left when it is taken off again."""
    cid = "pd_twin_matern12"
    c = R.ALL[cid]
    st, fm, panels = c["stationary"], c["form"], c["panels"]
    X, y, alpha, H, kap, Xs, grids = R.problem(cid)
    worst = 0.0
    for b in range(c["Buse"]):
        a = R.alpha64(X, y, alpha, H[b], st, fm)
        ref = R.reference(cid, b)
        t = P.tol("mean", kap[b], c["n"])
        good = max(R.errs(R.replica64(X, a, H[b], Xs, grids, panels, st, fm), ref)) / t
        with np.errstate(invalid="ignore"):  # (the residue can be negative: sqrt gives NaN, an infinite error)
            bad = max(R.errs(R.replica64(X, a, H[b], Xs, grids, panels, st, fm, minus=True), ref)) / t
        print("PRECISION pdep %s item %d: factored Q %.4f tol, full-minus-panel Q %.4g tol" % (cid, b, good, bad))
        worst = max(worst, bad)
        assert good <= 1.0 / MARGIN
    assert worst >= MARGIN
