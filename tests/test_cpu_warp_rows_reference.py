"""The reference of tests/test_gpu_warp_rows.py (tests/_warprows.py: every row of a WARP_CASES problem through its OWN warp,
long double) is right, shown without a GPU:

* reachable -- the fp64 replica (oracle/gp_oracle.py on scipy's Beta CDF) lies within tol / 10 of it on every row, as
  tests/test_cpu_precision.py asks of row 0;
* bites -- the mistake per-row warping can make, row b evaluated with row 0's warp on ONE side (training inputs, or query
  points), misses by at least 10 tol for b = 1, 2.  (The training-side slip moves alpha, mean and var; the query-side slip leaves
  alpha alone -- alpha never sees the queries -- and must show in the mean and in the variance.)"""
import pytest

import _warprows as WR

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

MARGIN = 10.0
CIDS = [c["id"] for c in WR.WARP_CASES]


@pytest.mark.parametrize("cid", CIDS)
def test_fp64_reaches_every_row(cid):
    for b in range(WR.ALL[cid]["B"]):
        errs = WR.row_errs(cid, b, WR.moments64(cid, b))
        for q, (e, t) in errs.items():
            print("%-14s row %d %-5s reachable err/tol %.2e (tol %.2e)" % (cid, b, q, e / t, t))
            assert e <= t / MARGIN, (cid, b, q, e, t)


@pytest.mark.parametrize("cid", CIDS)
def test_row_0s_warp_on_either_side_misses(cid):
    for b in range(1, WR.ALL[cid]["B"]):
        slips = {"train": (WR.moments64(cid, b, b_train=0), ("alpha", "mean", "var")),
                 "query": (WR.moments64(cid, b, b_query=0), ("mean", "var"))}
        for side, (got, qs) in slips.items():
            errs = WR.row_errs(cid, b, {q: got[q] for q in qs})
            for q, (e, t) in errs.items():
                print("%-14s row %d row 0's warp on the %-5s side: %-5s bites err/tol %.1e" % (cid, b, side, q, e / t))
                assert e >= MARGIN * t, (cid, b, side, q, e, t)
