"""Qualifies the inputs of the path minimiser's device test (tests/test_gpu_paths_minimize.py) without a
GPU: on the seven cases, the box and the starts of tests/_pathmin.py, scipy's L-BFGS-B on the fp64 restatement of a path and its
gradient (``gtol=1e-5, ftol=0, maxiter=200, maxls=30``) reaches a projected gradient <= 1e-5 from every one of the 52
(path, start) pairs.  The device test allows at most 5 pairs that do not converge; that cap rests on this reference having none.
Measured here: 52 of 52, smallest decrease from a start 3.5e-2, largest evaluation count 99."""
import numpy as np
from scipy.optimize import minimize

import _pathmin as M
import _pathref as R


def test_the_starts_are_the_lowest_rows_inside_the_box():
    n_pairs = 0
    for cid in M.SEARCH_CASES:
        X0, c = M.starts(cid), R.ALL[cid]
        assert X0.shape == (c["P"], M.N_STARTS, c["d"]) and c["m"] >= 255
        assert np.all(X0 >= M.LO) and np.all(X0 <= M.HI)
        f, _ = R.path64(cid)
        Xq = R.problem(cid)["Xq"]
        for p in range(c["P"]):
            rows = [int(np.flatnonzero(np.all(Xq == x, axis=1))[0]) for x in X0[p]]
            assert len(set(rows)) == M.N_STARTS and np.all(np.diff(f[p][rows]) >= 0.0)
            assert f[p][rows[-1]] == np.sort(f[p])[M.N_STARTS - 1]
        n_pairs += c["P"] * M.N_STARTS
    assert n_pairs == M.N_PAIRS


def test_the_reference_search_converges_from_every_start():
    converged, decrease, evals = 0, [], []
    for cid in M.SEARCH_CASES:
        X0, c = M.starts(cid), R.ALL[cid]
        for p in range(c["P"]):
            def fun(x, p=p):
                f, df, _s, _sg = M.path_at(cid, p, np.float64, R._solve_inv64, x[None, :])
                return float(f[0]), np.array(df[0], dtype=np.float64)

            for s in range(M.N_STARTS):
                f0 = fun(X0[p, s])[0]
                res = minimize(fun, X0[p, s].copy(), jac=True, method="L-BFGS-B", bounds=[(M.LO, M.HI)] * c["d"],
                               options=dict(gtol=M.GTOL, ftol=0.0, maxiter=M.MAX_ITER, maxls=30))
                pg = float(M.projected_gradient(res.x, fun(res.x)[1]))
                assert np.all(res.x >= M.LO) and np.all(res.x <= M.HI)
                converged += pg <= M.GTOL
                decrease.append(f0 - res.fun)
                evals.append(res.nfev)
                if pg > M.GTOL:
                    print("REFERENCE %s path %d start %d: |pg| %.3e after %d evaluations (%s)" % (cid, p, s, pg, res.nfev, res.message))
    print("REFERENCE converged %d / %d, smallest decrease %.3e, largest evaluation count %d"
          % (converged, len(evals), min(decrease), max(evals)))
    assert len(evals) == M.N_PAIRS and converged == M.N_PAIRS
    assert min(decrease) > 0.0
