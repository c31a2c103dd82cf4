"""Inputs of the path minimiser's tests (bgp_paths_minimize), shared by
tests/test_cpu_paths_minimize_reference.py and tests/test_gpu_paths_minimize.py: the seven cases of tests/_pathref.py with at
least 255 query rows, the box [-0.1, 1.1], and per path the 4 lowest rows of the case's ``Xq`` under the fp64 restatement as
starts -- 13 paths, 52 (path, start) pairs."""
import functools

import numpy as np

import _pathref as R

SEARCH_CASES = [R.CASES[j]["id"] for j in (1, 2, 4, 5, 7, 8, 9)]
LO, HI = -0.1, 1.1
N_STARTS = 4
N_PAIRS = 52
GTOL = 1e-5
MAX_ITER = 200


@functools.lru_cache(maxsize=None)
def starts(cid):
    """(P, 4, d): every path's 4 lowest rows of ``Xq`` (stable argsort of the fp64 restatement's values)."""
    f, _df = R.path64(cid)
    Xq = R.problem(cid)["Xq"]
    X0 = np.stack([Xq[np.argsort(f[p], kind="stable")[:N_STARTS]] for p in range(f.shape[0])])
    X0.setflags(write=False)
    return X0


def projected_gradient(x, g, lo=LO, hi=HI):
    """inf-norm of the projected gradient over the last axis: components that push out of the box at a bound count as zero."""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    g = np.where(((x <= lo) & (g > 0.0)) | ((x >= hi) & (g < 0.0)), 0.0, g)
    return np.abs(g).max(axis=-1)


def path_at(cid, p, xp, solve, Xq):
    """``_pathref._path`` of path ``p`` of the case at the rows ``Xq``: f, df, s, sg."""
    c, pr = R.ALL[cid], R.problem(cid)
    return R._path(xp, solve, pr["X"], pr["y"], pr["alpha"], pr["H"][pr["pidx"][p]], pr["omega"][p], pr["phase"][p], pr["w"][p],
                   pr["eps"][p], Xq, c["stationary"], c["form"])
