"""Host restatement of the joint batch selection on pathwise draws (``bgp_paths_select``), the definition it
is held to, and the case list of tests/test_gpu_qsel.py.  numpy only.

``select`` is the device's arithmetic in the documented order: for the improvement kind a loop over the paths s = 0 .. P - 1,
vectorised over the candidates, ``acc = acc + np.maximum(0.0, c[s] - F[s])`` from ``acc = 0``, one division by P at the end; the
pick is ``np.argmax`` over the candidates not chosen yet (ties to the lower index); then ``c = min(c, F[:, pick])``.  Fed with the
device's own draw matrix it reproduces picks and values bit for bit.  ``qei_mc`` is the definition: the Monte-Carlo q-EI of a set,
``mean_s max(0, inc_s - min_{j in S} F[s, j])``, in ``np.longdouble``."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)


def select(F, inc, forced, q, kind):
    """F (P, m) draws, inc (P,) incumbents, forced: indices taken as chosen first, kind "improvement" | "thompson".
    Returns (picks (q,) int, values (q, m))."""
    F = np.asarray(F, dtype=np.float64)
    P, m = F.shape
    c = np.array(inc, dtype=np.float64, copy=True)
    chosen = np.zeros(m, dtype=bool)
    for k in forced:
        c = np.minimum(c, F[:, k])
        chosen[k] = True
    picks, values = np.empty(q, dtype=np.int64), np.empty((q, m))
    for j in range(q):
        if kind == "improvement":
            acc = np.zeros(m)
            for s in range(P):
                acc = acc + np.maximum(0.0, c[s] - F[s])
            a = acc / float(P)
        else:
            a = -F[j % P]
        values[j] = a
        left = np.flatnonzero(~chosen)
        pick = int(left[np.argmax(a[left])])  # (np.argmax: the first of equal values, i.e. the lowest index)
        picks[j] = pick
        chosen[pick] = True
        if kind == "improvement":
            c = np.minimum(c, F[:, pick])
    return picks, values


def qei_mc(F, inc, S):
    """mean_s max(0, inc_s - min_{j in S} F[s, j]) in long double; 0 for the empty set."""
    S = list(S)
    if not S:
        return np.longdouble(0.0)
    F = np.asarray(F, dtype=np.longdouble)
    inc = np.asarray(inc, dtype=np.longdouble)
    gain = np.maximum(np.longdouble(0.0), inc - F[:, S].min(axis=1))
    return gain.sum() / np.longdouble(F.shape[0])


def definition_bound(F, c, i):
    """2 (P + 2) eps64 mean_s(|c_s| + |F[s, i]|): P rounded additions of rounded differences, worst case, and the division."""
    P = F.shape[0]
    return 2.0 * (P + 2) * EPS * float(np.mean(np.abs(c) + np.abs(F[:, i])))


# ---- the device cases -----------------------------------------------------------------------------------------------------------
# the values kernel stages the incumbents in LDS tiles of 256 paths (SEL_TC) and takes 64 candidates per workgroup (SEL_NT); the
# evaluator works on 256 rows per workgroup, 64 features / training points per tile
SEL_TC, SEL_NT = 256, 64


def _case(j, st, fm, n, d, m, P, **kw):
    return dict(id="qsel%d_%s_%s_n%d_d%d_m%d_P%d" % (j, st, fm, n, d, m, P), stationary=st, form=fm, n=n, d=d, m=m, P=P, F=kw.pop("F", 16),
                seed=2400 + j, **kw)


CASES = [
    _case(0, "matern52", "product", 1, 1, 1, 1),
    _case(1, "rbf", "sum", 65, 8, 2, 2),
    _case(2, "matern52", "product", 65, 8, 255, 63, dup_rows=True, train_row=True),
    _case(3, "rbf", "sum", 1, 32, 256, 64),
    _case(4, "matern52", "sum", 65, 1, 257, 65, dup_rows=True),
    _case(5, "rbf", "product", 65, 32, 513, 257, train_row=True),
    _case(6, "matern52", "product", 1, 8, 63, 255),
    _case(7, "rbf", "sum", 65, 1, 65, 256),
    _case(8, "matern52", "product", 65, 8, 64, 257),
]
ALL = {c["id"]: c for c in CASES}


def problem(cid):
    """dict: X, y, alpha, h (d + 2), Xc (m, d), omega, phase, w, eps -- P paths on ONE posterior."""
    c = ALL[cid]
    rng = np.random.RandomState(c["seed"])
    n, d, m, P = c["n"], c["d"], c["m"], c["P"]
    X = rng.uniform(size=(n, d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.randn(n)
    y = (y - y.mean()) / y.std() if n > 1 else np.array([0.3])
    h = np.concatenate([[np.log(0.8)], np.log(rng.uniform(0.3, 0.9, size=d) * np.sqrt(d)), [np.log(1e-2)]])
    Xc = rng.uniform(size=(m, d))
    if c.get("dup_rows") and m >= 8:
        Xc[5] = Xc[2]
        Xc[m - 1] = Xc[2]
    if c.get("train_row") and m >= 8:
        Xc[3] = X[n // 2]
    omega, phase = np.empty((P, c["F"], d)), np.empty((P, c["F"]))
    w, eps = np.empty((P, c["F"] + 1)), np.empty((P, n))
    nu = {"matern12": 0.5, "matern32": 1.5, "matern52": 2.5}.get(c["stationary"])
    for p in range(P):
        z = rng.standard_normal((c["F"], d))
        if nu is not None:
            z = z * np.sqrt(2.0 * nu / rng.chisquare(2.0 * nu, size=c["F"]))[:, None]
        omega[p], phase[p] = z, rng.uniform(0.0, 2.0 * np.pi, size=c["F"])
        w[p], eps[p] = rng.standard_normal(c["F"] + 1), rng.standard_normal(n)
    return dict(X=X, y=y, alpha=1e-8, h=h, Xc=Xc, omega=omega, phase=phase, w=w, eps=eps)
