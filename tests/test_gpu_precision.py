"""The fp64 device kernels against the extended-precision reference (oracle/hp_oracle.py) at condition-scaled tolerances
(tests/_precision.py::tol -- the one tolerance function; tests/test_cpu_precision.py shows fp64 LAPACK meets it with a 10x
margin and a single-precision slip misses it by 10x): the LML on every tile edge, dimension-staging edge and kernel family,
every factorisation schedule, the warped LML and posterior, the LML gradient, the posterior factors, predict, PVRS and the
sample_y transform.  Every test prints its worst err / tol (``pytest -s``); lines start with ``PRECISION``.
The moments after fantasy conditioning (``fant_mean`` / ``fant_var``) meet the same model in tests/test_gpu_fantasy.py; the
batched predictive pipeline (predict and covariance over many posteriors, the acquisition pass, sample_y's draw groups,
sample_y_batch, larger PVRS sets, the Gram form, the chunk loop) in tests/test_gpu_predictive_precision.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _precision as P
from conftest import ROOT

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)


@pytest.fixture(scope="module")
def lib():
    import bayes_skopt_amd  # noqa: F401
    from bayes_skopt_amd import _lib

    assert _lib.device_count() >= 1
    return _lib


def _report(tag, c, quantity, ratio):
    print("PRECISION %-40s %-9s %-7s %-6s err/tol %.3e" % (tag, c["stationary"], c["form"], quantity, ratio))


def _check(tag, c, quantity, err, t):
    _report(tag, c, quantity, err / t)
    assert err <= t, "%s %s: error %.3e > tol %.3e (%.1fx)" % (tag, quantity, err, t, err / t)


def _ctx(lib, c, X, y, alpha, max_batch):
    return lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=max_batch)


# ------------------------------------------------------------------------------------------------------------------------------
# LML
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in P.LML_CASES])
def test_lml(lib, cid):
    c = P.ALL[cid]
    X, y, alpha, H, kap = P.problem(cid)
    ctx = _ctx(lib, c, X, y, alpha, len(H))
    got, st = ctx.lml(H, return_status=True)
    ctx.close()
    assert np.all(st == 0)
    worst = max(P.err_lml(got[b], P.ref_lml(cid, b)) / P.tol("lml", kap[b], len(X)) for b in range(len(H)))
    _check(cid, c, "lml", worst, 1.0)


# ------------------------------------------------------------------------------------------------------------------------------
# every factorisation schedule
# ------------------------------------------------------------------------------------------------------------------------------
SCHED_FAMILY = {"id": "sched", "stationary": "matern52", "form": "product"}


def _sched_check(tag, cid, got, kap, n):
    worst = max(P.err_lml(got[b], P.ref_lml(cid, b % 3)) / P.tol("lml", kap[b], n) for b in range(len(got)))
    _check(tag, SCHED_FAMILY, "lml", worst, 1.0)


@pytest.mark.parametrize("n", [640, 1025, 2048])
@pytest.mark.parametrize("schedule", ["P1", "P2", "P16", "launch_free"])
def test_factorisation_schedules(lib, monkeypatch, n, schedule):
    """The launch schedule (bgp_set_persist(0)) with 1, 2 and 16 block columns per panel group (BGP_PANELS, read at context
    creation), and the launch-free kernel (bgp_set_persist(1)); persist_stats says which one ran."""
    cid, X, y, alpha, H, kap = P.sched_problem(n, 3)
    monkeypatch.delenv("BGP_PERSIST", raising=False)
    monkeypatch.delenv("BGP_PANELS", raising=False)
    if schedule != "launch_free":
        monkeypatch.setenv("BGP_PANELS", schedule[1:])
    ctx = _ctx(lib, SCHED_FAMILY, X, y, alpha, 3)
    ctx.set_persist(1 if schedule == "launch_free" else 0)
    got, st = ctx.lml(H, return_status=True)
    s = ctx.persist_stats()
    ctx.close()
    assert np.all(st == 0)
    if schedule == "launch_free":
        assert s["calls"] == 1 and s["timeouts"] == 0, s
    else:
        assert s["calls"] == 0, s
    _sched_check("%s_%s" % (cid, schedule), cid, got, kap, n)


@pytest.mark.parametrize("gen", ["0", "1"])
@pytest.mark.parametrize("n,B", [(1025, 48), (2048, 16)])
def test_syrk_gram_generation(lib, monkeypatch, n, B, gen):
    """BGP_SYRK_GEN (read per call): the kernel-matrix blocks generated inside the first panel group's trailing update, or all
    built in front of the factorisation; gen_stats says which.  (At n = 640 no batch that fits one stream group reaches the
    generator's work threshold.)"""
    cid, X, y, alpha, H, kap = P.sched_problem(n, B)
    monkeypatch.setenv("BGP_SYRK_GEN", gen)
    ctx = _ctx(lib, SCHED_FAMILY, X, y, alpha, B)
    ctx.set_persist(0)
    g0 = ctx.gen_stats()["batches"]
    got, st = ctx.lml(H, return_status=True)
    g1 = ctx.gen_stats()["batches"]
    ctx.close()
    assert np.all(st == 0)
    assert (g1 > g0) == (gen == "1"), (g0, g1)
    _sched_check("%s_B%d_syrkgen%s" % (cid, B, gen), cid, got, kap, n)


_PS_CHILD = r"""
import sys, json
sys.path.insert(0, %(root)r)
import numpy as np
import bayes_skopt_amd
from bayes_skopt_amd import _lib
X, y, alpha, H = (np.load(%(npz)r)[k] for k in ("X", "y", "alpha", "H"))
ctx = _lib.Context(X, y, alpha, form="product", stationary="matern52", max_batch=len(H))
ctx.set_persist(1)
v, st = ctx.lml(H, return_status=True)
tr = ctx.ps_trace()
print("RESULT " + json.dumps({"lml": [float(x).hex() for x in v], "status": st.tolist(), "ps": ctx.persist_stats(),
                              "tasks": None if tr is None else int(tr[1].shape[0])}))
ctx.close()
"""


def test_launch_free_variants_in_child_processes(tmp_path):
    """BGP_PS_PAIR (chain pairs) and BGP_PS_GEN (Gram blocks generated by the tile workers) are read once per process: each
    setting runs in a fresh child, one at a time, under its own time limit; the first failure stops the sequence.  With
    BGP_PS_TRACE=1 the launch-free kernel reports its task count, which tells the variants apart: chain pairs split the
    critical pre-updates into quadrants (another count), generation adds one task per lower block of every matrix."""
    B = 3
    for n in (640, 1025, 2048):
        cid, X, y, alpha, H, kap = P.sched_problem(n, B)
        npz = str(tmp_path / ("in_%d.npz" % n))
        np.savez(npz, X=X, y=y, alpha=np.broadcast_to(alpha, (n,)), H=H)
        nblk = -(-n // 128)
        tasks = {}
        for var, env in (("pair0", {"BGP_PS_PAIR": "0", "BGP_PS_GEN": "0"}), ("pair1", {"BGP_PS_PAIR": "1", "BGP_PS_GEN": "0"}),
                         ("gen1", {"BGP_PS_PAIR": "0", "BGP_PS_GEN": "1"})):
            e = dict(os.environ, BGP_PS_TRACE="1", **env)
            e.pop("BGP_PERSIST", None)
            res = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-c", _PS_CHILD % {"root": ROOT, "npz": npz}],
                                 env=e, capture_output=True, text=True)
            assert res.returncode == 0, (n, var, res.returncode, res.stderr[-3000:])
            out = json.loads([ln for ln in res.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            assert out["status"] == [0] * B and out["ps"]["calls"] == 1 and out["ps"]["timeouts"] == 0, out
            tasks[var] = out["tasks"]
            _sched_check("%s_ps_%s" % (cid, var), cid, np.array([float.fromhex(s) for s in out["lml"]]), kap, n)
        assert tasks["gen1"] - tasks["pair0"] == B * nblk * (nblk + 1) // 2, tasks  # the generator ran
        assert tasks["pair1"] != tasks["pair0"], tasks  # the chain pairs ran


# ------------------------------------------------------------------------------------------------------------------------------
# warped inputs
# ------------------------------------------------------------------------------------------------------------------------------
def _warp_sens(quantity_err):
    return quantity_err / P.F32


@pytest.mark.parametrize("cid", [c["id"] for c in P.WARP_CASES])
def test_warped_lml_and_posterior(lib, cid):
    from oracle import gp_oracle as O

    c = P.ALL[cid]
    X, y, alpha, H, _ = P.problem(cid)
    Xw, W, kap = P.warped_problem(cid)
    n, st, fm = len(X), c["stationary"], c["form"]
    ad = np.broadcast_to(alpha, (n,))
    ctx = _ctx(lib, c, X, y, alpha, len(H))
    got, status = ctx.lml_warped(H, W, return_status=True)
    assert np.all(status == 0)
    worst = 0.0
    for b in range(len(H)):
        ref = hp.lml(Xw[b], y, alpha, H[b], st, fm)
        sens = _warp_sens(P.err_lml(O.lml(P.to32(P.f(Xw[b])), y, ad, H[b], st, fm), ref))
        worst = max(worst, P.err_lml(got[b], ref) / P.tol("lml", kap[b], n, sens))
    _check(cid + "_lml_warped", c, "lml", worst, 1.0)
    # context-level warp: posterior and predict on warped training and query points
    sw = P.ref_set_warp(cid)
    ctx.set_warp(sw["W"])
    res = ctx.posterior(H[:1], want_alpha=True)
    assert res["status"][0] == 0
    mean, var = ctx.predict(H[:1], P.query(cid))
    ctx.set_warp(None)
    ctx.close()
    for q, got_q in (("alpha", res["alpha"][0]), ("mean", mean[0]), ("var", var[0])):
        e = P.err_rel_max(got_q, sw["ref"][q], sw["scale"][q])
        _check(cid + "_set_warp", c, q, e, P.tol(q, sw["kappa"], n, sw["sens"][q]))


# ------------------------------------------------------------------------------------------------------------------------------
# LML gradient
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in P.GRAD_CASES])
def test_lml_gradient(lib, cid):
    c = P.ALL[cid]
    X, y, alpha, H, kap = P.problem(cid)
    ctx = _ctx(lib, c, X, y, alpha, len(H))
    val, grad, st = ctx.lml_grad(H)
    ctx.close()
    assert np.all(st == 0)
    wg = wl = 0.0
    for b in range(len(H)):
        ref = P.ref_grad(cid, b)
        wg = max(wg, P.err_grad(grad[b], ref) / P.tol("grad", kap[b], len(X)))
        wl = max(wl, P.err_lml(val[b], ref) / P.tol("lml", kap[b], len(X)))
    _check(cid, c, "lml", wl, 1.0)
    _check(cid, c, "grad", wg, 1.0)


# ------------------------------------------------------------------------------------------------------------------------------
# posterior factors and predict
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in P.POST_CASES])
def test_posterior_and_predict(lib, cid):
    c = P.ALL[cid]
    X, y, alpha, H, kap = P.problem(cid)
    n, k = len(X), kap[0]
    ctx = _ctx(lib, c, X, y, alpha, 1)
    res = ctx.posterior(H[:1], want_L=True, want_alpha=True, want_K_inv=True)
    assert res["status"][0] == 0
    ref = P.ref_post(cid)
    _check(cid, c, "L", P.err_L(res["L"][0], ref), P.tol("L", k, n))
    _check(cid, c, "alpha", P.err_alpha(res["alpha"][0], ref), P.tol("alpha", k, n))
    _check(cid, c, "K_inv", P.err_K_inv(res["K_inv"][0], ref["K_inv"]), P.tol("K_inv", k, n))
    Xq = P.query(cid)
    for nz in (False, True):
        hk = H[:1].copy()
        if nz:
            hk[0, -1] = -np.inf  # noise_set_to_zero: the white level leaves the kernel, the factors stay
        mean, var, cov = ctx.predict(hk, Xq, return_cov=True)
        pr = P.ref_predict(cid, nz)
        pv = P.prior_var(cid, nz)
        tag = cid + ("_noise0" if nz else "_noise")
        _check(tag, c, "mean", P.err_rel_max(mean[0], pr["mean"], P.mean_scale(cid)), P.tol("mean", k, n))
        _check(tag, c, "var", P.err_rel_max(var[0], pr["var"], pv), P.tol("var", k, n))
        _check(tag + "_cov", c, "var", P.err_rel_max(cov[0], pr["cov"], pv), P.tol("var", k, n))
    ctx.close()


# ------------------------------------------------------------------------------------------------------------------------------
# PVRS and sample_y
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in P.PVRS_CASES])
def test_pvrs(lib, cid):
    c = P.ALL[cid]
    X, _y, alpha, H, kap = P.problem(cid)
    Xc, Xt = P.pvrs_inputs(cid)
    ctx = _ctx(lib, c, X, np.zeros(len(X)), alpha, 1)
    assert ctx.pvrs_prepare(H[0], c["vec_alpha"]) == 0
    covs = ctx.pvrs(H[0], Xc, Xt)
    ctx.close()
    _check(cid, c, "pvrs", P.err_rel_max(covs, P.ref_pvrs(cid)), P.tol("pvrs", kap[0], len(X)))


@pytest.mark.parametrize("cid", [c["id"] for c in P.SAMPLE_CASES])
def test_sample_y_fixed_z(lib, cid):
    c = P.ALL[cid]
    X, y, alpha, H, kap = P.problem(cid)
    ctx = _ctx(lib, c, X, y, alpha, 1)
    assert ctx.posterior(H[:1])["status"][0] == 0
    hk = H[0].copy()
    hk[-1] = -np.inf
    out = ctx.sample_y(0, hk, P.query(cid), P.sample_z(cid), jitter=P.SAMPLE_JITTER)
    ctx.close()
    _check(cid, c, "sample", P.err_rel_max(out, P.ref_sample(cid)), P.tol("sample", P.sample_kappa(cid), len(X)))
