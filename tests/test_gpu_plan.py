"""The executors follow the plan: for the case table of tests/golden/lml_schedule_mi355x.json, what a real LML call enqueued -- the
launch-free call, the batches and launches that generated their Gram blocks, the fused panel launches, and under per-launch timing
every launch by category -- is what ``Context.lml_plan`` predicted for THIS device's CU count; and the log-likelihoods of the
planned schedule are the bits of the plain one (``set_persist(0); set_panel_fused(0)``) on the same inputs."""
import numpy as np
import pytest

from _plan_cases import CASES, case_id

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import bayes_skopt_amd  # noqa: F401
    from bayes_skopt_amd import _lib

    assert _lib.device_count() >= 1
    return _lib


def _problem(n, d, B, seed):
    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(n, d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.randn(n)
    H = np.concatenate([[0.0], np.full(d, np.log(0.4)), [np.log(0.02)]]) + 0.15 * rng.randn(B, d + 2)
    return X, y, H, 0.1 * rng.randn(B, 2 * d)


def _counters(ctx):
    g = ctx.gen_stats()
    return np.array([ctx.persist_stats()["calls"], g["batches"], g["launches"], ctx.panel_fused_stats()["launches"]])


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_a_call_enqueues_what_the_plan_says(lib, c):
    n, B, d = c["n"], c["B"], c["d"]
    X, y, H, W = _problem(n, d, B, 7000 + n + B + d)
    ctx = lib.Context(X, y, 1e-10, max_batch=B)
    try:
        if c["streams"] is not None:
            ctx.set_streams(c["streams"])
        if c["panel_fused"] is not None:
            ctx.set_panel_fused(c["panel_fused"])
        if c["persist"] is not None:
            ctx.set_persist(c["persist"])

        def call():
            """(plan in front of the call, lml, status, counter deltas of the call)"""
            plan, before = ctx.lml_plan(B, warped=c["warped"]), _counters(ctx)
            lml, st = ctx.lml_warped(H, W, return_status=True) if c["warped"] else ctx.lml(H, return_status=True)
            return plan, lml.copy(), st.copy(), _counters(ctx) - before

        plan, lml, st, got = call()
        assert np.all(st == 0) and np.all(np.isfinite(lml))
        assert plan["nblk"] == -(-n // 128) and plan["ncu"] >= 1
        print(case_id(c), "ncu", plan["ncu"], plan["path"], "counters", [int(v) for v in got])
        assert list(got) == [plan["launch_free"], plan["gen_groups"], plan["generating"], plan["fused"]]
        assert ctx.persist_stats()["timeouts"] == 0

        ctx.set_timing(True)
        tplan, tlml, tst, tgot = call()
        t = ctx.last_timing()
        ctx.set_timing(False)
        assert tplan["path"] != "launch_free"
        assert list(tgot) == [0, tplan["gen_groups"], tplan["generating"], tplan["fused"]]
        launched = [t[k]["launches"] for k in ("kbuild", "potrf", "trsm", "syrk", "syrk_columns")]
        assert launched == [tplan[k] for k in ("kbuild", "potrf", "trsm", "syrk", "columns")]
        assert np.array_equal(tst, st) and np.array_equal(tlml, lml)

        ctx.set_persist(0)
        ctx.set_panel_fused(0)
        pplan, plml, pst, pgot = call()
        assert pplan["path"] != "launch_free" and pplan["fused"] == 0 and pgot[0] == 0 and pgot[3] == 0
        assert np.array_equal(pst, st)
        assert np.array_equal(plml, lml), "max |difference| %.3e" % np.abs(plml - lml).max()
    finally:
        ctx.close()
