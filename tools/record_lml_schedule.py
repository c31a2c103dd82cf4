"""Record what the library launches for an LML batch, case by case, on the MI355X: tests/golden/lml_schedule_mi355x.json.

Per case a fresh ``Context`` makes one ``lml`` / ``lml_warped`` call -- the deltas of ``persist_stats``, ``gen_stats`` and
``panel_fused_stats`` and, behind a launch-free call, the task total of ``ps_trace()`` -- and then the same call under
``set_timing(True)`` (no launch-free path there: every launch is counted) for the launch counts of ``last_timing()``.  Only calls
that the library had before the launch planner (csrc/bgp_plan.h) are used: run at the commit in front of it, the file is what
tests/test_cpu_plan.py holds the planner to.

    python tools/record_lml_schedule.py [--out tests/golden/lml_schedule_mi355x.json]

The cases run in ONE child process started with BGP_PS_TRACE=1 (read once per process).  The device must have 256 CUs: the
boundaries of the schedule depend on the count, and the file is refused otherwise.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# n, B, and what differs from d = 4, plain inputs, the context's default modes
CASES = [
    dict(n=100, B=8),
    dict(n=256, B=4),
    dict(n=384, B=130),
    dict(n=512, B=4),
    dict(n=512, B=32),
    dict(n=768, B=32),
    dict(n=1024, B=32),
    dict(n=1024, B=64),
    dict(n=1024, B=64, d=20),
    dict(n=1536, B=2),
    dict(n=1536, B=40),
    dict(n=896, B=72),
    dict(n=640, B=64, streams=2),
    dict(n=512, B=32, warped=True),
    dict(n=768, B=32, warped=True),
    dict(n=512, B=32, panel_fused=0),
    dict(n=512, B=32, panel_fused=1),
    dict(n=1024, B=32, persist=0),
    dict(n=512, B=32, persist=1),
]


def problem(n, d, B, seed):
    import numpy as np

    rng = np.random.RandomState(seed)
    X = rng.uniform(size=(n, d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.randn(n)
    H = np.concatenate([[0.0], np.full(d, np.log(0.4)), [np.log(0.02)]]) + 0.15 * rng.randn(B, d + 2)
    W = 0.1 * rng.randn(B, 2 * d)
    return X, y, H, W


def counters(ctx):
    g = ctx.gen_stats()
    return {"launch_free": ctx.persist_stats()["calls"], "gen_batches": g["batches"], "gen_launches": g["launches"],
            "fused_launches": ctx.panel_fused_stats()["launches"]}


def run_case(lib, case):
    """{"default": counters of the plain call (+ "ps_total"), "timed": counters and launch counts of the timed call}."""
    import numpy as np

    n, B, d = case["n"], case["B"], case.get("d", 4)
    X, y, H, W = problem(n, d, B, 7000 + n + B + d)
    ctx = lib.Context(X, y, 1e-10, max_batch=B)
    try:
        if "streams" in case:
            ctx.set_streams(case["streams"])
        if "panel_fused" in case:
            ctx.set_panel_fused(case["panel_fused"])
        if "persist" in case:
            ctx.set_persist(case["persist"])

        def call():
            before = counters(ctx)
            lml, st = ctx.lml_warped(H, W, return_status=True) if case.get("warped") else ctx.lml(H, return_status=True)
            assert np.all(st == 0) and np.all(np.isfinite(lml)), (case, st)
            after = counters(ctx)
            return {k: after[k] - before[k] for k in after}

        plain = call()
        trace = ctx.ps_trace() if plain["launch_free"] else None
        plain["ps_total"] = int(trace[1].shape[0]) if trace is not None else None
        ctx.set_timing(True)
        timed = call()
        t = ctx.last_timing()
        for k in ("kbuild", "potrf", "trsm", "syrk", "syrk_columns"):
            timed[k] = t[k]["launches"]
        assert timed.pop("launch_free") == 0  # (per-launch timing switches the launch-free path off)
    finally:
        ctx.close()
    return {"default": plain, "timed": timed}


def child(out):
    sys.path.insert(0, ROOT)
    import bayes_skopt_amd  # noqa: F401
    from bayes_skopt_amd import _lib

    records = []
    for case in CASES:
        rec = dict(n=case["n"], B=case["B"], d=case.get("d", 4), warped=bool(case.get("warped")), streams=case.get("streams"),
                   panel_fused=case.get("panel_fused"), persist=case.get("persist"))
        rec.update(run_case(_lib, case))
        records.append(rec)
        print(json.dumps(rec), flush=True)
    return records


def device_cus():
    src = "import torch; print(torch.cuda.get_device_properties(0).multi_processor_count)"
    return int(subprocess.run([sys.executable, "-c", src], check=True, capture_output=True, text=True).stdout.split()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "lml_schedule_mi355x.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        with open(a.out, "w") as f:
            json.dump(child(a.out), f)
        return 0
    ncu = device_cus()
    if ncu != 256:
        print("the device has %d CUs, not the 256 of an MI355X: nothing written" % ncu, file=sys.stderr)
        return 1
    tmp = a.out + ".cases"
    env = dict(os.environ, BGP_PS_TRACE="1")
    for k in ("BGP_PERSIST", "BGP_PANELS", "BGP_PANEL_FUSED", "BGP_STREAMS", "BGP_SYRK_GEN", "BGP_PS_PAIR", "BGP_PS_GEN"):
        env.pop(k, None)  # (the schedule of the defaults)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--out", tmp], check=True, env=env)
    with open(tmp) as f:
        cases = json.load(f)
    os.remove(tmp)
    with open(a.out, "w") as f:
        json.dump({"device_cus": ncu, "cases": cases}, f, indent=1)
        f.write("\n")
    print("wrote %s (%d cases)" % (a.out, len(cases)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
