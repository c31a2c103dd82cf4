"""Cost of a joint batch proposal on pathwise draws (bgp_paths_select, PosteriorPaths.select_batch, Optimizer.ask(strategy=
"joint_ei")) at config E shape: n = 974 training points, d = 8, 10 000 candidates, 1024 features per path.

Three things, each the median of --reps timed calls after one warm-up call, every timed call ending in a device synchronisation
(the entry points return after their downloads have landed):

* ``select``  (per P): ``Context.paths_select(Xc, q)`` on P open paths -- evaluation of the P x m draw matrix on the device, the
  incumbents from the paths at the training inputs, q greedy steps, picks and the q x m values back;
* ``numpy``   (same process, same state): the host route it replaces -- ``paths_eval(Xc)`` and ``paths_eval(X)`` (the P x m matrix
  and the P x n one cross PCIe) and the same greedy steps in vectorised numpy (one ``np.maximum(0, c[:, None] - F).sum(0) / P``
  pass over the matrix per step); the picks of the two routes are compared;
* ``ask``     (one fitted optimiser): the whole ``ask(q, "joint_ei", n_paths=P)`` -- path construction (posterior builds of the
  distinct chain rows on a context of its own, feature upload) included -- beside ``ask(q, "cl_min")`` with EI averaged over 128
  draws (the fantasy path of section 12) in the same process.

The driver (no --step) runs every step as a process of its own under its own time limit and merges their JSON into --out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, D, M, NF = 974, 8, 10000, 1024


def median_ms(fn, reps):
    fn()  # (warm-up: code objects, allocations, the pinned arena)
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": float(np.median(t)), "all_ms": [float(v) for v in t]}


def numpy_select(ctx, X, Xc, q):
    F, _ = ctx.paths_eval(Xc)
    FX, _ = ctx.paths_eval(X)
    c = FX.min(axis=1)
    chosen = np.zeros(F.shape[1], dtype=bool)
    picks = []
    for _ in range(q):
        a = np.maximum(0.0, c[:, None] - F).sum(axis=0) / F.shape[0]
        a[chosen] = -np.inf
        p = int(np.argmax(a))
        picks.append(p)
        chosen[p] = True
        c = np.minimum(c, F[:, p])
    return picks


def step_select(P, qs, reps):
    from bayes_skopt_amd import _lib
    from bayes_skopt_amd.bayesgpr import draw_path_variates

    rng = np.random.RandomState(0)
    X = rng.uniform(size=(N, D))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.randn(N)
    y = (y - y.mean()) / y.std()
    h = np.concatenate([[0.0], np.log(rng.uniform(0.5, 1.5, size=D)), [np.log(1e-2)]])
    Xc = rng.uniform(size=(M, D))
    ctx = _lib.Context(X, y, 1e-8, form="product", stationary="matern52", max_batch=1)
    assert np.all(ctx.posterior(h[None])["status"] == 0)
    hk = h.copy()
    hk[-1] = -np.inf
    omega, phase, w, eps = draw_path_variates(rng, P, NF, D, N, "matern52")
    ctx.paths_begin(np.zeros(P, dtype=np.int32), np.tile(hk, (P, 1)), np.full(P, h[-1]), omega, phase, w, eps)
    out = {"P": P, "eval_ms": median_ms(lambda: ctx.paths_eval(Xc), reps), "matrix_MB": P * M * 8 / 1e6}
    for q in qs:
        dev = ctx.paths_select(Xc, q)[0]
        host = numpy_select(ctx, X, Xc, q)
        out["q%d" % q] = {"select": median_ms(lambda: ctx.paths_select(Xc, q), reps),
                          "select_picks_only": median_ms(lambda: ctx.paths_select(Xc, q, want_values=False, want_incumbents=False), reps),
                          "numpy": median_ms(lambda: numpy_select(ctx, X, Xc, q), reps),
                          "picks_agree": [int(a) for a in dev] == host}
    ctx.close()
    return out


def step_ask(Ps, qs, reps):
    import bayes_skopt_amd as bask

    rng = np.random.RandomState(0)
    opt = bask.Optimizer(dimensions=[(0.0, 1.0)] * D, n_points=M, n_initial_points=N, init_strategy="r2", acq_func="ei", random_state=0)
    X = rng.uniform(size=(N, D)).tolist()
    t0 = time.perf_counter()
    opt.tell(X, [float(np.sin(3 * np.sum(x)) + 0.1 * rng.randn()) for x in X], n_samples=128, gp_samples=200, gp_burnin=10)
    out = {"tell_s": time.perf_counter() - t0, "draws": 128}
    for q in qs:
        res = {"cl_min": median_ms(lambda: opt.ask(q, "cl_min"), reps)}
        res["cl_min"]["path"] = opt._last_batch_info["path"]
        for P in Ps:
            res["joint_ei_P%d" % P] = median_ms(lambda: opt.ask(q, "joint_ei", n_paths=P, n_features=NF), reps)
            res["thompson_P%d" % P] = median_ms(lambda: opt.ask(q, "thompson", n_paths=P, n_features=NF), reps)
        out["q%d" % q] = res
    out["sample_paths_ms"] = {}
    for P in Ps:
        def build():
            opt.gp.sample_paths(n_paths=P, n_features=NF, random_state=0).close()
        out["sample_paths_ms"]["P%d" % P] = median_ms(build, reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["select", "ask"], default=None)
    ap.add_argument("--P", default="128,1024")
    ap.add_argument("--qs", default="4,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="time limit of a step's process (seconds)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paths_select_probe.json"))
    args = ap.parse_args()
    Ps, qs = [int(v) for v in args.P.split(",")], [int(v) for v in args.qs.split(",")]
    if args.step:
        from bayes_skopt_amd import _lib

        assert _lib.device_count() >= 1, "needs an MI355X"
        res = step_select(Ps[0], qs, args.reps) if args.step == "select" else step_ask(Ps, qs, args.reps)
        print("RESULT " + json.dumps(res))
        return 0
    doc = {"shape": {"n": N, "d": D, "m": M, "features": NF}, "reps": args.reps, "select": {}, "ask": None}
    steps = [("select", str(P)) for P in Ps] + [("ask", args.P)]
    for step, P in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--P", P, "--qs", args.qs, "--reps", str(args.reps)]
        try:
            run = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print("step %s P=%s: no result within %d s; stopping" % (step, P, args.limit), file=sys.stderr)
            return 124
        lines = [ln for ln in run.stdout.splitlines() if ln.startswith("RESULT ")]
        if run.returncode != 0 or not lines:  # (nothing more is started on the device after a failed step)
            print(run.stdout[-2000:], run.stderr[-4000:], file=sys.stderr)
            return run.returncode or 1
        res = json.loads(lines[-1][7:])
        if step == "select":
            doc["select"]["P%s" % P] = res
        else:
            doc["ask"] = res
        print("step %s P=%s done" % (step, P), flush=True)
    text = json.dumps(doc, indent=1)
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
