"""Why is the optimum better than the default?  The Shapley attribution of the surrogate mean at config E shape (n = 974 training
points, d = 8, Matern-5/2 product form, median GP) of P = 1 point against N = 256 background rows:

* (a) ONE device call (``bgp_shapley`` through ``Context.shapley``), interactions included;
* (b) the route it replaces: ``Context.predict`` on the 2^d N synthesised coalition rows, 65 536 per call on the same context, and
      the weights in numpy (``shapley_from_values``): the entry points the tree had before, not the code under test;
* (c) 16 hyper-posterior rows through (a) in one call;
* (d) d = 16, N = 64 on a context of its own (n = 974, fixed hyper-parameters), (a) only: 2^16 coalitions, 4.1e9 kernel values.

Median wall time of --reps runs after a warm-up, the device synchronised on both sides of every run; every step under a time limit
of its own (--step-seconds): a step that is merely slow ends the process at once with status 124, and nothing touches the device
after it.  The alarm is served between Python instructions, so a call that hangs inside the runtime is not ended by it: run the
probe under ``timeout -k`` as well.  (a) is also given as kernel values per second.  Writes one JSON document to stdout (and
--out)."""
import argparse
import json
import os
import signal
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.pdep_probe import fitted, timed  # noqa: E402


def by_predict(ctx, Hk, x, Z, rows_per_call):
    """Route (b): the coalition rows, ``rows_per_call`` at a time, through predict; the averages and the weights in numpy."""
    from bayes_skopt_amd._posterior import coalition_picks, coalition_rows, shapley_from_values

    N, d = Z.shape
    step, pick, v = max(1, rows_per_call // N), coalition_picks(d), []
    for m0 in range(0, 1 << d, step):
        v.append(ctx.predict(Hk, coalition_rows(x, Z, pick[m0:m0 + step]))[0].reshape(len(Hk), -1, N).mean(axis=2))
    v = np.concatenate(v, axis=1)
    phi, inter = shapley_from_values(v, d, True)
    return phi[:, None], v[:, 0], v[:, -1:], inter[:, None]


def limited(seconds, fn):
    """``fn()`` under an alarm: a step past its limit ends the process there (no clean-up: nothing more runs on the device)."""
    def late(_sig, _frm):
        print("step passed its limit of %d s" % seconds, file=sys.stderr, flush=True)
        os._exit(124)

    signal.signal(signal.SIGALRM, late)
    signal.alarm(seconds)
    try:
        return fn()
    finally:
        signal.alarm(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--background", type=int, default=256)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--rows-per-call", type=int, default=65536)
    ap.add_argument("--step-seconds", type=int, default=120)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bayes_skopt_amd as bask
    from bayes_skopt_amd._posterior import noise_off

    assert bask._lib.device_count() >= 1, "needs an MI355X"
    reps = max(3, args.reps)
    opt = limited(args.step_seconds, lambda: fitted(bask))
    gp = opt.gp
    n, d = gp._X_train_.shape
    sync = lambda: bask._lib.device_synchronize(gp.device)  # noqa: E731
    rng = np.random.RandomState(1)
    Xp, Z = opt.space.rvs_transformed(1, random_state=rng), opt.space.rvs_transformed(args.background, random_state=rng)
    values = float(n) * len(Z) * (1 << d)
    out = {"shape": {"n": int(n), "d": int(d), "background": len(Z), "points": 1, "coalitions": 1 << d, "kernel_values": values},
           "reps": reps}

    gp._post.make_resident(gp)
    H = gp._canonical(gp._kernel_theta_for_predict())
    a_ms, a_span, a_out = limited(args.step_seconds, lambda: timed(lambda: gp._ctx.shapley(H, Xp, Z, True), reps, sync))
    out["a_device_call"] = {"ms_median": a_ms, "ms_min_max": a_span, "kernel_values_per_s": values / (a_ms * 1e-3)}
    b_ms, b_span, b_out = limited(args.step_seconds, lambda: timed(
        lambda: by_predict(gp._ctx, noise_off(H), Xp[0], Z, args.rows_per_call), reps, sync))
    diff = {k: float(np.abs(np.asarray(x) - np.asarray(y)).max()) for k, x, y in zip(("phi", "base", "value", "inter"), a_out, b_out)}
    out["b_predict_route"] = {"ms_median": b_ms, "ms_min_max": b_span, "rows_per_call": args.rows_per_call,
                              "max_abs_difference_to_a": diff}
    out["b_over_a"] = b_ms / a_ms
    out["phi"] = a_out[0][0, 0].tolist()
    out["value_minus_base"] = float(a_out[2][0, 0] - a_out[1][0])

    rows = np.asarray(gp.chain_)[: args.rows]
    Hr = gp._post.build_rows(gp, rows)
    c_ms, c_span, _ = limited(args.step_seconds, lambda: timed(lambda: gp._ctx.shapley(Hr, Xp, Z, True), reps, sync))
    out["c_hyper_rows"] = {"rows": int(len(rows)), "ms_median": c_ms, "ms_min_max": c_span, "ms_per_row": c_ms / len(rows),
                           "kernel_values_per_s": len(rows) * values / (c_ms * 1e-3)}

    r16 = np.random.RandomState(2)
    X16 = r16.uniform(size=(int(n), 16))
    ctx = bask._lib.Context(X16, np.sin(3.0 * X16.sum(axis=1)), 1e-8, form="product", stationary="matern52", max_batch=1)
    try:
        H16 = np.concatenate([[0.0], np.full(16, 0.5), [-6.0]])[None, :]
        assert ctx.posterior(H16, want_alpha=False)["status"][0] == 0
        x16, Z16 = r16.uniform(size=(1, 16)), r16.uniform(size=(64, 16))
        d_ms, d_span, d_out = limited(args.step_seconds, lambda: timed(lambda: ctx.shapley(H16, x16, Z16, True), reps, sync))
    finally:
        ctx.close()
    v16 = float(n) * 64 * (1 << 16)
    out["d_sixteen_dimensions"] = {"n": int(n), "d": 16, "background": 64, "kernel_values": v16, "ms_median": d_ms, "ms_min_max": d_span,
                                   "kernel_values_per_s": v16 / (d_ms * 1e-3),
                                   "efficiency_gap": float(abs(d_out[0].sum() - (d_out[2][0, 0] - d_out[1][0])))}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
