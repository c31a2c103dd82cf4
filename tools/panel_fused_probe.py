#!/usr/bin/env python3
"""Fused panel launches (bgp_set_panel_fused: automatic rule / on) against the separate potrf + trsm4 launches (off) on the launch
schedule, by shape: ms per LML batch call, alternating, best of a few; identical results."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from bayes_skopt_amd import _lib  # noqa: E402

shapes = [(1024, 8, 128), (4096, 32, 8), (2048, 16, 32), (2048, 16, 64), (2048, 16, 128), (1536, 16, 200), (640, 4, 256)]
for n, d, B in shapes:
    rng = np.random.RandomState(n + B)
    X = rng.uniform(size=(n, d))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.randn(n)
    H = np.concatenate([[0.0], np.full(d, np.log(0.3)), [np.log(0.01)]]) + 0.05 * rng.randn(B, d + 2)
    ctx = _lib.Context(X, y, 1e-10, max_batch=B)
    ctx.set_persist(0)
    modes = (0, -1, 1)
    best = {m: 1e9 for m in modes}
    out, fused = {}, {}
    for rep in range(4):
        for mode in modes:
            ctx.set_panel_fused(mode)
            ctx.lml(H)
            before = ctx.panel_fused_stats()["launches"]
            t0 = time.perf_counter()
            for _ in range(5):
                out[mode] = ctx.lml(H).copy()
            best[mode] = min(best[mode], (time.perf_counter() - t0) / 5 * 1e3)
            fused[mode] = (ctx.panel_fused_stats()["launches"] - before) // 5
    same = np.array_equal(out[0], out[-1]) and np.array_equal(out[0], out[1])
    print("n=%5d d=%2d B=%3d  off %.3f ms, rule %.3f ms (%+.1f %%, %d fused launches), on %.3f ms (%+.1f %%, %d), identical %s"
          % (n, d, B, best[0], best[-1], (best[-1] / best[0] - 1) * 100, fused[-1], best[1], (best[1] / best[0] - 1) * 100, fused[1], same))
    ctx.close()
