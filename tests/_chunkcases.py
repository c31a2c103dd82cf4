"""Shared by tests/test_gpu_chunk_loops.py: the two chunk bounds of the posterior entry points (``BGP_ITEM_CHUNK``, ``BGP_ROW_CHUNK``;
bgp_plan.h, DESIGN.md sections 19 and 27), the chunk counts a bound must produce -- restated here from the case's numbers, never
read back from the library -- and the comparison every test ends with: bit equality of everything a call returned.

At the shapes of these tests every scratch budget (2^24 .. 2^30 doubles) holds the whole call, so the budget-derived chunk is the
batch itself and ``min(budget's chunk, N)`` is ``min(batch, N)``."""
import contextlib

import numpy as np

ITEM, ROW = "BGP_ITEM_CHUNK", "BGP_ROW_CHUNK"
ONE = {"items": 1, "rows": 1}


def _ceil(a, b):
    return -(-a // b)


def item_chunks(B, cap, round8=False):
    """Chunks of B posteriors under ``BGP_ITEM_CHUNK=cap``.  ``round8`` (``post_chunk`` of bgp_post.hip behind predict and the Gram
    predict): a chunk of at least 8 items that does not cover the batch is rounded down to a multiple of 8."""
    chunk = min(B, cap)
    if round8 and 8 <= chunk < B:
        chunk &= ~7
    return _ceil(B, chunk)


def row_chunks(m, cap, round_to=1):
    """Chunks of m query rows or starts under ``BGP_ROW_CHUNK=cap``.  ``round_to`` = 256: ``paths_eval_run`` rounds a chunk of at
    least 256 rows DOWN to a multiple of 256."""
    chunk = cap
    if round_to > 1 and chunk >= round_to:
        chunk -= chunk % round_to
    return _ceil(m, min(chunk, m))


def cand_chunks(m, forced, tile):
    """Candidate chunks of ``BGP_KG_CHUNK`` / ``BGP_JES_CHUNK`` (tile 128) and ``BGP_GCOV_CHUNK`` (tile 256): the forced size is
    rounded UP to the tile."""
    return _ceil(m, _ceil(forced, tile) * tile)


@contextlib.contextmanager
def forced(monkeypatch, **env):
    """The switches set for the calls inside the block (they are read at every call) and gone after it."""
    for k, v in env.items():
        monkeypatch.setenv(k, str(v))
    try:
        yield
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)


def assert_same_bits(got, want, what=""):
    """``np.array_equal`` on every array of two results of the same call -- tuples, lists and dicts are walked, None matches None,
    dtypes and shapes must agree, NaNs must sit in the same places (``equal_nan``: the payload of a NaN is not part of the contract),
    integer outputs are compared as they are."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and set(got) == set(want), what
        for k in want:
            assert_same_bits(got[k], want[k], "%s[%r]" % (what, k))
    elif isinstance(want, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(want), what
        for j, (g, w) in enumerate(zip(got, want)):
            assert_same_bits(g, w, "%s[%d]" % (what, j))
    elif want is None:
        assert got is None, what
    else:
        g, w = np.asarray(got), np.asarray(want)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, g.dtype, w.dtype, g.shape, w.shape)
        if w.dtype.kind == "f":
            assert np.array_equal(np.isnan(g), np.isnan(w)), "%s: NaN pattern differs" % what
            same = np.array_equal(g, w, equal_nan=True)
            with np.errstate(invalid="ignore"):
                worst = float(np.nanmax(np.abs(g - w))) if not same and g.size else 0.0
            assert same, "%s: %d of %d values differ, largest |d| %.3e" % (what, int(np.sum(~((g == w) | (np.isnan(g) & np.isnan(w))))),
                                                                          g.size, worst)
        else:
            assert np.array_equal(g, w), "%s differs" % what


def default_then_forced(monkeypatch, make_ctx, call, env, want):
    """The shape of every test: ``call(ctx)`` on a fresh context from ``make_ctx()`` with the switches unset -- ONE chunk of either
    loop must be reported -- then on another fresh context under ``env`` -- the chunk counts ``want`` (items, rows) must be
    reported -- and every output of the two must be the same bits.  Returns the default run's result."""
    ctx = make_ctx()
    try:
        base = call(ctx)
        assert ctx.chunk_stats() == ONE, ctx.chunk_stats()
    finally:
        ctx.close()
    with forced(monkeypatch, **env):
        ctx = make_ctx()
        try:
            got = call(ctx)
            stats = ctx.chunk_stats()
        finally:
            ctx.close()
    assert stats == {"items": want[0], "rows": want[1]}, (stats, want, env)
    assert want[0] > 1 or want[1] > 1
    assert_same_bits(got, base, "forced %s" % (env,))
    return base
