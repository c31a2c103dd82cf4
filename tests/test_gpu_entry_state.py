"""The resident-posterior entry points share one guard (``bgp_guard``), one exit path (``post_call``) and one owner of "what is
resident" (``BgpResident``).  This file holds the raw C calls of every consumer to that contract, at the
smallest shapes where each of them still launches (n = 20, d = 2, two posteriors, m = 12 queries):

* nothing built -> BGP_ERR_STATE (4), the text names the consumer and says ``resident``;
* every invalidator (new data, a context-level warp set or cleared, an LML gradient, a per-row-warped build, ``pvrs_prepare``) ends
  what a plain build made resident, for every consumer and for an open fantasy run;
* a submitted, uncollected LML batch -> 4 with ``pending``;
* a ``bgp_fantasy_begin`` that fails half way (its block cannot be allocated) leaves no fantasy state and no trace in later results.

Argument and capability checks keep their place in front of the "not resident" answer: under a context-level warp the four consumers
that do not support one (fantasy, prediction gradients, optimum search, paths) answer BGP_ERR_INVALID (1) with ``warped inputs``."""
import ctypes as C

import numpy as np
import pytest

from conftest import synth

pytestmark = pytest.mark.gpu

N, D, B2, M = 20, 2, 2, 12
STATE, INVALID = 4, 1


@pytest.fixture(scope="module")
def lib():
    import bayes_skopt_amd  # noqa: F401
    from bayes_skopt_amd import _lib

    assert _lib.device_count() >= 1
    return _lib


class Problem:
    """The inputs of every call (read only) and the buffers the raw calls write into."""

    def __init__(self):
        rng = np.random.RandomState(5)
        self.X, self.y = synth(N, D, seed=5)
        self.alpha = np.full(N, 1e-10)
        self.H = np.array([0.0, np.log(0.3), np.log(0.3), np.log(0.01)]) + 0.05 * rng.randn(B2, D + 2)
        self.Hk = self.H.copy()
        self.Hk[:, -1] = -np.inf  # (white level off: the latent function)
        self.noise = np.exp(self.H[:, -1])
        self.W = 0.2 * rng.randn(B2, 2 * D)
        self.Xq = rng.uniform(size=(M, D))
        self.z = rng.randn(B2, M)
        self.kinds = np.array([0, 2], dtype=np.int32)  # ACQ_EI, ACQ_LCB
        self.params = np.array([np.nan, 1.96])
        self.pidx = np.arange(B2, dtype=np.int32)
        self.lo, self.hi = np.zeros(D), np.ones(D)
        F = 4
        self.omega, self.phase = rng.randn(B2, F, D), rng.uniform(0.0, 2.0 * np.pi, size=(B2, F))
        self.w, self.eps = rng.randn(B2, F + 1), rng.randn(B2, N)
        self.ng = np.full(D, 3, dtype=np.int32)
        self.grid = np.ascontiguousarray(np.tile(np.linspace(0.0, 1.0, 3)[:, None], (1, D)))
        self.panels = np.array([[0, -1]], dtype=np.int32)
        self.out = np.empty(B2 * M * (2 + 2 * D))  # the largest output of any call below
        self.out2, self.out3, self.out4 = (np.empty_like(self.out) for _ in range(3))
        self.iout = [np.zeros(B2 * M, dtype=np.int32) for _ in range(3)]


@pytest.fixture(scope="module")
def prob():
    return Problem()


def _consumers(lib, p):
    """name -> (raw call (handle, B) -> code, refuses a context-level warp).  B = 1 or 2 posteriors; an index consumer reads
    posterior B - 1, a list consumer the posteriors 0 .. B - 1."""
    L, _p, nul = lib.load(), lib._p, C.cast(None, lib._dp)
    F = p.omega.shape[1]
    return {
        "bgp_predict_batch": (lambda h, B: L.bgp_predict_batch(h, B, _p(p.Hk), M, _p(p.Xq), _p(p.out), _p(p.out2), nul), False),
        "bgp_acq_batch": (lambda h, B: L.bgp_acq_batch(h, B, _p(p.Hk), M, _p(p.Xq), 0.0, 1.0, 2, _p(p.kinds), _p(p.params), B,
                                                       _p(p.out)), False),
        "bgp_pvrs": (lambda h, B: L.bgp_pvrs(h, _p(p.H), M, _p(p.Xq), 3, _p(p.Xq), _p(p.out)), False),
        "bgp_sample_y": (lambda h, B: L.bgp_sample_y(h, B - 1, _p(p.H[B - 1:]), M, _p(p.Xq), 2, _p(p.z), 1e-6, _p(p.out)), False),
        "bgp_sample_y_batch": (lambda h, B: L.bgp_sample_y_batch(h, B, _p(p.pidx), _p(p.H), M, _p(p.Xq), _p(p.z), 1e-6, _p(p.out),
                                                                 _p(p.iout[0])), False),
        "bgp_fantasy_begin": (lambda h, B: L.bgp_fantasy_begin(h, B, _p(p.Hk), _p(p.noise), M, _p(p.Xq), 0.0, 1.0, 2, _p(p.kinds),
                                                               _p(p.params), B, 2), True),
        "bgp_predict_grad_batch": (lambda h, B: L.bgp_predict_grad_batch(h, B, _p(p.Hk), M, _p(p.Xq), _p(p.out), _p(p.out2),
                                                                         _p(p.out3), _p(p.out4)), True),
        "bgp_minimize_starts": (lambda h, B: L.bgp_minimize_starts(h, B - 1, _p(p.Hk[B - 1:]), 0.0, 1.0, 1.96, 3, _p(p.Xq), _p(p.lo),
                                                                   _p(p.hi), 1e-5, 5, _p(p.out), _p(p.out2), _p(p.out3),
                                                                   _p(p.iout[0]), _p(p.iout[1]), _p(p.iout[2])), True),
        "bgp_paths_begin": (lambda h, B: L.bgp_paths_begin(h, B, _p(p.pidx), _p(p.Hk), _p(p.H[:, -1].copy()), F, _p(p.omega),
                                                           _p(p.phase), _p(p.w), _p(p.eps)), True),
        "bgp_partial_dependence": (lambda h, B: L.bgp_partial_dependence(h, B, _p(p.Hk), M, _p(p.Xq), 3, _p(p.ng), _p(p.grid), 1,
                                                                         _p(p.panels), _p(p.out)), False),
    }


def _answers(lib, p, ctx, B=B2):
    """{consumer: (code, error text of a refusal)} of one round over the table."""
    got = {}
    for name, (call, _) in _consumers(lib, p).items():
        rc = call(ctx._h, B)
        got[name] = (rc, lib.load().bgp_last_error().decode() if rc else "")
        print("ENTRY_STATE %-24s B=%d code %d %s" % (name, B, rc, got[name][1]))
    return got


def _assert_all(got, code, *words):
    for name, (rc, text) in got.items():
        assert rc == code, (name, rc, text)
        for w in (name,) + words if code else ():
            assert w in text, (name, w, text)


def _context(lib, p, build=True):
    ctx = lib.Context(p.X, p.y, p.alpha, max_batch=B2)
    if build:
        assert np.all(ctx.posterior(p.H)["status"] == 0)
    return ctx


# what ends the resident posteriors of a plain build: name -> (call, text every refusal then carries)
def _invalidators(p):
    return {
        "update_data": (lambda ctx: ctx.update_data(p.X, p.y, p.alpha), "resident"),
        "set_warp": (lambda ctx: ctx.set_warp(p.W[0]), "resident"),
        "clear_warp": (lambda ctx: ctx.set_warp(None), "resident"),
        "lml_grad": (lambda ctx: ctx.lml_grad(p.H), "resident"),
        "posterior_warped": (lambda ctx: ctx.posterior(p.H, warps=p.W), "per-row warped"),
    }


def test_nothing_built_every_consumer_answers_state(lib, prob):
    ctx = _context(lib, prob, build=False)
    _assert_all(_answers(lib, prob, ctx), STATE, "resident")
    ctx.close()


@pytest.mark.parametrize("which", ["update_data", "set_warp", "clear_warp", "lml_grad", "posterior_warped"])
def test_every_invalidator_ends_a_plain_build_for_every_consumer(lib, prob, which):
    end, word = _invalidators(prob)[which]
    ctx = _context(lib, prob)
    _assert_all(_answers(lib, prob, ctx), 0)
    end(ctx)
    got = _answers(lib, prob, ctx)
    if which == "set_warp":  # the capability check stands in front of the state check, as it always has
        table = _consumers(lib, prob)
        no_warp = {k: v for k, v in got.items() if table[k][1]}
        got = {k: v for k, v in got.items() if not table[k][1]}
        assert len(no_warp) == 4
        _assert_all(no_warp, INVALID, "warped inputs")
    _assert_all(got, STATE, word)
    if which == "posterior_warped":  # ... and their one reader is served
        ctx.predict_warped(prob.Hk, prob.Xq)
    ctx.close()


def test_pvrs_prepare_leaves_exactly_one_posterior(lib, prob):
    ctx = _context(lib, prob)
    assert ctx.pvrs_prepare(prob.H[:1], False) == 0
    _assert_all(_answers(lib, prob, ctx, B=1), 0)
    got = _answers(lib, prob, ctx, B=2)
    assert got.pop("bgp_pvrs")[0] == 0  # (reads posterior 0 whatever else is there)
    _assert_all(got, STATE, "resident")
    ctx.close()


def test_a_pending_batch_refuses_every_consumer_until_it_is_collected(lib, prob):
    ctx = _context(lib, prob)
    _assert_all(_answers(lib, prob, ctx), 0)
    assert ctx.lml_submit(prob.H)
    _assert_all(_answers(lib, prob, ctx), STATE, "pending")
    ctx.lml_wait()
    _assert_all(_answers(lib, prob, ctx), 0)
    ctx.close()


@pytest.mark.parametrize("which", ["update_data", "set_warp", "clear_warp", "lml_grad", "posterior_warped", "pvrs_prepare"])
def test_an_open_fantasy_run_ends_with_its_posteriors(lib, prob, which):
    p = prob
    end = (lambda ctx: ctx.pvrs_prepare(p.H[:1], False)) if which == "pvrs_prepare" else _invalidators(p)[which][0]
    ctx = _context(lib, p)
    ctx.fantasy_begin(p.Hk, p.noise, p.Xq, 0.0, 1.0, p.kinds, p.params, B2, 2)
    ctx.fantasy_step(0, None)
    end(ctx)
    nxt = np.zeros(1, dtype=np.int32)
    rc = lib.load().bgp_fantasy_step(ctx._h, 1, lib.BGP_LIE_KB, 0.0, lib._p(nxt), C.cast(None, lib._dp))
    assert rc == STATE, lib.load().bgp_last_error().decode()
    ctx.close()


def _fantasy_run(ctx, p):
    """begin at the M candidates + two kriging-believer steps: everything the run gives back."""
    ctx.fantasy_begin(p.Hk, p.noise, p.Xq, 0.0, 1.0, p.kinds, p.params, B2, 2)
    got, nxt = [], 0
    for _ in range(2):
        nxt, vals = ctx.fantasy_step(nxt, None, want_values=True)
        got += [np.array(nxt), vals, *ctx.fantasy_moments()]
    ctx.fantasy_end()
    return got


def test_a_failed_fantasy_begin_leaves_nothing_behind(lib, prob):
    """m = 200 000 candidates with qmax = 199 999 steps: the per-step buffer alone is 2 x 200 192 x 199 999 doubles (640 GB of the
    device's 288), so the state's block is refused behind the starting predict (2 x 200 192 x 128 doubles of cross matrix)."""
    p = prob
    fresh = _context(lib, p)
    want = _fantasy_run(fresh, p)
    fresh.close()
    ctx = _context(lib, p)
    before = ctx.predict(p.Hk, p.Xq)
    big = np.random.RandomState(6).uniform(size=(200_000, D))
    with pytest.raises(lib.BgpError) as err:
        ctx.fantasy_begin(p.Hk, p.noise, big, 0.0, 1.0, p.kinds, p.params, B2, 199_999)
    print("ENTRY_STATE failed begin:", err.value)
    assert "hipMalloc" in str(err.value) and "out of memory" in str(err.value)
    nxt = np.zeros(1, dtype=np.int32)
    rc = lib.load().bgp_fantasy_step(ctx._h, 0, lib.BGP_LIE_KB, 0.0, lib._p(nxt), C.cast(None, lib._dp))
    assert rc == STATE and "no fantasy state" in lib.load().bgp_last_error().decode()
    got = _fantasy_run(ctx, p)
    assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    after = ctx.predict(p.Hk, p.Xq)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    ctx.close()
