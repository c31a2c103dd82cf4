"""Diagonal factorisation and panel solve of a block column in ONE launch (``bgp_set_panel_fused`` / ``BGP_PANEL_FUSED``;
csrc/bgp_chol.hip::panel_kernel) against the separate ``potrf_kernel`` + ``trsm4_kernel`` launches it replaces on the LML path
of the launch schedule: the same code on the same inputs in the same order, so the log-likelihoods, the statuses, the factor
L and z = L^-1 y are the same BITS -- whatever the number of workgroups that share a matrix, on one walker-group stream or
two, with padded rows, generated Gram blocks and a matrix that is not positive definite beside regular ones."""
import numpy as np
import pytest

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
    return X, y, H


def _run(ctx, H, mode, which, streams=1):
    """(lml, status, [tril(L), z] of the slots `which`, fused launches of the call) on the launch schedule with the given mode."""
    ctx.set_persist(0)
    ctx.set_streams(streams)
    ctx.set_panel_fused(mode)
    before = ctx.panel_fused_stats()["launches"]
    lml, status = ctx.lml(H, return_status=True)
    lml, status = lml.copy(), status.copy()
    launched = ctx.panel_fused_stats()["launches"] - before
    fac = []
    for b in which:
        L, z = ctx.debug_workspace(b)
        fac.append((np.tril(L), z.copy()))
    return lml, status, fac, launched


# n, B: what the shape covers
SHAPES = [
    (256, 1),     # one fused column, one row block: the co-workers have no rows
    (256, 3),
    (384, 9),     # B8 = 16
    (640, 8),     # 4, 3, 2, 1 row blocks: odd and even shares
    (300, 5),     # identity padding
    (1536, 8),    # 12 block columns: four-panel groups (eight matrices are too few for the Gram generation: the Gram kernel runs)
    (1536, 32),   # ... and enough matrices for Gram blocks generated inside the trailing update (asserted through gen_stats)
    (384, 64),    # two walker-group streams (set_streams(2))
    (256, 130),   # more matrices than half the CUs: one workgroup per matrix (it writes to dW / dzf like any owner)
]


@pytest.mark.parametrize("n,B", SHAPES)
def test_fused_panel_launch_gives_the_bits_of_the_separate_launches(lib, n, B):
    d = 4
    X, y, H = _problem(n, d, B, 1000 + n + B)
    ctx = lib.Context(X, y, 1e-10, max_batch=B)
    which = range(B) if B <= 16 else [0, 1, B // 2, B - 1]
    streams = 2 if (n, B) == (384, 64) else 1
    gen0 = ctx.gen_stats()["batches"]
    lml0, st0, fac0, launched0 = _run(ctx, H, 0, which, streams)
    lml1, st1, fac1, launched1 = _run(ctx, H, 1, which, streams)
    generated = ctx.gen_stats()["batches"] - gen0
    ctx.close()
    if (n, B) == (1536, 32):
        assert generated == 2  # both calls generated their Gram blocks in the first panel group's updates
    nblk = -(-n // 128)
    assert launched0 == 0
    assert launched1 == (nblk - 1) * streams  # every block column that has a solve, on every stream
    assert np.all(st0 == 0) and np.all(np.isfinite(lml0))
    assert np.array_equal(st1, st0)
    assert np.array_equal(lml1, lml0), "max |difference| %.3e" % np.abs(lml1 - lml0).max()
    for (L0, z0), (L1, z1) in zip(fac0, fac1):
        assert np.all(np.isfinite(L0)) and np.all(np.isfinite(z0))
        assert np.array_equal(L1, L0), "max |difference| of L %.3e" % np.abs(L1 - L0).max()
        assert np.array_equal(z1, z0), "max |difference| of z %.3e" % np.abs(z1 - z0).max()


def test_a_matrix_that_is_not_positive_definite_fails_alone_and_alike(lib):
    """tests/test_gpu_edge.py's singular matrix (a duplicated point, no jitter, no noise: the second pivot is exactly 0) beside three
    regular ones: the same pivot index and -inf in both modes, the others' bits untouched."""
    n, d, B = 384, 2, 4
    X, y, _ = _problem(n, d, B, 66)
    X[1] = X[0]
    good = np.array([0.0, -1.0, -1.1, -3.0])
    bad = np.array([0.0, -1.0, -1.1, -np.inf])
    H = np.array([good, good + 0.1, bad, good - 0.1])
    ctx = lib.Context(X, y, np.zeros(n), max_batch=B)
    ok = [0, 1, 3]
    lml0, st0, fac0, _ = _run(ctx, H, 0, ok)
    lml1, st1, fac1, launched1 = _run(ctx, H, 1, ok)
    ctx.close()
    assert launched1 == 2
    assert list(st0) == [0, 0, 2, 0] and lml0[2] == -np.inf and np.all(np.isfinite(lml0[ok]))
    assert np.array_equal(st1, st0)
    assert np.array_equal(lml1, lml0)
    for (L0, z0), (L1, z1) in zip(fac0, fac1):
        assert np.array_equal(L1, L0) and np.array_equal(z1, z0)


def test_resident_sampler_run_is_the_same_in_both_modes(monkeypatch):
    """The device-resident ensemble sampler enqueues the same launch schedule between its step kernels: 16 walkers at n = 384 for 4
    steps give identical positions and log-probabilities with and without the fused panel launches."""
    import bayes_skopt_amd as bask
    from sklearn.gaussian_process.kernels import WhiteKernel

    n, d, walkers, steps = 384, 3, 16, 4
    rng = np.random.RandomState(4)
    X = rng.uniform(size=(n, d))
    y = np.sin(3 * X.sum(1)) + 0.1 * rng.randn(n)
    monkeypatch.setenv("BGP_PERSIST", "0")  # (read at context creation: the launch schedule, not the launch-free kernel)
    out = []
    for mode in ("0", "1"):
        monkeypatch.setenv("BGP_PANEL_FUSED", mode)
        kernel = bask.construct_default_kernel(list(range(d))) + WhiteKernel(1e-2)
        gp = bask.BayesGPR(kernel=kernel, random_state=11, normalize_y=True, resident_sampler=True)
        gp.kernel_ = kernel.clone_with_theta(kernel.theta)
        gp.noise_ = 1e-2
        gp.sample(X, y, n_desired_samples=walkers * steps, n_burnin=0, n_walkers_per_thread=walkers)
        s = gp._sampler
        assert s.resident_runs == 1
        out.append((s.get_chain().copy(), s.get_log_prob().copy(), gp._ctx.panel_fused_stats()["launches"]))
    assert out[0][2] == 0 and out[1][2] > 0
    assert out[0][0].shape == (steps, walkers, d + 2)
    assert np.array_equal(out[1][0], out[0][0])
    assert np.array_equal(out[1][1], out[0][1])
