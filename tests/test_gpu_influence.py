"""Case-deletion influence on the device (``bgp_influence``) through ``_lib.Context`` on the cases of
tests/_inflref.py: every output against the long-double refit, the bit-for-bit invariants, the ``v <= 0`` rule, the guards, and one
run through the public interface.  Lines printed with ``pytest -s`` start with ``PRECISION``."""
import numpy as np
import pytest

import _chunkcases as CC
import _inflref as R

pytestmark = pytest.mark.gpu

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

ERR_INVALID, ERR_STATE = 1, 4  # include/bgp.h
BITS, CHUNKS = "infl6_n257_m65_d1_matern32_sum_B3", "infl7_n257_m257_d17_matern52_sum_B1"


@pytest.fixture(scope="module")
def bask():
    import bayes_skopt_amd as bask

    assert bask._lib.device_count() >= 1
    return bask


def _hk(H):
    return np.column_stack([np.asarray(H, dtype=np.float64)[:, :-1], np.full(len(H), -np.inf)])


def _ctx(bask, X, y, alpha, H, family, build=True):
    ctx = bask._lib.Context(X, y, alpha, form=family[1], stationary=family[0], max_batch=len(H))
    assert not build or np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)
    return ctx


_case_ctx = lambda bask, cid, build=True: _ctx(bask, *R.problem(cid)[:4], R.ALL[cid]["family"], build)  # noqa: E731


def _call(ctx, cid, rows=None):
    H, _k, Xq, noise = R.problem(cid)[3:]
    rows = slice(0, R.ALL[cid]["Bq"]) if rows is None else rows
    return ctx.influence(_hk(H[rows]), noise[rows], Xq, R.ALL[cid]["n_focus"])


@pytest.mark.parametrize("cid", R.CIDS)
def test_every_output_matches_the_refit(bask, cid):
    ctx = _case_ctx(bask, cid)
    try:
        got = _call(ctx, cid)
    finally:
        ctx.close()
    assert not got["status"].any()
    for b in range(R.ALL[cid]["Bq"]):
        ratios = R.errs_over_tol(cid, b, {k: v[b] for k, v in got.items()}, "device")
        assert max(ratios.values()) <= 1.0, ratios


def test_same_bits_alone_in_a_batch_on_a_repeat_and_under_forced_chunks(bask, monkeypatch):
    H = R.problem(BITS)[3]
    ctx = _case_ctx(bask, BITS)
    try:
        first = _call(ctx, BITS)
        CC.assert_same_bits(_call(ctx, BITS), first, "repeat")
        for b in range(3):  # (posterior b alone: the only resident one)
            assert np.all(ctx.posterior(H[b : b + 1], want_alpha=False)["status"] == 0)
            CC.assert_same_bits(_call(ctx, BITS, slice(b, b + 1)), {k: v[b : b + 1] for k, v in first.items()}, "B = 1, b = %d" % b)
    finally:
        ctx.close()
    CC.default_then_forced(monkeypatch, lambda: _case_ctx(bask, CHUNKS), lambda c: _call(c, CHUNKS), {CC.ROW: 128},
                           (1, CC.row_chunks(R.ALL[CHUNKS]["m"], 128)))
    CC.default_then_forced(monkeypatch, lambda: _case_ctx(bask, BITS), lambda c: _call(c, BITS), {CC.ITEM: 2, CC.ROW: 128},
                           (CC.item_chunks(3, 2), 1))


def test_a_row_without_variance_gives_nothing_to_cook_and_kl(bask):
    X, y, alpha, H, Xq = R.zero_variance_problem()
    ctx = _ctx(bask, X, y, alpha, H, ("rbf", "product"))
    try:
        var = ctx.predict(_hk(H), Xq)[1][0]
        assert var[0] == 0.0 and var[1] > 0.0  # (the device's own clamped variance: the rule is reached)
        both, far = ctx.influence(_hk(H), [0.0], Xq), ctx.influence(_hk(H), [0.0], Xq[1:])  # (row 0 adds exact zeros: far's bits)
    finally:
        ctx.close()
    assert both["sum_cook"][0, 0] == far["sum_cook"][0, 0] > 0.0 and both["sum_kl"][0, 0] == far["sum_kl"][0, 0] > 0.0
    assert both["sum_dm2"][0, 0] > far["sum_dm2"][0, 0] and not both["status"].any()


def test_guards_refuse_before_any_launch(bask):
    H, _k, Xq, noise = R.problem(BITS)[3:]
    def refused(fn, code, match):
        with pytest.raises(bask._lib.BgpError, match=match) as e:
            fn()
        assert "(code %d)" % code in str(e.value)

    ctx = _case_ctx(bask, BITS, build=False)
    try:
        refused(lambda: _call(ctx, BITS), ERR_STATE, "bgp_influence.*resident")
        assert np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)
        first = _call(ctx, BITS)
        refused(lambda: ctx.influence(_hk(H), noise, Xq, len(Xq) + 1), ERR_INVALID, "bgp_influence")
        refused(lambda: ctx.influence(_hk(H), noise, Xq[:0], 0), ERR_INVALID, "bgp_influence")
        CC.assert_same_bits(_call(ctx, BITS), first, "after the refusals")
        ctx.set_warp(np.zeros(2))
        refused(lambda: _call(ctx, BITS), ERR_INVALID, "warped inputs")
    finally:
        ctx.close()
    X33 = np.random.RandomState(33).uniform(size=(8, 33))
    h33 = np.concatenate([[0.0], np.zeros(33), [np.log(1e-2)]])[None, :]
    big = _ctx(bask, X33, X33[:, 0], 1e-6, h33, ("matern52", "product"))
    try:
        refused(lambda: big.influence(_hk(h33), [1e-2], X33[:2], 0), ERR_INVALID, "d > 32")
    finally:
        big.close()


def _told(bask, warp):
    rng = np.random.RandomState(5)
    opt = bask.Optimizer([(0.0, 1.0), (0.0, 1.0)], n_points=60, n_initial_points=10, random_state=3,
                         gp_kwargs=dict(warp_inputs=True) if warp else None)
    X, y = rng.uniform(size=(20, 2)), 0.05 * rng.randn(20)
    y += np.sin(3.0 * X.sum(axis=1)) + 10.0 * np.sin(3.0 * X.sum(axis=1)).std() * (np.arange(20) == 7)
    opt.tell(X.tolist(), y.tolist(), gp_burnin=20, gp_samples=20, n_samples=0, progress=False)
    return opt


def test_the_public_interface_ranks_a_shifted_observation_first(bask, capfd):
    from bayes_skopt_amd import influence, utils

    keys = ("rms", "cook", "kl", "max_abs", "arg_max", "dmean_focus", "dstd_focus", "focus_z")
    opt = _told(bask, warp=False)
    out = opt.influence(n_samples=256, random_state=1)
    assert out["path"] == "device" and out["ranking"][0] == 7 and out["cook"].shape == (20,) and out["dmean_focus"].shape == (1, 20)
    again = utils.influence(opt._result(), n_samples=256, random_state=1)
    CC.assert_same_bits({k: again[k] for k in keys}, {k: out[k] for k in keys})
    # the median GP against its theta given twice as chain rows (batched build, weighted average, band): the focus sd is latent on both
    gp, F, Xr = opt.gp, np.array([[0.3, 0.6]]), np.random.RandomState(2).uniform(size=(64, 2))
    one, two = gp.influence(Xr, focus=F), gp.influence(Xr, focus=F, thetas=np.stack([gp._post_theta] * 2), weights=[1.0, 3.0])
    for k in keys:
        assert np.allclose(two[k], one[k], rtol=1e-9, atol=0), k
        assert k == "arg_max" or np.allclose(two["band"][k][0], one[k], rtol=1e-9, atol=0)
    with gp.noise_set_to_zero():
        sd = gp.predict(F, return_std=True)[1]
    assert np.allclose(one["focus_z"] * sd, one["dmean_focus"], rtol=1e-9, atol=0) and np.all(one["dstd_focus"] >= 0.0)
    capfd.readouterr()
    gp = _told(bask, warp=True).gp
    got, path = gp.influence(Xr, return_path=True)
    gp.influence(Xr)
    assert path == "host" and capfd.readouterr().err.count("influence: numpy on the downloaded inverse") == 1
    k = bask._posterior._with_white_zeroed(gp.kernel_)  # (the latent function: no white level in K_* or the prior variance)
    Ks = k(gp.warp(Xr), gp.X_train_)
    var = np.maximum(k.diag(gp.warp(Xr)) - np.einsum("ij,jk,ik->i", Ks, gp.K_inv_, Ks), 0.0)
    noise = gp._fantasy_base_alpha() + float(np.exp(gp._canonical(gp._post_theta)[0, -1]))
    want = influence.influence_values(Ks, gp.K_inv_, gp.alpha_, var, noise)
    assert np.allclose(got["cook"], want["sum_cook"] / 64, rtol=1e-9, atol=0) and np.allclose(
        got["rms"], np.sqrt(want["sum_dm2"] / 64) * gp._y_scale()[1], rtol=1e-9, atol=0)
