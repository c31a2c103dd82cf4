"""The predictive pipeline of csrc/bgp_post.hip -- batched predict and predictive covariance, the acquisition pass, the draws
of sample_y and sample_y_batch, PVRS, the Gram form -- against the extended-precision reference (oracle/hp_oracle.py) at the
tolerances of tests/_precision.py, on the shapes that enter each index branch of the tile kernels behind it (the case lists
say which); tests/test_cpu_precision.py qualifies every case without a GPU (fp64 LAPACK within tol / 10, a single-precision
slip beyond 10 tol).  Every test prints its err / tol (``pytest -s``); lines start with ``PRECISION``."""
import numpy as np
import pytest

import _precision as P

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


def _kernel_H(H, latent):
    """The hyper-vectors the kernel is evaluated with: ``noise_set_to_zero`` takes the white level out, the factors stay."""
    Hk = np.array(H, dtype=np.float64, copy=True)
    Hk[np.asarray(latent, dtype=bool), -1] = -np.inf
    return Hk


def _acq_plan(lib):
    code = {"EI": lib.ACQ_EI, "LCB": lib.ACQ_LCB, "MEAN": lib.ACQ_MEAN, "STD": lib.ACQ_STD}
    return [code[k] for k in P.ACQ_KINDS], P.ACQ_PARAMS


# ------------------------------------------------------------------------------------------------------------------------------
# batched predict, predictive covariance, the acquisition pass
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in P.PREDB_CASES])
def test_batched_predict_covariance_and_acquisitions(lib, cid):
    c = P.ALL[cid]
    X, y, alpha, H, kap = P.problem(cid)
    n, B, Xq = len(X), c["B"], P.query(cid)
    kinds, params = _acq_plan(lib)
    ctx = _ctx(lib, c, X, y, alpha, B)
    assert np.all(ctx.posterior(H)["status"] == 0)
    for nz in (False, True):
        Hk = _kernel_H(H, [nz] * B)
        mean, var = ctx.predict(Hk, Xq)
        cov = None
        if c["cov"]:
            mean_c, var_c, cov = ctx.predict(Hk, Xq, return_cov=True)
            np.testing.assert_array_equal(mean_c, mean)  # the covariance changes the chunking, never the moments
            np.testing.assert_array_equal(var_c, var)
        acq = ctx.acq(Hk, Xq, P.ACQ_Y_MEAN, P.ACQ_Y_STD, kinds, params, c["n_samples"])
        tag = cid + ("_noise0" if nz else "_noise")
        worst = {"mean": 0.0, "var": 0.0, "cov": 0.0}
        for b in range(B):
            pr, pv = P.ref_predict_b(cid, b, nz), P.prior_var(cid, nz, b)
            worst["mean"] = max(worst["mean"], P.err_rel_max(mean[b], pr["mean"], P.mean_scale(cid, b)) / P.tol("mean", kap[b], n))
            worst["var"] = max(worst["var"], P.err_rel_max(var[b], np.maximum(P.f(pr["var"]), 0), pv) / P.tol("var", kap[b], n))
            if cov is not None:
                worst["cov"] = max(worst["cov"], P.err_rel_max(cov[b], pr["cov"], pv) / P.tol("var", kap[b], n))
        _check(tag, c, "mean", worst["mean"], 1.0)
        _check(tag, c, "var", worst["var"], 1.0)
        if cov is not None:
            _check(tag + "_cov", c, "var", worst["cov"], 1.0)
        ra = P.ref_acq(cid, nz)
        assert ra["keep"].all()
        for k, r in enumerate(P.acq_ratio(acq, ra)):
            _check("%s_%s%d" % (tag, P.ACQ_KINDS[k], k), c, "acq", r, 1.0)
    ctx.close()


def test_predict_chunk_loop(lib):
    """1025 posteriors at m = 8192 run as two chunks of the batched predict (1008 + 17 items; the arithmetic is asserted in
    tests/test_cpu_precision.py).  Items on both sides of the cut and the last two equal, bit for bit, a call on posteriors
    rebuilt from their rows alone; three of them meet the long-double reference on the first 64 query rows; the acquisition
    pass of the full call agrees with the closed forms on the moments the same call returned."""
    cid = P.CHUNK_CASE["id"]
    c = P.ALL[cid]
    X, y, alpha, H, kap = P.problem(cid)
    n, Xq = len(X), P.query(cid)
    kinds, params = _acq_plan(lib)
    ctx = _ctx(lib, c, X, y, alpha, c["B"])
    assert np.all(ctx.posterior(H, want_alpha=False)["status"] == 0)
    mean, var = ctx.predict(H, Xq)
    acq = ctx.acq(H, Xq, 0.0, 1.0, kinds, params, c["n_samples"])
    want = ctx.acq_values(mean, np.sqrt(var), kinds, params, c["n_samples"])
    items = c["items"]
    assert np.all(ctx.posterior(H[items], want_alpha=False)["status"] == 0)
    mean_s, var_s = ctx.predict(H[items], Xq)
    ctx.close()
    np.testing.assert_array_equal(mean[items], mean_s)
    np.testing.assert_array_equal(var[items], var_s)
    r = c["ref_rows"]
    for b in c["ref_items"]:
        pr, ms, pv = P.ref_chunk(cid, b)
        _check("%s_item%d" % (cid, b), c, "mean", P.err_rel_max(mean[b, :r], pr["mean"], ms), P.tol("mean", kap[b], n))
        _check("%s_item%d" % (cid, b), c, "var", P.err_rel_max(var[b, :r], pr["var"], pv), P.tol("var", kap[b], n))
    for k, kind in enumerate(P.ACQ_KINDS):
        if kind == "EI":
            np.testing.assert_allclose(acq[k], want[k], rtol=1e-9, atol=1e-300)
        else:
            np.testing.assert_allclose(acq[k], want[k], rtol=1e-13)


# ------------------------------------------------------------------------------------------------------------------------------
# the Gram form
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in P.GRAM_CASES])
def test_gram_form(lib, cid):
    c = P.ALL[cid]
    X, y, alpha, _H, kap = P.problem(cid)
    n, B = len(X), c["B"]
    K, Ks, kss, Kss = (None if c["cov"] is False and j == 3 else np.array([P.gram_inputs(cid, b)[j] for b in range(B)])
                       for j in range(4))
    ctx = _ctx(lib, c, X, y, alpha, B)
    res = ctx.posterior_gram(K, use_alpha=True, want_L=True, want_alpha=True, want_K_inv=True)
    assert np.all(res["status"] == 0)
    out = ctx.predict_gram(Ks, kss, Kss)
    ctx.close()
    worst = {}
    for b in range(B):
        errs = P.gram_errs(cid, b, res["L"][b], res["alpha"][b], res["K_inv"][b], out[0][b], out[1][b],
                           out[2][b] if c["cov"] else None)
        for q, e in errs.items():
            worst[q] = max(worst.get(q, 0.0), e / P.tol("var" if q == "cov" else q, kap[b], n))
    for q, r in worst.items():
        _check(cid + ("_gram_cov" if q == "cov" else "_gram"), c, "var" if q == "cov" else q, r, 1.0)


# ------------------------------------------------------------------------------------------------------------------------------
# PVRS
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in P.PVRSB_CASES])
def test_pvrs(lib, cid):
    c = P.ALL[cid]
    X, _y, alpha, H, _kap = P.problem(cid)
    Xc, Xt = P.pvrs_inputs(cid)
    ctx = _ctx(lib, c, X, np.zeros(len(X)), alpha, 1)
    if c.get("warp"):
        ctx.set_warp(P.warp_params(cid)[0])
    assert ctx.pvrs_prepare(H[0], c["vec_alpha"]) == 0
    covs = ctx.pvrs(H[0], Xc, Xt)
    ctx.close()
    _check(cid, c, "pvrs", P.err_rel_max(covs, P.ref_pvrs(cid)), P.pvrs_tol(cid))


# ------------------------------------------------------------------------------------------------------------------------------
# sample_y and sample_y_batch
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c["id"] for c in P.SAMPLEB_CASES])
def test_sample_y_draw_groups_and_batch(lib, cid):
    """All draws of sample_y on one posterior (groups of 16), then sample_y_batch: item i on resident posterior pidx[i] with
    its own kernel vector and z.  In the isolation case the latent items' covariances are singular (a duplicated query row, no
    jitter) and nothing is asked of them; the regular items have status 0, meet the tolerance and are the same bits as in a
    call that holds them alone.
    ``sampleb_n257_m129`` (kappa(K) 7e4, kappa(cov + jitter) 2e5) is the case that moved the draws' covariance from the
    product with the explicit inverse (16 tol there) to the product with the factor's inverse."""
    c = P.ALL[cid]
    X, y, alpha, H, _kap = P.problem(cid)
    Xq, (zd, zb) = P.sampleb_query(cid), P.sampleb_z(cid)
    pidx, reg = c["pidx"], c["regular"]
    ctx = _ctx(lib, c, X, y, alpha, c["B"])
    assert np.all(ctx.posterior(H)["status"] == 0)
    lines = []
    if c["draws"]:
        out = ctx.sample_y(0, _kernel_H(H[:1], [True])[0], Xq, zd, jitter=c["jitter"])
        ref, t = P.ref_sampleb(cid, 0, True, zd)
        lines.append(("%s_%ddraws" % (cid, c["draws"]), P.err_rel_max(out, ref) / t))
        # per group of 16 draws: a slip in one group cannot hide behind the others' scale
        for r0 in range(0, c["draws"], 16):
            lines.append(("%s_draws%d+" % (cid, r0), P.err_rel_max(out[r0 : r0 + 16], ref[r0 : r0 + 16]) / t))
    Hk = _kernel_H(H[pidx], c["latent"])
    out, st = ctx.sample_y_batch(pidx, Hk, Xq, zb, jitter=c["jitter"])
    if len(reg) < len(pidx):
        alone, st_alone = ctx.sample_y_batch([pidx[i] for i in reg], Hk[reg], Xq, zb[reg], jitter=c["jitter"])
        assert np.all(st_alone == 0)
        np.testing.assert_array_equal(out[reg], alone)
    ctx.close()
    assert np.all(st[reg] == 0), st
    worst = 0.0
    for i in reg:
        ref, t = P.ref_sampleb(cid, pidx[i], c["latent"][i], zb[i : i + 1])
        worst = max(worst, P.err_rel_max(out[i], ref[0]) / t)
    lines.append((cid + "_batch", worst))
    for tag, r in lines:
        _report(tag, c, "sample", r)
    for tag, r in lines:
        assert r <= 1.0, "%s sample: error %.3f tol" % (tag, r)
