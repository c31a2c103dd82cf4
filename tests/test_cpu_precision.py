"""The precision model of tests/_precision.py is right, shown without a GPU on the whole case list of
tests/test_gpu_precision.py, against the extended-precision reference (oracle/hp_oracle.py):

* reachable -- fp64 LAPACK (oracle/gp_oracle.py) lies within tol / 10 of the reference, so a correct fp64 kernel is not
  near the edge and the GPU test cannot be flaky;
* bites -- the same computation with the inputs rounded to fp32, and separately with the Gram entries rounded to fp32,
  misses the reference by at least 10 tol on the LML, alpha and the gradient, so a single-precision slip fails it; so do
  fp32 inputs for the predictive mean and variance, fp32 augmented Gram matrices for PVRS and an fp32 predictive
  covariance for sample_y.
  (Rounding the inputs of a one-point problem changes nothing: that check is skipped at n = 1.)

Fantasy conditioning (FANTASY_CASES) is qualified the same way with the fp64 replica of the device recurrences
(``_precision.fantasy64``) in LAPACK's place: reachable at every step, and fp32 inputs, the dropped sum over the earlier steps
and a fantasy noise without base_alpha each miss by 10 tol.

The batched predictive cases of tests/test_gpu_predictive_precision.py are qualified here as well: PREDB_CASES (mean, variance,
covariance and the averaged acquisitions per item: fp64 reaches, fp32 inputs bite; the acquisition tolerance leaves no candidate
out), the Gram form on two of them (fp32 ``K`` bites), the added PVRS_CASES and SAMPLEB_CASES."""
import numpy as np
import pytest

import _precision as P

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

from oracle import gp_oracle as O  # noqa: E402

MARGIN = 10.0


def _report(name, reach, bite=None):
    print("%-44s reachable err/tol %.2e%s" % (name, reach, "" if bite is None else "   bites err/tol %.1e" % bite))


def test_every_family_reaches_a_ragged_tile_beyond_the_first_block():
    """Each of the eight kernel families runs the LML at three or more sizes, one of them > 128 with a ragged last tile."""
    for st, fm in P.FAMILIES:
        ns = {c["n"] for c in P.LML_CASES if (c["stationary"], c["form"]) == (st, fm)}
        assert len(ns) >= 3 and any(n > 128 and n % 128 for n in ns), (st, fm, sorted(ns))


def test_fantasy_cases_cover_every_family_and_the_device_edges():
    """Every kernel family conditions at least once; a ragged 64-point tile, a ragged 256-candidate block, the staging limit
    d = 32, fewer draws than resident posteriors, both lie kinds, both alpha kinds, six steps, and forced picks at index 0,
    m - 1, in the second 256-block and on a training point all appear."""
    cs = P.FANTASY_CASES
    assert {(c["stationary"], c["form"]) for c in cs} == set(P.FAMILIES)
    assert any(c["n"] % 64 for c in cs) and any(c["m"] % 256 for c in cs) and any(c["d"] == 32 for c in cs)
    assert {1, 63, 64, 65, 129, 257} <= {c["n"] for c in cs} and {2, 255, 256, 257, 513} <= {c["m"] for c in cs}
    assert {1, 17, 31, 32} <= {c["d"] for c in cs} and {1, 3} <= {c["Bf"] for c in cs}
    assert any(c["Bf"] < c["B"] for c in cs) and {c["kb"] for c in cs} == {False, True}
    assert {c["vec_alpha"] for c in cs} == {False, True} and max(len(c["picks"]) for c in cs) == 6
    assert any(c["base_alpha"] >= 1e-3 and not c["kb"] for c in cs)
    for c in cs:
        assert len(set(c["picks"])) == len(c["picks"]) < c["m"] and all(0 <= p < c["m"] for p in c["picks"])
    assert any(0 in c["picks"] for c in cs) and any(c["m"] - 1 in c["picks"] for c in cs)
    assert any(256 <= p for c in cs for p in c["picks"]) and any(c["twin"] is not None for c in cs)


def test_predictive_cases_cover_every_family_and_the_tile_kernels_index_branches():
    """From the case dicts alone: all eight families; a query set padded beyond 512 with fewer than 8 items (row tiles split
    over the XCDs); exactly 8 and more than 8 items (item -> XCD pinning); a training set padded beyond 512 (column panels);
    n and m both multiples of 128 (check-free epilogue); d on both sides of the 16-dimension staging passes; more than 16 and
    more than 32 draws (draw groups); a non-identity item -> posterior map with a repeat; more than 128 Thompson points and
    more than 512 candidates."""
    pad = lambda v: -(-v // 128) * 128  # noqa: E731
    pb, sb, pv = P.PREDB_CASES, P.SAMPLEB_CASES, P.PVRSB_CASES
    assert {(c["stationary"], c["form"]) for c in pb + sb + pv} == set(P.FAMILIES)
    assert any(pad(c["m"]) > 512 and c["B"] < 8 for c in pb)
    assert any(c["B"] == 8 for c in pb) and any(c["B"] > 8 for c in pb)
    assert any(pad(c["n"]) > 512 for c in pb)
    assert any(c["n"] % 128 == 0 and c["m"] % 128 == 0 for c in pb)
    assert {16, 17, 32, 33} <= {c["d"] for c in pb}
    assert any(c["n"] == 1 for c in pb) and any(c["m"] == 1 for c in pb)
    assert sum(c["n_samples"] != c["B"] for c in pb) >= 2
    assert any(pad(c["m"]) > 512 and c["cov"] for c in pb) and any(pad(c["n"]) > 512 and c["cov"] for c in pb)
    assert any(16 < c["draws"] <= 32 for c in sb) and any(c["draws"] > 32 for c in sb)
    assert any(c["pidx"] != list(range(len(c["pidx"]))) and len(set(c["pidx"])) < len(c["pidx"]) for c in sb)
    assert any(pad(c["m"]) > 512 for c in sb) and all(c["d"] == 2 for c in sb)
    assert all(c["jitter"] in (0.0, P.SAMPLE_JITTER) and max(c["pidx"]) < c["B"] for c in sb)
    assert any(c["dup_query"] and c["jitter"] == 0.0 and sum(c["latent"]) == 3 and len(c["regular"]) == 2 for c in sb)
    assert any(c["nt"] > 128 for c in pv) and any(c["nc"] > 512 for c in pv)
    assert any(c["nc"] == 1 for c in pv) and any(c.get("tp_is_cand") for c in pv) and any(c.get("warp") for c in pv)
    assert {c["id"] for c in P.GRAM_CASES} == {pb[1]["id"], pb[4]["id"]}
    ck = P.CHUNK_CASE  # two chunks of the 2^30-double scratch budget (multiples of 8 items), compared on both sides of the cut
    # (csrc/bgp_post.hip, predict_run: post_chunk(B, sKs + 2 mpad, 1 << 30, round to eights) -- keep in step with it)
    per_item = pad(ck["m"]) * (pad(ck["n"]) + 2)
    chunk = ((1 << 30) // per_item) & ~7
    assert chunk < ck["B"] <= 2 * chunk and {0, chunk - 1, chunk, ck["B"] - 1} <= set(ck["items"]) >= set(ck["ref_items"])


def test_chunk_case_reference_is_reachable():
    """The three items of the chunk case that meet the long-double reference on the device: fp64 LAPACK is within tol / 10,
    fp32 inputs miss by 10 tol."""
    cid = P.CHUNK_CASE["id"]
    c = P.ALL[cid]
    X, y, alpha, H, kap = P.problem(cid)
    n, Xq = len(X), P.query(cid)[: c["ref_rows"]]
    ad = np.broadcast_to(alpha, (n,))
    reach, bite = 0.0, np.inf
    for b in c["ref_items"]:
        pr, ms, pv = P.ref_chunk(cid, b)
        for slip in (False, True):
            m64, s64 = O.predict(P.to32(X) if slip else X, y, ad, H[b], P.to32(Xq) if slip else Xq, c["stationary"], c["form"])
            r = (P.err_rel_max(m64, pr["mean"], ms) / P.tol("mean", kap[b], n),
                 P.err_rel_max(s64**2, pr["var"], pv) / P.tol("var", kap[b], n))
            reach, bite = (reach, min(bite, *r)) if slip else (max(reach, *r), bite)
    _report(cid, reach, bite)
    assert reach <= 1 / MARGIN and bite >= MARGIN, (reach, bite)


def _moments64(cid, X, Xq, nz, y_mean=0.0, y_std=1.0):
    """fp64 (LAPACK) mean, std, cov per item of a batched case."""
    c = P.ALL[cid]
    _X, y, alpha, H, _ = P.problem(cid)
    ad = np.broadcast_to(alpha, (len(X),))
    res = [O.predict(X, y, ad, H[b], Xq, c["stationary"], c["form"], noise_zero=nz, y_mean=y_mean, y_std=y_std,
                     return_cov=c["cov"]) for b in range(c["B"])]
    return [np.array([r[j] for r in res]) for j in range(3 if c["cov"] else 2)]


@pytest.mark.parametrize("cid", [c["id"] for c in P.PREDB_CASES])
def test_batched_predict_and_acquisitions(cid):
    """Reach: the worst item, noise setting and (for acq) acquisition.  Bite of fp32 inputs: the LEAST-moved item, noise setting
    and acquisition -- every line the device test prints would miss by 10 tol."""
    c = P.ALL[cid]
    X, _y, _alpha, _H, kap = P.problem(cid)
    n, B, Xq = len(X), c["B"], P.query(cid)
    reach, bite = {"mean": 0.0, "var": 0.0, "acq": 0.0}, {"mean": np.inf, "var": np.inf, "acq": np.inf}
    for nz in (False, True):
        got = _moments64(cid, X, Xq, nz)
        m32, s32 = _moments64(cid, P.to32(X), P.to32(Xq), nz)[:2]  # the slip: the inputs rounded to fp32
        for b in range(B):
            pr, pv, ms = P.ref_predict_b(cid, b, nz), P.prior_var(cid, nz, b), P.mean_scale(cid, b)
            tm, tv, var_ref = P.tol("mean", kap[b], n), P.tol("var", kap[b], n), np.maximum(P.f(pr["var"]), 0)
            reach["mean"] = max(reach["mean"], P.err_rel_max(got[0][b], pr["mean"], ms) / tm)
            ev = P.err_rel_max(got[1][b] ** 2, var_ref, pv)
            if c["cov"]:
                ev = max(ev, P.err_rel_max(got[2][b], pr["cov"], pv))
            reach["var"] = max(reach["var"], ev / tv)
            bite["mean"] = min(bite["mean"], P.err_rel_max(m32[b], pr["mean"], ms) / tm)
            bite["var"] = min(bite["var"], P.err_rel_max(s32[b] ** 2, var_ref, pv) / tv)
        # the acquisition pass: the tolerance leaves no candidate out (from the reference alone), fp64 reaches it
        ra = P.ref_acq(cid, nz)
        assert ra["keep"].all(), (cid, nz, int((~ra["keep"]).sum()))
        mu, sd = _moments64(cid, X, Xq, nz, P.ACQ_Y_MEAN, P.ACQ_Y_STD)[:2]
        reach["acq"] = max(reach["acq"], P.acq_ratio(P.acq64(mu, sd, c["n_samples"]), ra).max())
        mu32, sd32 = _moments64(cid, P.to32(X), P.to32(Xq), nz, P.ACQ_Y_MEAN, P.ACQ_Y_STD)[:2]
        bite["acq"] = min(bite["acq"], P.acq_ratio(P.acq64(mu32, sd32, c["n_samples"]), ra).min())
    for q in reach:
        _report("%s %s" % (cid, q), reach[q], bite[q])
    assert max(reach.values()) <= 1 / MARGIN, (cid, reach)
    assert min(bite.values()) >= MARGIN, (cid, bite)


@pytest.mark.parametrize("cid", [c["id"] for c in P.GRAM_CASES])
def test_gram_form(cid):
    """posterior_gram / predict_gram: fp64 LAPACK from the fp64 matrices the device is handed reaches the long-double
    computation from the same matrices; ``K`` rounded to fp32 misses it."""
    from scipy.linalg import cho_solve, cholesky

    c = P.ALL[cid]
    X, y, alpha, _H, kap = P.problem(cid)
    n = len(X)
    reach, bite = 0.0, np.inf
    for b in range(c["B"]):
        K, Ks, kss, Kss = P.gram_inputs(cid, b)
        for K_used in (K, P.to32(K)):
            Kd = K_used.copy()
            Kd[np.diag_indices_from(Kd)] += alpha
            L = cholesky(Kd, lower=True, check_finite=False)
            a = cho_solve((L, True), y, check_finite=False)
            Ki = cho_solve((L, True), np.eye(n), check_finite=False)
            V = cho_solve((L, True), Ks.T, check_finite=False)
            errs = P.gram_errs(cid, b, L, a, Ki, Ks @ a, kss - np.einsum("ij,ji->i", Ks, V), None if Kss is None else Kss - Ks @ V)
            r = {q: e / P.tol("var" if q == "cov" else q, kap[b], n) for q, e in errs.items()}
            if K_used is K:
                reach = max(reach, max(r.values()))
            else:
                bite = min(bite, min(r.values()))
    _report(cid + " gram", reach, bite)
    assert reach <= 1 / MARGIN and bite >= MARGIN, (cid, reach, bite)


@pytest.mark.parametrize("cid", [c["id"] for c in P.SAMPLEB_CASES])
def test_sample_y_draw_groups_and_batch(cid):
    """The draws of sample_y on posterior 0 and every compared item of sample_y_batch: fp64 reaches, an fp32 predictive
    covariance bites."""
    from scipy.linalg import solve_triangular

    c = P.ALL[cid]
    X, y, alpha, H, _kap = P.problem(cid)
    Xq, (zd, zb) = P.sampleb_query(cid), P.sampleb_z(cid)
    eye = np.eye(len(Xq))
    jobs = ([(0, True, zd)] if c["draws"] else []) + [(c["pidx"][i], c["latent"][i], zb[i : i + 1]) for i in c["regular"]]
    reach, bite, form = 0.0, np.inf, {"fac": 0.0, "inv": 0.0}
    for b, latent, z in jobs:
        ad = np.broadcast_to(alpha, (len(X),))
        mean, _s, cov = O.predict(X, y, ad, H[b], Xq, c["stationary"], c["form"], noise_zero=latent, return_cov=True)
        ref, t = P.ref_sampleb(cid, b, latent, z)
        reach = max(reach, P.err_rel_max(mean[None, :] + z @ np.linalg.cholesky(cov + c["jitter"] * eye).T, ref) / t)
        L32 = np.linalg.cholesky(P.to32(cov) + c["jitter"] * eye)
        bite = min(bite, P.err_rel_max(mean[None, :] + z @ L32.T, ref) / t)
        # the device's formulation in fp64 numpy, cov = K_** - V V^T with V = K_* L^-T from the explicit inverse of the factor:
        # within tol / 10 as well; and the one it replaced, the product with the explicit K^-1 (printed: it misses)
        hk = H[b].copy()
        if latent:
            hk[-1] = -np.inf
        Ks = O.kernel_matrix(Xq, hk, c["stationary"], c["form"], Y=X)
        Kss = O.kernel_matrix(Xq, hk, c["stationary"], c["form"])
        L, Ki, _a = O.posterior(X, y, ad, H[b], c["stationary"], c["form"])
        V = Ks @ solve_triangular(L, np.eye(len(X)), lower=True, check_finite=False).T
        for name, cv in (("fac", Kss - V @ V.T), ("inv", Kss - (Ks @ Ki) @ Ks.T)):
            form[name] = max(form[name], P.err_rel_max(mean[None, :] + z @ np.linalg.cholesky(cv + c["jitter"] * eye).T, ref) / t)
    _report(cid, reach, bite)
    print("%-44s in fp64 with L^-1 err/tol %.2e   with K^-1 err/tol %.2e" % (cid, form["fac"], form["inv"]))
    assert reach <= 1 / MARGIN and form["fac"] <= 1 / MARGIN and bite >= MARGIN, (cid, reach, form, bite)


@pytest.mark.parametrize("cid", [c["id"] for c in P.FANTASY_CASES])
def test_fantasy_conditioning(cid):
    c = P.ALL[cid]
    X, y, alpha, H, _kap = P.problem(cid)
    Xc, picks, lies = P.fantasy_inputs(cid)
    n, st, fm, ba = len(X), c["stationary"], c["form"], c["base_alpha"]
    worst_reach, worst_bite = 0.0, np.inf
    for b in range(c["Bf"]):
        ref = P.ref_fantasy(cid, b)
        args = (y, alpha, H[b], Xc, picks, lies, ba, st, fm)
        mean, var = P.fantasy64(X, *args)
        slips = {"fp32 inputs": P.fantasy64(P.to32(X), y, alpha, H[b], P.to32(Xc), picks, lies, ba, st, fm),
                 "no sum over the earlier steps": P.fantasy64(X, *args, drop_prev=True)}
        if ba >= 1e-3:
            slips["noise without base_alpha"] = P.fantasy64(X, *args, noise=float(np.exp(H[b, -1])))
        for j in range(len(picks)):
            tols = (P.tol("fant_mean", ref["kappa"][j], n + j), P.tol("fant_var", ref["kappa"][j], n + j))
            errs = P.fantasy_errs(mean[j], var[j], ref, j)
            r = max(e / t for e, t in zip(errs, tols))
            assert r <= 1 / MARGIN, (cid, b, j, errs, tols)
            worst_reach = max(worst_reach, r)
            for name, (ms, vs) in slips.items():
                if name.startswith("no sum") and j == 0:
                    continue  # (the first step has no earlier one)
                bm, bv = (e / t for e, t in zip(P.fantasy_errs(ms[j], vs[j], ref, j), tols))
                # (the kriging believer leaves the means alone: only fp32 inputs reach them)
                bite = bv if c["kb"] and not name.startswith("fp32") else min(bm, bv)
                assert bite >= MARGIN, (cid, b, j, name, bm, bv)
                worst_bite = min(worst_bite, bite)
    _report(cid, worst_reach, worst_bite)


@pytest.mark.parametrize("cid", [c["id"] for c in P.LML_CASES + P.SCHED_CASES])
def test_lml_and_alpha(cid):
    c = P.ALL[cid]
    X, y, alpha, H, kap = P.problem(cid)
    n, st, fm = len(X), c["stationary"], c["form"]
    ad = np.broadcast_to(alpha, (n,))
    worst_reach, worst_bite = 0.0, np.inf
    for b in range(len(H)):
        ref = P.ref_lml(cid, b)
        tl, ta = P.tol("lml", kap[b], n), P.tol("alpha", kap[b], n)
        K = O.gram_with_jitter(X, ad, H[b], st, fm)
        v, a, _ = P.lml64(K, y)
        r = max(P.err_lml(v, ref) / tl, P.err_alpha(a, ref) / ta)
        assert r <= 1 / MARGIN, (cid, b, P.err_lml(v, ref), tl, P.err_alpha(a, ref), ta)
        np.testing.assert_allclose(v, O.lml(X, y, ad, H[b], st, fm), rtol=1e-15, atol=0)  # (the same fp64 computation)
        slips = [K.astype(np.float32).astype(np.float64)]
        if n > 1:
            slips.append(O.gram_with_jitter(P.to32(X), ad, H[b], st, fm))
        for Ks in slips:
            vs, as_, _ = P.lml64(Ks, y)
            bl, ba = P.err_lml(vs, ref) / tl, P.err_alpha(as_, ref) / ta
            assert bl >= MARGIN and ba >= MARGIN, (cid, b, bl, ba)
            worst_bite = min(worst_bite, bl, ba)
        worst_reach = max(worst_reach, r)
    _report(cid, worst_reach, worst_bite)


@pytest.mark.parametrize("cid", [c["id"] for c in P.GRAD_CASES])
def test_gradient(cid):
    c = P.ALL[cid]
    X, y, alpha, H, kap = P.problem(cid)
    n, st, fm = len(X), c["stationary"], c["form"]
    ad = np.broadcast_to(alpha, (n,))
    worst_reach, worst_bite = 0.0, np.inf
    for b in range(min(len(H), 2)):
        ref = P.ref_grad(cid, b)
        tg = P.tol("grad", kap[b], n)
        v, g = O.lml_and_grad(X, y, ad, H[b], st, fm)
        r = P.err_grad(g, ref) / tg
        assert r <= 1 / MARGIN, (cid, b, P.err_grad(g, ref), tg)
        assert P.err_lml(v, ref) <= P.tol("lml", kap[b], n) / MARGIN
        K = O.gram_with_jitter(X, ad, H[b], st, fm)
        slips = [P.grad64(P.to32(K), y, X, H[b], st, fm)]
        if n > 1:
            slips.append(P.grad64(O.gram_with_jitter(P.to32(X), ad, H[b], st, fm), y, P.to32(X), H[b], st, fm))
        for gs in slips:
            bg = P.err_grad(gs, ref) / tg
            assert bg >= MARGIN, (cid, b, bg)
            worst_bite = min(worst_bite, bg)
        worst_reach = max(worst_reach, r)
    _report(cid, worst_reach, worst_bite)


@pytest.mark.parametrize("cid", [c["id"] for c in P.POST_CASES])
def test_posterior_and_predict(cid):
    c = P.ALL[cid]
    X, y, alpha, H, kap = P.problem(cid)
    n, st, fm, k = len(X), c["stationary"], c["form"], kap[0]
    ad = np.broadcast_to(alpha, (n,))
    ref = P.ref_post(cid)
    L, Ki, a = O.posterior(X, y, ad, H[0], st, fm)
    errs = {"L": P.err_L(L, ref), "alpha": P.err_alpha(a, ref), "K_inv": P.err_K_inv(Ki, ref["K_inv"])}
    Xq = P.query(cid)
    for nz in (False, True):
        pr = P.ref_predict(cid, nz)
        mo, so, co = O.predict(X, y, ad, H[0], Xq, st, fm, noise_zero=nz, return_cov=True)
        pv = P.prior_var(cid, nz)
        errs["mean"] = max(errs.get("mean", 0), P.err_rel_max(mo, pr["mean"], P.mean_scale(cid)))
        errs["var"] = max(errs.get("var", 0), P.err_rel_max(so**2, np.maximum(P.f(pr["var"]), 0), pv),
                          P.err_rel_max(co, pr["cov"], pv))
    worst = max(e / P.tol(q, k, n) for q, e in errs.items())
    assert worst <= 1 / MARGIN, (cid, {q: (e, P.tol(q, k, n)) for q, e in errs.items()})
    # bites: the inputs rounded to fp32 move the mean and the variance by >= 10 tol
    pr = P.ref_predict(cid, False)
    m32, s32 = O.predict(P.to32(X), y, ad, H[0], P.to32(Xq), st, fm)
    bite = min(P.err_rel_max(m32, pr["mean"], P.mean_scale(cid)) / P.tol("mean", k, n),
               P.err_rel_max(s32**2, pr["var"], P.prior_var(cid, False)) / P.tol("var", k, n))
    assert bite >= MARGIN, (cid, bite)
    _report(cid, worst, bite)


@pytest.mark.parametrize("cid", [c["id"] for c in P.WARP_CASES])
def test_warped_lml(cid):
    c = P.ALL[cid]
    X, y, alpha, H, _ = P.problem(cid)
    Xw, W, kap = P.warped_problem(cid)
    n, st, fm = len(X), c["stationary"], c["form"]
    ad = np.broadcast_to(alpha, (n,))
    worst = 0.0
    for b in range(len(H)):
        ref = hp.lml(Xw[b], y, alpha, H[b], st, fm)
        v = O.lml_warped(X, y, ad, H[b], W[b], st, fm)
        sens = P.err_lml(O.lml(P.to32(P.f(Xw[b])), y, ad, H[b], st, fm), ref) / P.F32
        t = P.tol("lml", kap[b], n, sens)
        worst = max(worst, P.err_lml(v, ref) / t)
        assert P.err_lml(v, ref) <= t / MARGIN, (cid, b, P.err_lml(v, ref), t)
        assert P.err_lml(O.lml_warped(P.to32(X), y, ad, H[b], W[b], st, fm), ref) >= MARGIN * t
    # context-level warp: posterior alpha and predict on warped inputs (scipy's Beta CDF in fp64)
    sw = P.ref_set_warp(cid)
    Xw64, Xqw64 = O.warp_inputs(X, sw["W"]), O.warp_inputs(P.query(cid), sw["W"])
    m64, s64 = O.predict(Xw64, y, ad, H[0], Xqw64, st, fm)
    got = {"alpha": O.posterior(Xw64, y, ad, H[0], st, fm)[2], "mean": m64, "var": s64**2}
    for q in ("alpha", "mean", "var"):
        t = P.tol(q, sw["kappa"], n, sw["sens"][q])
        e = P.err_rel_max(got[q], sw["ref"][q], sw["scale"][q])
        assert e <= t / MARGIN, (cid, q, e, t)
        worst = max(worst, e / t)
    _report(cid, worst)


@pytest.mark.parametrize("cid", [c["id"] for c in P.PVRS_CASES + P.PVRSB_CASES])
def test_pvrs(cid):
    c = P.ALL[cid]
    X, _y, alpha, H, kap = P.problem(cid)
    Xc, Xt = P.pvrs_inputs(cid)
    if c.get("warp"):  # (scipy's Beta CDF in fp64, as the context-level warp of test_warped_lml)
        X, Xc, Xt = (O.warp_inputs(A, P.warp_params(cid)[0]) for A in (X, Xc, Xt))
    got = O.pvrs_covs(X, alpha if c["vec_alpha"] else None, H[0], Xc, Xt, c["stationary"], c["form"])
    ref = P.ref_pvrs(cid)
    t = P.pvrs_tol(cid)
    e = P.err_rel_max(got, ref) / t
    assert e <= 1 / MARGIN
    got32 = P.pvrs_gram32(X, alpha if c["vec_alpha"] else None, H[0], Xc, Xt, c["stationary"], c["form"])
    bite = P.err_rel_max(got32, ref) / t
    assert bite >= MARGIN, (cid, bite)
    _report(cid, e, bite)


@pytest.mark.parametrize("cid", [c["id"] for c in P.SAMPLE_CASES])
def test_sample_y(cid):
    c = P.ALL[cid]
    X, y, alpha, H, kap = P.problem(cid)
    Xq, z = P.query(cid), P.sample_z(cid)
    mean, _s, cov = O.predict(X, y, np.broadcast_to(alpha, (len(X),)), H[0], Xq, c["stationary"], c["form"],
                              noise_zero=True, return_cov=True)
    Lc = np.linalg.cholesky(cov + P.SAMPLE_JITTER * np.eye(len(Xq)))
    got = mean[None, :] + z @ Lc.T
    t = P.tol("sample", P.sample_kappa(cid), len(X))
    e = P.err_rel_max(got, P.ref_sample(cid)) / t
    assert e <= 1 / MARGIN
    # bites: the predictive covariance rounded to fp32 before its factorisation
    C32 = P.to32(cov) + P.SAMPLE_JITTER * np.eye(len(Xq))
    bite = P.err_rel_max(mean[None, :] + z @ np.linalg.cholesky(C32).T, P.ref_sample(cid)) / t
    assert bite >= MARGIN, (cid, bite)
    _report(cid, e, bite)
