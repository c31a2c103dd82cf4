"""The host loops that cut a call of a resident-posterior entry point into chunks because a scratch budget says so (DESIGN.md
section 27): ``bgp_cond_run`` behind knowledge gradient and joint entropy search, ``gcov_run``, ``predict_run`` (predict, the
per-row-warped predict, the acquisition pass, the mixture), ``bgp_predict_batch_gram``, ``bgp_sample_y_batch``,
``bgp_predict_grad_batch``, ``bgp_paths_eval`` and ``bgp_paths_minimize``.  Their budgets are 2^24 .. 2^30 doubles: the second
iteration of a loop -- base pointers advanced by a chunk -- runs only at production sizes.  ``BGP_ITEM_CHUNK`` (posteriors per
chunk) and ``BGP_ROW_CHUNK`` (query rows / starts per chunk) bound a chunk from above, so the second and third iterations run at
n <= 257, B <= 17, m <= 600.

Every test: the call on a fresh context with the switches unset -- ``bgp_chunk_stats`` must report ONE chunk -- then on another
fresh context with a switch set -- it must report the chunk count worked out here from the case's numbers -- and every output,
integer outputs and NaN patterns included, must be the same bits.  Items and rows are independent by construction (each entry
point has an "alone and in a crowd" test of its own), so equality is the assertion, not a tolerance.  The cases are those of the
features' own lists (tests/_kgref.py, _jesref.py, _gcovref.py, _precision.py, _pathref.py, _pathmin.py): their default outputs
are held to the long-double references by the features' own tests."""
import numpy as np
import pytest

import _chunkcases as CC
import _gcovref as GC
import _jesref as JR
import _kgref as KR
import _mixref as MR
import _pathref as PR
import _precision as P
from conftest import synth

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


def _hk(H):
    Hk = np.array(H, dtype=np.float64, copy=True)
    Hk[:, -1] = -np.inf
    return Hk


def _maker(lib, X, y, alpha, H, c, want_alpha=False, warps=None, max_batch=None):
    """A function that returns a fresh context of the case with the rows of ``H`` resident."""
    def make():
        ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=max_batch or len(H))
        assert np.all(ctx.posterior(H, want_alpha=want_alpha, warps=warps)["status"] == 0)
        return ctx

    return make


def _host_average(rows, ns, use):
    s = np.zeros(rows.shape[1])
    for b in use:
        s = s + rows[b] / float(ns)
    return s


# ------------------------------------------------------------------------------------------------------------------------------
# 1. knowledge gradient and joint entropy search: the posterior chunks of bgp_cond_run
# ------------------------------------------------------------------------------------------------------------------------------
KG_NS = 5  # n_samples of the average (deliberately not the number of rows)


def _kg(cid, M=None):
    c = KR.ALL[cid]
    X, y, alpha, H, _kap, Xc, A, noise = KR.problem(cid)
    return c, X, y, alpha, H, Xc, (A if M is None else A[:M]), noise


@pytest.mark.parametrize("cap", [2, 1])
@pytest.mark.parametrize("M", [None, 0], ids=["shared_set", "M0"])
def test_kg_posterior_chunks(lib, monkeypatch, cap, M):
    """Three posteriors as 2 + 1 and as 1 + 1 + 1, with the shared reference set (``dA + b0 sAx`` with sAx = 0, the resident
    ``K^-1`` / alpha of the chunk) and with M = 0 (the chunk's first stage skipped): the rows and the average."""
    c, X, y, alpha, H, Xc, A, noise = _kg("kg_B3_n65_d3", M)
    call = lambda ctx: ctx.knowledge_gradient(_hk(H), noise, Xc, A, KR.Y_STD, KG_NS)  # noqa: E731
    rows, avg = CC.default_then_forced(monkeypatch, _maker(lib, X, y, alpha, H, c), call, {CC.ITEM: cap}, (CC.item_chunks(3, cap), 1))
    assert np.array_equal(avg, _host_average(rows, KG_NS, range(3)))
    assert np.all(rows == 0.0) if M == 0 else (rows > 0.0).any()


@pytest.mark.parametrize("cap", [2, 1])
def test_jes_posterior_chunks(lib, monkeypatch, cap):
    """Every posterior with its OWN optimum points and values (``dA + b0 sAx`` with sAx = R d, ``dF + b0 M``) and the variances at
    them (``want_var``), as 2 + 1 and 1 + 1 + 1."""
    cid = "jes_B3_n65_d3"
    c = JR.ALL[cid]
    X, y, alpha, H, _kap, Xc, A, f, noise, tau = JR.problem(cid)
    call = lambda ctx: ctx.joint_entropy(_hk(H), noise, Xc, A, f, tau, JR.NS)  # noqa: E731
    rows, avg = CC.default_then_forced(monkeypatch, _maker(lib, X, y, alpha, H, c), call, {CC.ITEM: cap}, (CC.item_chunks(3, cap), 1))
    assert np.array_equal(avg, _host_average(rows, JR.NS, range(3)))
    assert not np.array_equal(rows[0], rows[2]) and not np.array_equal(rows[1], rows[2])


def test_kg_posterior_and_candidate_chunks_together(lib, monkeypatch):
    """m = 300 as 128 + 128 + 44 candidates inside posterior chunks of 2 + 1: both loop indices of ``dV + b0 mtot + m0`` non-zero."""
    c, X, y, alpha, H, Xc, A, noise = _kg("kg_B3_n64_d2_M3_m300")
    call = lambda ctx: ctx.knowledge_gradient(_hk(H), noise, Xc, A, KR.Y_STD, KG_NS)  # noqa: E731
    CC.default_then_forced(monkeypatch, _maker(lib, X, y, alpha, H, c), call, {CC.ITEM: 2, "BGP_KG_CHUNK": KR.CHUNK},
                           (2, CC.cand_chunks(300, KR.CHUNK, 128)))


def test_jes_posterior_and_candidate_chunks_together(lib, monkeypatch):
    cid = "jes_B3_n64_d2_R3_m300"
    c = JR.ALL[cid]
    X, y, alpha, H, _kap, Xc, A, f, noise, tau = JR.problem(cid)
    call = lambda ctx: ctx.joint_entropy(_hk(H), noise, Xc, A, f, tau, JR.NS)  # noqa: E731
    CC.default_then_forced(monkeypatch, _maker(lib, X, y, alpha, H, c), call, {CC.ITEM: 2, "BGP_JES_CHUNK": 128},
                           (2, CC.cand_chunks(300, 128, 128)))


@pytest.mark.parametrize("which", ["kg", "jes"])
def test_a_non_finite_posterior_of_the_second_chunk_drops_out_alone(lib, monkeypatch, which):
    """Row 2 is evaluated with a kernel constant that makes its values non-finite; it is in the SECOND chunk (``dbad + b0``), and the
    average is the fixed-order sum of rows 0 and 1 alone, each over n_samples.  JES: the constant is NaN, so every moment and every
    gain of the row is NaN.  KG returns 0 wherever ``s = var + noise`` is not positive -- a NaN variance included -- so there the
    constant is e^355 (1.5e154): the means stay finite, the quadratic form of the variance overflows (c^2 > 1.8e308), the variance
    is clipped to 0 at +inf or lost to NaN, and the candidates with s = noise > 0 and non-finite lines are NaN."""
    if which == "kg":
        c, X, y, alpha, H, Xc, A, noise = _kg("kg_B3_n65_d3")
        ns = KG_NS
        Hk = _hk(H)
        Hk[2, 0] = 355.0
        call = lambda ctx: ctx.knowledge_gradient(Hk, noise, Xc, A, KR.Y_STD, ns)  # noqa: E731
    else:
        c = JR.ALL["jes_B3_n65_d3"]
        X, y, alpha, H, _kap, Xc, A, f, noise, tau = JR.problem("jes_B3_n65_d3")
        ns = JR.NS
        Hk = _hk(H)
        Hk[2, 0] = np.nan
        call = lambda ctx: ctx.joint_entropy(Hk, noise, Xc, A, f, tau, ns)  # noqa: E731
    rows, avg = CC.default_then_forced(monkeypatch, _maker(lib, X, y, alpha, H, c), call, {CC.ITEM: 2}, (2, 1))
    assert np.all(np.isfinite(rows[:2])) and not np.all(np.isfinite(rows[2]))
    assert np.all(np.isfinite(avg)) and np.array_equal(avg, _host_average(rows, ns, (0, 1)))


# ------------------------------------------------------------------------------------------------------------------------------
# 2. the gradient covariance: gcov_run
# ------------------------------------------------------------------------------------------------------------------------------
GC_WANTS = [(True, False, False), (False, True, False), (False, False, True), (True, True, True)]


@pytest.mark.parametrize("want", GC_WANTS, ids=["dmean", "cov", "csum", "all"])
def test_gcov_posterior_chunks(lib, monkeypatch, want):
    """Three posteriors as 2 + 1; each output alone (the strided downloads ``(b0 m + m0) d`` / ``.. d d``, ``csum + b0 E``) and all."""
    cid = "gc_B3_n65_d3"
    c = GC.ALL[cid]
    X, y, alpha, H, _kap, Xq = GC.problem(cid)
    call = lambda ctx: ctx.grad_cov(H, Xq, *want)  # noqa: E731
    out = CC.default_then_forced(monkeypatch, _maker(lib, X, y, alpha, H, c), call, {CC.ITEM: 2}, (2, 1))
    assert [o is not None for o in out] == list(want)


@pytest.mark.parametrize("want", GC_WANTS, ids=["dmean", "cov", "csum", "all"])
def test_gcov_posterior_and_point_chunks_together(lib, monkeypatch, want):
    """m = 600 as 256 + 256 + 88 points inside posterior chunks of 2 + 1."""
    cid = "gc_B3_n64_d2_m600"
    c = GC.ALL[cid]
    X, y, alpha, H, _kap, Xq = GC.problem(cid)
    call = lambda ctx: ctx.grad_cov(H, Xq, *want)  # noqa: E731
    CC.default_then_forced(monkeypatch, _maker(lib, X, y, alpha, H, c), call, {CC.ITEM: 2, "BGP_GCOV_CHUNK": GC.RC},
                           (2, CC.cand_chunks(600, GC.RC, GC.RC)))


# ------------------------------------------------------------------------------------------------------------------------------
# 3. predict_run: predict with the covariance, the rounding to eights, per-row warps, the acquisition pass, the mixture
# ------------------------------------------------------------------------------------------------------------------------------
def _predb(j, rows=None):
    c = P.PREDB_CASES[j]
    X, y, alpha, H, _kap = P.problem(c["id"])
    Xq = P.query(c["id"])
    return c, X, y, alpha, H, (Xq if rows is None else Xq[:rows])


@pytest.mark.parametrize("j,rows", [(0, 300), (5, None)], ids=["n129_m300", "n1_m257"])
def test_predict_with_the_covariance(lib, monkeypatch, j, rows):
    """Three posteriors as 2 + 1 with ``cov``: ``cov + off m m`` beside the mean and the variance (latent and with the white level)."""
    c, X, y, alpha, H, Xq = _predb(j, rows)
    assert c["B"] == 3 and c["cov"]
    call = lambda ctx: [ctx.predict(Hk, Xq, return_cov=True) for Hk in (H, _hk(H))]  # noqa: E731
    CC.default_then_forced(monkeypatch, _maker(lib, X, y, alpha, H, c), call, {CC.ITEM: 2}, (2, 1))


@pytest.mark.parametrize("cap", [9, 8])
def test_predict_chunks_are_rounded_down_to_eights(lib, monkeypatch, cap):
    """17 posteriors: a bound of 9 is rounded down to 8 (``round8``), so both bounds run as 8 + 8 + 1."""
    c, X, y, alpha, H, Xq = _predb(8)
    assert c["B"] == 17 and CC.item_chunks(17, cap, round8=True) == 3
    call = lambda ctx: ctx.predict(H, Xq)  # noqa: E731
    CC.default_then_forced(monkeypatch, _maker(lib, X, y, alpha, H, c), call, {CC.ITEM: cap}, (3, 1))


def test_predict_of_per_row_warped_posteriors(lib, monkeypatch):
    """``bgp_predict_batch_warped``: item b's own warped queries and training inputs (the item strides ``qs`` / ``xs`` times ``off``)."""
    c = P.WARP_CASES[0]
    X, y, alpha, H, _ = P.problem(c["id"])
    W, Xq = P.warp_params(c["id"]), P.query(c["id"])
    assert c["B"] == 3
    call = lambda ctx: [ctx.predict_warped(Hk, Xq) for Hk in (H, _hk(H))]  # noqa: E731
    CC.default_then_forced(monkeypatch, _maker(lib, X, y, alpha, H, c, warps=W), call, {CC.ITEM: 2}, (2, 1))


@pytest.mark.parametrize("j,cap", [(3, 4), (8, 9)], ids=["B9_by_4", "B17_by_9"])
def test_the_acquisition_pass_behind_forced_chunks(lib, monkeypatch, j, cap):
    """``bgp_acq_batch`` reads every item's moments where the chunks left them (``dqB`` / ``doutB + off mpad``); n_samples != B."""
    c, X, y, alpha, H, Xq = _predb(j)
    assert c["n_samples"] != c["B"]
    code = {"EI": lib.ACQ_EI, "LCB": lib.ACQ_LCB, "MEAN": lib.ACQ_MEAN, "STD": lib.ACQ_STD}
    kinds = [code[k] for k in P.ACQ_KINDS]
    call = lambda ctx: ctx.acq(_hk(H), Xq, P.ACQ_Y_MEAN, P.ACQ_Y_STD, kinds, P.ACQ_PARAMS, c["n_samples"])  # noqa: E731
    CC.default_then_forced(monkeypatch, _maker(lib, X, y, alpha, H, c), call, {CC.ITEM: cap},
                           (CC.item_chunks(c["B"], cap, round8=True), 1))


def test_the_mixture_behind_forced_chunks(lib, monkeypatch):
    cid = "res_%s_latent" % P.PREDB_CASES[0]["id"]
    mc = MR.ALL[cid]
    c, X, y, alpha, H, Xq = _predb(0)
    inp = MR.inputs(cid)
    call = lambda ctx: ctx.predict_mixture(MR.h_kernel(cid), Xq, MR.Y_MEAN, MR.Y_STD, mc["probs"], at=inp["t"],  # noqa: E731
                                           weights=inp["weights"])
    out = CC.default_then_forced(monkeypatch, _maker(lib, X, y, alpha, H, c), call, {CC.ITEM: 2}, (2, 1))
    assert out["n_used"] == 3


# ------------------------------------------------------------------------------------------------------------------------------
# 4. bgp_predict_batch_gram
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,with_cov", [(0, True), (0, False), (1, False)], ids=["n577_cov", "n577", "n385_m300"])
def test_the_gram_predict(lib, monkeypatch, k, with_cov):
    """Three posteriors from host Gram matrices as 2 + 1: ``Ks + (off + b) m n``, ``kss + off m``, ``Kss + off m m``."""
    c = P.GRAM_CASES[k]
    cid = c["id"]
    X, y, alpha, _H, _kap = P.problem(cid)
    r = min(c["m"], 300)
    K, Ks, kss = (np.array([P.gram_inputs(cid, b)[j] for b in range(3)]) for j in range(3))
    Ks, kss = np.ascontiguousarray(Ks[:, :r]), np.ascontiguousarray(kss[:, :r])
    Kss = np.ascontiguousarray(np.array([P.gram_inputs(cid, b)[3] for b in range(3)])[:, :r, :r]) if with_cov else None
    assert not with_cov or c["cov"]

    def make():
        ctx = lib.Context(X, y, alpha, form=c["form"], stationary=c["stationary"], max_batch=3)
        assert np.all(ctx.posterior_gram(K, use_alpha=True)["status"] == 0)
        return ctx

    out = CC.default_then_forced(monkeypatch, make, lambda ctx: ctx.predict_gram(Ks, kss, Kss), {CC.ITEM: 2}, (2, 1))
    assert len(out) == (3 if with_cov else 2)


# ------------------------------------------------------------------------------------------------------------------------------
# 5. bgp_sample_y_batch: the one loop that does not synchronise the stream between its chunks
# ------------------------------------------------------------------------------------------------------------------------------
def _sampleb(cid):
    c = P.ALL[cid]
    X, y, alpha, H, _kap = P.problem(cid)
    return c, X, y, alpha, H, P.sampleb_query(cid), P.sampleb_z(cid)[1]


def _kernel_H(H, latent):
    Hk = np.array(H, dtype=np.float64, copy=True)
    Hk[np.asarray(latent, dtype=bool), -1] = -np.inf
    return Hk


def test_sample_y_batch_item_chunks(lib, monkeypatch):
    """Five items over three resident posteriors, ``pidx`` unsorted and repeated across the cuts, as 2 + 2 + 1: ``z + off m``,
    ``dpidx + off``, ``status + off``, ``out + off m``; the scratch, the staged uploads and the child's matrices are reused by the
    next chunk behind nothing but stream order."""
    cid = "sampleb_n129_m513"
    c, X, y, alpha, H, Xq, z = _sampleb(cid)
    pidx = c["pidx"]
    assert pidx == [2, 0, 2, 1, 0]
    Hk = _kernel_H(H[pidx], c["latent"])
    call = lambda ctx: ctx.sample_y_batch(pidx, Hk, Xq, z, jitter=c["jitter"])  # noqa: E731
    out, st = CC.default_then_forced(monkeypatch, _maker(lib, X, y, alpha, H, c, want_alpha=True), call, {CC.ITEM: 2}, (3, 1))
    assert np.all(st == 0) and st.dtype == np.int32


def test_sample_y_batch_child_context_reused_regrown_and_reused(lib, monkeypatch):
    """Forced, default, forced on ONE context: the child workspace is made for 2 matrices, regrown for 5, and reused for 2."""
    cid = "sampleb_n129_m513"
    c, X, y, alpha, H, Xq, z = _sampleb(cid)
    pidx = c["pidx"]
    Hk = _kernel_H(H[pidx], c["latent"])
    ctx = _maker(lib, X, y, alpha, H, c, want_alpha=True)()
    try:
        runs, stats = [], []
        for cap in (2, None, 2):
            with CC.forced(monkeypatch, **({CC.ITEM: cap} if cap else {})):
                runs.append(ctx.sample_y_batch(pidx, Hk, Xq, z, jitter=c["jitter"]))
                stats.append(ctx.chunk_stats()["items"])
    finally:
        ctx.close()
    assert stats == [3, 1, 3]
    CC.assert_same_bits(runs[0], runs[1], "forced, then default")
    CC.assert_same_bits(runs[2], runs[1], "forced again")


def test_sample_y_batch_a_singular_item_of_the_second_chunk(lib, monkeypatch):
    """The isolation case's shape (a duplicated query row, no jitter) with ONE latent item, item 2 -- the first of the second chunk:
    its covariance is singular and its status non-zero; every other item keeps the white level, has status 0 and the bits of the
    default run (``status + off``, and a failed matrix of the batched factorisation next to regular ones in a chunk)."""
    cid = "sampleb_isolation_n65_m130"
    c, X, y, alpha, H, Xq, z = _sampleb(cid)
    pidx, latent = c["pidx"], [False, False, True, False, False]
    assert c["jitter"] == 0.0 and c["dup_query"]
    Xq = Xq.copy()
    Xq[-8:] = Xq[3]  # (eight copies of one row: rank 8 short)
    Hk = _kernel_H(H[pidx], latent)
    call = lambda ctx: ctx.sample_y_batch(pidx, Hk, Xq, z, jitter=0.0)  # noqa: E731
    make = _maker(lib, X, y, alpha, H, c, want_alpha=True)
    ctx = make()
    try:
        base, st0 = call(ctx)
        assert ctx.chunk_stats() == CC.ONE
    finally:
        ctx.close()
    with CC.forced(monkeypatch, **{CC.ITEM: 2}):
        ctx = make()
        try:
            got, st = call(ctx)
            assert ctx.chunk_stats() == {"items": 3, "rows": 1}
        finally:
            ctx.close()
    print("CHUNKS sample_y_batch singular item: status default %s forced %s" % (st0.tolist(), st.tolist()))
    reg = [0, 1, 3, 4]
    assert st[2] != 0 and np.all(st[reg] == 0)
    assert np.array_equal(st, st0)
    CC.assert_same_bits(got[reg], base[reg], "regular items")


# ------------------------------------------------------------------------------------------------------------------------------
# 6. bgp_predict_grad_batch: chunks of query rows
# ------------------------------------------------------------------------------------------------------------------------------
PG_NLDS = 3072  # bgp_predgrad.hip: training points whose rows fit the workgroup's LDS


def _pg_problem(which):
    if which == "lds":  # (the three posteriors of tests/test_gpu_predgrad.py::test_rows_do_not_depend_on_what_shares_the_call)
        X, y, alpha, H = P._problem(200, 4, 41, "matern52", "product", 3, False)
        H[:, -1] = np.log(1e-2)
        Xq = np.random.RandomState(8).uniform(-0.1, 1.1, size=(257, 4))[:65]
    else:  # one training point more than the LDS rows hold: the k / g rows of a workgroup live in device scratch, ``rows``
        X, y = synth(PG_NLDS + 1, 2, 12)
        alpha = 1e-8
        H = np.array([0.1, np.log(0.3), np.log(0.4), np.log(1e-2)])[None, :] + np.array([[0.0], [0.1], [-0.1]]) * np.array([1.0, 1.0, -1.0, 0.0])
        Xq = np.random.RandomState(2).uniform(size=(65, 2))
    return X, y, alpha, H, Xq


@pytest.mark.parametrize("want_dvar", [True, False], ids=["dvar", "no_dvar"])
@pytest.mark.parametrize("which", ["lds", "scratch_rows"])
def test_predict_grad_row_chunks(lib, monkeypatch, which, want_dvar):
    """m = 65 as 32 + 32 + 1 rows for three posteriors: the strided downloads ``mean + m0``, ``dmean + m0 d`` of B rows each."""
    X, y, alpha, H, Xq = _pg_problem(which)
    assert (len(X) <= PG_NLDS) == (which == "lds") and len(X) <= PG_NLDS + 1
    c = dict(form="product", stationary="matern52")
    call = lambda ctx: ctx.predict_grad(H, Xq, want_dvar=want_dvar)  # noqa: E731
    out = CC.default_then_forced(monkeypatch, _maker(lib, X, y, alpha, H, c, want_alpha=True), call, {CC.ROW: 32},
                                 (1, CC.row_chunks(65, 32)))
    assert (out[3] is not None) == want_dvar and CC.row_chunks(65, 32) == 3


# ------------------------------------------------------------------------------------------------------------------------------
# 7. / 8. bgp_paths_eval and bgp_paths_minimize
# ------------------------------------------------------------------------------------------------------------------------------
PATH_CID = PR.CASES[4]["id"]  # three paths on two posteriors, F = 200, n = 130, d = 3


def _paths_maker(lib):
    from bayes_skopt_amd._posterior import noise_off

    c, pr = PR.ALL[PATH_CID], PR.problem(PATH_CID)
    assert c["P"] == 3

    def make():
        ctx = lib.Context(pr["X"], pr["y"], pr["alpha"], form=c["form"], stationary=c["stationary"], max_batch=2)
        assert np.all(ctx.posterior(pr["H"])["status"] == 0)
        Hp = pr["H"][pr["pidx"]]
        ctx.paths_begin(pr["pidx"], noise_off(Hp), Hp[:, -1], pr["omega"], pr["phase"], pr["w"], pr["eps"])
        return ctx

    return make, c, pr


@pytest.mark.parametrize("want_grad", [True, False], ids=["dout", "no_dout"])
@pytest.mark.parametrize("cap", [128, 300])
def test_paths_eval_row_chunks(lib, monkeypatch, cap, want_grad):
    """m = 300 (the case's 257 rows and 43 more): a bound of 128 runs as 128 + 128 + 44 with the device stride ``mc`` = 128 against
    the host stride m; a bound of 300 is rounded DOWN to 256 and runs as 256 + 44."""
    make, c, pr = _paths_maker(lib)
    Xq = np.vstack([pr["Xq"], np.random.RandomState(c["seed"] + 9).uniform(-0.1, 1.1, size=(300 - c["m"], c["d"]))])
    want = CC.row_chunks(300, cap, round_to=256)
    assert want == {128: 3, 300: 2}[cap]
    call = lambda ctx: ctx.paths_eval(Xq, want_grad=want_grad)  # noqa: E731
    CC.default_then_forced(monkeypatch, make, call, {CC.ROW: cap}, (1, want))


def test_paths_minimize_start_chunks(lib, monkeypatch):
    """Five starts per path (the five lowest rows of the case's queries under the fp64 restatement) as 2 + 2 + 1: the packing
    ``item = path ss + start`` with ss = 2, 2, 1.  All six outputs."""
    import _pathmin as M

    make, c, pr = _paths_maker(lib)
    f, _df = PR.path64(PATH_CID)
    X0 = np.stack([pr["Xq"][np.argsort(f[p], kind="stable")[:5]] for p in range(c["P"])])
    call = lambda ctx: ctx.paths_minimize(X0, M.LO, M.HI, gtol=M.GTOL, max_iter=M.MAX_ITER, want_grad=True)  # noqa: E731
    out = CC.default_then_forced(monkeypatch, make, call, {CC.ROW: 2}, (1, CC.row_chunks(5, 2)))
    assert set(out) == {"x", "fun", "grad", "iters", "evals", "status"} and out["x"].shape == (3, 5, 3)
    assert out["iters"].max() > 0 and CC.row_chunks(5, 2) == 3


# ------------------------------------------------------------------------------------------------------------------------------
# 9. the switches themselves
# ------------------------------------------------------------------------------------------------------------------------------
def _small(lib):
    X, y, alpha, H, Xq = _pg_problem("lds")  # n = 200, d = 4, three posteriors, 65 query rows
    return _maker(lib, X, y, alpha, H, dict(form="product", stationary="matern52"), want_alpha=True), H, Xq


@pytest.mark.parametrize("value", ["1000000", "0", "-3", "abc", ""])
def test_a_bound_above_the_budget_zero_negative_or_not_a_number_changes_nothing(lib, monkeypatch, value):
    """The switches are upper bounds: a value above what the budget gives leaves the chunk alone; 0, a negative number, an empty
    string and a non-number behave as unset.  One chunk is reported and the bits are the default's."""
    make, H, Xq = _small(lib)
    ctx = make()
    try:
        base = (ctx.predict(H, Xq), ctx.predict_grad(H, Xq))
        with CC.forced(monkeypatch, **{CC.ITEM: value, CC.ROW: value}):
            p = ctx.predict(H, Xq)
            sp = ctx.chunk_stats()
            g = ctx.predict_grad(H, Xq)
            sg = ctx.chunk_stats()
    finally:
        ctx.close()
    assert sp == CC.ONE and sg == CC.ONE
    CC.assert_same_bits((p, g), base, "BGP_*_CHUNK=%r" % value)


def test_the_switches_are_read_at_every_call(lib, monkeypatch):
    """Set, call, unset, call on one context -- for either switch."""
    make, H, Xq = _small(lib)
    ctx = make()
    try:
        with CC.forced(monkeypatch, **{CC.ITEM: 2, CC.ROW: 32}):
            p1 = ctx.predict(H, Xq)
            s1 = ctx.chunk_stats()
            g1 = ctx.predict_grad(H, Xq)
            t1 = ctx.chunk_stats()
        p2 = ctx.predict(H, Xq)
        s2 = ctx.chunk_stats()
        g2 = ctx.predict_grad(H, Xq)
        t2 = ctx.chunk_stats()
    finally:
        ctx.close()
    assert s1 == {"items": 2, "rows": 1} and t1 == {"items": 1, "rows": CC.row_chunks(len(Xq), 32)} and t1["rows"] == 3
    assert s2 == CC.ONE and t2 == CC.ONE
    CC.assert_same_bits((p1, g1), (p2, g2), "set, then unset")
