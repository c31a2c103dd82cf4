"""The device-resident ensemble sampler (``bgp_mcmc_run``, bgp_mcmc.hip; the fused n <= 128 half-step ``mcmc_small_kernel``,
bgp_chol.hip) against an independent replay: the cases shared by tests/test_cpu_mcmc_reference.py and
tests/test_gpu_mcmc_replay.py, the long-double replay of a plan, an fp64 replay of the same plan (the computation the device
restates) and the slips the comparison has to catch.

``replay(cid)`` restates one resident run without the device library: per half-step, in order, the proposal
``q = c - (c - s) z`` in fp64 with exactly this operation order (numpy neither reorders nor contracts: positions are comparable
bit for bit); the log-prior from the ``(kind, par)`` table by the three formulas documented in bgp_mcmc.h, in ``np.longdouble``,
summed in theta order; the canonical vector through ``h_src`` / ``h_fixed``; the LML from ``oracle.hp_oracle.lml``;
``lp = prior + LML`` rounded to fp64, a non-finite value (NaN included) -> -inf; accept iff ``factors + lp - logp[mover] > logu``;
after the second half of a step the ensemble and its log-probabilities go into the chain.  A log-prior that is not finite in fp64
decides ``lp = -inf`` whatever the LML is (finite: -inf; +inf or NaN: NaN -> -inf), so the LML of such a proposal is not computed.

The log-probabilities handed in with the start ensemble are the long-double values at the start positions rounded to fp64 (group
G overrides two of them with -inf): they are an INPUT of a run, the device copies them, and every stored log-probability is then
comparable with the reference on ``lp_scale`` = the ``scale`` of ``hp_oracle.lml`` + sum_k |prior term_k|, the absolute sum a
correct fp64 evaluation can lose digits on, against ``_precision.tol("lml", kappa, n)``.

``replay64(cid, slip)`` is the same loop with ``oracle.gp_oracle.lml`` (fp64 LAPACK) and the host's own prior callables (the
ones ``guess_priors`` hands out, ``scipy.stats.norm(...).logpdf`` for kind 3).  ``SLIPS`` are the mistakes a kernel could make
without any existing test noticing; tests/test_cpu_mcmc_reference.py shows that each changes the chain:

* ``no_jacobian``     the log-space Jacobian ``+ 0.5 t`` / ``+ t`` dropped from prior kinds 1 / 2
* ``fixed_counted``   the prior terms of the FIXED canonical entries added (the sum running over the canonical vector, not over
                      the walker): a case without fixed entries (every case of group A) has nothing for it to act on
* ``hsrc_shift``      ``h_src`` shifted by one
* ``chain_early``     the chain row written before the second half-step's accept
* ``stale_partner``   the order of "accept half-step h - 1" and "propose half-step h" swapped: a partner's row read as it stood
                      before its own update.  (Movers and partners of ONE half-step are disjoint, so within a half-step the
                      order of reading a partner and updating a mover cannot matter; across two it can.)
"""
import functools
import math

import numpy as np
import pytest

import _precision as P

hp = pytest.importorskip("oracle.hp_oracle")
if not hp.available():
    pytest.skip("np.longdouble has no 64-bit mantissa here: no extended-precision reference", allow_module_level=True)

LD = np.longdouble
MCMC_LDS_DOUBLES = 20480  # bgp_mcmc.hip
SLIPS = ("no_jacobian", "fixed_counted", "hsrc_shift", "chain_early", "stale_partner")
C_FIXED, LS_SHARED, S2_START = 1.5, 0.4, 1e-2


def expected_form(n, p, hp_, W):
    """The selection of ``bgp_mcmc_begin_ex`` restated (one rank, no warp): the form a shape takes."""
    if n <= 128 and p <= 64 and hp_ <= 64:
        return "fused"
    Ns = W // 2
    return "step_hbm" if W * p + W + 3 * Ns + 2 * Ns * p > MCMC_LDS_DOUBLES else "step_lds"


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
def _case(cid, group, n, d, family, vec_alpha, W, steps, seed, form, cfg="full", kinds=None, take=None, edges=False):
    """``cfg``: "full" (walker = canonical vector), "iso_fixc" (fixed signal variance, ONE length scale for all columns, free
    noise: p = 2), "fixnoise" (fixed noise: p = d + 1), "iso_fixc_wide" ("iso_fixc" as group E needs it).  ``kinds``: prior kind
    per walker entry (None: the two default families).  ``take``: rows of the problem in use (the growth test); ``edges``: the
    -inf / accept-test edges of group G.  ``form``: the form of the half-step the case was written for."""
    st, fm = family
    return dict(id=cid, group=group, n=n, d=d, stationary=st, form=fm, vec_alpha=vec_alpha, W=W, steps=steps, seed=seed,
                runs=form, cfg=cfg, kinds=kinds, take=take, edges=edges)


def _cases():
    F = P.FAMILIES
    out = []
    # A: the fused form on a ragged block, every family
    ns = [1, 2, 17, 64, 65, 127, 128]
    for j in range(8):
        n, d = ns[j % 7], 1 + j % 3
        out.append(_case("A%d_n%d_d%d_%s_%s_%s" % (j, n, d, F[j][0], F[j][1], "vec" if j % 2 else "scal"), "A", n, d, F[j],
                         bool(j % 2), 2 * (d + 2) + 2, 3, 2100 + j, "fused"))
    # B: the canonical map
    out.append(_case("B0_n60_d3_fixed_c_shared_ls", "B", 60, 3, ("matern52", "product"), False, 6, 3, 2120, "fused", cfg="iso_fixc"))
    out.append(_case("B1_n60_d3_fixed_noise", "B", 60, 3, ("matern32", "product"), True, 10, 3, 2121, "fused", cfg="fixnoise"))
    # C: prior kind 3
    out.append(_case("C0_n60_d2_normal_priors", "C", 60, 2, ("matern52", "product"), False, 10, 3, 2130, "fused", kinds=[3, 3, 3, 3]))
    out.append(_case("C1_n60_d2_mixed_priors", "C", 60, 2, ("rbf", "sum"), True, 10, 3, 2131, "fused", kinds=[1, 3, 2, 3]))
    # D: the smallest ensemble
    out.append(_case("D0_n17_d1_W2", "D", 17, 1, ("matern52", "product"), False, 2, 6, 2140, "fused"))
    # E: both sides of p, hp <= 64; W = 2 p + 2 (no cap needed: a long-double LML at n = 20 takes 4 ms)
    out.append(_case("E0_n20_d62_p64_hp64", "E", 20, 62, ("matern52", "product"), False, 130, 2, 2150, "fused"))
    out.append(_case("E1_n20_d63_p65_hp65", "E", 20, 63, ("matern52", "product"), False, 132, 2, 2151, "step_lds"))
    # (seed 2152 accepted all 12 of its moves -- p = 2: (p - 1) log z is small, the stretch move accepts 5 in 6 -- and a kernel
    # that always accepts would have passed; 2153 is the first seed from there up with a rejected move: 11 / 1)
    out.append(_case("E2_n20_d63_p2_hp65", "E", 20, 63, ("matern52", "product"), False, 6, 2, 2153, "step_lds", cfg="iso_fixc"))
    # F: both sides of the step kernel's 20 480 doubles at p = 72: 138 * 293 / 2 = 20 217, 140 * 293 / 2 = 20 510
    out.append(_case("F0_n20_d70_W138_lds", "F", 20, 70, ("matern52", "product"), False, 138, 2, 2160, "step_lds"))
    out.append(_case("F1_n20_d70_W140_hbm", "F", 20, 70, ("matern52", "product"), False, 140, 2, 2161, "step_hbm"))
    # G: -inf and the edges of the accept test, on the fused form and on the step kernel
    out.append(_case("G0_n60_d2_edges_fused", "G", 60, 2, ("matern52", "product"), False, 12, 3, 2170, "fused", edges=True))
    out.append(_case("G1_n129_d2_edges_step", "G", 129, 2, ("matern52", "product"), False, 12, 3, 2171, "step_lds", edges=True))
    # the growth test: ONE problem of 129 points, its first 127 / 128 / 129 rows
    for k in (127, 128, 129):
        out.append(_case("grow_n%d" % k, "grow", 129, 2, ("matern52", "product"), True, 10, 2, 2180, "fused" if k <= 128 else "step_lds",
                         take=k))
    return out


CASES = _cases()
ALL = {c["id"]: c for c in CASES}
SEGMENT_CASE = "A4_n65_d2_rbf_sum_scal"  # group H: begin / steps(1) / steps(2) / steps(1) / end; extended to 4 steps below
assert SEGMENT_CASE in ALL
ALL[SEGMENT_CASE]["steps"] = 4
GROW = ["grow_n127", "grow_n128", "grow_n129"]


# ------------------------------------------------------------------------------------------------------------------------------
# priors: the table the device reads, the long-double formulas of bgp_mcmc.h, the host's callables
# ------------------------------------------------------------------------------------------------------------------------------
def prior_terms_ld(kind, par, t):
    """The log-prior term of every walker entry in long double from the (kind, par) table -- bgp_mcmc.h::mcmc_prior,
    include/bgp.h -- with the table's fp64 parameters taken as exact."""
    t = np.asarray(t, dtype=np.float64).astype(LD)
    out = np.empty(len(t), dtype=LD)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(len(t)):
            a = [LD(float(v)) for v in par[k]]
            if kind[k] == 1:
                out[k] = a[0] - LD(0.5) * np.exp(t[k]) / a[1] + LD(0.5) * t[k]
            elif kind[k] == 2:
                out[k] = (LD(-2) * (np.exp(a[2] * (t[k] - a[0])) + np.exp(a[3] * (t[k] - a[1]))) - a[4]) + t[k]
            elif kind[k] == 3:
                y = (t[k] - a[0]) / a[1]
                out[k] = ((-(y * y)) / LD(2) - a[2]) - a[3]
            else:
                raise ValueError(kind[k])
    return out


_NORMAL = {"c": (0.0, 2.0), "ls": (-1.0, 1.5), "s2": (-4.0, 3.0)}  # (loc, scale) of the kind-3 prior per role


@functools.lru_cache(maxsize=None)
def _default_callables():
    from bayes_skopt_amd.utils import guess_priors
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel

    c, ls, s2 = guess_priors(ConstantKernel(1.0) * Matern(length_scale=0.3, nu=2.5) + WhiteKernel(1e-2))
    return {"c": c, "ls": ls, "s2": s2}


def _priors(roles, kinds):
    """(callables, kind, par) of the walker's entries: the host callable and what ``_device_prior`` reads off it."""
    import scipy.stats as st
    from bayes_skopt_amd.bayesgpr import _device_prior

    fns = []
    for k, role in enumerate(roles):
        want = (1 if role in ("c", "s2") else 2) if kinds is None else kinds[k]
        if want == 3:
            fns.append(st.norm(loc=_NORMAL[role][0], scale=_NORMAL[role][1]).logpdf)
        else:
            fns.append(_default_callables()["ls" if want == 2 else ("c" if role == "ls" else role)])
    table = [_device_prior(f) for f in fns]
    kind = np.array([t[0] for t in table], dtype=np.int32)
    assert kinds is None or list(kind) == list(kinds)
    return fns, kind, np.array([t[1] for t in table], dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------------------
# the inputs of a run
# ------------------------------------------------------------------------------------------------------------------------------
def build_plan(W, p, steps, seed, zz=None, logu=None):
    """(movers, partners, zz, factors, logu), each (2 steps, W / 2), drawn as ``_loopback_run`` of tests/test_gpu_resident.py
    draws them: ``EnsembleSampler._half_step_plans`` and ``np.log(rand)``.  ``zz`` / ``logu``: {(half-step, row): value} hand
    overrides of single entries (``factors`` keeps the value of the drawn z)."""
    from bayes_skopt_amd.sampler import EnsembleSampler

    planner = EnsembleSampler(W, p, lambda T: np.zeros(len(T)))
    planner.random_state = np.random.RandomState(seed).get_state()
    rows = list(planner._half_step_plans(steps))
    plan = [np.array([r[0] for r in rows], dtype=np.int32), np.array([r[1] for r in rows], dtype=np.int32),
            np.array([r[2][:, 0] for r in rows]), np.array([r[3] for r in rows]),
            np.log(np.random.RandomState(seed + 1).rand(2 * steps, W // 2))]
    for key, v in (zz or {}).items():
        plan[2][key] = v
    for key, v in (logu or {}).items():
        plan[4][key] = v
    return tuple(plan)


@functools.lru_cache(maxsize=None)
def inputs(cid):
    """Everything ``Context`` and ``Context.mcmc_run`` take for a case, as a dict: X, y, alpha, stationary, form; coords0, logp0,
    plan; h_src, h_fixed, prior_kind, prior_par; and for the replays the host prior callables ``fns`` with the role of every
    walker entry and of every canonical entry."""
    c = ALL[cid]
    n, d, st, fm = c["n"], c["d"], c["stationary"], c["form"]
    X, y, alpha, _H = P._problem(n, d, c["seed"], st, fm, 1, c["vec_alpha"])
    X = X * min(1.0, math.sqrt(3.0 / d))  # (d >> 3: the points stay within reach of a length scale of 0.3)
    if c["take"]:
        k = c["take"]
        X, y, alpha = X[:k].copy(), y[:k].copy(), (alpha[:k].copy() if c["vec_alpha"] else alpha)
    hroles = ["c"] + ["ls"] * d + ["s2"]
    full = np.array([0.0] + [math.log(0.3)] * d + [math.log(S2_START)])
    cfg = c["cfg"]
    if cfg == "full":
        h_src, h_fixed = np.arange(d + 2), np.zeros(d + 2)
    elif cfg == "iso_fixc":
        h_src = np.array([-1] + [0] * d + [1])
        h_fixed = np.where(h_src < 0, math.log(C_FIXED), 0.0)
        full[1 : d + 1] = math.log(LS_SHARED)
    elif cfg == "fixnoise":
        h_src = np.array(list(range(d + 1)) + [-1])
        h_fixed = np.where(h_src < 0, math.log(S2_START), 0.0)
    else:
        raise ValueError(cfg)
    p = int(h_src.max()) + 1
    roles = [hroles[int(np.flatnonzero(h_src == k)[0])] for k in range(p)]
    theta0 = np.array([full[int(np.flatnonzero(h_src == k)[0])] for k in range(p)])
    fns, kind, par = _priors(roles, c["kinds"])
    W, steps = c["W"], c["steps"]
    coords0 = theta0 + 1e-2 * np.random.RandomState(c["seed"] + 1).randn(W, p)
    inp = dict(X=X, y=y, alpha=alpha, stationary=st, form=fm, n=len(X), d=d, p=p, W=W, steps=steps, coords0=coords0,
               h_src=h_src.astype(np.int32), h_fixed=h_fixed.astype(np.float64), prior_kind=kind, prior_par=par, fns=fns,
               roles=roles, hroles=hroles)
    ref0 = [lp_ld(inp, coords0[w]) for w in range(W)]
    logp0 = np.array([r[0] for r in ref0])
    inp["scale0"] = np.array([r[1] for r in ref0])
    inp["kappa0"] = np.array([r[2] for r in ref0])
    assert np.all(np.isfinite(logp0))
    zz, logu, edges = {}, {}, {}
    if c["edges"]:
        plain = build_plan(W, p, steps, c["seed"] + 2)
        mv, pr = plain[0], plain[1]

        def z800(i):  # the z that puts entry 0 of proposal i of half-step 0 at 800 (the start rows are those it reads)
            s0, c0 = coords0[mv[0, i], 0], coords0[pr[0, i], 0]
            return (c0 - 800.0) / (c0 - s0)

        a, b = int(mv[0, 0]), int(mv[0, 1])
        logp0[[a, b]] = -np.inf             # two walkers handed in with -inf: a's first proposal is finite, ...
        zz[(0, 1)] = z800(1)                # ... b's is at exp(800): -inf - (-inf) is NaN, which is not >, rejected
        zz[(0, 2)] = z800(2)                # the same for a mover whose own log-probability is finite: rejected
        logu[(1, 1)] = -np.inf              # u = 0: accepted when lp is finite
        i1 = 0 if mv[2, 0] != b else 1
        logu[(2, i1)] = 0.0                 # u = 1 (on a mover whose own log-probability is finite)
        edges = dict(minus_inf_walkers=(a, b), first_finite_accept=[(0, 0)], nan_reject=(0, 1), inf_reject=(0, 2),
                     u_zero=(1, 1), u_one=(2, i1))
        hb, ib = [(h, int(np.flatnonzero(mv[h] == b)[0])) for h in (2, 3) if b in mv[h]][0]
        edges["first_finite_accept"].append((hb, ib))  # (b's first finite proposal is its move of the next step)
    inp["logp0"] = logp0
    inp["plan"] = build_plan(W, p, steps, c["seed"] + 2, zz=zz, logu=logu)
    inp["edges"] = edges
    return inp


# ------------------------------------------------------------------------------------------------------------------------------
# log-probability of one position: long double, and fp64 as the host computes it
# ------------------------------------------------------------------------------------------------------------------------------
def _canonical(inp, q, h_src=None):
    h_src = inp["h_src"] if h_src is None else h_src
    return np.array([q[s] if s >= 0 else f for s, f in zip(h_src, inp["h_fixed"])], dtype=np.float64)


def lp_ld(inp, q):
    """(lp rounded to fp64 with non-finite -> -inf, lp_scale, kappa) of position q; scale and kappa are NaN where lp is -inf."""
    terms = prior_terms_ld(inp["prior_kind"], inp["prior_par"], q)
    prior = LD(0)
    for t in terms:  # theta order
        prior = prior + t
    with np.errstate(over="ignore", invalid="ignore"):
        if not np.isfinite(np.float64(prior)):
            return -np.inf, np.nan, np.nan
    h = _canonical(inp, q)
    try:
        with np.errstate(all="ignore"):
            r = hp.lml(inp["X"], inp["y"], inp["alpha"], h, inp["stationary"], inp["form"])
            lp = np.float64(prior + r["lml"])
    except np.linalg.LinAlgError:
        return -np.inf, np.nan, np.nan
    if not np.isfinite(lp):
        return -np.inf, np.nan, np.nan
    scale = float(r["scale"] + np.abs(terms).sum())
    return float(lp), scale, P.kappa_of(inp["X"], inp["alpha"], h, inp["stationary"], inp["form"])


def lp_scale(inp, q):
    """The absolute sum a correct fp64 evaluation of lp(q) can lose digits on: ``scale`` of ``hp_oracle.lml`` + sum_k |prior_k|."""
    return lp_ld(inp, q)[1]


def _host_fns(inp, slip):
    fns = list(inp["fns"])
    if slip == "no_jacobian":
        jac = {1: 0.5, 2: 1.0, 3: 0.0}
        fns = [(lambda t, f=f, j=jac[int(k)]: f(t) - j * t) for f, k in zip(fns, inp["prior_kind"])]
    return fns


def lp_64(inp, q, slip=None):
    """lp of position q in fp64 as the host-driven loop computes it: the host callables summed in theta order +
    ``gp_oracle.lml``; non-finite -> -inf."""
    from oracle import gp_oracle as O

    h_src = np.roll(inp["h_src"], 1) if slip == "hsrc_shift" else inp["h_src"]
    with np.errstate(all="ignore"):
        prior = 0.0
        for f, t in zip(_host_fns(inp, slip), q):
            prior = prior + float(f(t))
        h = _canonical(inp, q, h_src)
        if slip == "fixed_counted":
            d = _default_callables()
            for j, s in enumerate(inp["h_src"]):
                if s < 0:
                    prior = prior + float(d[inp["hroles"][j]](h[j]))
        if not math.isfinite(prior):
            return -np.inf
        lp = prior + float(O.lml(inp["X"], inp["y"], np.broadcast_to(inp["alpha"], (inp["n"],)), h, inp["stationary"], inp["form"]))
    return lp if math.isfinite(lp) else -np.inf


# ------------------------------------------------------------------------------------------------------------------------------
# the replay
# ------------------------------------------------------------------------------------------------------------------------------
def _run(inp, lpfn, chain_early=False, stale_partner=False):
    """One resident run restated.  ``lpfn(q) -> (lp, scale, kappa)``.  Returns a dict: the five arrays of ``Context.mcmc_run``
    and per accept test (half-step, row) ``lp``, ``accepted``, ``finite`` (all four operands), ``margin``, ``scale`` and
    ``kappa`` of the proposal and of the mover's own log-probability; ``lps_scale`` / ``lps_kappa`` beside ``lps``."""
    movers, partners, zz, factors, logu = inp["plan"]
    nhalf, Ns = movers.shape
    W, p = inp["coords0"].shape
    coords, logp = inp["coords0"].copy(), inp["logp0"].copy()
    sc, kp = inp["scale0"].copy(), inp["kappa0"].copy()
    nacc = np.zeros(W, dtype=np.int64)
    chain, lps = np.empty((nhalf // 2, W, p)), np.empty((nhalf // 2, W))
    lsc, lkp = np.empty((nhalf // 2, W)), np.empty((nhalf // 2, W))
    rec = {k: np.full((nhalf, Ns), np.nan) for k in ("lp", "margin", "scale", "kappa", "scale_old", "kappa_old")}
    rec["accepted"], rec["finite"] = np.zeros((nhalf, Ns), dtype=bool), np.zeros((nhalf, Ns), dtype=bool)
    before = coords.copy()  # the ensemble before the previous half-step's accepts
    for h in range(nhalf):
        src = before if stale_partner else coords
        before = coords.copy()
        new = []
        for i in range(Ns):
            m, pr, z = int(movers[h, i]), int(partners[h, i]), zz[h, i]
            s, c = coords[m], src[pr]
            with np.errstate(all="ignore"):
                q = c - (c - s) * z
            lp, scale, kappa = lpfn(q)
            f, old, u = float(factors[h, i]), float(logp[m]), float(logu[h, i])
            t = f + lp - old  # (Python floats: -inf - -inf is a quiet NaN)
            acc = t > u
            fin = all(math.isfinite(v) for v in (f, lp, old, u))
            rec["lp"][h, i], rec["accepted"][h, i], rec["finite"][h, i] = lp, acc, fin
            rec["scale"][h, i], rec["kappa"][h, i], rec["scale_old"][h, i], rec["kappa_old"][h, i] = scale, kappa, sc[m], kp[m]
            if fin:
                rec["margin"][h, i] = abs(t - u)
            if acc:
                new.append((m, q, lp, scale, kappa))
        for m, q, lp, scale, kappa in new:
            coords[m], logp[m], sc[m], kp[m] = q, lp, scale, kappa
            nacc[m] += 1
        if (h & 1) == (0 if chain_early else 1):
            chain[h >> 1], lps[h >> 1], lsc[h >> 1], lkp[h >> 1] = coords, logp, sc, kp
    rec.update(chain=chain, lps=lps, coords=coords, logp=logp, naccepted=nacc, lps_scale=lsc, lps_kappa=lkp, logp_scale=sc,
               logp_kappa=kp)
    return rec


@functools.lru_cache(maxsize=None)
def replay_full(cid):
    inp = inputs(cid)
    return _run(inp, functools.partial(lp_ld, inp))


def replay(cid):
    """chain, lps, coords, logp, naccepted, margins of the long-double replay of a case; ``margins`` holds
    |factors + lp - logp[mover] - logu| of every accept test whose operands are all finite."""
    r = replay_full(cid)
    return r["chain"], r["lps"], r["coords"], r["logp"], r["naccepted"], r["margin"][r["finite"]]


@functools.lru_cache(maxsize=None)
def replay64(cid, slip=None):
    inp = inputs(cid)
    return _run(inp, lambda q: (lp_64(inp, q, slip), np.nan, np.nan), chain_early=slip == "chain_early",
                stale_partner=slip == "stale_partner")


def margin_bounds(cid):
    """Per accept test the bound its margin has to clear: 1000 x the LML tolerance on ``lp_scale``, of the proposal and of the
    mover's own log-probability (both enter the test), at their own kappas.  NaN where the test is not finite."""
    r, n = replay_full(cid), inputs(cid)["n"]
    out = np.full(r["margin"].shape, np.nan)
    for idx in zip(*np.nonzero(r["finite"])):
        out[idx] = 1000.0 * (P.tol("lml", r["kappa"][idx], n) * r["scale"][idx] + P.tol("lml", r["kappa_old"][idx], n) * r["scale_old"][idx])
    return out


def lps_tolerance(cid):
    """(tol of ``lps``, tol of ``logp_out``) in units of ``lp_scale``: ``_precision.tol("lml", kappa, n)`` at the stored position;
    NaN where the reference is -inf."""
    r, n = replay_full(cid), inputs(cid)["n"]
    f = np.vectorize(lambda k: P.tol("lml", k, n) if np.isfinite(k) else np.nan)
    return f(r["lps_kappa"]), f(r["logp_kappa"])
