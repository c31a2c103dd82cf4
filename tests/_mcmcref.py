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

Group W: walkers that carry their own input warp (``bgp_mcmc_begin_ex`` with ``nwarp`` = 2 d; ``Context.mcmc_run(..., nwarp=)``).
The walker is [ng kernel entries, alpha_1 .. alpha_d, beta_1 .. beta_d], the device's layout.  The replay of a warped proposal
is described at ``lp_ld``: positions in fp64 as before; every prior term from the table in long double; the kernel entries
summed in theta order, the warp entries as the pairs (alpha_k + beta_k) column by column, the two sums added; the inputs through
``hp_oracle.warp_inputs`` (mpmath, 40 digits), the LML on them.  The tolerance of a warped log-probability is
``_precision.tol("lml", kappa, n, sens)`` with kappa of the WARPED Gram matrix and the warp sensitivity ``sens``.  A warped
ensemble never takes the fused half-step.  ``WARP_SLIPS``, each shown to change a warped chain on the CPU:

* ``alpha_beta_swapped``   the scatter hands betas where alphas belong
* ``warp_of_mover``        warp parameters read from the mover's current row instead of from the proposal
* ``warp_shared``          every proposal of a half-step sees proposal 0's warped matrix (a zero stride)
* ``warp_offset_hp``       the warp entries taken from ``hp`` onward instead of from ``ng`` (W3: ng = 2, hp = 5)
* ``warp_priors_dropped``  the prior summed over the kernel entries only
* ``warp_identity``        the LML on the unwarped inputs

The pair W6 / W7 (d = 70: 210 Beta CDFs per evaluation, about 100 evaluations each) costs 4.8 s + 5.1 s of long-double replay
on the CPU, under the 20 s the pair was allowed; the whole of group W 36 s.
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
WARP_SLIPS = ("alpha_beta_swapped", "warp_of_mover", "warp_shared", "warp_offset_hp", "warp_priors_dropped", "warp_identity")
C_FIXED, LS_SHARED, S2_START = 1.5, 0.4, 1e-2


def expected_form(n, p, hp_, W, nwarp=0):
    """The selection of ``bgp_mcmc_begin_ex`` restated (one rank): the form a shape takes.  A warped ensemble (``nwarp`` = 2 d of
    its p entries are warp parameters) is never fused: the fused half-step builds its Gram matrix from the context's inputs."""
    if n <= 128 and p <= 64 and hp_ <= 64 and not nwarp:
        return "fused"
    Ns = W // 2
    return "step_hbm" if W * p + W + 3 * Ns + 2 * Ns * p > MCMC_LDS_DOUBLES else "step_lds"


# ------------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------------
def _case(cid, group, n, d, family, vec_alpha, W, steps, seed, form, cfg="full", kinds=None, take=None, edges=False, warp=False,
          normal=None, wcentre=(0.0, 0.0), wspread=1e-2):
    """``cfg``: "full" (walker = canonical vector), "iso_fixc" (fixed signal variance, ONE length scale for all columns, free
    noise: p = 2), "fixnoise" (fixed noise: p = d + 1), "iso_fixc_wide" ("iso_fixc" as group E needs it).  ``kinds``: prior kind
    per walker entry (None: the two default families).  ``take``: rows of the problem in use (the growth test); ``edges``: the
    -inf / accept-test edges of group G.  ``form``: the form of the half-step the case was written for.  ``warp``: the walker
    carries 2 d warp entries behind its kernel entries (roles "wa" x d, then "wb" x d: the device's layout), kind 3 unless
    ``kinds`` says otherwise; ``normal``: (loc, scale) of the kind-3 prior per role, over ``_NORMAL``; ``wcentre``: the centre
    of the start ensemble's (alpha, beta) entries, ``wspread`` their standard deviation (1e-2 like every other entry: W4 widens
    it so that a mover's warp differs from its proposal's by more than an accept margin)."""
    st, fm = family
    return dict(id=cid, group=group, n=n, d=d, stationary=st, form=fm, vec_alpha=vec_alpha, W=W, steps=steps, seed=seed,
                runs=form, cfg=cfg, kinds=kinds, take=take, edges=edges, warp=warp, normal=normal, wcentre=wcentre,
                wspread=wspread)


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
    # W: walkers that carry their own input warp (nwarp = 2 d), the smallest shapes at which each piece can still go wrong;
    # W = 2 p + 2.  Seeds: 2200 + 10 j; every one of them held the conditions of tests/test_cpu_mcmc_reference.py at the first
    # try (every finite accept test clears ``margin_bounds``, smallest margin / bound 3.5e4 on W3 and W4; accepted and rejected moves
    # on every case), so no seed was passed over for them -- W4 apart, see there.
    out.append(_case("W0_n17_d1_warp", "W", 17, 1, ("matern52", "product"), False, 12, 3, 2200, "step_lds", warp=True))
    out.append(_case("W1_n65_d2_rbf_sum_vec_warp", "W", 65, 2, ("rbf", "sum"), True, 18, 3, 2210, "step_lds", warp=True))
    out.append(_case("W2_n129_d2_m32_warp", "W", 129, 2, ("matern32", "product"), False, 18, 3, 2220, "step_lds", warp=True))
    # ng = 2 while hp = 5: the warp offset is NOT the canonical vector's length
    out.append(_case("W3_n60_d3_iso_fixc_warp", "W", 60, 3, ("matern52", "product"), False, 18, 3, 2230, "step_lds", cfg="iso_fixc",
                     warp=True))
    # different priors on alphas and betas, one beta entry of another kind, a start far from the identity warp
    # (the one case with seeds passed over, and not for a margin: W4 is the case EVERY warp slip has to change.  With 2240 the
    # swap of alphas and betas flipped none of its 48 accept tests, 2241 missed two slips, 2242 and 2243 one and three; 2244 is
    # the first seed at which all six change the chain.  Its margins hold like the others': tests/test_cpu_mcmc_reference.py.)
    out.append(_case("W4_n60_d2_fixnoise_m12_sum_warp_priors", "W", 60, 2, ("matern12", "sum"), False, 16, 3, 2244, "step_lds",
                     cfg="fixnoise", warp=True, kinds=[1, 2, 2, 3, 3, 3, 2], normal={"wa": (0.2, 0.3), "wb": (-0.1, 0.5)},
                     wcentre=(0.3, -0.2), wspread=0.2))
    out.append(_case("W5_n60_d2_edges_warp", "W", 60, 2, ("matern52", "product"), False, 18, 3, 2250, "step_lds", warp=True,
                     edges=True))
    # both sides of the step kernel's 20 480 doubles at p = 72 + 140: 48 * 212 + 48 + 72 + 48 * 212 = 20 472, W = 50: 21 325
    out.append(_case("W6_n3_d70_W48_lds_warp", "W", 3, 70, ("matern52", "product"), False, 48, 1, 2260, "step_lds", warp=True))
    out.append(_case("W7_n3_d70_W50_hbm_warp", "W", 3, 70, ("matern52", "product"), False, 50, 1, 2270, "step_hbm", warp=True))
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


# (loc, scale) of the kind-3 prior per role; "wa" / "wb": the reference's default warp priors
_NORMAL = {"c": (0.0, 2.0), "ls": (-1.0, 1.5), "s2": (-4.0, 3.0), "wa": (0.0, 0.3), "wb": (0.0, 0.3)}


@functools.lru_cache(maxsize=None)
def _default_callables():
    from bayes_skopt_amd.utils import guess_priors
    from sklearn.gaussian_process.kernels import ConstantKernel, Matern, WhiteKernel

    c, ls, s2 = guess_priors(ConstantKernel(1.0) * Matern(length_scale=0.3, nu=2.5) + WhiteKernel(1e-2))
    return {"c": c, "ls": ls, "s2": s2}


def _priors(roles, kinds, normal=None):
    """(callables, kind, par) of the walker's entries: the host callable and what ``_device_prior`` reads off it."""
    import scipy.stats as st
    from bayes_skopt_amd.bayesgpr import _device_prior

    normal = dict(_NORMAL, **(normal or {}))
    fns = []
    for k, role in enumerate(roles):
        want = (3 if role in ("wa", "wb") else 1 if role in ("c", "s2") else 2) if kinds is None else kinds[k]
        if want == 3:
            fns.append(st.norm(loc=normal[role][0], scale=normal[role][1]).logpdf)
        else:
            fns.append(_default_callables()["ls" if want == 2 else ("c" if role in ("ls", "wa", "wb") else role)])
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
    ng = int(h_src.max()) + 1  # kernel entries of the walker
    nwarp = 2 * d if c["warp"] else 0
    p = ng + nwarp
    roles = [hroles[int(np.flatnonzero(h_src == k)[0])] for k in range(ng)] + ["wa"] * (nwarp // 2) + ["wb"] * (nwarp // 2)
    theta0 = np.array([full[int(np.flatnonzero(h_src == k)[0])] for k in range(ng)] + [c["wcentre"][0]] * (nwarp // 2)
                      + [c["wcentre"][1]] * (nwarp // 2))
    fns, kind, par = _priors(roles, c["kinds"], c["normal"])
    W, steps = c["W"], c["steps"]
    spread = np.array([1e-2] * ng + [c["wspread"]] * nwarp)
    coords0 = theta0 + spread * np.random.RandomState(c["seed"] + 1).randn(W, p)
    plain = build_plan(W, p, steps, c["seed"] + 2)
    mv, pr = plain[0], plain[1]
    # the entry that proposals 1 and 2 of half-step 0 put at +-800 (group G: entry 0 at +800; warped: an ALPHA entry at +800 and
    # a BETA entry at -800)
    far = {1: (ng, 800.0), 2: (ng + nwarp // 2 + 1, -800.0)} if nwarp else {1: (0, 800.0), 2: (0, 800.0)}
    if c["edges"] and nwarp:
        # warped: the mover of such a proposal starts on its partner's row but for that entry, so q = c - (c - s) z leaves every
        # other entry where it was (c - 0 z = c exactly), every prior term is finite and the WARP entry alone decides lp = -inf
        for i, (col, _target) in far.items():
            row = coords0[pr[0, i]].copy()
            row[col] = coords0[mv[0, i], col]
            coords0[mv[0, i]] = row
    inp = dict(X=X, y=y, alpha=alpha, stationary=st, form=fm, n=len(X), d=d, p=p, ng=ng, nwarp=nwarp, W=W, steps=steps,
               coords0=coords0, h_src=h_src.astype(np.int32), h_fixed=h_fixed.astype(np.float64), prior_kind=kind, prior_par=par,
               fns=fns, roles=roles, hroles=hroles)
    ref0 = [lp_ld(inp, coords0[w]) for w in range(W)]
    logp0 = np.array([r[0] for r in ref0])
    inp["scale0"] = np.array([r[1] for r in ref0])
    inp["kappa0"] = np.array([r[2] for r in ref0])
    inp["sens0"] = np.array([r[3] for r in ref0])
    assert np.all(np.isfinite(logp0))
    zz, logu, edges = {}, {}, {}
    if c["edges"]:

        def z800(i):  # the z that puts entry far[i] of proposal i of half-step 0 at +-800 (the start rows are those it reads)
            col, target = far[i]
            s0, c0 = coords0[mv[0, i], col], coords0[pr[0, i], col]
            return (c0 - target) / (c0 - s0)

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


def _warp_ok(w):
    """The contract of a warp entry: ``exp(w)`` is a positive finite fp64 number (else there is no Beta distribution: the
    device's Beta CDF is NaN by construction, the factorisation fails, lp = -inf)."""
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp(np.asarray(w, dtype=np.float64))
    return bool(np.all((e > 0.0) & np.isfinite(e)))


def lp_ld(inp, q):
    """(lp rounded to fp64 with non-finite -> -inf, lp_scale, kappa, sens) of position q; scale, kappa and sens are NaN where lp
    is -inf.  Warped walkers (``nwarp`` = 2 d entries [alphas of all columns, betas of all columns] behind the ``ng`` kernel
    entries) -- what ``_eval_warp_priors`` of bayesgpr.py and ``mcmc_step_kernel`` both do, restated: the kernel entries' prior
    terms summed in theta order, the warp entries' as the pairs (alpha_k + beta_k) column by column on a sum of their own, the
    two sums added; the LML on ``hp_oracle.warp_inputs(X, q[ng:])`` (mpmath at 40 digits); a warp entry whose ``exp`` is not a
    positive finite fp64 number decides lp = -inf without an LML.  ``kappa`` is that of the WARPED Gram matrix, ``sens`` the
    warp sensitivity of tests/test_gpu_precision.py: the LML's response to the warped inputs rounded to fp32, over 2^-24
    (0 without a warp)."""
    bad = (-np.inf, np.nan, np.nan, np.nan)
    ng, dw = inp["ng"], inp["nwarp"] // 2
    terms = prior_terms_ld(inp["prior_kind"], inp["prior_par"], q)
    prior = LD(0)
    for t in terms[:ng]:  # theta order
        prior = prior + t
    if dw:
        w = LD(0)
        for k in range(dw):
            w = w + (terms[ng + k] + terms[ng + dw + k])
        prior = prior + w
    with np.errstate(over="ignore", invalid="ignore"):
        if not np.isfinite(np.float64(prior)):
            return bad
    if dw and not _warp_ok(q[ng:]):
        return bad
    h = _canonical(inp, q)
    X = hp.warp_inputs(inp["X"], q[ng:]) if dw else inp["X"]
    try:
        with np.errstate(all="ignore"):
            r = hp.lml(X, inp["y"], inp["alpha"], h, inp["stationary"], inp["form"])
            lp = np.float64(prior + r["lml"])
    except np.linalg.LinAlgError:
        return bad
    if not np.isfinite(lp):
        return bad
    scale = float(r["scale"] + np.abs(terms).sum())
    sens = 0.0
    if dw:
        from oracle import gp_oracle as O

        ad = np.broadcast_to(inp["alpha"], (inp["n"],))
        sens = P.err_lml(O.lml(P.to32(P.f(X)), inp["y"], ad, h, inp["stationary"], inp["form"]), r) / P.F32
    return float(lp), scale, P.kappa_of(P.f(X), inp["alpha"], h, inp["stationary"], inp["form"]), sens


def lp_scale(inp, q):
    """The absolute sum a correct fp64 evaluation of lp(q) can lose digits on: ``scale`` of ``hp_oracle.lml`` + sum_k |prior_k|."""
    return lp_ld(inp, q)[1]


def _host_fns(inp, slip):
    fns = list(inp["fns"])
    if slip == "no_jacobian":
        jac = {1: 0.5, 2: 1.0, 3: 0.0}
        fns = [(lambda t, f=f, j=jac[int(k)]: f(t) - j * t) for f, k in zip(fns, inp["prior_kind"])]
    return fns


def _warp_read(inp, q, slip, ctx):
    """The 2 d warp parameters a proposal's LML is computed under: its own last entries, or what a slip reads instead.
    ``ctx``: the mover's current row ``s``, all proposals of the half-step ``qs`` and this proposal's index ``i``."""
    ng, nw, p = inp["ng"], inp["nwarp"], inp["p"]
    if slip == "warp_of_mover":
        return ctx["s"][ng:]
    if slip == "warp_shared":
        return ctx["qs"][0][ng:]
    if slip == "warp_offset_hp":  # entries hp .. hp + 2 d of the flat (proposal, entry) array; zeros behind its end
        flat = np.concatenate([np.concatenate(ctx["qs"]), np.zeros(p)])
        lo = ctx["i"] * p + inp["d"] + 2
        return flat[lo : lo + nw]
    if slip == "alpha_beta_swapped":
        return np.concatenate([q[ng + nw // 2 :], q[ng : ng + nw // 2]])
    return q[ng:]


def lp_64(inp, q, slip=None, ctx=None):
    """lp of position q in fp64 as the host-driven loop computes it: the host callables of the kernel entries summed in theta
    order (+ those of the warp entries, pair by pair on a sum of their own: ``_eval_warp_priors``) + ``gp_oracle.lml`` (warped:
    ``gp_oracle.lml_warped``, scipy's Beta CDF); non-finite -> -inf, and the contract of the warp entries as in ``lp_ld``."""
    from oracle import gp_oracle as O

    ng, dw = inp["ng"], inp["nwarp"] // 2
    h_src = np.roll(inp["h_src"], 1) if slip == "hsrc_shift" else inp["h_src"]
    with np.errstate(all="ignore"):
        fns = _host_fns(inp, slip)
        prior = 0.0
        for f, t in zip(fns[:ng], q[:ng]):
            prior = prior + float(f(t))
        if dw and slip != "warp_priors_dropped":
            w = 0.0
            for k in range(dw):
                w = w + (float(fns[ng + k](q[ng + k])) + float(fns[ng + dw + k](q[ng + dw + k])))
            prior = prior + w
        h = _canonical(inp, q, h_src)
        if slip == "fixed_counted":
            d = _default_callables()
            for j, s in enumerate(inp["h_src"]):
                if s < 0:
                    prior = prior + float(d[inp["hroles"][j]](h[j]))
        if not math.isfinite(prior):
            return -np.inf
        ad = np.broadcast_to(inp["alpha"], (inp["n"],))
        if dw and slip != "warp_identity":
            wv = _warp_read(inp, q, slip, ctx)
            if not _warp_ok(wv):
                return -np.inf
            lp = prior + float(O.lml_warped(inp["X"], inp["y"], ad, h, wv, inp["stationary"], inp["form"]))
        else:
            lp = prior + float(O.lml(inp["X"], inp["y"], ad, h, inp["stationary"], inp["form"]))
    return lp if math.isfinite(lp) else -np.inf


# ------------------------------------------------------------------------------------------------------------------------------
# the replay
# ------------------------------------------------------------------------------------------------------------------------------
def _run(inp, lpfn, chain_early=False, stale_partner=False):
    """One resident run restated.  ``lpfn(q, ctx) -> (lp, scale, kappa, sens)``, ``ctx`` = the mover's current row ``s``, all
    proposals of the half-step ``qs`` and the proposal's index ``i`` (what the warp slips read).  Returns a dict: the five arrays
    of ``Context.mcmc_run`` and per accept test (half-step, row) ``lp``, ``accepted``, ``finite`` (all four operands),
    ``margin``, ``scale``, ``kappa`` and ``sens`` of the proposal and of the mover's own log-probability; ``lps_scale`` /
    ``lps_kappa`` / ``lps_sens`` beside ``lps``."""
    movers, partners, zz, factors, logu = inp["plan"]
    nhalf, Ns = movers.shape
    W, p = inp["coords0"].shape
    coords, logp = inp["coords0"].copy(), inp["logp0"].copy()
    sc, kp, se = inp["scale0"].copy(), inp["kappa0"].copy(), inp["sens0"].copy()
    nacc = np.zeros(W, dtype=np.int64)
    chain, lps = np.empty((nhalf // 2, W, p)), np.empty((nhalf // 2, W))
    lsc, lkp, lse = np.empty((nhalf // 2, W)), np.empty((nhalf // 2, W)), np.empty((nhalf // 2, W))
    rec = {k: np.full((nhalf, Ns), np.nan) for k in ("lp", "margin", "scale", "kappa", "sens", "scale_old", "kappa_old", "sens_old")}
    rec["accepted"], rec["finite"] = np.zeros((nhalf, Ns), dtype=bool), np.zeros((nhalf, Ns), dtype=bool)
    before = coords.copy()  # the ensemble before the previous half-step's accepts
    for h in range(nhalf):
        src = before if stale_partner else coords
        before = coords.copy()
        new, qs = [], []
        for i in range(Ns):  # every proposal of the half-step, then their log-probabilities: as the step kernel
            s, c = coords[int(movers[h, i])], src[int(partners[h, i])]
            with np.errstate(all="ignore"):
                qs.append(c - (c - s) * zz[h, i])
        for i in range(Ns):
            m, q = int(movers[h, i]), qs[i]
            lp, scale, kappa, sens = lpfn(q, dict(s=coords[m], qs=qs, i=i))
            f, old, u = float(factors[h, i]), float(logp[m]), float(logu[h, i])
            t = f + lp - old  # (Python floats: -inf - -inf is a quiet NaN)
            acc = t > u
            fin = all(math.isfinite(v) for v in (f, lp, old, u))
            rec["lp"][h, i], rec["accepted"][h, i], rec["finite"][h, i] = lp, acc, fin
            rec["scale"][h, i], rec["kappa"][h, i], rec["sens"][h, i] = scale, kappa, sens
            rec["scale_old"][h, i], rec["kappa_old"][h, i], rec["sens_old"][h, i] = sc[m], kp[m], se[m]
            if fin:
                rec["margin"][h, i] = abs(t - u)
            if acc:
                new.append((m, q, lp, scale, kappa, sens))
        for m, q, lp, scale, kappa, sens in new:
            coords[m], logp[m], sc[m], kp[m], se[m] = q, lp, scale, kappa, sens
            nacc[m] += 1
        if (h & 1) == (0 if chain_early else 1):
            chain[h >> 1], lps[h >> 1], lsc[h >> 1], lkp[h >> 1], lse[h >> 1] = coords, logp, sc, kp, se
    rec.update(chain=chain, lps=lps, coords=coords, logp=logp, naccepted=nacc, lps_scale=lsc, lps_kappa=lkp, lps_sens=lse,
               logp_scale=sc, logp_kappa=kp, logp_sens=se)
    return rec


@functools.lru_cache(maxsize=None)
def replay_full(cid):
    inp = inputs(cid)
    return _run(inp, lambda q, ctx: lp_ld(inp, q))


def replay(cid):
    """chain, lps, coords, logp, naccepted, margins of the long-double replay of a case; ``margins`` holds
    |factors + lp - logp[mover] - logu| of every accept test whose operands are all finite."""
    r = replay_full(cid)
    return r["chain"], r["lps"], r["coords"], r["logp"], r["naccepted"], r["margin"][r["finite"]]


@functools.lru_cache(maxsize=None)
def replay64(cid, slip=None):
    inp = inputs(cid)
    return _run(inp, lambda q, ctx: (lp_64(inp, q, slip, ctx), np.nan, np.nan, np.nan), chain_early=slip == "chain_early",
                stale_partner=slip == "stale_partner")


def margin_bounds(cid):
    """Per accept test the bound its margin has to clear: 1000 x the LML tolerance on ``lp_scale``, of the proposal and of the
    mover's own log-probability (both enter the test), at their own kappas (and warp sensitivities).  NaN where the test is
    not finite."""
    r, n = replay_full(cid), inputs(cid)["n"]
    out = np.full(r["margin"].shape, np.nan)
    for idx in zip(*np.nonzero(r["finite"])):
        out[idx] = 1000.0 * (P.tol("lml", r["kappa"][idx], n, r["sens"][idx]) * r["scale"][idx]
                             + P.tol("lml", r["kappa_old"][idx], n, r["sens_old"][idx]) * r["scale_old"][idx])
    return out


def proposal_tolerance(cid):
    """``_precision.tol("lml", kappa, n, sens)`` of every proposal of the replay whose lp is finite, in units of ``lp_scale``; NaN
    elsewhere."""
    r, n = replay_full(cid), inputs(cid)["n"]
    f = np.vectorize(lambda k, s: P.tol("lml", k, n, s) if np.isfinite(k) else np.nan)
    return f(r["kappa"], r["sens"])


def lps_tolerance(cid):
    """(tol of ``lps``, tol of ``logp_out``) in units of ``lp_scale``: ``_precision.tol("lml", kappa, n, sens)`` at the stored
    position; NaN where the reference is -inf."""
    r, n = replay_full(cid), inputs(cid)["n"]
    f = np.vectorize(lambda k, s: P.tol("lml", k, n, s) if np.isfinite(k) else np.nan)
    return f(r["lps_kappa"], r["lps_sens"]), f(r["logp_kappa"], r["logp_sens"])
