// What the library launches for a batch of LML factorisations: decided ONCE, here, in pure host code (plain C++17: no HIP type,
// no bgp_ctx; tools/plan_check.cpp compiles this header alone).  bgp_plan_lml maps a shape, the context's modes and the live
// switches to a BgpLmlPlan; bgp_lml_schedule spells the launches of one walker group out, for the executor (bgp_chol.hip) and for
// the launch count alike.  The executors -- bgp_lml_enqueue_dev (bgp_api.hip), bgp_launch_lml_group and
// bgp_launch_cholesky_persist (bgp_chol.hip), post_factor_child (bgp_post.hip) -- decide nothing.  The measured boundaries and
// the environment switches that feed them live here too (DESIGN.md sections 3, 4 and 19).
#pragma once
#include <cstdlib>
#include <cstring>

#if defined(__HIPCC__)
#define BGP_PLAN_HD static __host__ __device__ __forceinline__  // (the launch-free kernel counts its tasks with the same functions)
#else
#define BGP_PLAN_HD static inline
#endif

// ------------------------------------------------------------------------------------------
// The environment switches: every BGP_* name libbgp.so reads, WHEN it is read, its default and its meaning.  Every getenv of the
// library goes through bgp_switch; bgp_ctx_create's warning about an unknown BGP_* variable knows these names and the ones that
// only the Python layer and bench.py read (bgp_switches_elsewhere).
//   per context:  at bgp_ctx_create (BGP_PERSIST and BGP_PANEL_FUSED again by bgp_set_persist(-1) / bgp_set_panel_fused(-1))
//   per process:  once, at the first use (BGP_PS_PAIR / _GEN / _TRACE / _TIMEOUT_*: at the first launch-free call); the readers below are
//                 inline functions with external linkage, so their caches are ONE object per library, not one per translation unit
//   per call:     at every LML batch (the tests flip it inside one process)
// ------------------------------------------------------------------------------------------
enum BgpSwitch {
  BGP_SW_STREAMS, BGP_SW_PERSIST, BGP_SW_PANEL_FUSED, BGP_SW_PANELS,
  BGP_SW_WAIT, BGP_SW_DEBUG_TIMES, BGP_SW_PS_COOLDOWN, BGP_SW_PS_TIMEOUT_MS, BGP_SW_PS_TIMEOUT_TICKS, BGP_SW_PS_PAIR, BGP_SW_PS_GEN,
  BGP_SW_PS_TRACE, BGP_SW_COMM_TIMEOUT_S,
  BGP_SW_SYRK_GEN, BGP_SW_GCOV_CHUNK, BGP_SW_KG_CHUNK, BGP_SW_JES_CHUNK, BGP_SW_ITEM_CHUNK, BGP_SW_ROW_CHUNK,
  BGP_SW_COUNT
};
enum BgpSwitchRead { BGP_READ_CONTEXT, BGP_READ_PROCESS, BGP_READ_CALL };
struct BgpSwitchRow {
  const char* name;
  BgpSwitchRead when;
  const char* dflt;
  const char* meaning;
};
static const BgpSwitchRow bgp_switches[BGP_SW_COUNT] = {
    {"BGP_STREAMS", BGP_READ_CONTEXT, "1", "walker-group streams an LML batch of the launch schedule is split over (1..8)"},
    {"BGP_PERSIST", BGP_READ_CONTEXT, "by shape", "launch-free factorisation: 0 never, 1 whenever the batch fits"},
    {"BGP_PANEL_FUSED", BGP_READ_CONTEXT, "by shape", "diagonal block and panel solve in one launch: 0 never, 1 every column with a solve"},
    {"BGP_PANELS", BGP_READ_CONTEXT, "4 from n = 1536, else 2", "block columns per trailing update of the launch schedule (1..64)"},
    {"BGP_WAIT", BGP_READ_PROCESS, "poll", "block: the runtime's blocking wait instead of the active one"},
    {"BGP_DEBUG_TIMES", BGP_READ_PROCESS, "off", "set: host times of a training-set upload on stderr"},
    {"BGP_PS_COOLDOWN", BGP_READ_PROCESS, "256", "eligible calls on the launch schedule after a launch-free time-out"},
    {"BGP_PS_TIMEOUT_MS", BGP_READ_PROCESS, "500", "longest single wait inside the launch-free kernel, ms"},
    {"BGP_PS_TIMEOUT_TICKS", BGP_READ_PROCESS, "unset", "the same bound in 100 MHz ticks (tests: a bound no wait can meet)"},
    {"BGP_PS_PAIR", BGP_READ_PROCESS, "by shape", "launch-free path: 0 one, 1 two chain workgroups per matrix"},
    {"BGP_PS_GEN", BGP_READ_PROCESS, "by shape", "launch-free path: 0 Gram kernel in front, 1 Gram blocks by the tile workers"},
    {"BGP_PS_TRACE", BGP_READ_PROCESS, "0", "1: in-kernel time stamps of the launch-free call (bgp_debug_ps_trace)"},
    {"BGP_COMM_TIMEOUT_S", BGP_READ_PROCESS, "300", "longest wait for a peer of the multi-GPU exchange, s"},
    {"BGP_SYRK_GEN", BGP_READ_CALL, "1", "0: every Gram block by the Gram kernel, none generated inside the trailing update"},
    {"BGP_GCOV_CHUNK", BGP_READ_CALL, "by n and d", "query points per chunk of bgp_grad_cov, rounded up to 256 (tests: a small chunk against the default)"},
    {"BGP_KG_CHUNK", BGP_READ_CALL, "by n", "candidates per chunk of bgp_knowledge_gradient, rounded up to 128 (tests: a small chunk against the default)"},
    {"BGP_JES_CHUNK", BGP_READ_CALL, "by n", "candidates per chunk of bgp_joint_entropy, rounded up to 128 (tests: a small chunk against the default)"},
    {"BGP_ITEM_CHUNK", BGP_READ_CALL, "by the scratch budget", "upper bound on the posteriors per chunk of the batched posterior calls (tests: forced chunks against the default)"},
    {"BGP_ROW_CHUNK", BGP_READ_CALL, "by the scratch budget", "upper bound on the query rows / starts per chunk of bgp_predict_grad_batch, bgp_paths_eval, bgp_paths_minimize (tests)"},
};
// read elsewhere: by the Python layer and bench.py, never by libbgp.so
static const char* const bgp_switches_elsewhere[] = {"BGP_COMM_DIR", "BGP_COMM_PORT", "BGP_COMM_TCP", "BGP_COMM_JOB",
                                                     "BGP_DIST_BACKEND", "BGP_DIST_FORCE", "BGP_BENCH_TIMEOUT", "BGP_NO_ENV_DEFAULTS"};

static inline const char* bgp_switch(BgpSwitch s) { return getenv(bgp_switches[s].name); }
// 0 / 1 as set, -1 unset
static inline int bgp_switch_tristate(BgpSwitch s) {
  const char* e = bgp_switch(s);
  return e ? (atoi(e) != 0 ? 1 : 0) : -1;
}
// BGP_ITEM_CHUNK / BGP_ROW_CHUNK: an UPPER bound on a chunk that a scratch budget has sized -- min(chunk, N), so the switch shrinks
// a chunk and never enlarges it; unset, zero, negative or not a number: the budget alone decides
static inline size_t bgp_switch_cap(BgpSwitch s, size_t chunk) {
  const char* e = bgp_switch(s);
  const long long v = e ? atoll(e) : 0;
  return (v > 0 && (unsigned long long)v < chunk) ? (size_t)v : chunk;
}
static inline bool bgp_switch_known(const char* name, size_t len) {
  for (const BgpSwitchRow& r : bgp_switches)
    if (strlen(r.name) == len && strncmp(r.name, name, len) == 0) return true;
  for (const char* k : bgp_switches_elsewhere)
    if (strlen(k) == len && strncmp(k, name, len) == 0) return true;
  return false;
}
// the per-process switches of the launch-free call, each read at its first use
inline int bgp_switch_ps_pair() {
  static const int want = bgp_switch_tristate(BGP_SW_PS_PAIR);
  return want;
}
inline int bgp_switch_ps_gen() {
  static const int want = bgp_switch_tristate(BGP_SW_PS_GEN);
  return want;
}
inline bool bgp_switch_ps_trace() {
  static const bool want = bgp_switch_tristate(BGP_SW_PS_TRACE) == 1;
  return want;
}
// wall_clock64 ticks (100 MHz) a single wait inside the launch-free kernel may last.  Default 500 ms: a healthy call lasts at most
// ~20 ms, and two PROCESSES that share a GPU and meet in this path can block each other's resident workgroups (measured: one
// time-out in 1 800 calls each, results correct)
inline unsigned long long bgp_switch_ps_spin_limit() {
  static const unsigned long long limit = [] {
    const char* e = bgp_switch(BGP_SW_PS_TIMEOUT_MS);
    unsigned long long v = 100000ull * (unsigned long long)((e && atoi(e) > 0) ? atoi(e) : 500);
    const char* et = bgp_switch(BGP_SW_PS_TIMEOUT_TICKS);  // (tests: a bound no wait can meet)
    if (et && atoll(et) > 0) v = (unsigned long long)atoll(et);
    return v;
  }();
  return limit;
}

// ------------------------------------------------------------------------------------------
// The measured boundaries
// ------------------------------------------------------------------------------------------
// Shapes at which the tile workers generate the Gram blocks inside the launch-free kernel (PsArgs::gen) instead of a Gram kernel in
// front of it: where the chain is the bound and the tile side has the slack to take the extra work (measured: bgp_chol.hip)
// (tools/gen_probe.py, ms per LML call without -> with: 1024 x 24 0.488 -> 0.464, x 16 0.476 -> 0.456, x 8 0.460 -> 0.449; 768 x 32
// 0.383 -> 0.362; 1536 x 16 0.729 -> 0.719; 2048 x 8 0.927 -> 0.884; 512 x 32 0.260 -> 0.250; but 1024 x 32 0.522 -> 0.527, 2048 x 16
// 1.308 -> 1.357 and 3072 x 8 1.921 -> 1.936: there the tile side is the bound already and the blocks are extra work for it)
static inline bool bgp_ps_gen_auto_rule(int nblk, int B) { return nblk >= 4 && nblk <= 16 && B <= 32 && B * nblk <= 192; }
// Block columns of the launch schedule's LML path that take ONE fused launch (panel_kernel, bgp_chol.hip) instead of potrf_kernel +
// trsm4_kernel: nrb = row blocks under the diagonal block, B = matrices of the launch, ncu = the CUs the launch can count on (the
// device's, divided by the walker-group streams that factorise side by side).  bgp_panel_fused_wgs = workgroups per matrix, S.
// Measured per block column (config C: n = 2048 x 128 matrices, S = 2, one stream, rocprofv3 kernel trace, us, potrf + trsm4 -> fused):
//   nrb = 15: 31.8 + 130.7 -> 129.4   14: 31.0 + 113.9 -> 116.3   13: 30.6 + 105.9 -> 114.4   12: 30.8 + 100.5 -> 104.4
//   11: 31.9 + 92.5 -> 107.3   10: 31.7 + 84.1 -> 98.5   9: 31.2 + 72.6 -> 95.2   8: 30.8 + 65.4 -> 84.0   7: 31.1 + 60.4 -> 83.1
//   6: 30.9 + 47.6 -> 70.6   5: 31.1 + 44.5 -> 71.8   4: 31.2 + 37.5 -> 59.6   3: 31.0 + 27.9 -> 57.7   2: 31.0 + 18.2 -> 46.7
//   but nrb = 1: 30.8 + 12.3 -> 44.6 (one row block: 13 us behind the diagonal block's 31 either way, and the separate solve splits
//   it over two workgroups per matrix).  A fused launch costs the diagonal block plus ~12.3 us per row block of its busiest
//   workgroup: 1.481 -> 1.284 ms per half-step over the fifteen columns.
// So: at least two row blocks and at least two workgroups per matrix.  (One workgroup per matrix -- more than ncu / 2 matrices --
// leaves the solve to as many CUs as there are matrices, one row block after the other: ahead in two whole-call probes (1536 x 200:
// 5.48 -> 5.36 ms, 640 x 256: 0.89 -> 0.85), no per-column table yet: not taken.  docs/EXPERIMENTS.md G29.)
static inline int bgp_panel_fused_wgs(int nrb, int B, int ncu) {
  const int B8 = 8 * ((B + 7) / 8), s = ncu / B8;
  return s < 1 ? 1 : (s > nrb ? (nrb < 1 ? 1 : nrb) : s);
}
static inline bool bgp_panel_fused_rule(int nrb, int B, int ncu) { return nrb >= 2 && bgp_panel_fused_wgs(nrb, B, ncu) >= 2; }
// Batch sizes at which the launch-free factorisation wins over the multi-launch schedule (tools/persist_probe.py on MI355X,
// DESIGN.md section 4; wall time per LML call, launch schedule / launch-free, by n and number of matrices):
//   n =  768: 8: 0.91, 32: 1.07;   896: 16: 1.02, 48: 1.11
//   n = 1024: 1: 0.93, 4: 0.95, 8: 0.98, 16: 1.06, 24: 1.12, 32: 1.19, 48: 1.09, 64: 0.97;  975 x 50 (config E): 1.10
//   n = 1280: 8: 1.04, 32: 1.15, 48: 0.96;   1536: 1: 1.01, 4: 1.06, 16: 1.29, 32: 1.06, 48: 0.92
//   n = 2048: 1: 1.02, 4: 1.12, 9: 1.40, 16: 1.22, 24: 1.07, 32: 0.99, 48: 0.88;   3072: 1: 1.08, 8: 1.25, 16: 1.06, 24: 0.95
//   n = 4096: 1: 1.15, 2: 1.12, 4: 1.08, 8: 1.13, 16: 0.98;  one 10 112 x 10 112 covariance (sample_y): 1.15;  n <= 640: 0.92-0.97
// So: at least 6 block columns, matrices x block columns <= 400 (beyond that the tile side is the bound and the launch
// schedule's kernels are the better tile workers), and >= 100 unless there are at least 12 block columns.
// Chain PAIRS (two chain workgroups per matrix that alternate over the block columns; the critical pre-updates in quadrants that
// follow the chain's and the streamed solves' blocks column block by column block, on a critical pool of their own: bgp_pf.h,
// bgp_chol.hip) win where the chain is the bound -- few matrices.  Wall ms per LML call, best of {launches, launch-free} ->
// pairs (tools/persist_probe.py, MI355X, round 4):
//   n =  384 x 1: 0.173 -> 0.159;   512 x 1 / 4 / 8: 0.220 / 0.225 / 0.223 -> 0.197 / 0.203 / 0.218;   768 x 1 / 16: 0.318 / 0.356 -> 0.271 / 0.317
//   n = 1024 x 1 / 8 / 16 (32: 0.528 -> 0.630): 0.413 / 0.447 / 0.475 -> 0.349 / 0.414 / 0.430;   1280 x 12: 0.601 -> 0.554;   1152 x 14: 0.543 -> 0.500
//   n = 1408 x 9 / 12 (16: 0.663 -> 0.671): 0.639 / 0.652 -> 0.611 / 0.624;   1536 x 1 / 4 / 8 / 9 / 12 (16: 0.763 -> 0.789): 0.650 / 0.664 / 0.675 / 0.712 / 0.729 -> 0.506 / 0.546 / 0.579 / 0.659 / 0.722
//   n = 1792 x 4 / 8 (12: 0.919 -> 0.953): 0.765 / 0.789 -> 0.623 / 0.662;   2048 x 1 / 2 / 4 / 8 (12: 1.207 -> 1.284, 16: 1.305 -> 1.503): 0.861 / 0.865 / 0.889 / 0.925 -> 0.653 / 0.673 / 0.746 / 0.839
//   n = 2560 x 4 / 6 (8: 1.275 -> 1.381): 1.154 / 1.234 -> 1.081 / 1.230;   3072 x 1 / 2 / 3 / 4 (6: 1.798 -> 1.908): 1.326 / 1.341 / 1.473 / 1.639 -> 1.023 / 1.195 / 1.399 / 1.609
//   n = 3584 x 2 / 3 (4: 2.191 -> 2.179): 1.636 / 1.904 -> 1.504 / 1.817;   4096 x 1 / 2 / 3 (4: 2.831 -> 2.969): 1.730 / 2.112 / 2.472 -> 1.327 / 1.862 / 2.398
//   n = 4992 x 1 / 5120 x 1 (x 2: 2.906 -> 2.893) / 6144 x 1: 2.113 / 2.190 / 2.629 -> 1.601 / 1.641 / 2.326;   not 7168 x 1 (3.195 -> 3.189), 8192 x 1 (4.201 -> 4.406), 10 112 x 1
static inline bool bgp_pair_auto_rule(int nblk, int nb) {
  if (nblk < 3) return false;
  if (nblk <= 10) return nb <= 16 && nb * nblk * nblk <= 1200;
  if (nblk <= 12) return nb <= 12;
  return nb <= 8 && nb * nblk * nblk <= (nb <= 3 ? 3100 : 2400);  // (the tile side's work goes with matrices x block columns^2)
}
static inline bool bgp_persist_auto_rule(int nblk, int nb) {
  return bgp_pair_auto_rule(nblk, nb) || (nblk >= 6 && nb * nblk <= 400 && (nblk >= 12 || nb * nblk >= 100));
}
// Can this batch take the launch-free path?  (at least two block columns; a CU per matrix and at least as many, and at
// least 32, left for the tile workers -- a partitioned device with 32 CUs never takes it)
static inline bool bgp_persist_fits(int nblk, int ncu, int B) {
  return B >= 1 && B <= 64 && nblk >= 2 && nblk <= 255 && ncu - B >= (B > 32 ? B : 32);
}

// Tasks of the launch-free kernel's tile role (bgp_ps.hip): the critical tasks per block column and matrix are S(J+2, J), the np
// parts of P(J+2) (np = PsArgs::psplit: 2 column slices or 4 quadrants), the PS_ND(np) parts of Dg(J+2) and the PS_NQ(np) quadrants
// Q ahead of S(J+2, J)
#define PS_ND(np) ((np) == 4 ? 3 : 1)
#define PS_NQ(np) ((np) == 4 ? 4 : 0)
BGP_PLAN_HD int ps_crit_per_matrix(int nblk, int np) { return nblk > 2 ? (np + 1 + PS_ND(np) + PS_NQ(np)) * (nblk - 2) : 0; }
BGP_PLAN_HD int ps_bulk_per_matrix(int nblk) { return nblk > 3 ? (nblk - 3) * (nblk - 2) / 2 : 0; }
BGP_PLAN_HD int ps_tasks_per_matrix(int nblk, int np) { return ps_crit_per_matrix(nblk, np) + ps_bulk_per_matrix(nblk); }
static inline int bgp_ps_total_tasks(int B, int nblk, int np, int gen) {
  return B * (ps_tasks_per_matrix(nblk, np) + (gen ? nblk * (nblk + 1) / 2 : 0));
}

// ------------------------------------------------------------------------------------------
// The planner
// ------------------------------------------------------------------------------------------
#define BGP_PLAN_MATERN52 3      // bgp_kernel_spec::stationary, ::form of include/bgp.h (BGP_MATERN52, BGP_FORM_PRODUCT)
#define BGP_PLAN_FORM_PRODUCT 0
#define BGP_PLAN_GEN_MAX_D 16    // input dimensions the trailing update's Gram generator stages in one pass (KB_DK, bgp_kb.h)

struct BgpLmlShape {
  // the batch: nb matrices of nblk block columns of 128 (n rows, d input dimensions) on a device of ncu CUs
  int n, nblk, d, stationary, form, ncu, nb;
  int warped;  // every matrix from its own warped inputs (bgp_lml_batch_warped)
  int given;   // the matrices are in the workspace already (host Gram matrices, the covariances of sample_y): nothing is built or generated
  // the context's modes
  int timing, persist, panel_fused, panels, panels_auto, nstreams, streams_auto;
  // the live switches: BGP_SYRK_GEN (0 / 1), BGP_PS_PAIR, BGP_PS_GEN (0 / 1, -1 by shape)
  int syrk_gen, ps_pair, ps_gen;
  // The launch-free path may be taken now: no time-out keeps it off, the resident sampler does not forbid it.  bgp_ps_allowed COUNTS
  // the cool-down and may be asked for eligible batches only: the caller sets this to "not forbidden", asks
  // bgp_plan_wants_launch_free, then bgp_ps_allowed, and plans with the answer (bgp_plan_for, bgp_common.h).
  int ps_permitted;
};

// BGP_SYRK_GEN is read at every call; BGP_PS_PAIR / BGP_PS_GEN once per process, when the first batch takes (or, for
// bgp_debug_lml_plan, would take) the launch-free path -- the only path that reads them
static inline void bgp_shape_read_call_switches(BgpLmlShape& s) {
  const char* e = bgp_switch(BGP_SW_SYRK_GEN);  // (read per call: the tests flip it inside one process)
  s.syrk_gen = (e && e[0] == '0') ? 0 : 1;
  s.ps_pair = s.ps_gen = -1;
}
static inline void bgp_shape_read_ps_switches(BgpLmlShape& s) {
  s.ps_pair = bgp_switch_ps_pair();
  s.ps_gen = bgp_switch_ps_gen();
}

enum BgpLmlPath {
  BGP_PATH_SMALL = 0,        // n <= 128: Gram generation, factorisation and LML in ONE launch (potrf_kernel<1, ..>)
  BGP_PATH_LAUNCH_FREE = 1,  // ONE persistent kernel (ps_kernel, bgp_ps.hip), the Gram matrices built inside it or in front of it
  BGP_PATH_LAUNCHES = 2      // the launch schedule, walker group by walker group (bgp_lml_schedule)
};

struct BgpLmlPlan {
  BgpLmlShape in;
  int path;
  // walker groups: `share` streams factorise side by side (a fused launch sizes its grid for ncu / share CUs); group g is the
  // slice [g * gsz, g * gsz + group_nb(g)) on a stream of its own -- ONE group runs on the context's stream
  int share, gsz, ngroups;
  int P;  // block columns per trailing update
  // launch-free path (PsArgs, bgp_common.h)
  int pair, Bpad, nchain, psplit, dsplit, ncrit_stream, ncrit, ps_gen, total, tile_wgs;
  int gram_front;  // ... the Gram kernel goes in front of it (warped batches: always), 0: its tile workers generate the blocks (ps_gen) or the matrices are given

  int group_nb(int g) const { return in.nb - g * gsz < gsz ? in.nb - g * gsz : gsz; }
  // Gram generation inside the trailing update of group g (bgp_s4.h, S4GenF): where the pipelined Gram build would run anyway
  // (the same threshold), on matrices of at least two block columns with at most 16 input dimensions (one staging pass; at d = 32
  // the generator measured +1.2 % / -0.1 % at n = 4096 x 8 / 16 matrices, against -2 .. -4.5 % at d <= 16 from 32 matrices on:
  // tools/gen_shapes_probe.py); BGP_SYRK_GEN=0 switches it off (A/B measurements).
  int gen(int g) const {
    if (path != BGP_PATH_LAUNCHES || in.given) return 0;
    const int B8 = 8 * ((group_nb(g) + 7) / 8);
    return in.syrk_gen && in.d <= BGP_PLAN_GEN_MAX_D && in.nblk >= 2 && B8 * (in.nblk * (in.nblk + 1) / 2) >= 2048;
  }
  // workgroups per matrix of the fused launch of block column k in group g; 0: potrf_kernel + trsm4_kernel
  int fused_wgs(int g, int k) const {
    const int nrb = in.nblk - k - 1, ncu = in.ncu / (share < 1 ? 1 : share);
    const bool fuse = nrb > 0 && (in.panel_fused == 1 || (in.panel_fused == -1 && bgp_panel_fused_rule(nrb, group_nb(g), ncu)));
    return fuse ? bgp_panel_fused_wgs(nrb, group_nb(g), ncu) : 0;
  }
};

static inline bool bgp_plan_small(const BgpLmlShape& s) { return s.nblk == 1 && !s.warped && !s.given; }

// Everything that selects the launch-free path but the cool-down's answer: automatic below 64 matrices per call when the matrices
// have at least two block columns; never under per-launch timing (there are no launches to time)
static inline bool bgp_plan_wants_launch_free(const BgpLmlShape& s) {
  return !bgp_plan_small(s) && !s.timing && s.ps_permitted && bgp_persist_fits(s.nblk, s.ncu, s.nb) &&
         (s.persist == 1 || (s.persist == -1 && bgp_persist_auto_rule(s.nblk, s.nb)));
}

static inline BgpLmlPlan bgp_plan_lml(const BgpLmlShape& s) {
  BgpLmlPlan p{};
  p.in = s;
  const int nblk = s.nblk, nb = s.nb, ncu = s.ncu;
  // walker groups on separate streams (sizes are multiples of 8: one matrix slot per XCD)
  p.share = (s.streams_auto && nb < 64) ? 1 : s.nstreams;
  p.gsz = ((nb + p.share - 1) / p.share + 7) / 8 * 8;
  if (p.share == 1 || nb < 16 || s.warped || s.given) {
    p.share = 1;
    p.gsz = nb;
  }
  p.ngroups = nb > 0 ? (nb + p.gsz - 1) / p.gsz : 0;
  // P block columns per trailing update: 4 from n = 1536 upwards (config C: 16.5 vs 17.1 ms per step against P = 2
  // with the LDS-DMA kernels, whose look-ahead column launches are cheap enough), 2 below (P = 2, 3, 4 are equal
  // within noise at n = 1024); BGP_PANELS fixes it.
  p.P = s.panels_auto ? (nblk >= 12 ? 4 : 2) : s.panels;
  p.path = bgp_plan_small(s) ? BGP_PATH_SMALL : (bgp_plan_wants_launch_free(s) ? BGP_PATH_LAUNCH_FREE : BGP_PATH_LAUNCHES);
  if (p.path != BGP_PATH_LAUNCH_FREE) return p;
  // chain pairs (bgp_pf.h): two workgroups per matrix alternate over the block columns, the idle one preparing the next
  // diagonal block UNDER the other's factorisation; needs 2 * Bpad CUs and at least as many (and 32) left for the tile role.
  // BGP_PS_PAIR = 0 / 1 fixes it.
  p.Bpad = 8 * ((nb + 7) / 8);
  // automatic: where the chain is the bound and the pairs measured faster (bgp_pair_auto_rule)
  const bool pair_fits = nblk >= 3 && ncu - 2 * p.Bpad >= (nb > 32 ? nb : 32);
  p.pair = (pair_fits && (s.ps_pair == 1 || (s.ps_pair == -1 && bgp_pair_auto_rule(nblk, nb)))) ? 1 : 0;
  p.nchain = p.pair ? 2 * p.Bpad : nb;
  // P(I) -- the pre-update of block (I, I-1) that the chain waits for -- as ONE task behind a single chain workgroup, in four
  // 64 x 64 quadrants (and Dg(I) in three) behind chain pairs, whose cycle runs THROUGH this task (the
  // two-slice and the mixed variants measured slower and left the library in round 5)
  p.psplit = p.pair ? 4 : 1;
  p.dsplit = p.psplit == 4 ? 3 : 1;
  p.total = bgp_ps_total_tasks(nb, nblk, p.psplit, 0);
  // pair mode: the panel solves S(J+2, J) and S(J+3, J) follow pf_block(J) row block by row block (S(J+3, J) feeds the
  // quadrants ahead of the next column's critical solve; streaming fewer measured slower)
  p.ncrit_stream = 3;
  p.tile_wgs = p.total < ncu - p.nchain ? p.total : ncu - p.nchain;
  // critical pool of the tile role: the three tasks at the head of a block column -- S(J+2, J), P(J+2), Dg(J+2) -- get
  // workgroups of their own, one per task of a column.  Measured in round 3: with up to ~10 block columns the chain waits less
  // (n = 1024 x 32: 0.63 -> 0.59 ms, 975 x 50: 0.93 -> 0.84); with more, these left-looking tasks are long and want the
  // look-ahead the single list gives them (n = 2048 x 9: 1.20 -> 1.37 ms with the pool).
  // Chain pairs with more block columns: their 12 critical tasks per column and matrix are SHORT (quadrants that follow their
  // inputs) and numerous -- behind the long bulk solves of one list they start late: a pool of 48 (one matrix) / 96 workgroups
  // (n = 4096 x 1: 1.361 -> 1.330 ms, x 2: 2.022 -> 1.861; 1536 x 4: 0.588 -> 0.545, x 8: 0.666 -> 0.578, x 9: 0.847 -> 0.651)
  // One chain workgroup per matrix, re-measured at the end of round 4: the pool only pays from ~40 matrices on (975 x 50: 0.743 ->
  // 0.725 ms, 896 x 48: 0.543 -> 0.527); below, the single list is 2-5 % faster now (1024 x 32: 0.528 -> 0.518, x 24: 0.518 ->
  // 0.493, 1152 x 24: 0.580 -> 0.555, 975 x 25: 0.525 -> 0.508)
  const int half = p.tile_wgs / 2, per_col = (p.psplit + 1 + p.dsplit + (p.psplit == 4 ? 4 : 0)) * nb, pool = nb == 1 ? 48 : 96;
  p.ncrit = nblk <= 10 ? ((p.pair || nb > 32) ? (per_col < half ? per_col : half) : 0)
                       : (p.pair && p.psplit == 4 ? (pool < half ? pool : half) : 0);
  // (at least one workgroup is left for the bulk list whenever it has tasks: critical tasks spin-wait on bulk solves of the
  // previous column)
  if (p.ncrit > p.tile_wgs - 1) p.ncrit = p.tile_wgs - 1 > 0 ? p.tile_wgs - 1 : 0;
  // A plain LML batch (unwarped inputs, the context's hyper-parameters, diagonal additions): with one chain workgroup per matrix,
  // one ticket list and the default kernel form the tile workers generate the Gram matrices block by block at the head of that
  // list -- the chain starts on block (0, 0) ~10 us into the launch instead of behind a whole Gram kernel and a kernel boundary
  // (n = 1024 x 32: 63 + ~15 us) -- else the Gram kernel goes in front as before.  BGP_PS_GEN = 0 / 1 fixes it.
  const bool can = !s.given && !s.warped && !p.pair && p.ncrit == 0 && p.total > 0 && s.stationary == BGP_PLAN_MATERN52 &&
                   s.form == BGP_PLAN_FORM_PRODUCT;
  p.ps_gen = (can && (s.ps_gen == 1 || (s.ps_gen == -1 && bgp_ps_gen_auto_rule(nblk, nb)))) ? 1 : 0;
  p.gram_front = !s.given && !p.ps_gen;
  if (p.ps_gen) {
    p.total = bgp_ps_total_tasks(nb, nblk, p.psplit, 1);
    p.tile_wgs = p.total < ncu - p.nchain ? p.total : ncu - p.nchain;  // (gen adds tasks)
  }
  return p;
}

// ------------------------------------------------------------------------------------------
// The launch schedule of walker group g, launch by launch.  A group of P block columns is factorised with look-ahead column
// updates only, then everything to its right is updated ONCE with the whole K = 128 P panel (P times fewer passes over the
// trailing matrix):
//   potrf(k) trsm(k) | col k+1 (K=128) | potrf(k+1) trsm(k+1) | col k+2 (K=256) | ... | rest (K = 128 P)
// gen: only block column 0 of the kernel matrices has been built; the updates of the first panel group generate every other block
// as they touch it first.
// ------------------------------------------------------------------------------------------
enum BgpStepKind {
  BGP_STEP_PANEL,   // block column k: diagonal block and panel solve in one launch, S workgroups per matrix (timed under "trsm")
  BGP_STEP_POTRF,   // diagonal block k
  BGP_STEP_TRSM,    // panel solve of block column k
  BGP_STEP_COLUMN,  // look-ahead: block column j with the panels k .. (K = their width)
  BGP_STEP_UPDATE   // everything from block column j on with the panels k .. (K = their width)
};
struct BgpStep {
  int kind, k, S, K, j, gen;
};
template <class F>
static inline void bgp_lml_schedule(const BgpLmlPlan& p, int g, F&& launch) {
  const int nblk = p.in.nblk, gen = p.gen(g);
  for (int k = 0; k < nblk;) {
    const int np = p.P < nblk - k ? p.P : nblk - k;
    for (int j = 0; j < np; j++) {
      const int S = p.fused_wgs(g, k + j);
      if (S) {
        launch(BgpStep{BGP_STEP_PANEL, k + j, S, 0, 0, 0});
      } else {
        launch(BgpStep{BGP_STEP_POTRF, k + j, 0, 0, 0, 0});
        if (k + j + 1 >= nblk) break;
        launch(BgpStep{BGP_STEP_TRSM, k + j, 0, 0, 0, 0});
      }
      if (j + 1 < np) launch(BgpStep{BGP_STEP_COLUMN, k, 0, 128 * (j + 1), k + j + 1, gen && k == 0});
    }
    if (nblk - (k + np) > 0) launch(BgpStep{BGP_STEP_UPDATE, k, 0, 128 * np, k + np, gen && k == 0});
    k += np;
  }
}

// The launches a plan enqueues, by timing category (bgp_last_timing: a fused panel launch counts under trsm, a look-ahead column
// under syrk as well), and the fused and generating ones among them
struct BgpLmlLaunches {
  int kbuild, potrf, trsm, syrk, columns, fused, generating, launch_free;
};
static inline BgpLmlLaunches bgp_plan_launches(const BgpLmlPlan& p) {
  BgpLmlLaunches n{};
  if (p.path == BGP_PATH_SMALL) {
    n.potrf = 1;
  } else if (p.path == BGP_PATH_LAUNCH_FREE) {
    n.kbuild = p.gram_front;
    n.launch_free = 1;
  } else {
    for (int g = 0; g < p.ngroups; g++) {
      n.kbuild += p.in.given ? 0 : 1;
      bgp_lml_schedule(p, g, [&](const BgpStep& s) {
        n.potrf += s.kind == BGP_STEP_POTRF;
        n.trsm += s.kind == BGP_STEP_TRSM || s.kind == BGP_STEP_PANEL;
        n.fused += s.kind == BGP_STEP_PANEL;
        n.syrk += s.kind == BGP_STEP_COLUMN || s.kind == BGP_STEP_UPDATE;
        n.columns += s.kind == BGP_STEP_COLUMN;
        n.generating += s.gen;
      });
    }
  }
  return n;
}
