// Internal definitions shared by the libbgp translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "../../include/bgp.h"
#include "bgp_mem.h"
#include "bgp_plan.h"

#define BGP_NB 128          // block size of the right-looking Cholesky == tile edge
#define BGP_TILE_LD 129     // LDS leading dimension of a 128x128 tile (odd -> conflict-free columns)
#define BGP_MAX_D 256       // maximum input dimension
#define BGP_MAX_STREAMS 8

typedef double d2 __attribute__((ext_vector_type(2)));
typedef double d4 __attribute__((ext_vector_type(4)));

void bgp_set_error(const char* fmt, ...);
// A call of THIS thread has failed: none of the downloads it enqueued may be unpacked into its caller's buffers later.  Only the
// calling thread's entries go (one context per host thread: another thread's context keeps its staged downloads), and their
// streams stay marked busy -- their copies may still be in flight into the arena -- until they are synchronised or destroyed.
void bgp_xfer_drop_pending();
// The stream is about to be destroyed (and has been synchronised): drop what is left of it without unpacking.
void bgp_xfer_forget(hipStream_t st);

#define BGP_HIP(call)                                                                        \
  do {                                                                                       \
    hipError_t e__ = (call);                                                                 \
    if (e__ != hipSuccess) {                                                                 \
      bgp_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e__), __FILE__, __LINE__); \
      (void)hipGetLastError(); /* clear the sticky error so that later calls are not blamed */  \
      bgp_xfer_drop_pending(); /* no download of this call may be unpacked into the caller's buffers later */ \
      return BGP_ERR_HIP;                                                                    \
    }                                                                                        \
  } while (0)

// A stage that has failed has reported its error: pass its code on.
#define BGP_TRY(call)           \
  do {                          \
    const int rc__ = (call);    \
    if (rc__) return rc__;      \
  } while (0)

// ---- host <-> device transfers through pinned staging, and the active wait ----
// Every copy between a CALLER's buffer (pageable: numpy arrays) and the device goes through the library's own pinned
// arena.  An asynchronous copy straight from / to pageable memory makes the runtime lock and unlock the pages around it,
// and the unlocking was measured to trail the call: after a config-E PVRS tell (640 KB of candidates up, Thompson draws
// down) the device stayed "busy" for another 27 ms in five of six processes, which the NEXT tell's first synchronisation
// then paid (41 -> 70 ms per tell; tools/archive/tell_phase_probe.py).  bgp_memcpy_async / bgp_memcpy2d_async take the
// arguments of their HIP namesakes: host -> device packs the rows into the arena and copies from there; device -> host
// lands in the arena and is unpacked into the caller's buffer by bgp_stream_sync of that stream (every entry point
// synchronises before it returns).  Device -> device passes through.
struct BgpXfer {
  struct Block {
    char* p;
    size_t cap, off;
  };
  struct Pending {
    hipStream_t st;
    char* host;
    size_t hpitch;
    const char* stage;
    size_t width, height;
    std::thread::id owner;  // the thread that enqueued the download (a failing call drops ITS OWN downloads only)
  };
  std::vector<Block> blocks;
  std::vector<Pending> pending;
  std::vector<hipStream_t> busy;  // streams with staged host -> device data not yet known to have been consumed
  char* take(size_t bytes);
  void release(hipStream_t st);   // the stream has been synchronised: unpack its downloads, forget its uploads
  void maybe_reset();             // nothing staged is in flight any more: the arena starts over
};
// ONE arena per process behind a mutex (bgp_api.hip): the bookkeeping is keyed by STREAM, so whichever thread synchronises a
// stream unpacks that stream's downloads -- a thread-local arena left them behind when another thread than the enqueuing one
// waited.  Transfers above BGP_XFER_DIRECT bytes (predictive covariances, whole kernel matrices, debugging downloads) do not
// go through it: they are copied synchronously, straight between the caller's buffer and the device (nothing asynchronous
// is left behind either way), and an idle arena above BGP_XFER_KEEP bytes is given back.
#define BGP_XFER_DIRECT ((size_t)8 << 20)
#define BGP_XFER_KEEP ((size_t)64 << 20)
void bgp_xfer_release(hipStream_t st);
hipError_t bgp_memcpy2d_async(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
                              hipMemcpyKind kind, hipStream_t st);
static inline hipError_t bgp_memcpy_async(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t st) {
  return bgp_memcpy2d_async(dst, bytes, src, bytes, bytes, 1, kind, st);
}

// Wait for a stream the way the sampler's inner loop needs it: ACTIVELY.  hipStreamSynchronize's default wait parks
// the thread, and for the 0.5-1 ms device calls of the small-batch regime (config E: 26 calls of 50 proposals at
// n ~ 1000 per tell) the wake-up was measured BISTABLE on MI355X -- the same tell took 25 ms or 52 ms of MCMC, +1 ms per
// call, run to run and tell to tell.  Polling hipStreamQuery from the calling thread (which has nothing else to do)
// removes that.  The first 2 ms are a tight poll (the calls this exists for last 0.1-2 ms); a longer call (n = 4096 batches,
// the 10 112^2 covariance of sample_y) is polled every ~20 us with the core handed back in between, and after 200 ms the
// runtime's blocking wait takes over.  BGP_WAIT=block selects the runtime's wait from the start (A/B measurements,
// oversubscribed hosts).
int bgp_wait_spins();
static inline void bgp_cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#else
  std::this_thread::yield();
#endif
}
static inline hipError_t bgp_stream_sync(hipStream_t st) {
  hipError_t e = hipErrorNotReady;
  if (bgp_wait_spins()) {
    const auto t0 = std::chrono::steady_clock::now();
    bool slow = false;
    for (unsigned it = 0;; it++) {
      e = hipStreamQuery(st);
      if (e != hipErrorNotReady) break;
      (void)hipGetLastError();  // (hipErrorNotReady is recorded as the thread's last error)
      if (slow) {
        std::this_thread::sleep_for(std::chrono::microseconds(20));
        if ((it & 15) == 15 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) break;
      } else {
        if ((it & 63) == 63 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) slow = true;
        bgp_cpu_relax();
      }
    }
  }
  if (e == hipErrorNotReady) e = hipStreamSynchronize(st);
  if (e == hipSuccess) bgp_xfer_release(st);
  return e;
}

// What is resident in dKinv / dLinv / dalpha_sol (and dXwP / dwarpP), and nothing else: every invalidation is drop(), the end of a
// posterior build is commit(), and everybody else reads.
struct BgpResident {
  void drop() { B_ = 0, rowwarp_ = false; }  // nothing is resident any more (the generation stays)
  void commit(int B, bool rowwarp) { B_ = B, rowwarp_ = rowwarp, gen_++; }
  int B() const { return B_; }               // number of resident posteriors (0 = none)
  int gen() const { return gen_; }           // bumped by every build (a fantasy state checks that its posteriors are still there)
  // posterior b was built from dX through ITS OWN warp (bgp_posterior_batch_warped): it goes with its own training inputs in dXwP,
  // not with dXeff, and bgp_predict_batch_warped alone reads it
  bool rowwarp() const { return rowwarp_; }

 private:
  int B_ = 0, gen_ = 0;
  bool rowwarp_ = false;
};

struct bgp_ctx {
  int device = 0;
  int n = 0, d = 0, npad = 0, nblk = 0;
  int max_batch = 0;
  bgp_kernel_spec ks{};
  hipStream_t stream = nullptr;
  // walker groups: the batch of an LML call is split over nstreams HIP streams so that the
  // latency-bound potrf / small trsm launches of one group overlap the MFMA-bound syrk of another
  int panels = 2;        // right-looking LML path: block columns per trailing update (K = 128 * panels; env BGP_PANELS)
  int panels_auto = 1;   // no BGP_PANELS in the environment: chosen per problem size (bgp_chol.hip)
  int nstreams = 1;
  int streams_auto = 1;  // choose the group count per call from the batch size (see bgp_ctx_create)
  hipStream_t gstream[BGP_MAX_STREAMS] = {nullptr};
  hipEvent_t ev_ready = nullptr;
  hipEvent_t ev_done[BGP_MAX_STREAMS] = {nullptr};
  // resident training set (every buffer below is owned: bgp_mem.h; deleting the context frees them)
  BgpDev<double> dX;         // n*d  (original inputs)
  double* dXeff = nullptr;   // what the kernels read: dX, or dXw1 when a context-level warp is set (borrowed)
  BgpDev<double> dXw1;       // training inputs through the context-level Beta-CDF warp
  BgpDev<double> dXwB;       // per-walker warped inputs of a warped LML batch (max_batch * n * d)
  BgpDev<double> dwarp;      // context-level warp parameters (2d, log space)
  BgpDev<double> dwarpB;     // per-walker warp parameters (max_batch * 2d)
  int has_warp = 0;
  BgpDev<double> dXs;        // scaled inputs of the current batch, k-major: max_batch * dpad * npad (bgp_kbuild.hip)
  BgpDev<double> dy;         // npad (zero padded); dy.cap is the row capacity of dX, dy and dalpha
  BgpDev<double> dalpha;     // npad
  // per-batch workspace
  BgpDev<double> dK;         // max_batch * npad*npad   working matrices (become L in place)
  BgpDev<double> dW;         // max_batch * nblk * 128*128  inverses of the diagonal blocks
  BgpDev<double> dyw;        // max_batch * npad        working rhs (becomes z = L^-1 y)
  BgpDev<double> dacc;       // max_batch * 4           {logdet, z^T z, -, -}
  BgpDev<double> dh;         // max_batch * (d+2)       canonical hyper-parameters
  BgpDev<double> dlml;       // max_batch
  BgpDev<int> dstatus;       // max_batch
  // resident posteriors (K^-1 full symmetric npad x npad each, alpha = K^-1 y; L^-1 lower triangular with zeros above, for
  // the predictive covariances that a Cholesky factorisation reads: bgp_sample_y, bgp_sample_y_batch)
  BgpDev<double> dKinv;
  BgpDev<double> dLinv;
  BgpDev<double> dalpha_sol;
  BgpResident post;          // how many of them, of which build, per-row warped or not
  // per-row-warped resident posteriors: buffers of their own (a warped LML batch between build and predict overwrites dXwB / dwarpB)
  BgpDev<double> dXwP;       // post.B() * n * d   warped training inputs of every resident posterior
  BgpDev<double> dwarpP;     // post.B() * 2d      their warp parameters (log space)
  // scratch for predict / pvrs (grown on demand, carved through BgpScratch below)
  BgpDev<char> dscratch;
  int scratch_live = 0;        // pointers carved out of dscratch are in use: a second carve would free them (BgpScratch)
  BgpDev<double> drowpart;     // column-tile partials of the predictive-variance row dots
  // asynchronous LML batch (bgp_lml_batch_submit / _wait): pinned result buffers and the pending batch size
  BgpPinned<double> hstage;  // pinned staging of the training set (bgp_ctx_update_data)
  BgpPinned<double> hh;      // pinned copy of the submitted hyper-parameter block
  BgpPinned<double> hwarp;   // pinned copy of the submitted per-walker warp parameters (max_batch * 2d)
  BgpPinned<double> hlml;
  BgpPinned<int> hstatus;
  int pending_B = 0;
  bgp_ctx* child = nullptr;  // cached workspace of bgp_sample_y (covariance Cholesky); it BORROWS this context's stream
  // launch-free factorisation of small batches (ps_kernel): flag block, pinned error word, trace buffer
  int ncu = 0;               // CUs of the device (the launch-free kernel takes one workgroup per CU)
  int persist = -1;          // env BGP_PERSIST: 0 never, 1 whenever possible, -1 (unset) automatic by batch size
  BgpDev<unsigned> ps_flags;
  BgpPinned<unsigned> ps_herr;  // pinned: error word of the last persistent call
  int ps_inflight = 0;          // a persistent call is on the stream (its error word is checked behind the sync)
  int ps_disabled = 0;          // a persistent call timed out: multi-launch path (see bgp_ps_note_timeout)
  int ps_cooldown = 0;          // eligible calls left on the multi-launch path before the launch-free one is tried again
  long long gen_batches = 0, gen_launches = 0;  // bgp_lml_gen_stats
  // launch schedule, LML path: diagonal block + panel solve of a block column in one launch (panel_kernel, bgp_chol.hip)
  // (0 here: a context made without bgp_ctx_create -- the covariance workspace of sample_y -- is READ in place and never fuses)
  int panel_fused = 0;          // bgp_ctx_create, env BGP_PANEL_FUSED: 0 never, 1 every block column that has a solve, -1 (unset) bgp_panel_fused_rule
  long long fused_launches = 0; // panel_kernel launches enqueued by this context (bgp_panel_fused_stats)
  BgpDev<double> dzf;           // max_batch * npad: z_k of the fused block columns (segment k of dyw keeps y_k there)
  std::vector<unsigned char> fused_col;  // [slot * nblk + k] = 1: the last factorisation of the slot left L_kk in dW and z_k in dzf
  long long ps_calls = 0;       // launch-free calls enqueued by this context (bgp_persist_stats)
  long long ps_timeouts = 0;    // ... of which timed out and were redone by launches
  int pending_warped = 0;       // the pending batch carries per-walker warps (redo path of bgp_lml_batch_wait)
  struct bgp_fantasy_state* fantasy = nullptr;  // an open batch proposal (bgp_fantasy_begin .. bgp_fantasy_end; bgp_fantasy.hip)
  long long fant_stats[2] = {0, 0};             // fantasy begins / steps run on this context (bgp_fantasy_stats)
  struct bgp_paths_state* paths = nullptr;      // pathwise posterior draws (bgp_paths_begin .. bgp_paths_end; bgp_paths.hip)
  long long paths_stats[2] = {0, 0};            // paths begins / evals run on this context (bgp_paths_stats)
  int mix_last[4] = {0, 0, 0, 0};               // last mixture pass: rows used, largest solver step / bracket-move counts (bgp_mixture_stats)
  long long chunk_last[2] = {0, 0};             // last chunked posterior call: item chunks, row / candidate chunks (bgp_chunk_stats)
  struct bgp_mcmc_state* mcmc = nullptr;  // an open device-resident sampler run (bgp_mcmc_begin .. bgp_mcmc_end; bgp_mcmc.hip)
  int ps_forbid = 0;            // the device-resident sampler redoes a run after a time-out: launches only, on every rank
  int ps_resident = 0;          // the device-resident sampler is enqueuing: no per-call copy of the error word (its kernels read it)
  BgpDev<unsigned long long> ps_trace;  // BGP_PS_TRACE=1: device buffer of in-kernel time stamps (bgp_debug_ps_trace)
  int ps_trace_B = 0, ps_trace_nblk = 0, ps_trace_total = 0;
  // timing
  int timing = 0;
  double t_ms[6] = {0, 0, 0, 0, 0, 0};  // K-build, potrf, trsm, syrk (all), whole call, look-ahead column launches of syrk
  int t_cnt[6] = {0, 0, 0, 0, 0, 0};
  std::vector<hipEvent_t> ev;  // (start, stop) pairs of the launches of the current call
  std::vector<int> evcat;
};

// Per-launch HIP-event timing on the context's stream (only when ctx->timing != 0).
// Categories: 0 K-build, 1 potrf, 2 trsm, 3 syrk (bulk update of a panel group), 5 syrk look-ahead column launch (counted
// under 3 as well; bgp_last_timing_columns reports the split).
static inline void bgp_tbegin(bgp_ctx* c, int cat, hipStream_t st = nullptr) {
  if (!c->timing) return;
  hipEvent_t a, b;
  (void)hipEventCreate(&a);
  (void)hipEventCreate(&b);
  (void)hipEventRecord(a, st ? st : c->stream);
  c->ev.push_back(a);
  c->ev.push_back(b);
  c->evcat.push_back(cat);
}
static inline void bgp_tend(bgp_ctx* c, hipStream_t st = nullptr) {
  if (!c->timing) return;
  (void)hipEventRecord(c->ev.back(), st ? st : c->stream);
}
static inline void bgp_tcollect(bgp_ctx* c) {
  if (!c->timing) return;
  (void)hipStreamSynchronize(c->stream);
  for (size_t i = 0; i < c->evcat.size(); i++) {
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, c->ev[2 * i], c->ev[2 * i + 1]);
    c->t_ms[c->evcat[i]] += ms;
    c->t_cnt[c->evcat[i]] += 1;
    if (c->evcat[i] == 5) {  // a look-ahead column launch is a trailing-update launch too
      c->t_ms[3] += ms;
      c->t_cnt[3] += 1;
    }
    (void)hipEventDestroy(c->ev[2 * i]);
    (void)hipEventDestroy(c->ev[2 * i + 1]);
  }
  c->ev.clear();
  c->evcat.clear();
}

#define BGP_MAX_DEVICES 64
// ---- launch-free factorisation of small batches (bgp_chol.hip: ps_chain_kernel, bgp_syrk4.hip: ps_tile_kernel) ----
// Flag block of one persistent factorisation (32-bit words, zeroed by a memset node in front of every call):
//   [PS_TICKET + 2 + 8 pool + x]  next task of the tile kernel's list (pool, XCD x)      [PS_ERROR]  != 0: a wait timed out: everybody leaves
//   wready[b * nblk + J]          1 when potrf(J) of matrix b has published L_JJ, W_JJ, z_J (or the matrix has failed)
//   diagrdy[b * nblk + I]         1 when the diagonal block (I, I) carries the panels 0 .. I-2 (the chain applies panel I-1)
//   xready[(b * nblk + I) * nblk + J]   1 when the panel block X_IJ is final, I > J
//   subrdy[b * nblk + I]          1 when block (I, I-1) carries the panels 0 .. I-2 (the chain solves it)
//   wrow[b * nblk + J]            pair mode: number of 16-row blocks of W_JJ = L_JJ^-1 that are complete in memory (0 .. 7; the
//                                 eighth goes out with wready[J])
//   xcol[(b * nblk + I) * 3 + d]  pair mode: number of 16-column blocks of the panel block X_{I, I-1-d} that are complete in memory
//                                 (0 .. 8), d = 0: the chain helper's block, d = 1, 2: the streamed panel solves S(I, I-2), S(I, I-3);
//                                 the quadrant pre-updates that they feed consume them column block by column block
//   s2rdy[b * nblk + I]           counts the quadrants of block (I, I-2) that carry the panels 0 .. I-3 (the solve S(I, I-2) waits for 4)
#define PS_TICKET 0
#define PS_ERROR 1
#define PS_HDR 32
#define PS_XCOL(B, nblk) (PS_HDR + (size_t)(B) * (nblk) * (4 + (nblk)))  // (behind wrow; three words per (b, I))
#define PS_S2RDY(B, nblk) (PS_HDR + (size_t)(B) * (nblk) * (7 + (nblk)))
struct PsArgs {
  double* K;          // B working matrices (ld x ld, row-major), become L in place
  double* W;          // B x nblk inverses of the diagonal blocks
  double* yw;         // B working right-hand sides (become z)
  double* acc;        // B x 4 running {log det, z^T z}
  double* lml;
  int* status;
  unsigned* flags;    // the block above
  int n, ld, nblk, B, ystride;
  size_t mstride;
  int total;          // tasks of the tile kernel (0: two block columns, the chain does everything)
  int ncrit;          // workgroups of the tile kernel's critical pool (0: one list)
  int pair;           // 1: TWO chain workgroups per matrix that alternate over the block columns (bgp_pf.h, ps_chain_role)
  int Bpad;           // pair mode: chain workgroup p of matrix b is block p * Bpad + b (Bpad = B rounded up to 8: same XCD)
  int nchain;         // chain workgroups at the head of the grid (B, or 2 * Bpad)
  int psplit;         // parts a pre-update task P(I) is dealt out in (1, or 4 quadrants behind chain pairs): subrdy[I] counts to psplit
  int dsplit;         // parts of a diagonal block's task Dg(I) (3 quadrants with psplit == 4, else 1): diagrdy[I] counts to dsplit
  int ncrit_stream;   // pair mode: panel solves S(I, J) with I <= J + ncrit_stream follow pf_block(J) row block by row block
  unsigned long long spin_limit;  // wall_clock64 ticks (100 MHz) a single wait may last before the call is abandoned
  unsigned long long* trace;      // debugging (BGP_PS_TRACE=1): wall-clock stamps, chain: 8 per (b, J), tile: 8 per task
  // gen = 1: the Gram matrices are generated INSIDE this launch -- the first B nblk (nblk + 1) / 2 tickets of the tile list are one
  // 128 x 128 block each (kb_tile, bgp_kb.h; block (I, 0) also sets up row block I of the right-hand side), genrdy[b][I][J] tells
  // its consumer -- instead of by a Gram kernel in front of it (Matern-5/2 product form, one chain workgroup per matrix, one list)
  int gen, d;
  const double* X;      // n x d training inputs
  const double* alpha;  // n diagonal additions
  const double* H;      // B x (d + 2) canonical hyper-parameters
  const double* y;      // n
};
//   genrdy[(b * nblk + I) * nblk + J]   gen = 1: block (I, J) of matrix b has been generated (behind s2rdy)
#define PS_GEN(B, nblk) (PS_HDR + (size_t)(B) * (nblk) * (8 + (nblk)))
static inline size_t ps_flag_words(int B, int nblk) { return PS_HDR + (size_t)B * nblk * (8 + 2 * (size_t)nblk); }
// A launch-free call timed out (a wait outlasted BGP_PS_TIMEOUT_MS: its workgroups were not co-resident -- another context,
// process or RCCL kernel held CUs -- or the device was oversubscribed).  One transient event must not cost the context
// the path for life: the next BGP_PS_COOLDOWN eligible calls go by launches, then the launch-free path is tried again;
// after the third time-out it stays off (bgp_set_persist(ctx, 1) re-arms it).  bgp_persist_stats reports the counts.
int bgp_ps_cooldown_calls();  // BGP_PS_COOLDOWN, default 256 (bgp_api.hip)
static inline void bgp_ps_note_timeout(bgp_ctx* c, const char* what) {
  c->ps_timeouts++;
  c->ps_disabled = 1;
  c->ps_cooldown = c->ps_timeouts >= 3 ? 0 : bgp_ps_cooldown_calls() + 1;  // (+ 1: the redo of this very batch counts one)
  if (c->ps_timeouts <= 3)
    fprintf(stderr, "libbgp: warning: the launch-free factorisation timed out (a wait outlasted BGP_PS_TIMEOUT_MS); %s on the "
                    "multi-launch path, which this context keeps %s (time-out %lld of this context; bgp_persist_stats)\n", what,
            c->ps_cooldown ? "for its next eligible calls (BGP_PS_COOLDOWN, 256)" : "from now on", c->ps_timeouts);
}
// Behind the synchronisation of a launch-free call: did a wait inside it time out?  `ran` is the context whose flag block and error
// word the call used -- `c` itself, or the child that factorises a covariance for it; the word is cleared, the time-out is counted
// on `c`, and the caller redoes the work by launches.
static inline bool bgp_ps_timed_out(bgp_ctx* c, bgp_ctx* ran, const char* what) {
  if (!ran->ps_herr || *ran->ps_herr == 0) return false;
  *ran->ps_herr = 0;
  bgp_ps_note_timeout(c, what);
  return true;
}
// (call only when the batch is otherwise eligible: the cool-down counts eligible calls)
static inline bool bgp_ps_allowed(bgp_ctx* c) {
  if (!c->ps_disabled) return true;
  if (c->ps_cooldown > 0 && --c->ps_cooldown == 0) c->ps_disabled = 0;
  return false;
}
static_assert(BGP_PLAN_MATERN52 == BGP_MATERN52 && BGP_PLAN_FORM_PRODUCT == BGP_FORM_PRODUCT, "bgp_plan.h restates include/bgp.h");
// What the planner (bgp_plan.h) reads of a context: nb matrices of w's shape under w's modes and the live switches.
static inline BgpLmlShape bgp_lml_shape(const bgp_ctx* w, int nb, int warped, int given) {
  BgpLmlShape s{};
  s.n = w->n, s.nblk = w->nblk, s.d = w->d, s.stationary = w->ks.stationary, s.form = w->ks.form, s.ncu = w->ncu, s.nb = nb;
  s.warped = warped != 0, s.given = given != 0;
  s.timing = w->timing, s.persist = w->persist, s.panel_fused = w->panel_fused;
  s.panels = w->panels, s.panels_auto = w->panels_auto, s.nstreams = w->nstreams, s.streams_auto = w->streams_auto;
  bgp_shape_read_call_switches(s);
  return s;
}
// The plan of a batch that is about to be enqueued.  `permitted`: the caller does not rule the launch-free path out; the planner
// says whether the batch is eligible otherwise, the cool-down of `c` -- asked, and counted, for eligible batches only -- has the last
// word, and a launch-free call is counted on `c`.
static inline BgpLmlPlan bgp_plan_for(bgp_ctx* c, BgpLmlShape s, bool permitted) {
  s.ps_permitted = permitted;  // (for the planner's answer "eligible but for the cool-down")
  s.ps_permitted = bgp_plan_wants_launch_free(s) && bgp_ps_allowed(c);
  if (s.ps_permitted) {
    c->ps_calls++;
    bgp_shape_read_ps_switches(s);
  }
  return bgp_plan_lml(s);
}
int bgp_launch_cholesky_persist(bgp_ctx* ctx, const BgpLmlPlan& plan);
int bgp_lml_redo_if_abandoned(bgp_ctx* ctx, int B);
int bgp_lml_enqueue_dev(bgp_ctx* ctx, int nb, int warped);  // bgp_api.hip: Gram build + factorisation + LML of c->dh[0 .. nb), on the device only
int bgp_ensure_warp_buffers(bgp_ctx* ctx);                  // bgp_api.hip: the per-walker warp buffers of a warped LML batch exist
void bgp_fantasy_abandon(bgp_ctx* ctx);  // bgp_fantasy.hip: drop an open batch proposal (context teardown)
void bgp_paths_abandon(bgp_ctx* ctx);  // bgp_paths.hip: drop the pathwise draws (context teardown, new training data)
void bgp_mcmc_abandon(bgp_ctx* ctx);  // bgp_mcmc.hip: drop an open sampler run (context teardown, failed calls)
// the launch-free call of a batch whose results are discarded anyway: forget it (no time-out is counted, nothing is redone)
static inline void bgp_ps_clear_inflight(bgp_ctx* c) {
  c->ps_inflight = 0;
  if (c->ps_herr) *c->ps_herr = 0;
}
int bgp_ps_ensure_flags(bgp_ctx* ctx, int B);

// ONE guard for the entry points that read or replace the resident posteriors (bgp_post.hip, bgp_fantasy.hip, bgp_predgrad.hip,
// bgp_paths.hip, bgp_paths_select.hip, bgp_pdep.hip, bgp_cv.hip, bgp_sobol.hip, bgp_gcov.hip, bgp_cond.hip, bgp_kg.hip, bgp_jes.hip, bgp_warp.hip, bgp_mix.hip).  An entry point calls it FIRST, with its name and the kind of posteriors it reads; one
// that counts them calls it again with the count where its "not resident" answer stands today, behind its argument and capability
// checks (BGP_ERR_INVALID goes before BGP_ERR_STATE there).  Always: the context is there and no submitted batch is pending -- the
// workspace belongs to a batch submitted with bgp_lml_batch_submit until bgp_lml_batch_wait has collected it; that much is every
// other entry point's guard too (bgp_api.hip, bgp_gram.hip, bgp_mcmc.hip, bgp_comm.hip).
//   BGP_POST_PLAIN    the resident posteriors are not per-row warped: they go with the shared c->dXeff
//   BGP_POST_ROWWARP  they are (bgp_predict_batch_warped, bgp_predict_mixture_warped)
//   count > 0: at least `count` are resident (index b: b + 1);  idx: every idx[0 .. nidx) names a resident one.
// Nothing is launched and nothing changes on a refusal.
enum BgpPostKind { BGP_POST_ANY, BGP_POST_PLAIN, BGP_POST_ROWWARP };
static inline int bgp_guard(const bgp_ctx* c, const char* who, BgpPostKind kind = BGP_POST_ANY, int count = 0,
                            const int* idx = nullptr, int nidx = 0) {
  if (!c) {
    bgp_set_error("%s: NULL ctx", who);
    return BGP_ERR_INVALID;
  }
  const char* why = nullptr;
  if (c->pending_B != 0)
    why = "a submitted batch is still pending (call bgp_lml_batch_wait)";
  else if (kind == BGP_POST_PLAIN && c->post.rowwarp())
    why = "the resident posteriors are per-row warped (bgp_posterior_batch_warped): only bgp_predict_batch_warped reads them; "
          "build plain posteriors first";
  else if (kind == BGP_POST_ROWWARP && !c->post.rowwarp())
    why = "the resident posteriors are not per-row warped (call bgp_posterior_batch_warped first)";
  else if ((count > 0 || nidx > 0) && c->post.B() == 0)
    why = "no resident posteriors (build them first: bgp_posterior_batch and its kin)";
  if (why) {
    bgp_set_error("%s: %s", who, why);
    return BGP_ERR_STATE;
  }
  if (count > c->post.B()) {
    bgp_set_error("%s: needs %d posteriors, %d resident", who, count, c->post.B());
    return BGP_ERR_STATE;
  }
  for (int i = 0; i < nidx; i++)
    if (idx[i] < 0 || idx[i] >= c->post.B()) {
      bgp_set_error("%s: item %d names posterior %d, %d resident", who, i, idx[i], c->post.B());
      return BGP_ERR_STATE;
    }
  return BGP_OK;
}

// ONE exit path for every entry point that touches the device with scratch (bgp_post.hip, bgp_paths.hip, bgp_paths_select.hip, bgp_pdep.hip, bgp_cv.hip, bgp_sobol.hip, bgp_gcov.hip, bgp_cond.hip, bgp_kg.hip, bgp_jes.hip,
// bgp_predgrad.hip, bgp_fantasy.hip, bgp_warp.hip, bgp_mix.hip; their stages return from the middle, with BGP_HIP or a plain return): the body
// runs on the context's device, and a failed call waits for what it enqueued -- its kernels run over scratch that the next call may
// carve again --, clears the sticky HIP error, and none of its downloads is unpacked into the caller's arrays later.  The success
// path is the body's own.
template <class Body>
static inline int post_call(bgp_ctx* c, Body&& body) {
  const int rc = [&]() -> int {
    BGP_HIP(hipSetDevice(c->device));
    return body();
  }();
  if (rc != BGP_OK) {
    (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    bgp_xfer_drop_pending();
    bgp_xfer_release(c->stream);
  }
  return rc;
}

// The context's scratch, carved by ONE layout per call (bgp_mem.h; every region on 16 bytes).  A carve may free and re-allocate
// dscratch, so the pointers of an earlier one would dangle: while a BgpScratch that has carved is in scope, another carve of the
// same context is refused.  (No scratch user calls another one inside that scope today.)
struct BgpScratch {
  bgp_ctx* c;
  bool mine = false;
  explicit BgpScratch(bgp_ctx* ctx) : c(ctx) {}
  BgpScratch(const BgpScratch&) = delete;
  ~BgpScratch() {
    if (mine) c->scratch_live = 0;
  }
  template <class Layout>
  int carve(Layout&& layout) {
    if (c->scratch_live) {
      bgp_set_error("libbgp: the context's scratch is carved while an earlier carve of it is in use");
      return BGP_ERR_STATE;
    }
    c->scratch_live = 1;
    mine = true;
    return bgp_carve(c->dscratch, 16, layout);
  }
};
void bgp_free_child(bgp_ctx* ctx);
// make the matrix workspace at least `doubles` large (and the per-item side buffers consistent)
int bgp_grow_workspace(bgp_ctx* ctx, size_t doubles);
// posterior build on the augmented matrices; use_alpha == 0 drops alpha_diag (PVRS quirk).  Kgram != nullptr: the B kernel
// matrices come from the host (n x n each, bgp_gram.hip) instead of the device Gram build, h is not read.  want_Linv: L^-1
// stays resident beside K^-1 (the draws read it; the LML gradient does not)
// warp != nullptr (B x 2d, host): item b is built from c->dX through its own warp instead of c->dXeff; the warped inputs and the
// warp parameters of all B items stay resident in c->dXwP / c->dwarpP (bgp_posterior_batch_warped)
int bgp_posterior_build(bgp_ctx* c, int B, const double* h, int use_alpha, double* L, double* alpha, double* K_inv,
                        double* lml, int* status, const double* Kgram = nullptr, bool want_Linv = true,
                        const double* warp = nullptr);
// host kernel matrices -> working matrices (bgp_gram.hip)
int bgp_gram_load(bgp_ctx* c, int nb, const double* K, int augmented, int use_alpha);

// ---- kernels launched across translation units ----
// K-build: lower-triangular tiles of the jittered Gram matrix of walker b into dK[b] (npad x npad).
int bgp_launch_kbuild(bgp_ctx* ctx, int B, int full_square, int augmented, int use_alpha);
// same for the slice [off, off+B) of the current batch on an explicit stream
int bgp_launch_kbuild_slice(bgp_ctx* ctx, int off, int B, hipStream_t st, int full_square, int augmented,
                            int use_alpha);
// per-walker inputs: dXb + b * xstride (xstride == 0: shared)
int bgp_launch_kbuild_x(bgp_ctx* ctx, int off, int B, hipStream_t st, int full_square, int augmented, int use_alpha,
                        const double* dXb, size_t xstride);
// Cross kernel matrix k(Xq, X_train) for hyper-vector index b: out is m x ldo row-major (device).
int bgp_launch_kcross(bgp_ctx* ctx, const double* dh_b, int m, const double* dXq, int nx, const double* dXt,
                      double* dout, int ldo);
// the same for nb hyper-vectors dH (nb x (d+2)) into dout + b * ostride
int bgp_launch_kcross_batch(bgp_ctx* ctx, int nb, const double* dH, int m, const double* dXq, int nx, const double* dXt,
                            double* dout, int ldo, size_t ostride);
int bgp_launch_kcross_matvec(bgp_ctx* ctx, int nb, const double* dH, int m, const double* dXq, int nx, const double* dXt,
                             double* dout, int ldo, size_t ostride, const double* vec, size_t svec, double* dpart);
// ... with per-item queries dXq + b * qstride and training inputs dXt + b * xstride (stride 0: shared; the three above forward here)
int bgp_launch_kcross_matvec_x(bgp_ctx* ctx, int nb, const double* dH, int m, const double* dXq, size_t qstride, int nx,
                               const double* dXt, size_t xstride, double* dout, int ldo, size_t ostride, const double* vec,
                               size_t svec, double* dpart);
// Blocked Cholesky of the B matrices in dK (in place) + forward substitution + LML.
// Beta-CDF warp of n x d inputs for B parameter sets (bgp_warp.hip)
int bgp_launch_warp(bgp_ctx* c, hipStream_t st, const double* dX, const double* dW, double* dout, int n, int B,
                    size_t ostride);
int bgp_launch_cholesky(bgp_ctx* ctx, int B, int augmented);
// bgp_post.hip: `rows` query rows to the device, through the context-level warp when one is set (predict's staging; bgp_pdep.hip, bgp_sobol.hip)
int post_stage_queries(bgp_ctx* c, double* dst, const double* src, int rows);
// n <= 128: K-build + factorisation + LML of the slice [off, off+B) in ONE launch (bgp_chol.hip, potrf_kernel<1,..>)
int bgp_launch_lml_small(bgp_ctx* ctx, int off, int B, hipStream_t st);
// walker group g of a plan on the launch schedule, on stream st (bgp_chol.hip; the Gram build of the group is in front of it)
int bgp_launch_lml_group(bgp_ctx* ctx, const BgpLmlPlan& plan, int g, hipStream_t st);
struct S4Gen {           // what the trailing update's Gram generator reads (S4GenF, bgp_s4.h)
  const double* Xs;     // scaled inputs, k-major: dpad x npad doubles per matrix slot
  const double* H;      // canonical hyper-parameters, d + 2 per matrix
  const double* alpha;  // per-point jitter added to the diagonal (nullable)
  int n, d, dpad, npad;
};
int bgp_lml_gen_args(const bgp_ctx* ctx, int off, S4Gen* out);
// bgp_syrk4.hip, NT products on the LDS-DMA ring for nb items (item b's B operand is Bm + (pidxB ? pidxB[b] : b) * sB; M, N multiples
// of 64): mode 0: C = A B^T; mode 1: C -= A B^T on the lower tiles of a square C; mode 2: C -= A B^T on all tiles
void bgp_launch_gemm4(hipStream_t st, int mode, const double* A, const double* Bm, int ldx, int M, int N, int K, double* C,
                      int ldc, int nb, size_t sA, size_t sB, size_t sC, const int* pidxB);
// bgp_syrk4.hip: column-tile partials of a_i^T S_b a_i for the rows of A_b (M x n, zero padded, multiples of 128; S symmetric) into
// part = nb * (n / bgp_rowquad_tile()) * M doubles; rowdot_reduce_kernel adds them
void bgp_launch_rowquad(hipStream_t st, const double* A, int lda, size_t sA, const double* S, int lds_, size_t sS,
                        const int* pidx, int M, int n, int nb, double* part);
int bgp_rowquad_tile();
// bgp_post.hip: out[b][i] = sum_t part[(b tn + t) M + i], t ascending (out packed with stride M); grid (ceil(M / 256), items)
__global__ void rowdot_reduce_kernel(const double* __restrict__ part, int tn, int M, double* __restrict__ out);
// bgp_post.hip: var[b][i] = max(0, kernel_.diag of H[b] incl. the white level - q[b][i]), i < m; grid (ceil(m / 256), items)
__global__ void finish_var_kernel(const double* __restrict__ q, size_t sq, const double* __restrict__ H, int d, int form,
                                  int m, double* __restrict__ var, size_t so);
// bgp_post.hip: C[i][i] += v, i < m; grid ceil(m / 256)
__global__ void add_diag_kernel(double* __restrict__ C, int ld, int m, double v);
// bgp_post.hip, the closed forms and the average of bgp_acq_batch.  mumin[b] = np.min of draw b's means (NaN if any is); grid (draws)
__global__ void __launch_bounds__(256) acq_mumin_kernel(const double* __restrict__ mean, size_t smean, int m,
                                                         double y_mean, double y_std, double* __restrict__ mumin);
// T[(k B + b) sm + i] = acquisition k of draw b at candidate i, bad[k B + b] |= "not finite"; grid (ceil(m / 256), draws)
__global__ void __launch_bounds__(256) acq_values_kernel(const double* __restrict__ mean, const double* __restrict__ var,
                                                          size_t sm, int m, int B, double y_mean, double y_std, int n_acq,
                                                          const int* __restrict__ kinds,
                                                          const double* __restrict__ params,
                                                          const double* __restrict__ mumin, double* __restrict__ T,
                                                          int* __restrict__ bad);
// acc[k sm + i] = sum over b ascending of T[(k B + b) sm + i] / n_samples, a draw with bad[k B + b] left out; grid (ceil(m / 256), n_acq)
__global__ void __launch_bounds__(256) acq_sum_kernel(const double* __restrict__ T, const int* __restrict__ bad, size_t sm,
                                                       int m, int B, int n_samples, double* __restrict__ acc);
// bgp_fantasy.hip: argmax over the candidates not chosen yet (np.argmax's order: ties to the lower index); one workgroup of 1024
__global__ void __launch_bounds__(1024) fant_argmax_kernel(const double* __restrict__ acc, const int* __restrict__ chosen, int m,
                                                           int* __restrict__ next);

static inline int pad_to(int v, int q) { return (v + q - 1) / q * q; }

// bgp_post.hip, the latent moments of `rows` query rows for nb items as bgp_predict_batch computes them -- five launches: the cross
// build K_* = k_b(Xq_b, Xt_b) with the column-tile partials of K_* alpha_b, rowdot_reduce_kernel (mean), bgp_launch_rowquad on
// K_* and K_b^-1, rowdot_reduce_kernel, the kernel diagonal minus that in place (variance).  Item b reads dH + b (d + 2), dXq + b qstride, dXt + b xstride
// (stride 0: shared), alpha + b npad, Kinv + b npad^2 and writes dKs + b sKs (leading dimension ldk), dmpart (nb * (npad / 128) *
// pad128(rows)), dmean / dvar + b pad128(rows).  dvar == nullptr: the first two launches only.  The row-dot partials go to
// c->drowpart, grown here when it is too small (a caller that loops sizes it before its loop).
int bgp_launch_moments(bgp_ctx* c, int nb, const double* dH, int rows, const double* dXq, size_t qstride, const double* dXt,
                       size_t xstride, const double* alpha, const double* Kinv, double* dKs, int ldk, size_t sKs, double* dmpart,
                       double* dmean, double* dvar);

// ---- the hyper-posterior mixture pass (bgp_mix.hip): behind the batched predict (predict_run, bgp_post.hip)
// for bgp_predict_mixture / bgp_predict_mixture_warped, on uploaded moments for bgp_mixture_values ----
struct BgpMixPlan {                  // the host side of one pass (arguments of the entry points, include/bgp.h)
  const double* weights;             // B, or nullptr: every row counts 1
  double y_mean, y_std;
  int Q;
  const double *probs, *t;           // Q probabilities; m values for at_t (nullptr without it)
  double *moments, *quant, *at_t;    // 3 x m, Q x m, 3 x m; each may be nullptr
  int* n_used;
};
struct BgpMixScratch {               // device regions of bgp_mix_run
  double *dmu = nullptr, *dsd = nullptr, *dw = nullptr, *dwn = nullptr, *dprobs = nullptr, *dt = nullptr, *dmom = nullptr,
         *dat = nullptr, *dquant = nullptr;
  int *dbad = nullptr, *dused = nullptr, *dstat = nullptr;
  void take(BgpCarve& s, int B, int mpad, int Q);
};
int bgp_mix_check(const char* who, int B, const BgpMixPlan& mp);  // the argument rules: BGP_ERR_INVALID, nothing launched
// the pass on B device rows of stride mpad, enqueued on the context's stream with its downloads; the caller synchronises
int bgp_mix_run(bgp_ctx* c, int B, int m, int mpad, const double* dmean, const double* dvar, const BgpMixPlan& mp,
                const BgpMixScratch& ms);
// bgp_post.hip: predict_run on the first B resident posteriors with the pass behind the moments (nothing else is downloaded)
int bgp_predict_run_mix(bgp_ctx* c, int B, const double* h_kernel, int m, const double* Xq, const BgpMixPlan& mp, bool rowwarp);

// ---- moments of candidates conditional on point sets: the pipeline behind bgp_knowledge_gradient and bgp_joint_entropy
// (bgp_cond.hip) ----
struct BgpCondPlan {
  int Mp, M64;  // points as stored (rows of R, columns of C: pad128, at least 128) and as multiplied (pad64)
  int mtot;     // pad128 of the candidates: the row stride of the value matrix
  int mc;       // candidates per chunk
  int tq;       // column tiles of the row-dot partials
  int Bc;       // posteriors per chunk: K_*, C, R and P of a chunk within 2^29 doubles together
  size_t sKs, sC, sR, sAx;  // item strides of K_*, C, R / P and of the point sets (0: one shared set)
};
struct BgpCondReq {
  int B, m, M;                               // posteriors, candidates, points per set (0: none, stage 1 is skipped)
  const double *h_kernel, *noise, *Xcand;    // host: B x (d + 2), B, m x d
  const double* Xpts;                        // host: the point sets (M x d each)
  bool per_posterior;                        // one set per posterior (B sets) instead of one shared set
  const double* fpts;                        // host, B x M values that go with the points, or nullptr (not carved then)
  bool want_var;                             // the latent variance at the points (not carved otherwise)
  BgpSwitch chunk_switch;                    // the caller's candidate-chunk switch (tests)
  int n_samples;                             // divisor of the average
  double *rows, *avg;                        // host outputs: B x m values, m averaged values (either may be nullptr)
};
struct BgpCondChunk {                // posteriors b0 .. b0 + nb, candidates m0 .. m0 + mm; every pointer is that of item b0
  int b0, nb, m0, mm;
  const double *muA, *vA;            // [b][j] latent mean / variance at the points (stride Mp; vA only with want_var)
  const double* fpts;                // [b][j] (stride M; only when given)
  const double* Cv;                  // [b][i][j] = cov_b(point j, candidate i) (row stride Mp, item stride sC; not written when M == 0)
  int Mp;
  size_t sC;
  const double *mean, *var;          // [b][i] latent moments of the chunk (stride sm)
  size_t sm;
  const double* noise;               // [b]
  double* out;                       // [b][i] values of the chunk (stride so)
  size_t so;
  int* bad;                          // [b] "a value is not finite" (zero on entry)
};
BgpCondPlan bgp_cond_plan(const bgp_ctx* c, const BgpCondReq& q);
// Uploads, stage 1 per chunk of posteriors, stage 2 per chunk of candidates followed by `score` (ONE launch of the caller's scoring
// kernel on the context's stream), then the average, the downloads and the stream sync.
int bgp_cond_run(bgp_ctx* c, const BgpCondReq& q, const std::function<void(const BgpCondChunk&)>& score);
