// Batched right-looking blocked Cholesky + fused forward substitution + LML
// (SURVEY.md 8a rows a2, a3).
//
// Replaces, per walker:  L = cholesky(K, lower=True)          sklearn/_gpr.py:587 (LAPACK dpotrf)
//                        alpha = cho_solve((L, True), y)      sklearn/_gpr.py:597 (dpotrs)
//                        -1/2 y.alpha - sum log diag L - n/2 log 2pi       sklearn/_gpr.py:609-613
// using  y^T K^-1 y = z^T z  with  z = L^-1 y  (one forward substitution, fused into the panel
// kernels; the back substitution is only needed for posterior builds, bgp_post.hip).
//
// Block size NB = 128; per block column k, batched over the B walkers:
//   potrf_kernel  one workgroup per walker: diagonal block in LDS -> L_kk, W_kk = L_kk^-1,
//                 z_k = W_kk y_k, running log-det and z^T z                    (latency: 128 sequential pivots)
//   panel solve   X_i = A_ik W_kk^T  (fp64 MFMA),  y_i -= X_i z_k
//   trailing upd. A_ij -= X_i X_j^T  (fp64 MFMA; the n^3/3 bulk -- the kernel the roofline fraction is quoted on)
// Panel solve and trailing update are trsm4_kernel / syrk4_kernel on the LDS-DMA ring (bgp_syrk4.hip):
//   * LML path (bgp_lml_batch; the MCMC hot loop): the schedule the planner chose (bgp_plan.h: bgp_plan_lml, bgp_lml_schedule),
//     enqueued group by group by bgp_launch_lml_group;
//   * posterior builds on the augmented matrix (bgp_post.hip; once per sample(), per hyper-posterior draw of an
//     acquisition and per gradient evaluation): the same kernels in single-panel mode with the active-row remap of
//     bgp_rowblk (bgp_device.h);
//   * small batches of the LML path and sample_y's covariance: ONE persistent kernel instead of the launches
//     (bgp_launch_cholesky_persist below, ps_kernel in bgp_ps.hip, the diagonal-block code of both in bgp_pf.h).
// (Round 1's VGPR-staged trsm_kernel / syrk_kernel / syrk2_kernel / trsm8_kernel and the left-looking variant are A/B
// references of the benches under tools/legacy/ now; they are not part of libbgp.so.)
#include "bgp_common.h"
#include "bgp_device.h"

#include "bgp_gemm.h"

#include <algorithm>
#include <cstdlib>
#include <vector>

// ------------------------------------------------------------------------------------------
// potrf: diagonal block k of every walker, one workgroup (8 waves) per walker, block in LDS (pf_block, bgp_pf.h).
//
// The 128x128 block is processed as 8x8 sub-blocks of 16 by a two-stage software pipeline inside the
// workgroup.  Wave 0 is the PANEL wave: per step sb it completes row block sb (panel product with the
// previous 16x16 inverse, last rank-16 term of the diagonal block), factorises the diagonal block in
// registers (one matrix row per lane, 64-bit DPP row broadcasts) and publishes its inverse M_sb.  Waves 1-3 and
// 5-7 are UPDATE waves running one phase behind: phase p (after M_p is published) forms the panel blocks X_{I,p}
// of the rows I >= p+2 and applies
//     column p+1: terms t = p-1, p        column p+2: terms t <= p-1  (and t = p on its diagonal block)
// so every block column c is complete (terms t <= c-3 in phase c-2, t = c-2, c-1 in phase c-1) when the
// panel wave needs it; they also form row sb-1 of W = L^-1 while the panel wave factorises block sb.  The
// only thing on the critical path is the 16-pivot chain (8 x ~2 us); one barrier per step.
// Panel products are formed transposed (X^T = M T^T): their C-layout registers are directly the A and
// the B operand of the following rank-16 updates (for v_mfma_f64_16x16x4_f64 the C/D row map
// (lane>>4)+4*reg coincides with the A and the B operand's k map for k-slice reg), so nothing
// round-trips through LDS.  W is kept TRANSPOSED in the otherwise unused upper triangle of the LDS
// tile, where later rows read it with the ordinary row-major operand pattern; z_k = W y_k, log-det and
// z^T z finish the launch.
// ------------------------------------------------------------------------------------------
#ifdef PF_TRACE  // phase timestamps of workgroup 0 (tools/potrf_bench.hip); compiled out of the product library
__device__ unsigned long long pf_trace[32];
__device__ unsigned long long pf_trace_w[8 * 32];  // per wave: [2 sb] start of the wave's step, [2 sb + 1] its end (before the barrier)
#define PF_T(i) do { if (threadIdx.x == 0 && blockIdx.x == 0) pf_trace[i] = wall_clock64(); } while (0)
#define PF_TW(i) do { if ((threadIdx.x & 63) == 0 && blockIdx.x == 0) pf_trace_w[(threadIdx.x >> 6) * 32 + (i)] = wall_clock64(); } while (0)
extern "C" int bgp_debug_potrf_trace(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(pf_trace), sizeof(pf_trace)) == hipSuccess ? 0 : 1;
}
extern "C" int bgp_debug_potrf_trace_w(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(pf_trace_w), sizeof(pf_trace_w)) == hipSuccess ? 0 : 1;
}
#else
#define PF_T(i)
#define PF_TW(i)
#endif
#include "bgp_pf.h"
#include "bgp_mcmc.h"

template <int GEN, int STAT, int FORM>
__global__ void __launch_bounds__(PF_THREADS) potrf_kernel(double* __restrict__ Kbuf, double* __restrict__ Wbuf,
                                                     double* __restrict__ yw, double* __restrict__ accb,
                                                     double* __restrict__ lml, int* __restrict__ status, int n,
                                                     int ld, size_t mstride, int ystride, int nblk, int k, PfGen gen) {
  const int b = blockIdx.x;
  if (!GEN && status[b] != 0) return;
  PfPre nopre;  // (launch schedule: nothing to request ahead)
  nopre.state = 0;
  (void)pf_block<GEN, STAT, FORM, 0>(b, Kbuf, Wbuf, yw, accb, lml, status, n, ld, mstride, ystride, nblk, k, gen, false, nullptr,
                                     PsArgs(), nopre);
}

// ------------------------------------------------------------------------------------------
// Block column k of the LML path in ONE launch: diagonal factorisation and panel solve, W_kk never leaves LDS.
//
// Apart, potrf_kernel keeps one CU per matrix busy for ~30 us while the others idle, writes W_kk to memory only for trsm4_kernel to
// stream it back through every 64-row workgroup's ring, and that solve is a chain of ten dependent memory round trips per workgroup.
// Here matrix b gets S workgroups (b, p), p < S, each a whole CU with pf_block's LDS, that do not talk to each other:
//   1. every one of them factorises block (k, k) -- the same code on the same inputs, so the same bits, on CUs that had nothing to do;
//   2. with W_kk and z_k in its own LDS, workgroup p solves the row blocks i = k+1+p, k+1+p+S, ...:  X_i = A_ik W_kk^T in place,
//      y_i -= X_i z_k (pf_solve_mma / pf_solve_out, bgp_pf.h: step 1 of the launch-free chain role, the arithmetic of
//      trsm4_kernel), A fragments straight from memory into registers, those of the next row block requested before this one's MFMAs.
// In-place outputs would be a hazard: the co-workers (p >= 1) read block (k, k) and y_k as INPUTS and may start arbitrarily late.
// So nobody writes them: the owner (p = 0) alone puts L_kk into slot (b, k) of dW (nothing needs W_kk in memory any more), z_k into
// row b of `zbuf`, and updates acc / lml / status; block (k, k) of dK and segment k of yw keep their pre-factorisation contents
// (bgp_debug_workspace assembles L and z from both places).  A workgroup whose factorisation fails returns without solving.
// Workgroup id = p * B8 + b: the S workgroups of a matrix land on the XCD b % 8 and share its L2 for block (k, k).
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PF_THREADS) panel_kernel(double* __restrict__ Kbuf, double* __restrict__ Wbuf,
                                                           double* __restrict__ yw, double* __restrict__ zbuf,
                                                           double* __restrict__ accb, double* __restrict__ lml,
                                                           int* __restrict__ status, int n, int ld, size_t mstride, int ystride,
                                                           int nblk, int k, int B, int B8, int S) {
  __shared__ int st_lds;
  const int b = blockIdx.x % B8, p = blockIdx.x / B8;
  if (b >= B) return;
  // (one reader: the owner may set the status while a co-worker starts, and the workgroup must leave or stay as a whole)
  if (threadIdx.x == 0) st_lds = status[b];
  __syncthreads();
  if (st_lds != 0) return;
  PfPre nopre;
  nopre.state = 0;
  PfFuse fu;
  fu.L = p == 0 ? Wbuf + ((size_t)b * nblk + k) * (128 * 128) : nullptr;
  fu.z = zbuf + (size_t)b * ystride + k * 128;
  if (pf_block<0, 0, 0, 0, 1>(b, Kbuf, Wbuf, yw, accb, lml, status, n, ld, mstride, ystride, nblk, k, PfGen(), false, nullptr, PsArgs(),
                              nopre, fu))
    return;
  const PfLds lds = pf_lds();
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lr = lane & 15, lk = lane >> 4;
  int i = k + 1 + p;
  if (i >= nblk) return;
  double* const Ak = Kbuf + (size_t)b * mstride + (size_t)k * 128;  // block column k of the matrix
  double* const yb = yw + (size_t)b * ystride;
  const size_t rowoff = (size_t)(16 * w + lr) * ld;
  // Two fragment sets, half of the second at a time (three halves fit the register file beside the solve, four spilled): the
  // k-groups 0-3 of row block i + S are requested before the MFMAs of row block i, the k-groups 4-7 behind its k-step 15, into the
  // registers that the first half of row block i has left by then.
  double af[32], alo[16], ahi[16];
  pf_afrag_issue(Ak + (size_t)i * 128 * ld + rowoff, lk, af);
#pragma unroll 1
  for (; i < nblk; i += S) {
    asm volatile("" ::: "memory");  // (nothing in this loop writes LDS: without this, every W operand of the solve is hoisted out of it and spills)
    const bool more = i + S < nblk;  // (uniform)
    const double* const An = Ak + (size_t)(i + S) * 128 * ld + rowoff;
    if (more) pf_afrag_issue_half<0>(An, lk, alo);
    double* const yi = yb + i * 128;
    pf_afrag_transpose(af);
    d4 x[8];
#pragma unroll
    for (int j = 0; j < 8; j++) x[j] = (d4){0.0, 0.0, 0.0, 0.0};
    pf_solve_mma(af, lds.s, lds.Minv, lr, lk, x, [&] {
      if (more) pf_afrag_issue_half<1>(An, lk, ahi);
    });
    d4 yv;  // (requested behind the MFMAs: the registers are full until then; the X stores cover most of its latency)
#pragma unroll
    for (int r = 0; r < 4; r++) yv[r] = yi[16 * w + lk + 4 * r];
    pf_solve_out(x, lds.zpart, Ak + (size_t)i * 128 * ld, ld, w, lr, lk, yv, yi);
    if (more) {
#pragma unroll
      for (int t = 0; t < 16; t++) {
        af[t] = alo[t];
        af[16 + t] = ahi[t];
      }
    }
  }
}

// Device-resident ensemble sampler, n <= 128 (bgp_mcmc.hip): half-step h in ONE launch.  Workgroup i = proposal i of the half-step:
// q = c - (c - s) z from the ensemble in HBM, its log-prior (terms summed in theta order) and canonical hyper-parameters; the Gram
// block, its factorisation and the log-likelihood exactly as potrf_kernel<1, ...> (pf_block); then the accept test of ITS walker --
// the only writer of that walker's row, and nobody reads a mover's row in the half-step in which it moves (partners come from the
// other half) -- and the walker's row of the chain (a walker moves once per step: its row of step h / 2 is final here).
template <int STAT, int FORM>
__global__ void __launch_bounds__(PF_THREADS) mcmc_small_kernel(McmcArgs a, int h, double* __restrict__ lml, int* __restrict__ status,
                                                               int n, PfGen gen) {
#pragma clang fp contract(off)
  __shared__ double sh_qv[64], sh_pt[64];
  __shared__ double sh_prior;
  __shared__ int sh_acc;
  const int i = blockIdx.x, tid = threadIdx.x, p = a.p;
  const int m = a.movers[(size_t)h * a.Ns + i], pr = a.partners[(size_t)h * a.Ns + i];
  if (tid < p) {
    const double z = a.zz[(size_t)h * a.Ns + i];
    const double s = a.coords[(size_t)m * p + tid], c = a.coords[(size_t)pr * p + tid];
    const double v = c - (c - s) * z;
    sh_qv[tid] = v;
    if (!(v > -INFINITY && v < INFINITY)) {
      a.info[0] = 1u;
      if (v != v) {
        if (a.info[3] == 0u) a.info[3] = (unsigned)h + 1u;
      } else if (a.info[2] == 0u) {
        a.info[2] = (unsigned)h + 1u;
      }
    }
    sh_pt[tid] = mcmc_prior(a.prior_kind[tid], a.prior_par + 5 * tid, v);
  }
  __syncthreads();
  if (tid == 0) {
    double lp = 0.0;
    for (int k = 0; k < p; k++) lp += sh_pt[k];
    sh_prior = lp;
  }
  if (tid < a.hp) a.dh[(size_t)i * a.hp + tid] = a.h_src[tid] >= 0 ? sh_qv[a.h_src[tid]] : a.h_fixed[tid];
  __syncthreads();  // (the hyper-parameters are read back from memory by this workgroup only)
  PfPre nopre;
  nopre.state = 0;
  (void)pf_block<1, STAT, FORM, 0>(i, nullptr, nullptr, nullptr, nullptr, lml, status, n, 128, (size_t)0, 0, 1, 0, gen, false, nullptr,
                                   PsArgs(), nopre);
  __syncthreads();
  if (tid == 0) {
    double lp = sh_prior + lml[i];
    if (!(lp > -INFINITY && lp < INFINITY)) lp = -INFINITY;
    const bool acc = a.factors[(size_t)h * a.Ns + i] + lp - a.logp[m] > a.logu[(size_t)h * a.Ns + i];
    if (acc) {
      a.logp[m] = lp;
      a.nacc[m] += 1;
    }
    sh_acc = acc ? 1 : 0;
    a.lps[(size_t)(h >> 1) * a.W + m] = acc ? lp : a.logp[m];
  }
  __syncthreads();
  if (tid < p) {
    const double v = sh_acc ? sh_qv[tid] : a.coords[(size_t)m * p + tid];
    if (sh_acc) a.coords[(size_t)m * p + tid] = v;
    a.chain[((size_t)(h >> 1) * a.W + m) * p + tid] = v;
  }
}

int bgp_launch_mcmc_small(bgp_ctx* ctx, hipStream_t st, const McmcArgs& a, int h) {
  if (a.p > 64 || a.hp > 64) {
    bgp_set_error("bgp_launch_mcmc_small: more than 64 entries per walker");
    return BGP_ERR_INVALID;
  }
  PfGen g;
  g.X = ctx->dXeff;
  g.alpha = ctx->dalpha;
  g.H = ctx->dh;
  g.y = ctx->dy;
  g.d = ctx->d;
  KB_DISPATCH(ctx->ks.stationary, ctx->ks.form,
              hipLaunchKernelGGL((mcmc_small_kernel<S, F>), dim3(a.Ns), dim3(PF_THREADS), 0, st, a, h, ctx->dlml, ctx->dstatus, ctx->n, g));
  BGP_HIP(hipGetLastError());
  return BGP_OK;
}

// Debugging aid / accuracy test: the pivot root of the diagonal-block factorisation (pf_pivot_root) on n arguments.
__global__ void pivot_root_kernel(const double* __restrict__ x, double* __restrict__ s, double* __restrict__ iv, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double a, b;
  pf_pivot_root(x[i], a, b);
  s[i] = a;
  iv[i] = b;
}
extern "C" int bgp_debug_pivot_root(int device, int n, const double* x, double* sqrt_out, double* rsqrt_out) {
  if (n <= 0 || !x || !sqrt_out || !rsqrt_out) {
    bgp_set_error("bgp_debug_pivot_root: bad argument");
    return BGP_ERR_INVALID;
  }
  BGP_HIP(hipSetDevice(device));
  double* d = nullptr;
  BGP_HIP(hipMalloc(&d, (size_t)3 * n * sizeof(double)));
  hipError_t e = hipMemcpy(d, x, (size_t)n * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(pivot_root_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d, d + n, d + 2 * (size_t)n, n);
    e = hipMemcpy(sqrt_out, d + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
  }
  if (e == hipSuccess) e = hipMemcpy(rsqrt_out, d + 2 * (size_t)n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost);
  (void)hipFree(d);
  BGP_HIP(e);
  return BGP_OK;
}

// ------------------------------------------------------------------------------------------
// Launch-free factorisation of SMALL batches (B <= 64 matrices, or one large matrix): ONE persistent kernel per batch
// instead of ~3 dependent launches per block column (ps_kernel, bgp_ps.hip; the diagonal-block code is bgp_pf.h).
//
// Why: with few matrices the chain of dependent launches is the critical path -- potrf(k) keeps B of the 256 CUs busy
// for 30 us while the rest idle, and the trailing update of step k cannot overlap the next panel (stream / event
// look-ahead was measured slower than the chain it shortens: events cost more than they hide).  Here the diagonal-block
// chain and the tile work run SIDE BY SIDE inside one launch and talk through device-scope flags:
//   * chain role (workgroups 0 .. B-1, one per matrix; ps_chain_role, bgp_pf.h): walks the block columns J = 0 .. nblk-1:
//     factorises block (J, J) (pf_block: the same code as potrf_kernel), publishes L_JJ / W_JJ / z_J (wready[J]), then
//     solves block (J+1, J) and applies the last panel to block (J+1, J+1) ITSELF -- the next tile never leaves its LDS;
//   * tile role (the other workgroups, one per remaining CU; ps_tile_role, bgp_ps.hip): draw left-looking block tasks
//     from ticket counters in an order that is topological for the dependency graph -- panel solves S(I, J), I >= J+2, and
//     the pre-updates that hand blocks (I, I-1) and (I, I) to the chain -- waiting on / raising xready, subrdy, diagrdy.
// Both roles need a whole CU (157 / 128 KB of LDS, one array), the grid has at most one workgroup per CU and the
// dispatcher places workgroups in index order: the chain's B workgroups are resident before any tile workgroup, whatever
// else the GPU is doing.  (Round 3's first version ran two kernels on a pair of CU-masked streams: event hops, cold
// hardware queues -- ~45 us per call -- masks that only place properly for 1-4 or 8 CUs per XCD, and time-sliced queues
// once a few dozen masked streams were alive.)
// Every wait is bounded (PsArgs::spin_limit): a timeout raises the error word, both roles drain, and the host redoes
// the batch on the multi-launch path.  Arithmetic, operand order and summation order are those of the multi-launch path:
// the log-likelihoods are bit-identical (tests/test_gpu_persist.py).
// ------------------------------------------------------------------------------------------
void bgp_launch_ps(hipStream_t st, const PsArgs& a, int nwg);

// BGP_PS_TRACE=1: the time stamps of the last launch-free call (100 MHz wall clock): dims = {B, nblk, total tasks};
// chain (B x nblk x 8) then tile (total x 8): see tools/persist_trace.py.
extern "C" int bgp_debug_ps_trace(bgp_ctx* c, int* dims, unsigned long long* out, size_t cap) {
  if (!c || !dims) return BGP_ERR_INVALID;
  dims[0] = c->ps_trace_B;
  dims[1] = c->ps_trace_nblk;
  dims[2] = c->ps_trace_total;
  const size_t need = (size_t)c->ps_trace_B * c->ps_trace_nblk * 8 + (size_t)c->ps_trace_total * 8;
  if (!out || !c->ps_trace || need == 0) return BGP_OK;
  if (cap < need) return BGP_ERR_INVALID;
  BGP_HIP(hipSetDevice(c->device));
  BGP_HIP(hipMemcpy(out, c->ps_trace, need * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return BGP_OK;
}

// the flag block of a launch-free call with B matrices exists (grown with 50 % head room; contents undefined)
int bgp_ps_ensure_flags(bgp_ctx* c, int B) {
  const size_t words = ps_flag_words(B, c->nblk);
  return c->ps_flags.ensure(words, words + words / 2);
}

// Host side of the launch-free factorisation as the planner laid it out (bgp_plan.h: chain pairs, critical pool, task total, tile
// workgroups, Gram blocks inside the launch or by a kernel in front of it): ONE kernel on c->stream -- the chain workgroups + the
// tile workgroups -- and the copy of the error word to pinned memory (ctx->ps_herr): != 0 after the synchronisation means a wait
// timed out and the caller redoes the batch on the multi-launch path.  A warped batch's Gram matrices are on the stream already.
int bgp_launch_cholesky_persist(bgp_ctx* c, const BgpLmlPlan& plan) {
  const int nblk = c->nblk, ld = c->npad, B = plan.in.nb;
  if (plan.path != BGP_PATH_LAUNCH_FREE) {
    bgp_set_error("bgp_launch_cholesky_persist: B = %d, nblk = %d outside the persistent path's range", B, nblk);
    return BGP_ERR_INVALID;
  }
  if (!c->ps_herr) {
    const int rch = c->ps_herr.ensure(1);
    if (rch) return rch;
    *c->ps_herr = 0;
  }
  std::fill(c->fused_col.begin(), c->fused_col.end(), 0);  // (this path leaves every block of L and z in place)
  const size_t words = ps_flag_words(B, nblk);
  BGP_TRY(bgp_ps_ensure_flags(c, B));
  // (the device-resident sampler's step kernel has zeroed the block in front of this call: one dispatch less per half-step)
  if (!c->ps_resident) BGP_HIP(hipMemsetAsync(c->ps_flags, 0, words * sizeof(unsigned), c->stream));
  if (plan.gram_front && !plan.in.warped) BGP_TRY(bgp_launch_kbuild(c, B, 0, 0, 1));
  PsArgs a;
  a.K = c->dK;
  a.W = c->dW;
  a.yw = c->dyw;
  a.acc = c->dacc;
  a.lml = c->dlml;
  a.status = c->dstatus;
  a.flags = c->ps_flags;
  a.n = c->n;
  a.ld = ld;
  a.nblk = nblk;
  a.B = B;
  a.ystride = ld;
  a.mstride = (size_t)ld * ld;
  a.total = plan.total;
  a.ncrit = plan.ncrit;
  a.pair = plan.pair;
  a.Bpad = plan.Bpad;
  a.nchain = plan.nchain;
  a.psplit = plan.psplit;
  a.dsplit = plan.dsplit;
  a.ncrit_stream = plan.ncrit_stream;
  a.gen = plan.ps_gen;
  a.d = c->d;
  a.X = c->dXeff;
  a.alpha = c->dalpha;
  a.H = c->dh;
  a.y = c->dy;
  a.spin_limit = bgp_switch_ps_spin_limit();
  a.trace = nullptr;
  if (bgp_switch_ps_trace()) {
    const size_t need = (size_t)B * nblk * 8 + (size_t)a.total * 8;
    BGP_TRY(c->ps_trace.ensure(need));
    BGP_HIP(hipMemsetAsync(c->ps_trace, 0, need * sizeof(unsigned long long), c->stream));
    a.trace = c->ps_trace;
    c->ps_trace_B = B;
    c->ps_trace_nblk = nblk;
    c->ps_trace_total = a.total;
  }
  bgp_launch_ps(c->stream, a, plan.nchain + plan.tile_wgs);
  if (!c->ps_resident)
    BGP_HIP(hipMemcpyAsync(c->ps_herr, c->ps_flags + PS_ERROR, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
  BGP_HIP(hipGetLastError());
  return BGP_OK;
}

// LDS-DMA pipelined trailing update and panel solve (bgp_syrk4.hip)
void bgp_launch_syrk4(hipStream_t st, int B8, double* dK, const int* dstatus, int ld, size_t mstride, int nblk, int kp,
                      int K, int jstart, int colmode, int B);
void bgp_launch_trsm4(hipStream_t st, int B, double* dK, double* dW, double* dyw, int* dstatus, int ld, size_t mstride,
                      int ystride, int nblk, int k, int augmented);

void bgp_launch_potrf(bgp_ctx* ctx, hipStream_t st, int B, double* dK, double* dW, double* dyw, double* dacc,
                      double* dlml, int* dstatus, int ld, size_t mstride, int ystride, int k) {
  hipLaunchKernelGGL((potrf_kernel<0, 0, 0>), dim3(B), dim3(PF_THREADS), 0, st, dK, dW, dyw, dacc, dlml, dstatus, ctx->n, ld,
                     mstride, ystride, ctx->nblk, k, PfGen());
}

// Fused LML of a batch at n <= 128: ONE launch (Gram generation + factorisation + forward substitution + LML in the
// walker's workgroup).  dXb / xstride: per-walker warped inputs or the shared training set (xstride == 0 only).
int bgp_launch_lml_small(bgp_ctx* ctx, int off, int B, hipStream_t st) {
  PfGen g;
  g.X = ctx->dXeff;
  g.alpha = ctx->dalpha;
  g.H = ctx->dh + (size_t)off * (ctx->d + 2);
  g.y = ctx->dy;
  g.d = ctx->d;
  bgp_tbegin(ctx, 1, st);
  KB_DISPATCH(ctx->ks.stationary, ctx->ks.form,
              hipLaunchKernelGGL((potrf_kernel<1, S, F>), dim3(B), dim3(PF_THREADS), 0, st, (double*)nullptr,
                                 (double*)nullptr, (double*)nullptr, (double*)nullptr, ctx->dlml + off, ctx->dstatus + off,
                                 ctx->n, 128, (size_t)0, 0, 1, 0, g));
  bgp_tend(ctx, st);
  BGP_HIP(hipGetLastError());
  return BGP_OK;
}

void bgp_launch_syrk4_gen(hipStream_t st, int B8, double* dK, const int* dstatus, int ld, size_t mstride, int nblk, int kp,
                          int K, int jstart, int colmode, int B, const S4Gen& gen, int stationary, int form);

// Walker group g of a plan on the launch schedule (LML only: matrices npad x npad): the list of launches is the planner's
// (bgp_lml_schedule, bgp_plan.h); here are the buffers of the group's slice, the launches, their timing brackets and the counters.
int bgp_launch_lml_group(bgp_ctx* ctx, const BgpLmlPlan& plan, int g, hipStream_t st) {
  const int nblk = ctx->nblk, ld = ctx->npad, off = g * plan.gsz, B = plan.group_nb(g);
  const size_t mstride = (size_t)ld * ld;
  const int ystride = ld;
  const int B8 = 8 * ((B + 7) / 8);
  double* dK = ctx->dK + (size_t)off * mstride;
  double* dW = ctx->dW + (size_t)off * nblk * (128 * 128);
  double* dyw = ctx->dyw + (size_t)off * ystride;
  double* dzf = ctx->dzf + (size_t)off * ystride;  // z_k of the fused block columns (panel_kernel)
  double* dacc = ctx->dacc + (size_t)off * 4;
  double* dlml = ctx->dlml + off;
  int* dstatus = ctx->dstatus + off;
  if (ctx->fused_col.size() < (size_t)ctx->max_batch * nblk) ctx->fused_col.resize((size_t)ctx->max_batch * nblk, 0);
  S4Gen ga{};
  if (plan.gen(g)) {
    BGP_TRY(bgp_lml_gen_args(ctx, off, &ga));
    ctx->gen_batches++;
  }
  // the update of block columns j .. with the panels kp .. (K = their width); colmode 1: block column j alone
  auto update = [&](const BgpStep& s, int colmode) {
    if (s.gen) {
      bgp_launch_syrk4_gen(st, B8, dK, dstatus, ld, mstride, nblk, s.k, s.K, s.j, colmode, B, ga, ctx->ks.stationary, ctx->ks.form);
      ctx->gen_launches++;
    } else
      bgp_launch_syrk4(st, B8, dK, dstatus, ld, mstride, nblk, s.k, s.K, s.j, colmode, B);
  };
  bgp_lml_schedule(plan, g, [&](const BgpStep& s) {
    if (s.kind == BGP_STEP_PANEL || s.kind == BGP_STEP_POTRF)
      for (int bb = 0; bb < B; bb++) ctx->fused_col[(size_t)(off + bb) * nblk + s.k] = s.kind == BGP_STEP_PANEL;
    switch (s.kind) {
      case BGP_STEP_PANEL:  // (timed as the panel phase under "trsm")
        bgp_tbegin(ctx, 2, st);
        hipLaunchKernelGGL(panel_kernel, dim3(s.S * B8), dim3(PF_THREADS), 0, st, dK, dW, dyw, dzf, dacc, dlml, dstatus, ctx->n, ld,
                           mstride, ystride, nblk, s.k, B, B8, s.S);
        ctx->fused_launches++;
        break;
      case BGP_STEP_POTRF:
        bgp_tbegin(ctx, 1, st);
        hipLaunchKernelGGL((potrf_kernel<0, 0, 0>), dim3(B), dim3(PF_THREADS), 0, st, dK, dW, dyw, dacc, dlml, dstatus, ctx->n, ld,
                           mstride, ystride, nblk, s.k, PfGen());
        break;
      case BGP_STEP_TRSM:
        bgp_tbegin(ctx, 2, st);
        bgp_launch_trsm4(st, B, dK, dW, dyw, dstatus, ld, mstride, ystride, nblk, s.k, 0);
        break;
      case BGP_STEP_COLUMN:
        bgp_tbegin(ctx, 5, st);
        update(s, 1);
        break;
      case BGP_STEP_UPDATE:
        bgp_tbegin(ctx, 3, st);
        update(s, 0);
        break;
    }
    bgp_tend(ctx, st);
  });
  BGP_HIP(hipGetLastError());
  return BGP_OK;
}

// Posterior build: nblk steps on the (2 npad) x (2 npad) augmented matrices [[K, .], [I, 0]], the ring kernels in single-panel
// mode with the active-row remap of bgp_rowblk (nblk active row blocks at every step).  Nothing to decide: no plan.
static int launch_cholesky_augmented(bgp_ctx* ctx, int B) {
  const int nblk = ctx->nblk, ld = 2 * ctx->npad, ystride = ld, B8 = 8 * ((B + 7) / 8);
  const size_t mstride = (size_t)ld * ld;
  hipStream_t st = ctx->stream;
  double *dK = ctx->dK, *dW = ctx->dW, *dyw = ctx->dyw, *dacc = ctx->dacc, *dlml = ctx->dlml;
  int* dstatus = ctx->dstatus;
  std::fill(ctx->fused_col.begin(), ctx->fused_col.end(), 0);
  for (int k = 0; k < nblk; k++) {
    bgp_tbegin(ctx, 1, st);
    hipLaunchKernelGGL((potrf_kernel<0, 0, 0>), dim3(B), dim3(PF_THREADS), 0, st, dK, dW, dyw, dacc, dlml, dstatus, ctx->n,
                       ld, mstride, ystride, nblk, k, PfGen());
    bgp_tend(ctx, st);
    bgp_tbegin(ctx, 2, st);
    bgp_launch_trsm4(st, B, dK, dW, dyw, dstatus, ld, mstride, ystride, nblk, k, 1);
    bgp_tend(ctx, st);
    bgp_tbegin(ctx, 3, st);
    bgp_launch_syrk4(st, B8, dK, dstatus, ld, mstride, nblk, k, 128, 0, 2, B);
    bgp_tend(ctx, st);
  }
  BGP_HIP(hipGetLastError());
  return BGP_OK;
}

// B matrices that are in the workspace already (host Gram matrices; augmented: a posterior build), by launches on the context's stream
int bgp_launch_cholesky(bgp_ctx* ctx, int B, int augmented) {
  if (augmented) return launch_cholesky_augmented(ctx, B);
  return bgp_launch_lml_group(ctx, bgp_plan_lml(bgp_lml_shape(ctx, B, 0, 1)), 0, ctx->stream);
}
