// Variance-based (Sobol') sensitivity indices of the surrogate mean by the pick-freeze design.
//
// For resident posterior b with mean mu_b, two sample matrices A, Bm (N x d) and T terms, each a set of dimensions as a mask M_t:
//   fA_i = mu_b(A_i),  fB_i = mu_b(Bm_i),  fT_ti = mu_b(A_i with the columns in M_t taken from Bm_i)
//   f0  = (1 / 2N) sum_i (fA_i + fB_i)                         V   = (1 / 2N) sum_i ((fA_i - f0)^2 + (fB_i - f0)^2)
//   C_t = (1 / N)  sum_i (fB_i - f0) (fT_ti - fA_i)   (closed) J_t = (1 / 2N) sum_i (fA_i - fT_ti)^2   (total)
// Phase 1, sobol_mean_kernel: ONE routine for every mean.  A thread owns one synthetic row: it picks every column from the scaled
// A_i or the scaled Bm_i by its mask (fA is the empty mask, fB the full one), holds the row in registers and runs over the training
// points, whose scaled rows and alpha arrive as LDS broadcasts.  The squared distance is a sum of squares in x / l (fma, ascending
// dimension), never "the distance of A_i minus the swapped terms plus the new ones".  Rows are padded with zeros to DP = 8, 16 or 32
// columns on both sides: a padded column adds fma(0, 0, q) = q, so the bits do not depend on DP and the loop over the columns is
// fully unrolled (no register array is indexed at run time).  The means go to scratch, (T + 2) N per posterior.
// Phase 2 reduces them in a fixed order: chunks of SB_RC samples, a fixed tree inside a chunk, the chunk partials added in ascending
// order; f0 first, then the centred sums.  fp64 VALU work, no MFMA shape.  Plain launches; no workgroup waits for another; no
// floating-point atomics; every loop is bounded by an argument.  A term's values depend on the posterior, A, Bm and that term alone.
#include "bgp_common.h"
#include "bgp_device.h"

#define SB_TJ 64        // training points per LDS tile
#define SB_RC 256       // samples per chunk of the reduction (fixed: the order of accumulation must not depend on N, T or B)
#define SB_DMAX 32      // input dimensions: one mask bit each (larger d: the caller's route over predict)
#define SB_TMAX 4096    // terms per call
#define SB_NMAX (1 << 24)  // samples per call

// out[b][r][k] = in[r][k] / l_bk for k < d, 0 for d <= k < dp
__global__ void __launch_bounds__(256) sobol_scale_kernel(const double* __restrict__ in, int rows, int d, int dp,
                                                          const double* __restrict__ H, double* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (idx >= (size_t)rows * dp) return;
  const size_t r = idx / dp;
  const int k = (int)(idx - r * dp);
  out[(size_t)b * rows * dp + idx] = (k < d) ? in[r * d + k] / exp(H[(size_t)b * (d + 2) + 1 + k]) : 0.0;
}

// Thread tid of workgroup (blockIdx.x, y, z): sample i = 256 blockIdx.x + tid, row kind y (0: fA, 1: fB, 2 + t: term t), posterior z.
// LDS: SB_TJ x DP scaled training rows + SB_TJ alphas (16.5 KB at DP = 32), both read as broadcasts.
template <int STAT, int FORM, int DP>
__global__ void __launch_bounds__(256) sobol_mean_kernel(const double* __restrict__ Us, const double* __restrict__ ua,
                                                         const double* __restrict__ ub, const double* __restrict__ H,
                                                         const double* __restrict__ alpha, const unsigned* __restrict__ masks,
                                                         int n, int npad, int d, int N, int T, double* __restrict__ F) {
#pragma clang fp contract(off)
  __shared__ double Ut[SB_TJ * DP];
  __shared__ double al[SB_TJ];
  const int tid = threadIdx.x, kind = blockIdx.y, b = blockIdx.z;
  const int i = blockIdx.x * 256 + tid;
  const bool live = i < N;
  const unsigned full = (d >= 32) ? 0xffffffffu : ((1u << d) - 1u);
  const unsigned mask = (kind == 0) ? 0u : (kind == 1) ? full : masks[kind - 2];
  const double cst = exp(H[(size_t)b * (d + 2)]);
  const double* Ub = Us + (size_t)b * n * DP;
  const double* ab = alpha + (size_t)b * npad;
  double u[DP];
  {
    const size_t row = ((size_t)b * N + (live ? i : 0)) * DP;  // (a thread past N reads row 0 and writes nothing)
#pragma unroll
    for (int k = 0; k < DP; k++) u[k] = ((mask >> k) & 1u) ? ub[row + k] : ua[row + k];
  }
  double acc = 0.0;
  for (int j0 = 0; j0 < n; j0 += SB_TJ) {
    const int jc = min(SB_TJ, n - j0);
    __syncthreads();
    for (int idx = tid; idx < jc * DP; idx += 256) Ut[idx] = Ub[(size_t)j0 * DP + idx];
    if (tid < jc) al[tid] = ab[j0 + tid];
    __syncthreads();
    for (int j = 0; j < jc; j++) {
      double q = 0.0;
#pragma unroll
      for (int k = 0; k < DP; k++) {
        const double df = u[k] - Ut[j * DP + k];
        q = fma(df, df, q);
      }
      acc = fma(kb_value<STAT, FORM>(q, cst), al[j], acc);
    }
  }
  if (live) F[((size_t)b * (T + 2) + kind) * N + i] = acc;
}

// the sum of the workgroup's 256 values in a fixed tree; the result is in every thread
static __device__ __forceinline__ double sobol_tree(double v, double* sh) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = v;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sh[tid] = sh[tid] + sh[tid + o];
    __syncthreads();
  }
  return sh[0];
}

// p0[b][c] = sum over chunk c of (fA_i + fB_i)
__global__ void __launch_bounds__(SB_RC) sobol_f0_part_kernel(const double* __restrict__ F, int N, int T, int nchunk,
                                                              double* __restrict__ p0) {
#pragma clang fp contract(off)
  __shared__ double sh[SB_RC];
  const int c = blockIdx.x, b = blockIdx.y, i = c * SB_RC + threadIdx.x;
  const double* fA = F + (size_t)b * (T + 2) * N;
  const double* fB = fA + N;
  const double s = sobol_tree(i < N ? fA[i] + fB[i] : 0.0, sh);
  if (threadIdx.x == 0) p0[(size_t)b * nchunk + c] = s;
}

// out[r] = (sum of part[r][0 .. nchunk), ascending chunk) / den
__global__ void __launch_bounds__(256) sobol_sum_kernel(const double* __restrict__ part, int rows, int nchunk, double den,
                                                        double* __restrict__ out) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  double s = 0.0;
  for (int c = 0; c < nchunk; c++) s += part[(size_t)r * nchunk + c];
  out[r] = s / den;
}

// blockIdx.y = 0: pV[b][c] = sum over chunk c of (fA - f0)^2 + (fB - f0)^2;  blockIdx.y = 1 + t: pC[b][t][c] = sum of
// (fB - f0) (fT - fA) and pJ[b][t][c] = sum of (fA - fT)^2
__global__ void __launch_bounds__(SB_RC) sobol_centred_part_kernel(const double* __restrict__ F, const double* __restrict__ f0,
                                                                   int N, int T, int nchunk, double* __restrict__ pV,
                                                                   double* __restrict__ pC, double* __restrict__ pJ) {
#pragma clang fp contract(off)
  __shared__ double sh[SB_RC];
  const int c = blockIdx.x, y = blockIdx.y, b = blockIdx.z, i = c * SB_RC + threadIdx.x;
  const bool live = i < N;
  const double* fA = F + (size_t)b * (T + 2) * N;
  const double* fB = fA + N;
  const double m = f0[b];
  const double a = live ? fA[i] : 0.0, bb = live ? fB[i] : 0.0;
  if (y == 0) {
    const double da = a - m, db = bb - m;
    const double s = sobol_tree(live ? da * da + db * db : 0.0, sh);
    if (threadIdx.x == 0) pV[(size_t)b * nchunk + c] = s;
    return;
  }
  const int t = y - 1;
  const double ft = live ? fA[(size_t)(2 + t) * N + i] : 0.0;
  const double dt = ft - a;
  const double sc = sobol_tree(live ? (bb - m) * dt : 0.0, sh);
  const double sj = sobol_tree(live ? dt * dt : 0.0, sh);
  if (threadIdx.x == 0) {
    pC[((size_t)b * T + t) * nchunk + c] = sc;
    pJ[((size_t)b * T + t) * nchunk + c] = sj;
  }
}

template <int DP>
static void sobol_launch_means(bgp_ctx* c, int B, int N, int T, const double* dUs, const double* dua, const double* dub,
                               const double* dH, const unsigned* dmasks, double* dF) {
  const dim3 grid((N + 255) / 256, T + 2, B);
  KB_DISPATCH(c->ks.stationary, c->ks.form,
              hipLaunchKernelGGL((sobol_mean_kernel<S, F, DP>), grid, dim3(256), 0, c->stream, dUs, dua, dub, dH, c->dalpha_sol,
                                 dmasks, c->n, c->npad, c->d, N, T, dF));
}

static int sobol_run(bgp_ctx* c, int B, const double* h_kernel, int N, const double* A, const double* Bm, int T,
                     const unsigned* masks, double* f0, double* V, double* closed, double* total) {
  const int n = c->n, d = c->d, dp = d <= 8 ? 8 : d <= 16 ? 16 : 32, nchunk = (N + SB_RC - 1) / SB_RC;
  const size_t p = d + 2;
  double *dA, *dB, *dH, *dUs, *dua, *dub, *dF, *dp0, *dpV, *dpC, *dpJ, *dout;
  unsigned* dmasks;
  BgpScratch live(c);
  BGP_TRY(live.carve([&](BgpCarve& s) {
    dA = s.take<double>((size_t)N * d);
    dB = s.take<double>((size_t)N * d);
    dH = s.take<double>((size_t)B * p);
    dUs = s.take<double>((size_t)B * n * dp);
    dua = s.take<double>((size_t)B * N * dp);
    dub = s.take<double>((size_t)B * N * dp);
    dmasks = s.take<unsigned>((size_t)T);
    dF = s.take<double>((size_t)B * (T + 2) * N);  // the means: all the scratch that grows with N T
    dp0 = s.take<double>((size_t)B * nchunk);
    dpV = s.take<double>((size_t)B * nchunk);
    dpC = s.take<double>((size_t)B * T * nchunk);
    dpJ = s.take<double>((size_t)B * T * nchunk);
    dout = s.take<double>((size_t)B * (2 + 2 * (size_t)T));  // f0 (B), V (B), closed (B T), total (B T)
  }));
  hipStream_t st = c->stream;
  double *df0 = dout, *dV = dout + B, *dC = dout + 2 * (size_t)B, *dJ = dC + (size_t)B * T;
  // both matrices the way predict's queries go up: through the context-level warp when one is set
  BGP_TRY(post_stage_queries(c, dA, A, N));
  BGP_TRY(post_stage_queries(c, dB, Bm, N));
  BGP_HIP(bgp_memcpy_async(dH, h_kernel, (size_t)B * p * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(dmasks, masks, (size_t)T * sizeof(unsigned), hipMemcpyHostToDevice, st));
  const auto blocks = [](size_t items) { return (unsigned)((items + 255) / 256); };
  hipLaunchKernelGGL(sobol_scale_kernel, dim3(blocks((size_t)n * dp), B), dim3(256), 0, st, c->dXeff, n, d, dp, dH, dUs);
  hipLaunchKernelGGL(sobol_scale_kernel, dim3(blocks((size_t)N * dp), B), dim3(256), 0, st, dA, N, d, dp, dH, dua);
  hipLaunchKernelGGL(sobol_scale_kernel, dim3(blocks((size_t)N * dp), B), dim3(256), 0, st, dB, N, d, dp, dH, dub);
  if (dp == 8)
    sobol_launch_means<8>(c, B, N, T, dUs, dua, dub, dH, dmasks, dF);
  else if (dp == 16)
    sobol_launch_means<16>(c, B, N, T, dUs, dua, dub, dH, dmasks, dF);
  else
    sobol_launch_means<32>(c, B, N, T, dUs, dua, dub, dH, dmasks, dF);
  hipLaunchKernelGGL(sobol_f0_part_kernel, dim3(nchunk, B), dim3(SB_RC), 0, st, dF, N, T, nchunk, dp0);
  hipLaunchKernelGGL(sobol_sum_kernel, dim3(blocks(B)), dim3(256), 0, st, dp0, B, nchunk, 2.0 * (double)N, df0);
  hipLaunchKernelGGL(sobol_centred_part_kernel, dim3(nchunk, T + 1, B), dim3(SB_RC), 0, st, dF, df0, N, T, nchunk, dpV, dpC, dpJ);
  hipLaunchKernelGGL(sobol_sum_kernel, dim3(blocks(B)), dim3(256), 0, st, dpV, B, nchunk, 2.0 * (double)N, dV);
  hipLaunchKernelGGL(sobol_sum_kernel, dim3(blocks((size_t)B * T)), dim3(256), 0, st, dpC, B * T, nchunk, (double)N, dC);
  hipLaunchKernelGGL(sobol_sum_kernel, dim3(blocks((size_t)B * T)), dim3(256), 0, st, dpJ, B * T, nchunk, 2.0 * (double)N, dJ);
  BGP_HIP(hipGetLastError());
  BGP_HIP(bgp_memcpy_async(f0, df0, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_memcpy_async(V, dV, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_memcpy_async(closed, dC, (size_t)B * T * sizeof(double), hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_memcpy_async(total, dJ, (size_t)B * T * sizeof(double), hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_stream_sync(st));
  return BGP_OK;
}

extern "C" int bgp_sobol_indices(bgp_ctx* c, int B, const double* h_kernel, int N, const double* A, const double* Bm, int T,
                                 const unsigned* masks, double* f0, double* V, double* closed, double* total) {
  BGP_TRY(bgp_guard(c, "bgp_sobol_indices", BGP_POST_PLAIN));
  if (!h_kernel || !A || !Bm || !masks || !f0 || !V || !closed || !total || B <= 0 || B > 65535 || N <= 0 || N > SB_NMAX ||
      T <= 0 || T > SB_TMAX) {
    bgp_set_error("bgp_sobol_indices: bad argument (1 <= B <= 65535, 1 <= N <= %d, 1 <= T <= %d)", SB_NMAX, SB_TMAX);
    return BGP_ERR_INVALID;
  }
  const int d = c->d;
  if (d > SB_DMAX) {
    bgp_set_error("bgp_sobol_indices: d > %d is not supported", SB_DMAX);
    return BGP_ERR_INVALID;
  }
  for (int t = 0; t < T; t++)
    if (d < 32 && (masks[t] >> d) != 0u) {
      bgp_set_error("bgp_sobol_indices: term %d = 0x%x names a dimension outside [0, %d)", t, masks[t], d);
      return BGP_ERR_INVALID;
    }
  if ((double)B * (double)(T + 2) * (double)N > (double)((size_t)1 << 30)) {
    bgp_set_error("bgp_sobol_indices: more than 2^30 means (B (T + 2) N) in one call");
    return BGP_ERR_INVALID;
  }
  BGP_TRY(bgp_guard(c, "bgp_sobol_indices", BGP_POST_PLAIN, B));
  return post_call(c, [&] { return sobol_run(c, B, h_kernel, N, A, Bm, T, masks, f0, V, closed, total); });
}
