// Posterior covariance of the surrogate's gradient and the active-subspace sums.
//
// With G_jk(x) = d k(x, X_j) / dx_k = cf fac(r_j) (x_k - X_jk) / l_k^2 (cf = c in the product form, 1 in the sum form; fac as in
// bgp_predgrad.hip; the constant and white terms add nothing) and H0 = diag(cf phi / l_k^2), phi = -fac(0) (1 RBF, 3 Matern 3/2,
// 5/3 Matern 5/2), for resident posterior b and query point x_s:
//   g(x)  = G(x)^T alpha                   gradient of the mean                                  (d)
//   Sigma = H0 - G(x)^T K^-1 G(x)          posterior covariance of grad f(x), latent function      (d x d)
//   C_mean = (1 / m) sum_s g(x_s) g(x_s)^T     C_cov = (1 / m) sum_s Sigma(x_s)
// Stages, plain launches on the context's stream:
//   1  gcov_build_kernel     R (rows (s, k), a point's d rows contiguous; columns j; zero padded to 128 rows and npad columns).  A
//                            workgroup owns 64 training points (LDS tile, k-major) and GC_PT query points (LDS broadcasts); a wave
//                            takes a point, a lane a training point; the squared distance once per (point, training point), a sum of
//                            squares in ascending k.
//   2  bgp_launch_gemm4      P = R K^-1 on the LDS-DMA ring (fp64 MFMA): the hot product, 2 n^2 m d flops per posterior.
//   3  gcov_contract_kernel  one workgroup per (point, posterior): g_k = sum_j alpha_j R[(s,k),j] and, for k >= l only,
//                            Q[k,l] = sum_j P[(s,k),j] R[(s,l),j]; Sigma = H0 - Q mirrored, the diagonal clipped at 0.  A pair's sum
//                            is dealt over JS(d) interleaved slices of j (a function of d alone), each ascending, the slices added in
//                            ascending order.
//   4  gcov_part_kernel / gcov_accum_kernel / gcov_finish_kernel   g g^T and Sigma over the points: chunks of 256 points by GLOBAL
//                            point index, a fixed tree inside a chunk (butterfly inside a wave, the four waves ascending), chunk
//                            partials added in ascending order, one division by m.
// No workgroup waits for another; no floating-point atomics; every loop is bounded by an argument.  A point's g and Sigma depend on
// the posterior and that point alone (not on m, B, the other points or the chunking); the sums on the posterior and the ordered point
// list alone.  Matern 1/2 is not mean-square differentiable: refused.
#include "bgp_common.h"
#include "bgp_device.h"

#define GC_DMAX 32          // input dimensions
#define GC_TJ 64            // training points per LDS tile
#define GC_PT 16            // query points per workgroup of the build
#define GC_LD 65            // LDS leading dimension of a d x 64 tile (odd: the rows of a pair's operands fall on different banks)
#define GC_RC 256           // points per chunk of the reduction (fixed: the order of accumulation must not depend on m or B)
#define GC_EB 128           // entries of (g g^T, Sigma) per workgroup of the reduction
#define GC_MDMAX (1 << 24)  // m d per call
#define GC_UMAX 3           // (pair, slice) units per thread of the contraction: (GC_DMAX (GC_DMAX + 1) / 2 + GC_DMAX) / 256, rounded up

// R[b][(s d + k) npad + j] for the points s of this chunk; grid (npad / 64, points / GC_PT, posteriors)
template <int STAT, int FORM>
__global__ void __launch_bounds__(256) gcov_build_kernel(const double* __restrict__ X, int n, int npad, int d,
                                                         const double* __restrict__ H, const double* __restrict__ Xq, int mm,
                                                         size_t sR, double* __restrict__ R) {
#pragma clang fp contract(off)
  __shared__ double Xt[GC_DMAX * GC_TJ];
  __shared__ double xq[GC_PT * GC_DMAX];
  __shared__ double il[GC_DMAX];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int j0 = blockIdx.x * GC_TJ, s0 = blockIdx.y * GC_PT, b = blockIdx.z;
  const double* h = H + (size_t)b * (d + 2);
  if (tid < d) il[tid] = 1.0 / exp(h[1 + tid]);
  for (int idx = tid; idx < GC_TJ * d; idx += 256) {
    const int jj = idx / d, k = idx - jj * d;
    Xt[k * GC_TJ + jj] = (j0 + jj < n) ? X[(size_t)(j0 + jj) * d + k] : 0.0;
  }
  for (int idx = tid; idx < GC_PT * d; idx += 256) {
    const int p = idx / d, k = idx - p * d;
    xq[p * GC_DMAX + k] = (s0 + p < mm) ? Xq[(size_t)(s0 + p) * d + k] : 0.0;
  }
  __syncthreads();
  const double cst = exp(h[0]);
  const int j = j0 + lane;
  double* Rb = R + (size_t)b * sR;
  for (int p = wv; p < GC_PT; p += 4) {
    const int s = s0 + p;
    if (s >= mm) break;
    double r2 = 0.0;
    for (int k = 0; k < d; k++) {
      const double df = (xq[p * GC_DMAX + k] - Xt[k * GC_TJ + lane]) * il[k];
      r2 = fma(df, df, r2);
    }
    double S, fac;
    kb_stationary_fac<STAT>(r2, S, fac);
    const double g = (FORM == BGP_FORM_PRODUCT) ? cst * fac : fac;
    for (int k = 0; k < d; k++) {
      const double u = ((xq[p * GC_DMAX + k] - Xt[k * GC_TJ + lane]) * il[k]) * il[k];
      Rb[((size_t)s * d + k) * npad + j] = (j < n) ? g * u : 0.0;  // (j < npad: the grid covers npad / 64 tiles)
    }
  }
}

// rows [r0, r1) of every posterior's R: zeros (the 128-row padding that the product reads)
__global__ void __launch_bounds__(256) gcov_zero_rows_kernel(double* __restrict__ R, size_t sR, int r0, int r1, int npad) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < (size_t)(r1 - r0) * npad) R[(size_t)blockIdx.y * sR + (size_t)r0 * npad + idx] = 0.0;
}

// slices a pair's sum over j is dealt in: the largest power of two <= 256 / (pairs of d), between 1 and 64 -- a function of d alone
static __host__ __device__ __forceinline__ int gcov_slices(int d) {
  const int pairs = d * (d + 1) / 2 + d;
  int js = 1;
  while (js < 64 && 2 * js * pairs <= 256) js *= 2;
  return js;
}

// One workgroup per (point s, posterior b).  Pair p < d: g_p (operands alpha, R row p); pair d + q: Q[k][l], q = k (k + 1) / 2 + l,
// l <= k (operands P row k, R row l; only when P != nullptr).  fam: phi of the family.
__global__ void __launch_bounds__(256) gcov_contract_kernel(const double* __restrict__ R, const double* __restrict__ P, size_t sR,
                                                            const double* __restrict__ alphaB, const double* __restrict__ H,
                                                            int product, double phi, int n, int npad, int d, int mm,
                                                            double* __restrict__ gout, double* __restrict__ cov) {
#pragma clang fp contract(off)
  __shared__ double At[(GC_DMAX + 1) * GC_LD];  // P rows of the point, row d: alpha
  __shared__ double Rt[GC_DMAX * GC_LD];
  __shared__ double part[GC_UMAX * 256];
  const int tid = threadIdx.x, s = blockIdx.x, b = blockIdx.y;
  const int js = gcov_slices(d);
  const int npair = d + (P ? d * (d + 1) / 2 : 0), units = npair * js;
  const double* Rb = R + (size_t)b * sR + (size_t)s * d * npad;
  const double* Pb = P ? P + (size_t)b * sR + (size_t)s * d * npad : nullptr;
  const double* ab = alphaB + (size_t)b * npad;
  int ia[GC_UMAX], ib[GC_UMAX], sl[GC_UMAX];
  double acc[GC_UMAX];
#pragma unroll
  for (int i = 0; i < GC_UMAX; i++) {
    const int u = tid + 256 * i;
    const int p = u / js;
    sl[i] = (u < units) ? u - p * js : GC_TJ;  // (a unit past the end runs no step)
    acc[i] = 0.0;
    if (p < d || u >= units) {
      ia[i] = d, ib[i] = (u < units) ? p : 0;
    } else {
      const int q = p - d;
      int k = 0;
      while ((k + 1) * (k + 2) / 2 <= q) k++;  // (at most d steps)
      ia[i] = k, ib[i] = q - k * (k + 1) / 2;
    }
  }
  for (int j0 = 0; j0 < n; j0 += GC_TJ) {  // (j0 + 64 <= npad; the columns n .. npad of R are zeros)
    __syncthreads();
    for (int idx = tid; idx < d * GC_TJ; idx += 256) {
      const int k = idx >> 6, jj = idx & 63;
      Rt[k * GC_LD + jj] = Rb[(size_t)k * npad + j0 + jj];
      if (Pb) At[k * GC_LD + jj] = Pb[(size_t)k * npad + j0 + jj];
    }
    if (tid < GC_TJ) At[d * GC_LD + tid] = (j0 + tid < n) ? ab[j0 + tid] : 0.0;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < GC_UMAX; i++)
      for (int jj = sl[i]; jj < GC_TJ; jj += js) acc[i] = fma(At[ia[i] * GC_LD + jj], Rt[ib[i] * GC_LD + jj], acc[i]);
  }
#pragma unroll
  for (int i = 0; i < GC_UMAX; i++) part[tid + 256 * i] = acc[i];
  __syncthreads();
  const size_t o = (size_t)b * mm + s;
  for (int p = tid; p < npair; p += 256) {
    double q = 0.0;
    for (int t = 0; t < js; t++) q += part[p * js + t];
    if (p < d) {
      gout[o * d + p] = q;
      continue;
    }
    const int qq = p - d;
    int k = 0;
    while ((k + 1) * (k + 2) / 2 <= qq) k++;
    const int l = qq - k * (k + 1) / 2;
    double v;
    if (k == l) {
      const double ilk = 1.0 / exp(H[(size_t)b * (d + 2) + 1 + k]);
      const double h0 = ((product ? exp(H[(size_t)b * (d + 2)]) * phi : phi) * ilk) * ilk;
      v = h0 - q;
      v = v > 0.0 ? v : 0.0;  // (clipped at 0 as the predictive variance is)
    } else {
      v = 0.0 - q;
    }
    cov[(o * d + k) * d + l] = v;
    cov[(o * d + l) * d + k] = v;
  }
}

// part[b][c][e] = sum over the 256 points of chunk c of entry e: e < d d: g_k g_l, else Sigma_kl.  grid (chunks, entry blocks, posteriors)
__global__ void __launch_bounds__(GC_RC) gcov_part_kernel(const double* __restrict__ G, const double* __restrict__ S, int mm, int d,
                                                          int nch, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double wp[GC_EB * 4];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = blockIdx.x, e0 = blockIdx.y * GC_EB, b = blockIdx.z;
  const int dd = d * d, s = c * GC_RC + tid;
  const bool live = s < mm;
  const size_t o = (size_t)b * mm + (live ? s : 0);
  for (int i = 0; i < GC_EB; i++) {
    const int e = e0 + i;
    if (e >= 2 * dd) break;
    double v = 0.0;
    if (live) {
      if (e < dd) {
        const int k = e / d, l = e - k * d;
        v = G[o * d + k] * G[o * d + l];
      } else {
        v = S[o * dd + (e - dd)];
      }
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
    if (lane == 0) wp[i * 4 + wv] = v;
  }
  __syncthreads();
  if (tid < GC_EB && e0 + tid < 2 * dd)
    part[((size_t)b * nch + c) * (2 * dd) + e0 + tid] = ((wp[tid * 4] + wp[tid * 4 + 1]) + wp[tid * 4 + 2]) + wp[tid * 4 + 3];
}

// acc[b][e] += part[b][0 .. nch)[e], ascending chunk
__global__ void __launch_bounds__(256) gcov_accum_kernel(const double* __restrict__ part, int nch, int E, double* __restrict__ acc) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (e >= E) return;
  double s = acc[(size_t)b * E + e];
  for (int c = 0; c < nch; c++) s += part[((size_t)b * nch + c) * E + e];
  acc[(size_t)b * E + e] = s;
}

__global__ void __launch_bounds__(256) gcov_finish_kernel(double* __restrict__ acc, size_t items, double den) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < items) acc[i] = acc[i] / den;
}

// Points per chunk: a multiple of GC_RC (the reduction's chunks go by global point index) that depends on n and d alone, so that a
// posterior's R stays within 2^25 doubles where 256 points allow it.  BGP_GCOV_CHUNK (tests): another size, rounded up to GC_RC.
static size_t gcov_point_chunk(int npad, int d) {
  size_t mc = (((size_t)1 << 25) / ((size_t)npad * d)) / GC_RC * GC_RC;
  if (const char* e = bgp_switch(BGP_SW_GCOV_CHUNK)) {
    const long v = atol(e);
    if (v > 0) mc = ((size_t)v + GC_RC - 1) / GC_RC * GC_RC;
  }
  return std::min<size_t>(std::max<size_t>(mc, GC_RC), (size_t)1 << 19);  // (the build's grid: chunk / GC_PT <= 65535 in y)
}

static int gcov_run(bgp_ctx* c, int B, const double* h_kernel, int m, const double* Xq, double* dmean, double* cov, double* csum) {
  const int n = c->n, d = c->d, npad = c->npad, dd = d * d, E = 2 * dd;
  const size_t p = d + 2;
  const bool wantP = cov || csum;
  const size_t mc = std::min(gcov_point_chunk(npad, d), ((size_t)m + GC_RC - 1) / GC_RC * GC_RC);
  const size_t rows = (mc * d + 127) / 128 * 128, sR = rows * npad;  // a posterior's R (and P) of one point chunk
  // posteriors per chunk: R and P of a chunk within 2^29 doubles together
  // (BGP_ITEM_CHUNK, tests: forced posterior chunks against the default)
  const int Bc = (int)bgp_switch_cap(BGP_SW_ITEM_CHUNK, std::max<size_t>(1, std::min<size_t>((size_t)B, ((size_t)1 << 28) / sR)));
  const int nchmax = (int)(mc / GC_RC);
  double *dXq, *dH, *dR, *dP = nullptr, *dG, *dS = nullptr, *dpart = nullptr, *dacc = nullptr;
  BgpScratch live(c);
  BGP_TRY(live.carve([&](BgpCarve& s) {
    dXq = s.take<double>(mc * d);
    dH = s.take<double>((size_t)B * p);
    dR = s.take<double>((size_t)Bc * sR);
    if (wantP) dP = s.take<double>((size_t)Bc * sR);
    dG = s.take<double>((size_t)Bc * mc * d);
    if (wantP) dS = s.take<double>((size_t)Bc * mc * dd);
    if (csum) {
      dpart = s.take<double>((size_t)Bc * nchmax * E);
      dacc = s.take<double>((size_t)Bc * E);
    }
  }));
  hipStream_t st = c->stream;
  const double phi = c->ks.stationary == BGP_RBF ? 1.0 : c->ks.stationary == BGP_MATERN32 ? 3.0 : 5.0 / 3.0;
  const int product = c->ks.form == BGP_FORM_PRODUCT;
  const auto blocks = [](size_t items) { return (unsigned)((items + 255) / 256); };
  BGP_HIP(bgp_memcpy_async(dH, h_kernel, (size_t)B * p * sizeof(double), hipMemcpyHostToDevice, st));
  c->chunk_last[0] = c->chunk_last[1] = 0;
  for (int b0 = 0; b0 < B; b0 += Bc) {
    const int nb = std::min(Bc, B - b0);
    const double* dHb = dH + (size_t)b0 * p;
    c->chunk_last[0]++;
    if (csum) BGP_HIP(hipMemsetAsync(dacc, 0, (size_t)nb * E * sizeof(double), st));
    for (size_t m0 = 0; m0 < (size_t)m; m0 += mc) {
      const int mm = (int)std::min(mc, (size_t)m - m0);
      if (b0 == 0) c->chunk_last[1]++;
      const int md = mm * d, mdpad = (md + 127) / 128 * 128;
      BGP_HIP(bgp_memcpy_async(dXq, Xq + m0 * d, (size_t)md * sizeof(double), hipMemcpyHostToDevice, st));
      KB_DISPATCH(c->ks.stationary, c->ks.form,
                  hipLaunchKernelGGL((gcov_build_kernel<S, F>), dim3(npad / GC_TJ, (mm + GC_PT - 1) / GC_PT, nb), dim3(256), 0, st,
                                     c->dXeff, n, npad, d, dHb, dXq, mm, sR, dR));
      if (mdpad > md)
        hipLaunchKernelGGL(gcov_zero_rows_kernel, dim3(blocks((size_t)(mdpad - md) * npad), nb), dim3(256), 0, st, dR, sR, md, mdpad,
                           npad);
      if (wantP)
        bgp_launch_gemm4(st, 0, dR, c->dKinv + (size_t)b0 * npad * npad, npad, mdpad, npad, npad, dP, npad, nb, sR,
                         (size_t)npad * npad, sR, nullptr);
      hipLaunchKernelGGL(gcov_contract_kernel, dim3(mm, nb), dim3(256), 0, st, dR, dP, sR, c->dalpha_sol + (size_t)b0 * npad, dHb,
                         product, phi, n, npad, d, mm, dG, dS);
      if (csum) {
        const int nch = (mm + GC_RC - 1) / GC_RC;
        hipLaunchKernelGGL(gcov_part_kernel, dim3(nch, (E + GC_EB - 1) / GC_EB, nb), dim3(GC_RC), 0, st, dG, dS, mm, d, nch, dpart);
        hipLaunchKernelGGL(gcov_accum_kernel, dim3(blocks(E), nb), dim3(256), 0, st, dpart, nch, E, dacc);
      }
      BGP_HIP(hipGetLastError());
      const size_t wg = (size_t)md * sizeof(double), wc = (size_t)md * d * sizeof(double);
      if (dmean)
        BGP_HIP(bgp_memcpy2d_async(dmean + ((size_t)b0 * m + m0) * d, (size_t)m * d * sizeof(double), dG, wg, wg, nb,
                                   hipMemcpyDeviceToHost, st));
      if (cov)
        BGP_HIP(bgp_memcpy2d_async(cov + ((size_t)b0 * m + m0) * dd, (size_t)m * dd * sizeof(double), dS, wc, wc, nb,
                                   hipMemcpyDeviceToHost, st));
      BGP_HIP(bgp_stream_sync(st));  // (the next chunk reuses the buffers)
    }
    if (csum) {
      hipLaunchKernelGGL(gcov_finish_kernel, dim3(blocks((size_t)nb * E)), dim3(256), 0, st, dacc, (size_t)nb * E, (double)m);
      BGP_HIP(hipGetLastError());
      BGP_HIP(bgp_memcpy_async(csum + (size_t)b0 * E, dacc, (size_t)nb * E * sizeof(double), hipMemcpyDeviceToHost, st));
      BGP_HIP(bgp_stream_sync(st));
    }
  }
  return BGP_OK;
}

extern "C" int bgp_grad_cov(bgp_ctx* c, int B, const double* h_kernel, int m, const double* Xq, double* dmean, double* cov,
                            double* csum) {
  BGP_TRY(bgp_guard(c, "bgp_grad_cov", BGP_POST_PLAIN));
  if (!h_kernel || !Xq || (!dmean && !cov && !csum) || m <= 0 || B <= 0 || B > 65535) {
    bgp_set_error("bgp_grad_cov: bad argument (1 <= B <= 65535, 1 <= m, at least one output)");
    return BGP_ERR_INVALID;
  }
  if (c->d > GC_DMAX || c->has_warp) {
    bgp_set_error("bgp_grad_cov: %s", c->has_warp ? "warped inputs are not supported" : "d > 32 is not supported");
    return BGP_ERR_INVALID;
  }
  if (c->ks.stationary == BGP_MATERN12) {
    bgp_set_error("bgp_grad_cov: the Matern 1/2 kernel is not differentiable (no gradient covariance exists)");
    return BGP_ERR_INVALID;
  }
  if ((double)m * (double)c->d > (double)GC_MDMAX) {
    bgp_set_error("bgp_grad_cov: m d = %.0f exceeds %d", (double)m * (double)c->d, GC_MDMAX);
    return BGP_ERR_INVALID;
  }
  BGP_TRY(bgp_guard(c, "bgp_grad_cov", BGP_POST_PLAIN, B));
  return post_call(c, [&] { return gcov_run(c, B, h_kernel, m, Xq, dmean, cov, csum); });
}
