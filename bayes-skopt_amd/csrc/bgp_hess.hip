// Posterior of the surrogate's Hessian.
//
// With z_k = (x_k - X_jk) / l_k, r^2 = sum_k z_k^2, fac(r) = S'(r) / r as in bgp_predgrad.hip and fac2(r) = fac'(r) / r (RBF:
// exp(-r^2 / 2); Matern 5/2: (25 / 3) exp(-sqrt5 r)), cf = c in the product form and 1 in the sum form (the constant and white terms
// add nothing), T = d (d + 1) / 2 and vech order (k, l), k >= l, row-major over the lower triangle:
//   h_kl(j) = d^2 k(x, X_j) / dx_k dx_l = cf [fac delta_kl / l_k^2 + fac2 z_k z_l / (l_k l_l)]        row (k, l) of R(x), T x n
//   Hbar    = R(x) alpha                                                                             Hessian of the mean
//   P0[(k,l),(p,q)] = cf psi (delta_kl delta_pq + delta_kp delta_lq + delta_kq delta_lp) / (l_k l_l l_p l_q),   psi = fac2(0)
//   Cov[H_kl, H_pq] = P0 - R(x) K^-1 R(x)^T                                                           T x T, latent function
// Stages, plain launches on the context's stream:
//   1  hess_build_kernel     R (a point's Tp = pad16(T) rows contiguous; columns j; the rows T .. Tp, the rows up to the 128-row pad
//                            and the columns n .. npad are zeros written by the same kernel).  A workgroup owns 64 training points
//                            (LDS tile, k-major) and HS_PT query points; a wave takes a point, a lane a training point; z / l is held
//                            once per (point, training point) in the lane's own LDS column, r^2 is a sum of squares in ascending k,
//                            fac and fac2 are evaluated once and feed all T rows.
//   2  bgp_launch_gemm4      P = R K^-1 on the LDS-DMA ring (fp64 MFMA): the hot product, 2 npad^2 m Tp flops per posterior.
//   3  hess_contract_kernel  one workgroup per (point, posterior): Q = P_s R_s^T (Tp x Tp, k-depth npad) on v_mfma_f64_16x16x4_f64,
//                            the lower-triangle 16 x 16 tiles only, tile t = ti (ti + 1) / 2 + tj on wave t mod 4; both operands
//                            arrive in 64-column LDS chunks in ascending order; Hbar = R_s alpha in the same pass on the VALU, a row
//                            per thread, ascending j.  Epilogue from the accumulators: P0 - Q, the diagonal clipped at 0, the lower
//                            triangle mirrored, the variances picked from the diagonal.
// No workgroup waits for another; no floating-point atomics; every loop is bounded by an argument.  A point's outputs depend on the
// posterior and that point alone (not on m, B, the other points, the outputs asked for or the chunking).  Matern 3/2 (fac2 ~ 1 / r)
// and Matern 1/2 have no mean-square second derivative: refused.
#include "bgp_common.h"
#include "bgp_device.h"
#include "bgp_gemm.h"

#define HS_DMAX 16           // input dimensions
#define HS_TMAX 144          // pad16(16 * 17 / 2)
#define HS_TJ 64             // training points per LDS tile / columns per chunk of the contraction
#define HS_PT 8              // query points per workgroup of the build (two per wave)
#define HS_LD 68             // LDS leading dimension of a 64-column chunk: lane (lr, lk) reads row lr, column 4 kk + lk, i.e. eight-byte
                             // word 68 lr + lk = 4 lr + lk mod 32: rows lr and lr + 8 share a bank (two-way over the 64 lanes, where
                             // 64 would be sixteen-way); 16-byte aligned rows.  The conflict rate was not measured.
#define HS_NTW 12            // tiles per wave: 45 lower tiles of a 9 x 9 tile grid over 4 waves, rounded up
#define HS_ROWMAX (1 << 22)  // m Tp per call

// fac as kb_stationary_fac has it (character for character) and fac2 = fac' / r in the form that needs no division: at r = 0 it is psi
template <int STAT>
static __device__ __forceinline__ void hess_facs(double r2, double& fac, double& fac2) {
#pragma clang fp contract(off)
  if (STAT == BGP_RBF) {
    const double S = kb_exp_neg(0.5 * r2);
    fac = -S;
    fac2 = S;
    return;
  }
  const double r = kb_sqrt_pos(r2);
  const double t = r * 2.23606797749979;  // math.sqrt(5)
  const double e = kb_exp_neg(t);
  fac = -(5.0 / 3.0) * ((1.0 + t) * e);
  fac2 = (25.0 / 3.0) * e;
}

// R[b][(s Tp + t) npad + j] for the points s of this chunk and every row below `rows` (the 128-row pad: points past mm are zeros);
// grid (npad / 64, ceil(ceil(rows / Tp) / HS_PT), posteriors)
template <int STAT, int FORM>
__global__ void __launch_bounds__(256) hess_build_kernel(const double* __restrict__ X, int n, int npad, int d, int T, int Tp,
                                                         const double* __restrict__ H, const double* __restrict__ Xq, int mm,
                                                         int rows, size_t sR, double* __restrict__ R) {
#pragma clang fp contract(off)
  __shared__ double Xt[HS_DMAX * HS_TJ];
  __shared__ double xq[HS_PT * HS_DMAX];
  __shared__ double il[HS_DMAX];
  __shared__ double wz[4 * HS_DMAX * HS_TJ];  // wave w, dimension k, lane: z_k / l_k of the wave's point (a lane reads its own column)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int j0 = blockIdx.x * HS_TJ, s0 = blockIdx.y * HS_PT, b = blockIdx.z;
  const double* h = H + (size_t)b * (d + 2);
  if (tid < d) il[tid] = 1.0 / exp(h[1 + tid]);
  for (int idx = tid; idx < HS_TJ * d; idx += 256) {
    const int jj = idx / d, k = idx - jj * d;
    Xt[k * HS_TJ + jj] = (j0 + jj < n) ? X[(size_t)(j0 + jj) * d + k] : 0.0;
  }
  for (int idx = tid; idx < HS_PT * d; idx += 256) {
    const int p = idx / d, k = idx - p * d;
    xq[p * HS_DMAX + k] = (s0 + p < mm) ? Xq[(size_t)(s0 + p) * d + k] : 0.0;
  }
  __syncthreads();
  const double cst = exp(h[0]);
  const int j = j0 + lane;  // (j < npad: the grid covers npad / 64 tiles)
  double* Rb = R + (size_t)b * sR;
  double* w = wz + wv * (HS_DMAX * HS_TJ) + lane;
  for (int p = wv; p < HS_PT; p += 4) {
    const int s = s0 + p;
    const long long row0 = (long long)s * Tp;
    if (row0 >= rows) break;
    const bool live = s < mm && j < n;
    double fac = 0.0, fac2 = 0.0;
    if (s < mm) {
      double r2 = 0.0;
      for (int k = 0; k < d; k++) {
        const double z = (xq[p * HS_DMAX + k] - Xt[k * HS_TJ + lane]) * il[k];
        r2 = fma(z, z, r2);
        w[k * HS_TJ] = z * il[k];
      }
      hess_facs<STAT>(r2, fac, fac2);
    }
    int t = 0;
    for (int k = 0; k < d; k++) {
      const double wk = live ? w[k * HS_TJ] : 0.0;
      for (int l = 0; l <= k; l++, t++) {
        if (row0 + t >= rows) continue;
        double v = 0.0;
        if (live) {
          v = (fac2 * wk) * w[l * HS_TJ];
          if (l == k) v = v + fac * (il[k] * il[k]);
          if (FORM == BGP_FORM_PRODUCT) v = cst * v;
        }
        Rb[(size_t)(row0 + t) * npad + j] = v;
      }
    }
    for (; t < Tp; t++)
      if (row0 + t < rows) Rb[(size_t)(row0 + t) * npad + j] = 0.0;
  }
}

// vech index t -> (k, l), k >= l (at most d steps)
static __device__ __forceinline__ void hess_unvech(int t, int& k, int& l) {
  k = 0;
  while ((k + 1) * (k + 2) / 2 <= t) k++;
  l = t - k * (k + 1) / 2;
}

// One workgroup per (point s, posterior b); dynamic LDS: the 64-column chunk of the point's Tp rows of R, then (P != nullptr) of P.
// hm / hv: [b][s][d][d], hc: [b][s][T][T] (each may be nullptr; hv and hc are not written without P).
__global__ void __launch_bounds__(256) hess_contract_kernel(const double* __restrict__ R, const double* __restrict__ P, size_t sR,
                                                            const double* __restrict__ alphaB, const double* __restrict__ H,
                                                            int product, double psi, int n, int npad, int d, int T, int Tp, int mm,
                                                            double* __restrict__ hm, double* __restrict__ hv,
                                                            double* __restrict__ hc) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) double hs_dyn[];
  __shared__ double al[HS_TJ];
  __shared__ double il[HS_DMAX];
  __shared__ int vk[HS_TMAX], vl[HS_TMAX];
  double* const Rs = hs_dyn;
  double* const Ps = hs_dyn + (size_t)Tp * HS_LD;
  const int tid = threadIdx.x, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int s = blockIdx.x, b = blockIdx.y;
  const double* Rb = R + (size_t)b * sR + (size_t)s * Tp * npad;
  const double* Pb = P ? P + (size_t)b * sR + (size_t)s * Tp * npad : nullptr;
  const double* ab = alphaB + (size_t)b * npad;
  if (tid < d) il[tid] = 1.0 / exp(H[(size_t)b * (d + 2) + 1 + tid]);
  if (tid < Tp) {
    int k = 0, l = 0;
    if (tid < T) hess_unvech(tid, k, l);
    vk[tid] = k, vl[tid] = l;
  }
  // the wave's tiles: t = wv, wv + 4, ... of the lower triangle of the (Tp / 16)^2 tile grid
  const int nt = Tp / 16, ntile = nt * (nt + 1) / 2;
  int ti[HS_NTW], tj[HS_NTW];
  d4 acc[HS_NTW];
#pragma unroll
  for (int i = 0; i < HS_NTW; i++) {
    const int t = wv + 4 * i;
    ti[i] = -1, tj[i] = 0;
    if (Pb && t < ntile) hess_unvech(t, ti[i], tj[i]);
    acc[i] = (d4){0.0, 0.0, 0.0, 0.0};
  }
  double hb = 0.0;
  for (int j0 = 0; j0 < n; j0 += HS_TJ) {  // (j0 + 64 <= npad; the columns n .. npad of R are zeros)
    __syncthreads();
    for (int idx = tid; idx < Tp * HS_TJ; idx += 256) {
      const int row = idx >> 6, jj = idx & 63;
      Rs[row * HS_LD + jj] = Rb[(size_t)row * npad + j0 + jj];
      if (Pb) Ps[row * HS_LD + jj] = Pb[(size_t)row * npad + j0 + jj];
    }
    if (tid < HS_TJ) al[tid] = (j0 + tid < n) ? ab[j0 + tid] : 0.0;
    __syncthreads();
    if (tid < T)
      for (int jj = 0; jj < HS_TJ; jj++) hb = fma(Rs[tid * HS_LD + jj], al[jj], hb);
#pragma unroll
    for (int i = 0; i < HS_NTW; i++) {
      if (ti[i] < 0) continue;
      const double* pa = Ps + (ti[i] * 16 + lr) * HS_LD + lk;
      const double* pb = Rs + (tj[i] * 16 + lr) * HS_LD + lk;
#pragma unroll
      for (int kk = 0; kk < HS_TJ / 4; kk++) acc[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kk * 4], pb[kk * 4], acc[i], 0, 0, 0);
    }
  }
  __syncthreads();  // (vk, vl, il at n = 0 steps; nothing else)
  const size_t o = (size_t)b * mm + s;
  if (hm && tid < T) {
    const int k = vk[tid], l = vl[tid];
    hm[(o * d + k) * d + l] = hb;
    hm[(o * d + l) * d + k] = hb;
  }
  if (!Pb) return;
  const double base = product ? exp(H[(size_t)b * (d + 2)]) * psi : psi;
#pragma unroll
  for (int i = 0; i < HS_NTW; i++) {
    if (ti[i] < 0) continue;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = GK_ROWB(ti[i] * 16, 0, lane, r), col = GK_COLB(tj[i] * 16, 0, lane);
      if (row >= T || col > row) continue;
      const int k = vk[row], l = vl[row], p = vk[col], q = vl[col];
      const int cnt = (int)(k == l && p == q) + (int)(k == p && l == q) + (int)(k == q && l == p);
      const double p0 = cnt ? ((((base * (double)cnt) * il[k]) * il[l]) * il[p]) * il[q] : 0.0;
      double v = p0 - acc[i][r];
      if (row == col) v = v > 0.0 ? v : 0.0;  // (clipped at 0 as the predictive variance is)
      if (hc) {
        hc[(o * T + row) * T + col] = v;
        hc[(o * T + col) * T + row] = v;
      }
      if (hv && row == col) {
        hv[(o * d + k) * d + l] = v;
        hv[(o * d + l) * d + k] = v;
      }
    }
  }
}

static inline int hess_tp(int d) { return (d * (d + 1) / 2 + 15) / 16 * 16; }

// Points per chunk: a function of n and d alone, so that a posterior's R stays within 2^25 doubles where one point allows it.
// BGP_HESS_CHUNK (tests): another size.
static size_t hess_point_chunk(int npad, int Tp) {
  size_t mc = ((size_t)1 << 25) / ((size_t)npad * Tp);
  if (const char* e = bgp_switch(BGP_SW_HESS_CHUNK)) {
    const long v = atol(e);
    if (v > 0) mc = (size_t)v;
  }
  return std::min<size_t>(std::max<size_t>(mc, 1), (size_t)1 << 16);  // (the build's grid: chunk / HS_PT <= 65535 in y)
}

static int hess_run(bgp_ctx* c, int B, const double* h_kernel, int m, const double* Xq, double* hmean, double* hvar, double* hcov) {
  const int n = c->n, d = c->d, npad = c->npad, dd = d * d, T = d * (d + 1) / 2, Tp = hess_tp(d), TT = T * T;
  const size_t p = d + 2;
  const bool wantP = hvar || hcov;
  const size_t mc = std::min(hess_point_chunk(npad, Tp), (size_t)m);
  const size_t rowsmax = (mc * Tp + 127) / 128 * 128, sR = rowsmax * npad;  // a posterior's R (and P) of one point chunk
  // posteriors per chunk: R and P of a chunk within 2^29 doubles together
  // (BGP_ITEM_CHUNK, tests: forced posterior chunks against the default)
  const int Bc = (int)bgp_switch_cap(BGP_SW_ITEM_CHUNK, std::max<size_t>(1, std::min<size_t>((size_t)B, ((size_t)1 << 28) / sR)));
  double *dXq, *dH, *dR, *dP = nullptr, *dM = nullptr, *dV = nullptr, *dC = nullptr;
  BgpScratch live(c);
  BGP_TRY(live.carve([&](BgpCarve& s) {
    dXq = s.take<double>(mc * d);
    dH = s.take<double>((size_t)B * p);
    dR = s.take<double>((size_t)Bc * sR);
    if (wantP) dP = s.take<double>((size_t)Bc * sR);
    if (hmean) dM = s.take<double>((size_t)Bc * mc * dd);
    if (hvar) dV = s.take<double>((size_t)Bc * mc * dd);
    if (hcov) dC = s.take<double>((size_t)Bc * mc * TT);
  }));
  hipStream_t st = c->stream;
  const double psi = c->ks.stationary == BGP_RBF ? 1.0 : 25.0 / 3.0;
  const int product = c->ks.form == BGP_FORM_PRODUCT;
  const size_t lds = (size_t)(wantP ? 2 : 1) * Tp * HS_LD * sizeof(double);
  if (lds > 64 * 1024)  // (more dynamic LDS than the default limit has to be asked for)
    BGP_HIP(hipFuncSetAttribute((const void*)hess_contract_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  BGP_HIP(bgp_memcpy_async(dH, h_kernel, (size_t)B * p * sizeof(double), hipMemcpyHostToDevice, st));
  c->chunk_last[0] = c->chunk_last[1] = 0;
  for (int b0 = 0; b0 < B; b0 += Bc) {
    const int nb = std::min(Bc, B - b0);
    const double* dHb = dH + (size_t)b0 * p;
    c->chunk_last[0]++;
    for (size_t m0 = 0; m0 < (size_t)m; m0 += mc) {
      const int mm = (int)std::min(mc, (size_t)m - m0);
      if (b0 == 0) c->chunk_last[1]++;
      const int rows = (mm * Tp + 127) / 128 * 128, pts = (rows + Tp - 1) / Tp;
      BGP_HIP(bgp_memcpy_async(dXq, Xq + m0 * d, (size_t)mm * d * sizeof(double), hipMemcpyHostToDevice, st));
      const dim3 grid(npad / HS_TJ, (pts + HS_PT - 1) / HS_PT, nb);
#define HS_BUILD(S, F)                                                                                                          \
  hipLaunchKernelGGL((hess_build_kernel<S, F>), grid, dim3(256), 0, st, c->dXeff, n, npad, d, T, Tp, dHb, dXq, mm, rows, sR, dR)
      if (c->ks.stationary == BGP_RBF) {
        if (product) HS_BUILD(BGP_RBF, BGP_FORM_PRODUCT);
        else HS_BUILD(BGP_RBF, BGP_FORM_SUM);
      } else {
        if (product) HS_BUILD(BGP_MATERN52, BGP_FORM_PRODUCT);
        else HS_BUILD(BGP_MATERN52, BGP_FORM_SUM);
      }
#undef HS_BUILD
      if (wantP)
        bgp_launch_gemm4(st, 0, dR, c->dKinv + (size_t)b0 * npad * npad, npad, rows, npad, npad, dP, npad, nb, sR,
                         (size_t)npad * npad, sR, nullptr);
      hipLaunchKernelGGL(hess_contract_kernel, dim3(mm, nb), dim3(256), lds, st, dR, dP, sR, c->dalpha_sol + (size_t)b0 * npad, dHb,
                         product, psi, n, npad, d, T, Tp, mm, dM, dV, dC);
      BGP_HIP(hipGetLastError());
      const size_t wd = (size_t)mm * dd * sizeof(double), wc = (size_t)mm * TT * sizeof(double);
      if (hmean)
        BGP_HIP(bgp_memcpy2d_async(hmean + ((size_t)b0 * m + m0) * dd, (size_t)m * dd * sizeof(double), dM, wd, wd, nb,
                                   hipMemcpyDeviceToHost, st));
      if (hvar)
        BGP_HIP(bgp_memcpy2d_async(hvar + ((size_t)b0 * m + m0) * dd, (size_t)m * dd * sizeof(double), dV, wd, wd, nb,
                                   hipMemcpyDeviceToHost, st));
      if (hcov)
        BGP_HIP(bgp_memcpy2d_async(hcov + ((size_t)b0 * m + m0) * TT, (size_t)m * TT * sizeof(double), dC, wc, wc, nb,
                                   hipMemcpyDeviceToHost, st));
      BGP_HIP(bgp_stream_sync(st));  // (the next chunk reuses the buffers)
    }
  }
  return BGP_OK;
}

extern "C" int bgp_hess_cov(bgp_ctx* c, int B, const double* h_kernel, int m, const double* Xq, double* hmean, double* hvar,
                            double* hcov) {
  BGP_TRY(bgp_guard(c, "bgp_hess_cov", BGP_POST_PLAIN));
  if (!h_kernel || !Xq || (!hmean && !hvar && !hcov) || m <= 0 || B <= 0 || B > 65535) {
    bgp_set_error("bgp_hess_cov: bad argument (1 <= B <= 65535, 1 <= m, at least one output)");
    return BGP_ERR_INVALID;
  }
  if (c->d > HS_DMAX || c->has_warp) {
    bgp_set_error("bgp_hess_cov: %s", c->has_warp ? "warped inputs are not supported" : "d > 16 is not supported");
    return BGP_ERR_INVALID;
  }
  if (c->ks.stationary != BGP_RBF && c->ks.stationary != BGP_MATERN52) {
    bgp_set_error("bgp_hess_cov: the Matern %s kernel is not twice differentiable (no Hessian covariance exists)",
                  c->ks.stationary == BGP_MATERN12 ? "1/2" : "3/2");
    return BGP_ERR_INVALID;
  }
  if ((double)m * (double)hess_tp(c->d) > (double)HS_ROWMAX) {
    bgp_set_error("bgp_hess_cov: m Tp = %.0f exceeds %d", (double)m * (double)hess_tp(c->d), HS_ROWMAX);
    return BGP_ERR_INVALID;
  }
  BGP_TRY(bgp_guard(c, "bgp_hess_cov", BGP_POST_PLAIN, B));
  return post_call(c, [&] { return hess_run(c, B, h_kernel, m, Xq, hmean, hvar, hcov); });
}
