// Joint entropy search acquisition on the resident posteriors.
//
// For resident posterior b, its OWN optimum samples (a_r, f_r), r < R, a candidate x, nu_b > 0 the variance of an observation (as
// bgp_knowledge_gradient takes noise) and tau >= 0 a jitter on the noiseless optimum observation, in normalised-y units:
//   mu, v      latent mean / variance of x                  mu_r, v_r   latent mean / variance of a_r
//   c_r = cov_b(a_r, x) = k_b(a_r, x) - k_b(a_r, X) K_b^-1 k_b(X, x)                       w_r = v_r + tau
//   m_r = mu + c_r (f_r - mu_r) / w_r      v_s = max(v - c_r^2 / w_r, 0)                   (conditioning on f(a_r) = f_r)
//   z_r = (f_r - m_r) / sqrt(v_s)          v_t = clip(v_s F(z_r), 0, v_s)                  (f(x) >= f_r: lower truncation)
//   F(z) = 1 - lam (lam - z),  lam = phi(z) / Phi(-z)                                      (variance factor of the truncated normal)
//   g_r = max(1/2 [log(v + nu_b) - log(v_t + nu_b)], 0)            gain_b(x) = (1 / R) sum_r g_r
// w_r <= 0: the sample conditions nothing (m_r = mu, v_s = v); v_s <= 0: v_t = 0.
// Stages, plain launches on the context's stream (1 and 2 are those of bgp_kg.hip with a point set per posterior):
//   1  optimum rows, once per chunk of posteriors: R_b = k_b(A_b, X) with the partials of mu_r = R_b alpha_b (kbuild_cross_kernel, per-item
//      queries), P_b = R_b K_b^-1 on the LDS-DMA ring (bgp_launch_gemm4 mode 0), v_r by predict's variance launches on the rows of R_b.
//   2  per chunk of candidates: K_*, mean and variance by the launches of bgp_predict_batch (the same bits);
//      C = k_b(chunk, A_b) - K_* P_b^T (cross build with per-item columns, then mode 2 of gemm4_kernel).  C[x][r] = cov_b(a_r, x).
//   3  jes_gain_kernel: one wave per (posterior, candidate), four candidates of one posterior per workgroup; per optimum sample the
//      workgroup keeps 1 / w_r, (f_r - mu_r) / w_r and f_r in LDS (the two divisions by w_r are formed once per workgroup, not per
//      candidate: m_r = mu + c_r [(f_r - mu_r) / w_r], v_s = v - c_r c_r [1 / w_r]).  A lane owns r = lane + 64 t, adds its terms in
//      ascending t; the 64 lanes are added by a fixed xor butterfly (32, 16, .. 1); one division by R.
//   4  the average over the posteriors: acq_sum_kernel of bgp_acq_batch.
// F: below JES_F_SWITCH the definition with erfcx, lam = sqrt(2 / pi) / erfcx(z / sqrt 2); from it on the Laplace continued fraction
// of the Mills ratio, lam = z + T, T = 1 / (z + U), U = 2 / (z + 3 / (z + 4 / ...)) cut at JES_F_DEPTH, F = T (U - T): no cancellation.
// U is evaluated bottom-up as a ratio N / D scaled by 1 / z (N_k = k D_{k+1} / z, D_k = D_{k+1} + N_{k+1} / z): one division, not 40.
// No workgroup waits for another; no floating-point atomics (one integer flag per posterior); every loop is bounded by an argument.
#include "bgp_common.h"
#include "bgp_device.h"

#define JES_DMAX 32       // input dimensions
#define JES_RMAX 255      // optimum samples per posterior
#define JES_SLOTS 256     // sample slots of a workgroup (4 per lane)
#define JES_SPL 4         // slots per lane
#define JES_F_SWITCH 4.0  // z from which F is the continued fraction
#define JES_F_DEPTH 40    // its last partial numerator

// bgp_post.hip: the pieces of bgp_predict_batch and the average of bgp_acq_batch
__global__ void rowdot_reduce_kernel(const double* __restrict__ part, int tn, int M, double* __restrict__ out);
__global__ void finish_var_kernel(const double* __restrict__ q, size_t sq, const double* __restrict__ H, int d, int form, int m,
                                  double* __restrict__ var, size_t so);
__global__ void acq_sum_kernel(const double* __restrict__ T, const int* __restrict__ bad, size_t sm, int m, int B, int n_samples,
                               double* __restrict__ acc);
void bgp_launch_gemm4(hipStream_t st, int mode, const double* A, const double* Bm, int ldx, int M, int N, int K, double* C,
                      int ldc, int nb, size_t sA, size_t sB, size_t sC, const int* pidxB);
void bgp_launch_rowquad(hipStream_t st, const double* A, int lda, size_t sA, const double* S, int lds_, size_t sS,
                        const int* pidx, int M, int n, int nb, double* part);
int bgp_rowquad_tile();

// the variance factor of a normal truncated below at z (a function of z alone)
static __device__ __forceinline__ double jes_F(double z) {
#pragma clang fp contract(off)
  if (z < JES_F_SWITCH) {
    const double lam = 0.79788456080286535588 / erfcx(z * 0.70710678118654752440);
    return 1.0 - lam * (lam - z);
  }
  const double rz = 1.0 / z;
  double N = 0.0, D = 1.0;
  for (int k = JES_F_DEPTH; k >= 2; k--) {
    const double Nk = ((double)k * rz) * D;
    D = D + rz * N;
    N = Nk;
  }
  const double U = N / D;
  const double T = 1.0 / (z + U);
  return T * (U - T);
}

// One wave per (candidate i of this chunk, posterior b); grid (ceil(mm / 4), posteriors).
//   muA, vA [b][r]   latent mean / variance at the optimum points (stride sA)      fopt[b][r]  optimum values (stride R)
//   Cv[b][i][r]      cov_b(a_r, x_i) (row stride Mp, item stride sC)               mean, var   [b][i] of the chunk (stride sm)
//   gain[b][i]       out (stride sg; the caller offsets it by the chunk)
__global__ void __launch_bounds__(256) jes_gain_kernel(const double* __restrict__ muA, const double* __restrict__ vA, size_t sA,
                                                       const double* __restrict__ fopt, const double* __restrict__ Cv, size_t sC,
                                                       int Mp, const double* __restrict__ mean, const double* __restrict__ var,
                                                       size_t sm, const double* __restrict__ noise, double tau, int R, int mm,
                                                       double* __restrict__ gain, size_t sg, int* __restrict__ bad) {
#pragma clang fp contract(off)
  __shared__ double srw[JES_SLOTS], sdl[JES_SLOTS], sf[JES_SLOTS];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wv, b = blockIdx.y;
  {
    const int r = threadIdx.x;  // (256 threads, R <= 255 slots)
    if (r < R) {
      const double f = fopt[(size_t)b * R + r];
      const double w = vA[(size_t)b * sA + r] + tau;
      const bool on = w > 0.0;  // (w <= 0, or not a number: the sample conditions nothing)
      srw[r] = on ? 1.0 / w : 0.0;
      sdl[r] = on ? (f - muA[(size_t)b * sA + r]) / w : 0.0;
      sf[r] = f;
    }
  }
  __syncthreads();
  if (i >= mm) return;  // (wave-uniform)
  const double mu = mean[(size_t)b * sm + i], v = var[(size_t)b * sm + i], nu = noise[b];
  const double lv = log(v + nu);
  const double* crow = Cv + (size_t)b * sC + (size_t)i * Mp;
  const int nt = (R + 63) >> 6;  // slots per lane in use (wave-uniform)
  double sum = 0.0;
#pragma unroll
  for (int t = 0; t < JES_SPL; t++) {
    if (t >= nt) break;
    const int r = lane + 64 * t;
    if (r < R) {
      const double c = crow[r];
      const double mr = mu + c * sdl[r];
      double vs = v - (c * c) * srw[r];
      vs = (vs < 0.0) ? 0.0 : vs;
      double vt = 0.0;
      if (vs > 0.0) {
        const double z = (sf[r] - mr) / sqrt(vs);
        vt = vs * jes_F(z);
        vt = (vt < 0.0) ? 0.0 : ((vt > vs) ? vs : vt);
      }
      double g = 0.5 * (lv - log(vt + nu));
      g = (g > 0.0) ? g : ((g == g) ? 0.0 : g);
      sum += g;
    }
  }
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) sum += __shfl_xor(sum, w, 64);
  const double out = sum / (double)R;
  if (lane == 0) {
    gain[(size_t)b * sg + i] = out;
    if (!isfinite(out)) atomicOr(&bad[b], 1);
  }
}

static inline int jes_pad(int v, int q) { return (v + q - 1) / q * q; }

// Candidates per chunk: a multiple of 128 that depends on n alone, so that a posterior's K_* stays within 2^24 doubles.
// BGP_JES_CHUNK (tests): another size, rounded up to 128.
static size_t jes_cand_chunk(int npad) {
  size_t mc = (((size_t)1 << 24) / (size_t)npad) / 128 * 128;
  if (const char* e = bgp_switch(BGP_SW_JES_CHUNK)) {
    const long v = atol(e);
    if (v > 0) mc = ((size_t)v + 127) / 128 * 128;
  }
  return std::min<size_t>(std::max<size_t>(mc, 128), (size_t)1 << 18);
}

static int jes_run(bgp_ctx* c, int B, const double* h_kernel, const double* noise, int m, const double* Xcand, int R,
                   const double* Xopt, const double* fopt, double tau, int n_samples, double* gain, double* avg) {
  const int n = c->n, d = c->d, npad = c->npad;
  const size_t p = d + 2;
  const int Mp = std::max(jes_pad(R, 128), 128), M64 = jes_pad(R, 64);  // rows of R_b / columns of C as stored, and as multiplied
  const int mtot = jes_pad(m, 128);
  const int mc = (int)std::min<size_t>(jes_cand_chunk(npad), (size_t)mtot);
  const int tq = npad / bgp_rowquad_tile();
  const size_t sKs = (size_t)mc * npad, sC = (size_t)mc * Mp, sR = (size_t)Mp * npad, sAx = (size_t)R * d;
  // posteriors per chunk: K_*, C, R_b and P_b of a chunk within 2^29 doubles together
  const int Bc = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, ((size_t)1 << 29) / (sKs + sC + 2 * sR)));
  double *dXc, *dA, *dF, *dH, *dnoise, *dR, *dP, *dmuA, *dvA, *dpartA, *dKs, *dmpart, *dmean, *dvar, *dCv, *dG, *davg;
  int* dbad;
  BgpScratch live(c);
  BGP_TRY(live.carve([&](BgpCarve& s) {
    dXc = s.take<double>((size_t)m * d);
    dA = s.take<double>((size_t)B * sAx);
    dF = s.take<double>((size_t)B * R);
    dH = s.take<double>((size_t)B * p);
    dnoise = s.take<double>(B);
    dR = s.take<double>((size_t)Bc * sR);
    dP = s.take<double>((size_t)Bc * sR);
    dmuA = s.take<double>((size_t)Bc * Mp);
    dvA = s.take<double>((size_t)Bc * Mp);
    dpartA = s.take<double>((size_t)Bc * (npad / 128) * Mp);
    dKs = s.take<double>((size_t)Bc * sKs);
    dmpart = s.take<double>((size_t)Bc * (npad / 128) * mc);
    dmean = s.take<double>((size_t)Bc * mc);
    dvar = s.take<double>((size_t)Bc * mc);
    dCv = s.take<double>((size_t)Bc * sC);
    dG = s.take<double>((size_t)B * mtot);
    davg = s.take<double>(mtot);
    dbad = s.take<int>(B);
  }));
  BGP_TRY(c->drowpart.ensure((size_t)Bc * tq * std::max(mc, Mp)));
  hipStream_t st = c->stream;
  BGP_HIP(bgp_memcpy_async(dXc, Xcand, (size_t)m * d * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(dA, Xopt, (size_t)B * sAx * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(dF, fopt, (size_t)B * R * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(dH, h_kernel, (size_t)B * p * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(dnoise, noise, (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(hipMemsetAsync(dbad, 0, (size_t)B * sizeof(int), st));
  for (int b0 = 0; b0 < B; b0 += Bc) {
    const int nb = std::min(Bc, B - b0);
    const double* dHb = dH + (size_t)b0 * p;
    const double* dAb = dA + (size_t)b0 * sAx;
    const double* Kinv = c->dKinv + (size_t)b0 * npad * npad;
    const double* al = c->dalpha_sol + (size_t)b0 * npad;
    // R_b = k_b(A_b, X) with the column-tile partials of R_b alpha_b, P_b = R_b K_b^-1 (K^-1 symmetric: an NT product), and the
    // variance at the optimum points by predict's launches on the rows of R_b (rows past R are zero)
    BGP_TRY(bgp_launch_kcross_matvec_x(c, nb, dHb, R, dAb, sAx, n, c->dXeff, 0, dR, npad, sR, al, (size_t)npad, dpartA));
    hipLaunchKernelGGL(rowdot_reduce_kernel, dim3((Mp + 255) / 256, nb), dim3(256), 0, st, dpartA, npad / 128, Mp, dmuA);
    bgp_launch_gemm4(st, 0, dR, Kinv, npad, M64, npad, npad, dP, npad, nb, sR, (size_t)npad * npad, sR, nullptr);
    bgp_launch_rowquad(st, dR, npad, sR, Kinv, npad, (size_t)npad * npad, nullptr, Mp, npad, nb, c->drowpart);
    hipLaunchKernelGGL(rowdot_reduce_kernel, dim3((Mp + 255) / 256, nb), dim3(256), 0, st, c->drowpart, tq, Mp, dvA);
    hipLaunchKernelGGL(finish_var_kernel, dim3((R + 255) / 256, nb), dim3(256), 0, st, dvA, (size_t)Mp, dHb, d, c->ks.form, R, dvA,
                       (size_t)Mp);
    BGP_HIP(hipGetLastError());
    for (int m0 = 0; m0 < m; m0 += mc) {
      const int mm = std::min(mc, m - m0), mmp = jes_pad(mm, 128);
      const double* dXq = dXc + (size_t)m0 * d;
      // mean and variance of the chunk: the launches of bgp_predict_batch (strides of this chunk: mmp)
      BGP_TRY(bgp_launch_kcross_matvec(c, nb, dHb, mm, dXq, n, c->dXeff, dKs, npad, sKs, al, (size_t)npad, dmpart));
      hipLaunchKernelGGL(rowdot_reduce_kernel, dim3((mmp + 255) / 256, nb), dim3(256), 0, st, dmpart, npad / 128, mmp, dmean);
      bgp_launch_rowquad(st, dKs, npad, sKs, Kinv, npad, (size_t)npad * npad, nullptr, mmp, npad, nb, c->drowpart);
      hipLaunchKernelGGL(rowdot_reduce_kernel, dim3((mmp + 255) / 256, nb), dim3(256), 0, st, c->drowpart, tq, mmp, dvar);
      hipLaunchKernelGGL(finish_var_kernel, dim3((mm + 255) / 256, nb), dim3(256), 0, st, dvar, (size_t)mmp, dHb, d, c->ks.form, mm,
                         dvar, (size_t)mmp);
      BGP_HIP(hipGetLastError());
      // C = k_b(chunk, A_b) - K_* P_b^T: the hot product, on the columns 0 .. pad64(R) only
      BGP_TRY(bgp_launch_kcross_matvec_x(c, nb, dHb, mm, dXq, 0, R, dAb, sAx, dCv, Mp, sC, nullptr, 0, nullptr));
      bgp_launch_gemm4(st, 2, dKs, dP, npad, jes_pad(mm, 64), M64, npad, dCv, Mp, nb, sKs, sR, sC, nullptr);
      hipLaunchKernelGGL(jes_gain_kernel, dim3((mm + 3) / 4, nb), dim3(256), 0, st, dmuA, dvA, (size_t)Mp, dF + (size_t)b0 * R, dCv, sC,
                         Mp, dmean, dvar, (size_t)mmp, dnoise + b0, tau, R, mm, dG + (size_t)b0 * mtot + m0, (size_t)mtot, dbad + b0);
      BGP_HIP(hipGetLastError());
    }
  }
  if (avg) {
    hipLaunchKernelGGL(acq_sum_kernel, dim3((m + 255) / 256, 1), dim3(256), 0, st, dG, dbad, (size_t)mtot, m, B, n_samples, davg);
    BGP_HIP(hipGetLastError());
    BGP_HIP(bgp_memcpy_async(avg, davg, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  if (gain)
    BGP_HIP(bgp_memcpy2d_async(gain, (size_t)m * sizeof(double), dG, (size_t)mtot * sizeof(double), (size_t)m * sizeof(double), B,
                               hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_stream_sync(st));
  return BGP_OK;
}

extern "C" int bgp_joint_entropy(bgp_ctx* c, int B, const double* h_kernel, const double* noise, int m, const double* Xcand, int R,
                                 const double* Xopt, const double* fopt, double tau, int n_samples, double* gain, double* avg) {
  BGP_TRY(bgp_guard(c, "bgp_joint_entropy", BGP_POST_PLAIN));
  if (!h_kernel || !noise || !Xcand || !Xopt || !fopt || (!gain && !avg) || m < 1 || m > (1 << 24) || B <= 0 || B > 65535 || R < 1 ||
      n_samples <= 0) {
    bgp_set_error("bgp_joint_entropy: bad argument (1 <= B <= 65535, 1 <= m <= 2^24, 1 <= R, 1 <= n_samples, at least one output)");
    return BGP_ERR_INVALID;
  }
  if (R > JES_RMAX) {
    bgp_set_error("bgp_joint_entropy: R = %d optimum samples exceed %d", R, JES_RMAX);
    return BGP_ERR_INVALID;
  }
  if (c->d > JES_DMAX || c->has_warp) {
    bgp_set_error("bgp_joint_entropy: %s", c->has_warp ? "warped inputs are not supported" : "d > 32 is not supported");
    return BGP_ERR_INVALID;
  }
  if (!(tau >= 0.0) || !std::isfinite(tau)) {
    bgp_set_error("bgp_joint_entropy: tau must be finite and >= 0");
    return BGP_ERR_INVALID;
  }
  for (int b = 0; b < B; b++)
    if (!(noise[b] > 0.0) || !std::isfinite(noise[b])) {
      bgp_set_error("bgp_joint_entropy: noise[%d] must be finite and > 0", b);
      return BGP_ERR_INVALID;
    }
  for (size_t k = 0; k < (size_t)B * R; k++)
    if (!std::isfinite(fopt[k])) {
      bgp_set_error("bgp_joint_entropy: fopt[%zu] is not finite", k);
      return BGP_ERR_INVALID;
    }
  BGP_TRY(bgp_guard(c, "bgp_joint_entropy", BGP_POST_PLAIN, B));
  return post_call(c, [&] { return jes_run(c, B, h_kernel, noise, m, Xcand, R, Xopt, fopt, tau, n_samples, gain, avg); });
}
