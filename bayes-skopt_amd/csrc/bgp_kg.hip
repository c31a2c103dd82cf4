// Knowledge-gradient acquisition on the resident posteriors.
//
// For resident posterior b, reference points A = (a_0 .. a_{M-1}), a candidate x and s = var_b(x) + noise_b (var_b latent, noise_b the
// variance of a fantasy observation as bgp_fantasy_begin takes it) the M + 1 lines in Z ~ N(0, 1) are
//   p_j = mu_b(a_j)   q_j = cov_b(a_j, x) / sqrt(s)   (j < M)        p_M = mu_b(x)   q_M = var_b(x) / sqrt(s)
//   cov_b(a, x) = k_b(a, x) - k_b(a, X) K_b^-1 k_b(X, x)             (latent: no white term)
//   KG_b(x) = min_j p_j - E[min_j (p_j + q_j Z)] >= 0, exactly 0 where s <= 0
// Stages, plain launches on the context's stream:
//   1  reference rows, once per chunk of posteriors: R = k_b(A, X) and mu_b(A) = R alpha_b by the cross build (kbuild_cross_kernel,
//      rows zero padded to 128), P = R K_b^-1 on the LDS-DMA ring (bgp_launch_gemm4).
//   2  per chunk of candidates: K_* = k_b(chunk, X), mean and variance as bgp_predict_batch computes them (the same launches, the same
//      bits); k_b(chunk, A) by the cross build into C, then C -= K_* P^T on the ring (mode 2 of gemm4_kernel): the hot product,
//      2 n m pad64(M) flops per posterior.  C[x][j] = cov_b(a_j, x).
//   3  kg_envelope_kernel: one wave per (posterior, candidate).  The lower envelope by pairwise interval clipping, sort-free: line j
//      is the minimum on [lo_j, hi_j] = the intersection over i of {z : (q_j - q_i) z <= p_i - p_j}; a bound is kept as a fraction
//      (numerator, positive denominator; denominator 0 = infinite) and two bounds are compared by cross-multiplication, so the M^2 loop
//      holds no division.  A line that owns an interval contributes (p_j - p*) (Phi(hi) - Phi(lo)) + q_j (phi(lo) - phi(hi)), p* = min p.
//      Divisions per candidate: 1 (1 / sqrt(s)) + 2 (M + 1) (the two bounds of every line).
//   4  the average over the posteriors: bgp_acq_batch's kernel (acq_sum_kernel: ascending posterior, value / n_samples, a posterior
//      with a non-finite value contributes nothing).
// No workgroup waits for another; no floating-point atomics (one integer flag per posterior: "a value is not finite"); every loop is
// bounded by an argument.  A candidate's value depends on the posterior, the ordered reference list and that candidate alone: a lane
// adds its lines in ascending j = lane + 64 t, the 64 lanes are added by a fixed butterfly.
#include "bgp_common.h"
#include "bgp_device.h"

#define KG_DMAX 32    // input dimensions
#define KG_MMAX 255   // reference points
#define KG_LMAX 256   // lines of a candidate (KG_MMAX + 1)
#define KG_LPL 4      // lines per lane (KG_LMAX / 64)

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

static __device__ __forceinline__ double kg_wave_min(double v) {
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) v = fmin(v, __shfl_xor(v, w, 64));
  return v;
}

// One wave per (candidate i of this chunk, posterior b); grid (ceil(mm / 4), posteriors).
//   muA[b][j]   mean at the reference points (stride sMu)          Cv[b][i][j]  cov_b(a_j, x_i) (row stride Mp, item stride sC)
//   mean, var   [b][i] of the chunk (stride sm)                    kg[b][i]     out (stride sk; the caller offsets it by the chunk)
__global__ void __launch_bounds__(256) kg_envelope_kernel(const double* __restrict__ muA, size_t sMu, const double* __restrict__ Cv,
                                                          size_t sC, int Mp, const double* __restrict__ mean,
                                                          const double* __restrict__ var, size_t sm,
                                                          const double* __restrict__ noise, int M, int mm, double y_std,
                                                          double* __restrict__ kg, size_t sk, int* __restrict__ bad) {
#pragma clang fp contract(off)
  __shared__ double sp[4][KG_LMAX], sq[4][KG_LMAX];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wv, b = blockIdx.y;
  const bool live = i < mm;  // (wave-uniform, as everything below that branches on it)
  const int L = M + 1;
  double pj[KG_LPL], qj[KG_LPL];
  double s = 0.0;
  int finite = 1;
  if (live) {
    const double v = var[(size_t)b * sm + i];
    s = v + noise[b];
    const double rs = (s > 0.0) ? 1.0 / sqrt(s) : 0.0;
#pragma unroll
    for (int t = 0; t < KG_LPL; t++) {
      const int j = lane + 64 * t;
      pj[t] = 0.0, qj[t] = 0.0;
      if (j < L) {
        pj[t] = (j < M) ? muA[(size_t)b * sMu + j] : mean[(size_t)b * sm + i];
        qj[t] = ((j < M) ? Cv[(size_t)b * sC + (size_t)i * Mp + j] : v) * rs;
        sp[wv][j] = pj[t], sq[wv][j] = qj[t];
        if (!isfinite(pj[t]) || !isfinite(qj[t])) finite = 0;
      }
    }
  }
  __syncthreads();
  if (!live) return;
  double out;
  if (!(s > 0.0)) {
    out = 0.0;  // (the rule of the expected improvement at std <= 0)
  } else if (!__all(finite)) {
    out = NAN;
  } else {
    double pmin = INFINITY;
#pragma unroll
    for (int t = 0; t < KG_LPL; t++)
      if (lane + 64 * t < L) pmin = fmin(pmin, pj[t]);
    pmin = kg_wave_min(pmin);
    // the interval of every line of this lane: lo = ln / ld, hi = hn / hd (ld, hd >= 0; 0: infinite)
    double ln[KG_LPL], ld[KG_LPL], hn[KG_LPL], hd[KG_LPL];
    int dead[KG_LPL];
#pragma unroll
    for (int t = 0; t < KG_LPL; t++) ln[t] = -1.0, ld[t] = 0.0, hn[t] = 1.0, hd[t] = 0.0, dead[t] = (lane + 64 * t >= L);
    const int nt = (L + 63) >> 6;  // line slots per lane in use (wave-uniform: the slots past it hold no line and add an exact 0)
    for (int k = 0; k < L; k++) {
      const double pk = sp[wv][k], qk = sq[wv][k];  // (one address for the wave: a broadcast)
#pragma unroll
      for (int t = 0; t < KG_LPL; t++) {
        if (t >= nt) break;
        const int j = lane + 64 * t;
        const double dq = qj[t] - qk, dp = pk - pj[t];  // line j is not above line k where dq z <= dp
        if (dq > 0.0) {
          if (dp * hd[t] < hn[t] * dq) hn[t] = dp, hd[t] = dq;
        } else if (dq < 0.0) {
          if ((0.0 - dp) * ld[t] > ln[t] * (0.0 - dq)) ln[t] = 0.0 - dp, ld[t] = 0.0 - dq;
        } else if (k != j && (pk < pj[t] || (pk == pj[t] && k < j))) {
          dead[t] = 1;  // equal slopes: the lower intercept wins; exact duplicates: the lower index
        }
      }
    }
    double sum = 0.0;
#pragma unroll
    for (int t = 0; t < KG_LPL; t++) {
      if (t >= nt) break;
      const bool owns = !dead[t] && (ld[t] == 0.0 || hd[t] == 0.0 || ln[t] * hd[t] < hn[t] * ld[t]);
      // (both quotients are formed by every lane: 2 divisions per line, none in the loop above)
      const double lo = (ld[t] == 0.0) ? -INFINITY : ln[t] / ld[t];
      const double hi = (hd[t] == 0.0) ? INFINITY : hn[t] / hd[t];
      // Phi(hi) - Phi(lo), taken in the lower tail when the interval lies in the upper one (no 1 - 1e-17 differences)
      const double r2 = 0.70710678118654752440;
      const double dPhi = (lo >= 0.0) ? 0.5 * (erfc(lo * r2) - erfc(hi * r2)) : 0.5 * (erfc((0.0 - hi) * r2) - erfc((0.0 - lo) * r2));
      const double dphi = (exp(-(lo * lo) / 2.0) - exp(-(hi * hi) / 2.0)) / 2.5066282746310002;  // phi(lo) - phi(hi) = int z phi
      const double term = (pj[t] - pmin) * dPhi + qj[t] * dphi;
      sum += owns ? term : 0.0;
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) sum += __shfl_xor(sum, w, 64);
    out = 0.0 - sum;  // min p - E[min] = -(E[min] - p*)
    out = (out > 0.0) ? out : ((out == out) ? 0.0 : out);
    out = out * y_std;
  }
  if (lane == 0) {
    kg[(size_t)b * sk + i] = out;
    if (!isfinite(out)) atomicOr(&bad[b], 1);
  }
}

static inline int kg_pad(int v, int q) { return (v + q - 1) / q * q; }

// Candidates per chunk: a multiple of 128 that depends on n alone, so that a posterior's K_* stays within 2^24 doubles.  BGP_KG_CHUNK
// (tests): another size, rounded up to 128.
static size_t kg_cand_chunk(int npad) {
  size_t mc = (((size_t)1 << 24) / (size_t)npad) / 128 * 128;
  if (const char* e = bgp_switch(BGP_SW_KG_CHUNK)) {
    const long v = atol(e);
    if (v > 0) mc = ((size_t)v + 127) / 128 * 128;
  }
  return std::min<size_t>(std::max<size_t>(mc, 128), (size_t)1 << 18);
}

static int kg_run(bgp_ctx* c, int B, const double* h_kernel, const double* noise, int m, const double* Xcand, int M,
                  const double* Xref, double y_std, int n_samples, double* kg, double* avg) {
  const int n = c->n, d = c->d, npad = c->npad;
  const size_t p = d + 2;
  const int Mp = std::max(kg_pad(M, 128), 128), M64 = kg_pad(M, 64);  // rows of R / columns of C as stored, and as multiplied
  const int mtot = kg_pad(m, 128);
  const int mc = (int)std::min<size_t>(kg_cand_chunk(npad), (size_t)mtot);
  const int tq = npad / bgp_rowquad_tile();
  const size_t sKs = (size_t)mc * npad, sC = (size_t)mc * Mp, sR = (size_t)Mp * npad;
  // posteriors per chunk: K_*, C, R and P of a chunk within 2^29 doubles together
  const int Bc = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, ((size_t)1 << 29) / (sKs + sC + 2 * sR)));
  double *dXc, *dA, *dH, *dnoise, *dR, *dP, *dmuA, *dpartA, *dKs, *dmpart, *dmean, *dvar, *dCv, *dKG, *davg;
  int* dbad;
  BgpScratch live(c);
  BGP_TRY(live.carve([&](BgpCarve& s) {
    dXc = s.take<double>((size_t)m * d);
    dA = s.take<double>((size_t)std::max(M, 1) * d);
    dH = s.take<double>((size_t)B * p);
    dnoise = s.take<double>(B);
    dR = s.take<double>((size_t)Bc * sR);
    dP = s.take<double>((size_t)Bc * sR);
    dmuA = s.take<double>((size_t)Bc * Mp);
    dpartA = s.take<double>((size_t)Bc * (npad / 128) * Mp);
    dKs = s.take<double>((size_t)Bc * sKs);
    dmpart = s.take<double>((size_t)Bc * (npad / 128) * mc);
    dmean = s.take<double>((size_t)Bc * mc);
    dvar = s.take<double>((size_t)Bc * mc);
    dCv = s.take<double>((size_t)Bc * sC);
    dKG = s.take<double>((size_t)B * mtot);
    davg = s.take<double>(mtot);
    dbad = s.take<int>(B);
  }));
  BGP_TRY(c->drowpart.ensure((size_t)Bc * tq * mc));
  hipStream_t st = c->stream;
  BGP_HIP(bgp_memcpy_async(dXc, Xcand, (size_t)m * d * sizeof(double), hipMemcpyHostToDevice, st));
  if (M > 0) BGP_HIP(bgp_memcpy_async(dA, Xref, (size_t)M * d * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(dH, h_kernel, (size_t)B * p * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(dnoise, noise, (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(hipMemsetAsync(dbad, 0, (size_t)B * sizeof(int), st));
  for (int b0 = 0; b0 < B; b0 += Bc) {
    const int nb = std::min(Bc, B - b0);
    const double* dHb = dH + (size_t)b0 * p;
    const double* Kinv = c->dKinv + (size_t)b0 * npad * npad;
    const double* al = c->dalpha_sol + (size_t)b0 * npad;
    if (M > 0) {
      // R = k_b(A, X) with the column-tile partials of R alpha_b, then P = R K_b^-1 (K^-1 symmetric: an NT product)
      BGP_TRY(bgp_launch_kcross_matvec(c, nb, dHb, M, dA, n, c->dXeff, dR, npad, sR, al, (size_t)npad, dpartA));
      hipLaunchKernelGGL(rowdot_reduce_kernel, dim3((Mp + 255) / 256, nb), dim3(256), 0, st, dpartA, npad / 128, Mp, dmuA);
      bgp_launch_gemm4(st, 0, dR, Kinv, npad, M64, npad, npad, dP, npad, nb, sR, (size_t)npad * npad, sR, nullptr);
      BGP_HIP(hipGetLastError());
    }
    for (int m0 = 0; m0 < m; m0 += mc) {
      const int mm = std::min(mc, m - m0), mmp = kg_pad(mm, 128);
      const double* dXq = dXc + (size_t)m0 * d;
      // mean and variance of the chunk: the launches of bgp_predict_batch (strides of this chunk: mmp)
      BGP_TRY(bgp_launch_kcross_matvec(c, nb, dHb, mm, dXq, n, c->dXeff, dKs, npad, sKs, al, (size_t)npad, dmpart));
      hipLaunchKernelGGL(rowdot_reduce_kernel, dim3((mmp + 255) / 256, nb), dim3(256), 0, st, dmpart, npad / 128, mmp, dmean);
      bgp_launch_rowquad(st, dKs, npad, sKs, Kinv, npad, (size_t)npad * npad, nullptr, mmp, npad, nb, c->drowpart);
      hipLaunchKernelGGL(rowdot_reduce_kernel, dim3((mmp + 255) / 256, nb), dim3(256), 0, st, c->drowpart, tq, mmp, dvar);
      hipLaunchKernelGGL(finish_var_kernel, dim3((mm + 255) / 256, nb), dim3(256), 0, st, dvar, (size_t)mmp, dHb, d, c->ks.form, mm,
                         dvar, (size_t)mmp);
      BGP_HIP(hipGetLastError());
      if (M > 0) {
        // C = k_b(chunk, A) - K_* P^T: the hot product, on the columns 0 .. pad64(M) only
        BGP_TRY(bgp_launch_kcross_batch(c, nb, dHb, mm, dXq, M, dA, dCv, Mp, sC));
        bgp_launch_gemm4(st, 2, dKs, dP, npad, kg_pad(mm, 64), M64, npad, dCv, Mp, nb, sKs, sR, sC, nullptr);
      }
      hipLaunchKernelGGL(kg_envelope_kernel, dim3((mm + 3) / 4, nb), dim3(256), 0, st, dmuA, (size_t)Mp, dCv, sC, Mp, dmean, dvar,
                         (size_t)mmp, dnoise + b0, M, mm, y_std, dKG + (size_t)b0 * mtot + m0, (size_t)mtot, dbad + b0);
      BGP_HIP(hipGetLastError());
    }
  }
  if (avg) {
    hipLaunchKernelGGL(acq_sum_kernel, dim3((m + 255) / 256, 1), dim3(256), 0, st, dKG, dbad, (size_t)mtot, m, B, n_samples, davg);
    BGP_HIP(hipGetLastError());
    BGP_HIP(bgp_memcpy_async(avg, davg, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  if (kg)
    BGP_HIP(bgp_memcpy2d_async(kg, (size_t)m * sizeof(double), dKG, (size_t)mtot * sizeof(double), (size_t)m * sizeof(double), B,
                               hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_stream_sync(st));
  return BGP_OK;
}

extern "C" int bgp_knowledge_gradient(bgp_ctx* c, int B, const double* h_kernel, const double* noise, int m, const double* Xcand,
                                      int M, const double* Xref, double y_std, int n_samples, double* kg, double* avg) {
  BGP_TRY(bgp_guard(c, "bgp_knowledge_gradient", BGP_POST_PLAIN));
  if (!h_kernel || !noise || !Xcand || (!kg && !avg) || m < 1 || m > (1 << 24) || B <= 0 || B > 65535 || M < 0 || (M > 0 && !Xref) ||
      n_samples <= 0) {
    bgp_set_error("bgp_knowledge_gradient: bad argument (1 <= B <= 65535, 1 <= m <= 2^24, 0 <= M, 1 <= n_samples, at least one output)");
    return BGP_ERR_INVALID;
  }
  if (M > KG_MMAX) {
    bgp_set_error("bgp_knowledge_gradient: M = %d reference points exceed %d", M, KG_MMAX);
    return BGP_ERR_INVALID;
  }
  if (c->d > KG_DMAX || c->has_warp) {
    bgp_set_error("bgp_knowledge_gradient: %s", c->has_warp ? "warped inputs are not supported" : "d > 32 is not supported");
    return BGP_ERR_INVALID;
  }
  BGP_TRY(bgp_guard(c, "bgp_knowledge_gradient", BGP_POST_PLAIN, B));
  return post_call(c, [&] { return kg_run(c, B, h_kernel, noise, m, Xcand, M, Xref, y_std, n_samples, kg, avg); });
}
