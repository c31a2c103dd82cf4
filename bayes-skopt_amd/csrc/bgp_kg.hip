// Knowledge-gradient acquisition on the resident posteriors.
//
// For resident posterior b, reference points A = (a_0 .. a_{M-1}), a candidate x and s = var_b(x) + noise_b (var_b latent, noise_b the
// variance of a fantasy observation as bgp_fantasy_begin takes it) the M + 1 lines in Z ~ N(0, 1) are
//   p_j = mu_b(a_j)   q_j = cov_b(a_j, x) / sqrt(s)   (j < M)        p_M = mu_b(x)   q_M = var_b(x) / sqrt(s)
//   cov_b(a, x) = k_b(a, x) - k_b(a, X) K_b^-1 k_b(X, x)             (latent: no white term)
//   KG_b(x) = min_j p_j - E[min_j (p_j + q_j Z)] >= 0, exactly 0 where s <= 0
// Stages 1, 2 and 4 -- mu_b(A), the candidates' moments, C[x][j] = cov_b(a_j, x), the average over the posteriors -- are the
// conditional-moments pipeline of bgp_cond.hip with ONE point set shared by the posteriors and no point variances.  Stage
//   3  kg_envelope_kernel: one wave per (posterior, candidate).  The lower envelope by pairwise interval clipping, sort-free: line j
//      is the minimum on [lo_j, hi_j] = the intersection over i of {z : (q_j - q_i) z <= p_i - p_j}; a bound is kept as a fraction
//      (numerator, positive denominator; denominator 0 = infinite) and two bounds are compared by cross-multiplication, so the M^2 loop
//      holds no division.  A line that owns an interval contributes (p_j - p*) (Phi(hi) - Phi(lo)) + q_j (phi(lo) - phi(hi)), p* = min p.
//      Divisions per candidate: 1 (1 / sqrt(s)) + 2 (M + 1) (the two bounds of every line).
// No workgroup waits for another; no floating-point atomics (one integer flag per posterior: "a value is not finite"); every loop is
// bounded by an argument.  A candidate's value depends on the posterior, the ordered reference list and that candidate alone: a lane
// adds its lines in ascending j = lane + 64 t, the 64 lanes are added by a fixed butterfly.
#include "bgp_common.h"
#include "bgp_device.h"

#define KG_DMAX 32    // input dimensions
#define KG_MMAX 255   // reference points
#define KG_LMAX 256   // lines of a candidate (KG_MMAX + 1)
#define KG_LPL 4      // lines per lane (KG_LMAX / 64)

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

// Everything but the scoring launch is the conditional-moments pipeline (bgp_cond.hip): one shared point set, no point variances.
static int kg_run(bgp_ctx* c, int B, const double* h_kernel, const double* noise, int m, const double* Xcand, int M,
                  const double* Xref, double y_std, int n_samples, double* kg, double* avg) {
  BgpCondReq q{};
  q.B = B, q.m = m, q.M = M, q.h_kernel = h_kernel, q.noise = noise, q.Xcand = Xcand, q.Xpts = Xref;
  q.chunk_switch = BGP_SW_KG_CHUNK, q.n_samples = n_samples, q.rows = kg, q.avg = avg;
  return bgp_cond_run(c, q, [&](const BgpCondChunk& k) {
    hipLaunchKernelGGL(kg_envelope_kernel, dim3((k.mm + 3) / 4, k.nb), dim3(256), 0, c->stream, k.muA, (size_t)k.Mp, k.Cv, k.sC, k.Mp,
                       k.mean, k.var, k.sm, k.noise, M, k.mm, y_std, k.out, k.so, k.bad);
  });
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
