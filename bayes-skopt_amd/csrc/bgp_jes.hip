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
// Stages 1, 2 and 4 -- mu_r and v_r, the candidates' moments, C[x][r] = cov_b(a_r, x), the average over the posteriors -- are the
// conditional-moments pipeline of bgp_cond.hip with one point set per posterior and the point variances.  Stage
//   3  jes_gain_kernel: one wave per (posterior, candidate), four candidates of one posterior per workgroup; per optimum sample the
//      workgroup keeps 1 / w_r, (f_r - mu_r) / w_r and f_r in LDS (the two divisions by w_r are formed once per workgroup, not per
//      candidate: m_r = mu + c_r [(f_r - mu_r) / w_r], v_s = v - c_r c_r [1 / w_r]).  A lane owns r = lane + 64 t, adds its terms in
//      ascending t; the 64 lanes are added by a fixed xor butterfly (32, 16, .. 1); one division by R.
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

// Everything but the scoring launch is the conditional-moments pipeline (bgp_cond.hip): one point set per posterior, with the
// optimum values and the variances at the points.
static int jes_run(bgp_ctx* c, int B, const double* h_kernel, const double* noise, int m, const double* Xcand, int R,
                   const double* Xopt, const double* fopt, double tau, int n_samples, double* gain, double* avg) {
  BgpCondReq q{};
  q.B = B, q.m = m, q.M = R, q.h_kernel = h_kernel, q.noise = noise, q.Xcand = Xcand, q.Xpts = Xopt;
  q.per_posterior = true, q.fpts = fopt, q.want_var = true;
  q.chunk_switch = BGP_SW_JES_CHUNK, q.n_samples = n_samples, q.rows = gain, q.avg = avg;
  return bgp_cond_run(c, q, [&](const BgpCondChunk& k) {
    hipLaunchKernelGGL(jes_gain_kernel, dim3((k.mm + 3) / 4, k.nb), dim3(256), 0, c->stream, k.muA, k.vA, (size_t)k.Mp, k.fpts, k.Cv,
                       k.sC, k.Mp, k.mean, k.var, k.sm, k.noise, tau, R, k.mm, k.out, k.so, k.bad);
  });
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
