// The hyper-posterior mixture on the device: the posterior predictive at a point once the kernel
// hyper-parameters are integrated out is  sum_b w^_b N(mu_b(x), sd_b(x)^2)  over B posteriors (chain rows).  ONE pass serves the
// three entry points: bgp_predict_mixture and bgp_predict_mixture_warped run it behind the batched predict on the B x mpad means
// and variances that predict_run keeps on the device (bgp_post.hip, next to the acquisition pass), bgp_mixture_values on
// caller-supplied ones.
//
// Definitions, per point i and row b (mean, var: normalised-y moments, row-major B x mpad):
//   mu_bi = y_std * mean_bi + y_mean,  sd_bi = sqrt(var_bi * (y_std * y_std))           (acq_values_kernel's expressions)
//   w_b = weights[b], 1 when weights is NULL.  Row b is USED iff w_b > 0 and all of its m means and variances are finite.
//   W = sum of w_b over the used rows, b ascending;  w^_b = w_b / W;  *n_used = their count (0: every output NaN, BGP_OK).
//   moments (3 x m):  mean_i = sum w^_b mu_bi;  within_i = sum w^_b sd_bi^2;  between_i = sum w^_b (mu_bi - mean_i)^2, in a second
//     pass against the finished mean (>= 0, exactly 0 for one row).
//   at_t (3 x m), z_bi = (t_i - mu_bi) / sd_bi:  cdf_i = sum w^_b Phi(z_bi),  sf_i = sum w^_b Phi(-z_bi) -- each tail summed on its
//     own from e = erfc(|z| / sqrt 2) / 2 (the tail that |z| cuts off is e, the other one 1 - e), so a 1e-300 tail keeps its relative
//     accuracy;  logpdf_i = log sum w^_b exp(-z^2 / 2) / (sd_bi sqrt(2 pi)) = A + log sum w^_b exp(a_b - A) - log(2 pi) / 2 with
//     a_b = -z^2 / 2 - log sd_bi and A = max a_b.  A component with sd = 0 is a step at mu (Phi = 1 where t >= mu, else 0) and adds
//     nothing to the density; logpdf is -inf when no used component has sd > 0.
//   quant (Q x m):  q_pi = inf {t : F_i(t) >= p}.  g(t) = F_i(t) - p for p <= 0.5 and (1 - p) - S_i(t) above (1 - p is exact there);
//     the answer is the upper end of a bracket [lo, hi] with g(lo) < 0 <= g(hi) whose ends are adjacent doubles.
//     Bracket: [min_b, max_b] of mu_bi + z_p sd_bi over the used rows, z_p from the DEVICE's inverse normal (normcdfinv of p, or minus
//     that of 1 - p); an end whose evaluated g has the wrong sign (z_p's rounding, one component) moves outwards by
//     max(sd, |end|) 2^-40, doubling.  Steps: Newton from the end with the smaller |g| with the mixture density as the slope, aimed
//     PAST the Newton point by (2^-8 |step| + 2 eps |t|) 4^k, k the Newton steps in a row that did not cross the root, so that the
//     far end comes in as well; bisection whenever that point is not strictly inside the bracket or the bracket has not halved
//     over the last two steps.  Every sign is that of the evaluated g, so the
//     result is a deterministic function of the point's column; a quantile carried by an atom comes back as exactly its mu.
//     Iteration cap BGP_MIX_ITMAX = 200: the upper end of the bracket reached by then is returned (g(hi) >= 0 still holds).
// Every sum runs over the used rows in ascending b in ONE thread per point (the moments are row-major, adjacent lanes read adjacent
// addresses); no floating-point atomics, no contraction.  A point's results do not depend on the other points unless they drop a row.
#include "bgp_common.h"

#include <cmath>

#define BGP_MIX_ITMAX 200

void BgpMixScratch::take(BgpCarve& s, int B, int mpad, int Q) {
  dmu = s.take<double>((size_t)B * mpad);
  dsd = s.take<double>((size_t)B * mpad);
  dw = s.take<double>(B);
  dwn = s.take<double>(B);
  dprobs = s.take<double>(BGP_MIX_QMAX);
  dt = s.take<double>(mpad);
  dmom = s.take<double>((size_t)3 * mpad);
  dat = s.take<double>((size_t)3 * mpad);
  dquant = s.take<double>((size_t)(Q > 0 ? Q : 1) * mpad);
  dbad = s.take<int>(B);
  dused = s.take<int>(B);
  dstat = s.take<int>(4);
}

// mu, sd of every row in y units; bad[b] |= "a mean or a variance of row b is not finite".  grid (ceil(m / 256), rows)
__global__ void __launch_bounds__(256) mix_prep_kernel(const double* __restrict__ mean, const double* __restrict__ var, size_t sm,
                                                        int m, double y_mean, double y_std, double* __restrict__ mu,
                                                        double* __restrict__ sd, int* __restrict__ bad) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= m) return;
  const double me = mean[(size_t)b * sm + i], va = var[(size_t)b * sm + i];
  mu[(size_t)b * sm + i] = y_std * me + y_mean;
  sd[(size_t)b * sm + i] = sqrt(va * (y_std * y_std));
  if (!isfinite(me) || !isfinite(va)) atomicOr(&bad[b], 1);
}

// used rows, W in ascending b, w^_b; stat = {n_used, 0, 0, 0}.  One thread.
__global__ void mix_norm_kernel(const double* __restrict__ w, const int* __restrict__ bad, int B, double* __restrict__ wn,
                                int* __restrict__ used, int* __restrict__ stat) {
#pragma clang fp contract(off)
  if (blockIdx.x || threadIdx.x) return;
  double W = 0.0;
  int nu = 0;
  for (int b = 0; b < B; b++) {
    const int u = (w[b] > 0.0 && !bad[b]) ? 1 : 0;
    used[b] = u;
    if (u) W += w[b], nu++;
  }
  for (int b = 0; b < B; b++) wn[b] = used[b] ? w[b] / W : 0.0;
  stat[0] = nu, stat[1] = 0, stat[2] = 0, stat[3] = 0;
}

struct MixCol {  // one point's column of the row-major moments
  const double *mu, *sd, *wn;
  const int* used;
  size_t sm;
  int B;
};

// The tail sum at t (up: S = sum w^ Phi(-z), else F = sum w^ Phi(z)) and the mixture density there.
static __device__ __forceinline__ void mix_tail(const MixCol& c, double t, bool up, double& tail, double& dens) {
#pragma clang fp contract(off)
  double s = 0.0, f = 0.0;
#pragma unroll 1
  for (int b = 0; b < c.B; b++) {
    if (!c.used[b]) continue;
    const double m_ = c.mu[(size_t)b * c.sm], s_ = c.sd[(size_t)b * c.sm], w = c.wn[b];
    if (s_ > 0.0) {
      const double z = (t - m_) / s_;
      const double e = 0.5 * erfc(fabs(z) * 0.70710678118654752440);
      const double ph = up ? (z >= 0.0 ? e : 1.0 - e) : (z <= 0.0 ? e : 1.0 - e);
      s += w * ph;
      f += w * (exp(-(z * z) / 2.0) / (s_ * 2.5066282746310002));  // sqrt(2 pi)
    } else {
      const double ph = (s_ == 0.0) ? ((up ? (t < m_) : (t >= m_)) ? 1.0 : 0.0) : NAN;
      s += w * ph;
    }
  }
  tail = s, dens = f;
}

// q_p of one point (header comment); iters / grows: the steps and the bracket moves it took.  The tail sum has ONE call site (its
// erfc and exp are inlined once): the stages -- 0 / 1 evaluate the ends, 2 / 3 move an end outwards, 4 shrink -- share the loop.
static __device__ __forceinline__ double mix_quantile(const MixCol& c, double p, int& iters, int& grows) {
#pragma clang fp contract(off)
  const bool up = p > 0.5;
  const double target = up ? 1.0 - p : p;
  const double zp = up ? -normcdfinv(target) : normcdfinv(p);
  double lo = INFINITY, hi = -INFINITY, smax = 0.0;
  for (int b = 0; b < c.B; b++) {
    if (!c.used[b]) continue;
    const double s_ = c.sd[(size_t)b * c.sm];
    const double v = c.mu[(size_t)b * c.sm] + zp * s_;
    lo = fmin(lo, v), hi = fmax(hi, v), smax = fmax(smax, s_);
  }
  double glo = 0.0, flo = 0.0, ghi = 0.0, fhi = 0.0, tn = lo, step = 0.0, w1 = INFINITY, w2 = INFINITY, boost = 1.0;
  int stage = 0, ng = 0, it = 0, newton = 0;  // newton: the step under evaluation started from lo (1) / hi (-1)
  for (;;) {
    double tl, ft;
    mix_tail(c, tn, up, tl, ft);
    const double gt = up ? target - tl : tl - target;
    if (stage == 0) {
      glo = gt, flo = ft;
      if (hi == lo) {
        ghi = gt, fhi = ft, stage = 2;
      } else {
        stage = 1, tn = hi;
        continue;
      }
    } else if (stage == 1) {
      ghi = gt, fhi = ft, stage = 2;
    } else if (stage == 2) {  // (the old lower end has g >= 0: it is an upper end)
      hi = lo, ghi = glo, fhi = flo;
      lo = tn, glo = gt, flo = ft;
    } else if (stage == 3) {
      lo = hi, glo = ghi, flo = fhi;
      hi = tn, ghi = gt, fhi = ft;
    } else {
      // a Newton step that did not cross the root leaves the far end where it was: the next one aims four times as far past
      if (newton) boost = ((newton > 0) == (gt < 0.0)) ? boost * 4.0 : 1.0;
      if (gt < 0.0)
        lo = tn, glo = gt, flo = ft;
      else
        hi = tn, ghi = gt, fhi = ft;
    }
    if (stage == 2) {
      if (glo >= 0.0 && ng < 2200) {
        if (step == 0.0) step = fmax(fmax(smax, fabs(lo)) * 9.094947017729282e-13, 2.2250738585072014e-308);  // 2^-40
        tn = lo - step, step *= 2.0, ng++;
        continue;
      }
      stage = 3, step = 0.0;
    }
    if (stage == 3) {
      if (ghi < 0.0 && ng < 4400) {
        if (step == 0.0) step = fmax(fmax(smax, fabs(hi)) * 9.094947017729282e-13, 2.2250738585072014e-308);
        tn = hi + step, step *= 2.0, ng++;
        continue;
      }
      stage = 4;
    }
    if (it >= BGP_MIX_ITMAX) break;
    const double wd = hi - lo, mid = lo + 0.5 * wd;
    if (!(mid > lo && mid < hi)) break;  // adjacent doubles (or a NaN column)
    tn = mid, newton = 0;
    if (!(wd > 0.5 * w2)) {
      const bool from_lo = -glo <= ghi;
      const double tb = from_lo ? lo : hi, dir = from_lo ? 1.0 : -1.0, s = -(from_lo ? glo : ghi) / (from_lo ? flo : fhi);
      const double over = (fabs(s) * 0.00390625 + 4.440892098500626e-16 * fabs(tb)) * boost;  // 2^-8 of the step + 2 eps |t|
      const double cnd = tb + (s + dir * over);
      if (cnd > lo && cnd < hi) tn = cnd, newton = from_lo ? 1 : -1;
    }
    w2 = w1, w1 = wd, it++;
  }
  iters = it, grows = ng;
  return hi;
}

// The three kernels of the pass: one thread per point (mix_quant_kernel: per point and probability, grid.y = q) walks the used rows
// in ascending b.  grid.x = ceil(m / 256).  stat[0] == 0 (no row is used): NaN.
__global__ void __launch_bounds__(256) mix_moments_kernel(const double* __restrict__ mu, const double* __restrict__ sd, size_t sm,
                                                           int m, int B, const int* __restrict__ used,
                                                           const double* __restrict__ wn, const int* __restrict__ stat,
                                                           double* __restrict__ mom) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  double mean = 0.0, within = 0.0, between = 0.0;
  for (int b = 0; b < B; b++) {
    if (!used[b]) continue;
    const double m_ = mu[(size_t)b * sm + i], s_ = sd[(size_t)b * sm + i];
    mean += wn[b] * m_;
    within += wn[b] * (s_ * s_);
  }
  for (int b = 0; b < B; b++) {
    if (!used[b]) continue;
    const double dm = mu[(size_t)b * sm + i] - mean;
    between += wn[b] * (dm * dm);
  }
  if (stat[0] == 0) mean = within = between = NAN;
  mom[i] = mean, mom[sm + i] = within, mom[2 * sm + i] = between;
}

__global__ void __launch_bounds__(256) mix_at_kernel(const double* __restrict__ mu, const double* __restrict__ sd, size_t sm, int m,
                                                      int B, const int* __restrict__ used, const double* __restrict__ wn,
                                                      const int* __restrict__ stat, const double* __restrict__ tpt,
                                                      double* __restrict__ at) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= m) return;
  const double t = tpt[i];
  double F = 0.0, S = 0.0, A = -INFINITY;
#pragma unroll 1
  for (int b = 0; b < B; b++) {
    if (!used[b]) continue;
    const double m_ = mu[(size_t)b * sm + i], s_ = sd[(size_t)b * sm + i], w = wn[b];
    if (s_ > 0.0) {
      const double z = (t - m_) / s_;
      const double e = 0.5 * erfc(fabs(z) * 0.70710678118654752440);
      F += w * (z <= 0.0 ? e : 1.0 - e);
      S += w * (z >= 0.0 ? e : 1.0 - e);
      A = fmax(A, -(z * z) / 2.0 - log(s_));
    } else {
      const double st = (s_ == 0.0) ? (t >= m_ ? 1.0 : 0.0) : NAN;
      F += w * st;
      S += w * (1.0 - st);
    }
  }
  double lp = -INFINITY;
  if (A > -INFINITY || isnan(A)) {
    double acc = 0.0;
#pragma unroll 1
    for (int b = 0; b < B; b++) {
      if (!used[b]) continue;
      const double s_ = sd[(size_t)b * sm + i];
      if (!(s_ > 0.0)) continue;
      const double z = (t - mu[(size_t)b * sm + i]) / s_;
      acc += wn[b] * exp((-(z * z) / 2.0 - log(s_)) - A);
    }
    lp = (A + log(acc)) - 0.91893853320467274178;  // log(2 pi) / 2
  }
  if (stat[0] == 0) F = S = lp = NAN;
  at[i] = F, at[sm + i] = S, at[2 * sm + i] = lp;
}

// stat[1], stat[2]: the largest step / bracket-move counts of the solver (integer atomicMax)
__global__ void __launch_bounds__(256) mix_quant_kernel(const double* __restrict__ mu, const double* __restrict__ sd, size_t sm,
                                                         int m, int B, const int* __restrict__ used,
                                                         const double* __restrict__ wn, int* __restrict__ stat,
                                                         const double* __restrict__ probs, double* __restrict__ quant) {
  const int i = blockIdx.x * 256 + threadIdx.x, q = blockIdx.y;
  if (i >= m) return;
  if (stat[0] == 0) {
    quant[(size_t)q * sm + i] = NAN;
    return;
  }
  const MixCol c{mu + i, sd + i, wn, used, sm, B};
  int it, ng;
  quant[(size_t)q * sm + i] = mix_quantile(c, probs[q], it, ng);
  atomicMax(&stat[1], it);
  atomicMax(&stat[2], ng);
}

int bgp_mix_check(const char* who, int B, const BgpMixPlan& mp) {
  if (B <= 0 || mp.Q < 0 || mp.Q > BGP_MIX_QMAX || (mp.Q > 0 && !mp.probs) || (mp.quant && mp.Q == 0) || (mp.at_t && !mp.t) ||
      !mp.n_used) {
    bgp_set_error("%s: bad argument (0 <= Q <= %d, probs with Q > 0, t with at_t, n_used)", who, BGP_MIX_QMAX);
    return BGP_ERR_INVALID;
  }
  for (int q = 0; q < mp.Q; q++)
    if (!(mp.probs[q] > 0.0 && mp.probs[q] < 1.0)) {
      bgp_set_error("%s: probs[%d] = %g is not inside (0, 1)", who, q, mp.probs[q]);
      return BGP_ERR_INVALID;
    }
  for (int b = 0; mp.weights && b < B; b++)
    if (!(mp.weights[b] >= 0.0) || !std::isfinite(mp.weights[b])) {
      bgp_set_error("%s: weights[%d] = %g is negative or not finite", who, b, mp.weights[b]);
      return BGP_ERR_INVALID;
    }
  return BGP_OK;
}

// The pass on dmean / dvar (B rows of stride mpad, on the device): enqueues uploads, up to five launches and the downloads on the
// context's stream; the caller waits (bgp_stream_sync) before it reads the outputs, *n_used and c->mix_last.
int bgp_mix_run(bgp_ctx* c, int B, int m, int mpad, const double* dmean, const double* dvar, const BgpMixPlan& mp,
                const BgpMixScratch& ms) {
  hipStream_t st = c->stream;
  const size_t row = (size_t)m * sizeof(double), pitch = (size_t)mpad * sizeof(double);
  const std::vector<double> ones(mp.weights ? 0 : B, 1.0);  // (an upload is packed into the pinned arena before the call returns)
  BGP_HIP(bgp_memcpy_async(ms.dw, mp.weights ? mp.weights : ones.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
  if (mp.Q) BGP_HIP(bgp_memcpy_async(ms.dprobs, mp.probs, (size_t)mp.Q * sizeof(double), hipMemcpyHostToDevice, st));
  if (mp.at_t) BGP_HIP(bgp_memcpy_async(ms.dt, mp.t, row, hipMemcpyHostToDevice, st));
  BGP_HIP(hipMemsetAsync(ms.dbad, 0, (size_t)B * sizeof(int), st));
  hipLaunchKernelGGL(mix_prep_kernel, dim3((m + 255) / 256, B), dim3(256), 0, st, dmean, dvar, (size_t)mpad, m, mp.y_mean,
                     mp.y_std, ms.dmu, ms.dsd, ms.dbad);
  hipLaunchKernelGGL(mix_norm_kernel, dim3(1), dim3(64), 0, st, (const double*)ms.dw, (const int*)ms.dbad, B, ms.dwn, ms.dused,
                     ms.dstat);
  const dim3 gm((m + 255) / 256);
  if (mp.moments)
    hipLaunchKernelGGL(mix_moments_kernel, gm, dim3(256), 0, st, (const double*)ms.dmu, (const double*)ms.dsd, (size_t)mpad, m, B,
                       (const int*)ms.dused, (const double*)ms.dwn, (const int*)ms.dstat, ms.dmom);
  if (mp.at_t)
    hipLaunchKernelGGL(mix_at_kernel, gm, dim3(256), 0, st, (const double*)ms.dmu, (const double*)ms.dsd, (size_t)mpad, m, B,
                       (const int*)ms.dused, (const double*)ms.dwn, (const int*)ms.dstat, (const double*)ms.dt, ms.dat);
  if (mp.quant)
    hipLaunchKernelGGL(mix_quant_kernel, dim3((m + 255) / 256, mp.Q), dim3(256), 0, st, (const double*)ms.dmu,
                       (const double*)ms.dsd, (size_t)mpad, m, B, (const int*)ms.dused, (const double*)ms.dwn, ms.dstat,
                       (const double*)ms.dprobs, ms.dquant);
  BGP_HIP(hipGetLastError());
  if (mp.moments) BGP_HIP(bgp_memcpy2d_async(mp.moments, row, ms.dmom, pitch, row, 3, hipMemcpyDeviceToHost, st));
  if (mp.quant) BGP_HIP(bgp_memcpy2d_async(mp.quant, row, ms.dquant, pitch, row, mp.Q, hipMemcpyDeviceToHost, st));
  if (mp.at_t) BGP_HIP(bgp_memcpy2d_async(mp.at_t, row, ms.dat, pitch, row, 3, hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_memcpy_async(c->mix_last, ms.dstat, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
  return BGP_OK;
}

static int mix_resident(bgp_ctx* c, const char* who, bool rowwarp, int B, const double* h_kernel, const double* weights, int m,
                        const double* Xq, double y_mean, double y_std, int Q, const double* probs, const double* t,
                        double* moments, double* quant, double* at_t, int* n_used) {
  const BgpPostKind kind = rowwarp ? BGP_POST_ROWWARP : BGP_POST_PLAIN;
  BGP_TRY(bgp_guard(c, who, kind));
  if (!h_kernel || !Xq || m <= 0 || B <= 0) {
    bgp_set_error("%s: bad argument", who);
    return BGP_ERR_INVALID;
  }
  const BgpMixPlan mp{weights, y_mean, y_std, Q, probs, t, moments, quant, at_t, n_used};
  BGP_TRY(bgp_mix_check(who, B, mp));
  BGP_TRY(bgp_guard(c, who, kind, B));
  const int rc = post_call(c, [&] { return bgp_predict_run_mix(c, B, h_kernel, m, Xq, mp, rowwarp); });
  if (rc == BGP_OK) *n_used = c->mix_last[0];
  return rc;
}

extern "C" int bgp_predict_mixture(bgp_ctx* c, int B, const double* h_kernel, const double* weights, int m, const double* Xq,
                                   double y_mean, double y_std, int Q, const double* probs, const double* t, double* moments,
                                   double* quant, double* at_t, int* n_used) {
  return mix_resident(c, "bgp_predict_mixture", false, B, h_kernel, weights, m, Xq, y_mean, y_std, Q, probs, t, moments, quant,
                      at_t, n_used);
}

extern "C" int bgp_predict_mixture_warped(bgp_ctx* c, int B, const double* h_kernel, const double* weights, int m,
                                          const double* Xq, double y_mean, double y_std, int Q, const double* probs,
                                          const double* t, double* moments, double* quant, double* at_t, int* n_used) {
  return mix_resident(c, "bgp_predict_mixture_warped", true, B, h_kernel, weights, m, Xq, y_mean, y_std, Q, probs, t, moments,
                      quant, at_t, n_used);
}

extern "C" int bgp_mixture_values(bgp_ctx* c, int B, int m, const double* mean, const double* var, const double* weights,
                                  double y_mean, double y_std, int Q, const double* probs, const double* t, double* moments,
                                  double* quant, double* at_t, int* n_used) {
  BGP_TRY(bgp_guard(c, "bgp_mixture_values"));
  if (!mean || !var || m <= 0 || B <= 0) {
    bgp_set_error("bgp_mixture_values: bad argument");
    return BGP_ERR_INVALID;
  }
  const BgpMixPlan mp{weights, y_mean, y_std, Q, probs, t, moments, quant, at_t, n_used};
  BGP_TRY(bgp_mix_check("bgp_mixture_values", B, mp));
  const int rc = post_call(c, [&]() -> int {
    const int mpad = pad_to(m, 128);
    const size_t row = (size_t)m * sizeof(double), pitch = (size_t)mpad * sizeof(double);
    double *dmean, *dvar;
    BgpMixScratch ms;
    BgpScratch live(c);
    BGP_TRY(live.carve([&](BgpCarve& s) {
      dmean = s.take<double>((size_t)B * mpad);
      dvar = s.take<double>((size_t)B * mpad);
      ms.take(s, B, mpad, Q);
    }));
    BGP_HIP(bgp_memcpy2d_async(dmean, pitch, mean, row, row, B, hipMemcpyHostToDevice, c->stream));
    BGP_HIP(bgp_memcpy2d_async(dvar, pitch, var, row, row, B, hipMemcpyHostToDevice, c->stream));
    BGP_TRY(bgp_mix_run(c, B, m, mpad, dmean, dvar, mp, ms));
    BGP_HIP(bgp_stream_sync(c->stream));
    return BGP_OK;
  });
  if (rc == BGP_OK) *n_used = c->mix_last[0];
  return rc;
}

extern "C" int bgp_mixture_stats(bgp_ctx* c, long long* out) {
  BGP_TRY(bgp_guard(c, "bgp_mixture_stats"));
  if (!out) {
    bgp_set_error("bgp_mixture_stats: bad argument");
    return BGP_ERR_INVALID;
  }
  out[0] = c->mix_last[1], out[1] = c->mix_last[2];
  return BGP_OK;
}
