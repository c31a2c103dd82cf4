// The whole-workgroup evaluator of the predictive mean / variance and their gradients at ONE point, shared by
// the translation units that run it: bgp_predgrad.hip (bgp_predict_grad_batch, bgp_minimize_starts) and bgp_profile.hip
// (bgp_profile_dependence).  Every function is static: each unit compiles its own copy of the same operations.
#pragma once
#include "bgp_device.h"
#include "bgp_bfgs.h"

// (PG_NT threads in PG_NW waves, PG_DMAX dimensions, the line-search cap PG_LS_MAX: bgp_bfgs.h)
#define PG_NLDS 3072              // training points whose k / g rows fit the workgroup's LDS (2 x 24 KB); beyond: device scratch rows
#define PG_RS (PG_DMAX + 1)       // stride of a wave's partial sums

struct PgWork {                   // LDS of one evaluation
  double x[PG_DMAX];              // the query point
  double il[PG_DMAX];             // 1 / length scale
  double red[PG_NW * PG_RS];      // wave partials
  double mean, var;
  double dmean[PG_DMAX], dvar[PG_DMAX];
};

static __device__ __forceinline__ double pg_wave_sum(double s) {
#pragma clang fp contract(off)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  return s;
}

// dst[t] = scale il_t sum_i w_i (x_t - X_it) il_t with w_i = a_i gb_i (a == nullptr: gb_i): the contraction of dmean and dvar.  Lane
// (t, half) of wave wv owns dimension t over the points 2 wv + half, + 2 PG_NW, ...; the two halves, then the waves in ascending
// order.  Ends with a barrier.
static __device__ __forceinline__ void pg_wsum(const double* __restrict__ X, int n, int d, const double* __restrict__ a,
                                               const double* gb, PgWork& W, double scale, double* dst) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, t = lane & 31;
  double acc = 0.0;
  if (t < d) {
    const double xl = W.x[t], ill = W.il[t];
    for (int i = 2 * wv + (lane >> 5); i < n; i += 2 * PG_NW) {
      const double w = a ? a[i] * gb[i] : gb[i];
      acc = fma(w, (xl - X[(size_t)i * d + t]) * ill, acc);
    }
  }
  acc += __shfl_xor(acc, 32, 64);
  if (lane < d) W.red[wv * PG_RS + 1 + lane] = acc;
  __syncthreads();
  if (tid < d) {
    double s = 0.0;
    for (int w = 0; w < PG_NW; w++) s += W.red[w * PG_RS + 1 + tid];
    dst[tid] = scale * (s * W.il[tid]);
  }
  __syncthreads();
}

// mean / dmean (and, with want_var, var / dvar) of one posterior at W.x into W.  Called by every thread of the workgroup; W.x and
// W.il may have been written just before (the function starts with a barrier) and W's results are visible to every thread on return.
template <int STAT, int FORM>
static __device__ __noinline__ void pg_eval(const double* __restrict__ X, int n, int d, const double* __restrict__ alpha,
                               const double* __restrict__ Kinv, int npad, double cst, double kdiag, bool want_var, double* kb,
                               double* gb, PgWork& W) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  __syncthreads();
  // pass 1: k_i, g_i = cf fac_i, the mean
  double am = 0.0;
  for (int i = tid; i < n; i += PG_NT) {
    const double* xi = X + (size_t)i * d;
    double r2 = 0.0;
    for (int t = 0; t < d; t++) {
      const double df = (W.x[t] - xi[t]) * W.il[t];
      r2 = fma(df, df, r2);
    }
    double S, fac;
    kb_stationary_fac<STAT>(r2, S, fac);
    const double k = kb_with_constant<FORM>(cst, S);
    kb[i] = k;
    gb[i] = (FORM == BGP_FORM_PRODUCT) ? cst * fac : fac;
    am = fma(k, alpha[i], am);
  }
  am = pg_wave_sum(am);
  if (lane == 0) W.red[wv * PG_RS] = am;
  __syncthreads();  // (the k / g rows are complete behind it too)
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < PG_NW; w++) s += W.red[w * PG_RS];
    W.mean = s;
  }
  pg_wsum(X, n, d, alpha, gb, W, 1.0, W.dmean);
  if (!want_var) return;
  // pass 2: v_j = (K^-1 k)_j, four rows per wave and step; g_j becomes v_j g_j
  double q = 0.0;
  for (int j0 = wv * 4; j0 < n; j0 += PG_NW * 4) {  // (rows j0 .. j0 + 3 < npad: a multiple of 128)
    const double* K0 = Kinv + (size_t)j0 * npad;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    for (int i = lane; i < n; i += 64) {
      const double kk = kb[i];
      a0 = fma(K0[i], kk, a0);
      a1 = fma(K0[(size_t)npad + i], kk, a1);
      a2 = fma(K0[2 * (size_t)npad + i], kk, a2);
      a3 = fma(K0[3 * (size_t)npad + i], kk, a3);
    }
    const double v[4] = {pg_wave_sum(a0), pg_wave_sum(a1), pg_wave_sum(a2), pg_wave_sum(a3)};
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int j = j0 + r;
      if (j < n) {
        q = fma(kb[j], v[r], q);
        if (lane == 0) gb[j] = v[r] * gb[j];
      }
    }
  }
  if (lane == 0) W.red[wv * PG_RS] = q;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < PG_NW; w++) s += W.red[w * PG_RS];
    const double vv = kdiag - s;
    W.var = vv > 0.0 ? vv : 0.0;  // (clipped at 0 as bgp_predict_batch clips)
  }
  pg_wsum(X, n, d, nullptr, gb, W, -2.0, W.dvar);
}

// the workgroup's k / g rows: dynamic LDS, or its slice of the device scratch
static __device__ __forceinline__ void pg_rows(double* dyn, double* scratch, int n, int npad, int wg, double*& kb, double*& gb) {
  if (scratch) {
    kb = scratch + (size_t)wg * 2 * npad;
    gb = kb + npad;
  } else {
    kb = dyn;
    gb = dyn + n;
  }
}

// f and its gradient (y units) from the evaluation in W; where y_std sqrt(var) <= 1e-8 the std term contributes no gradient
// (skopt's allclose(std, 0) rule, BayesGPR._predict_gradients)
static __device__ __forceinline__ double pg_objective(const PgWork& W, double y_mean, double y_std, double kappa) {
#pragma clang fp contract(off)
  double f = y_mean + y_std * W.mean;
  if (kappa != 0.0) f = f + kappa * (y_std * sqrt(W.var));
  return f;
}
static __device__ __forceinline__ double pg_gradient(const PgWork& W, int t, double y_std, double kappa) {
#pragma clang fp contract(off)
  double g = y_std * W.dmean[t];
  if (kappa != 0.0) {
    const double sd = y_std * sqrt(W.var);
    if (sd > 1e-8) g = g + kappa * (W.dvar[t] / sd * (0.5 * (y_std * y_std)));
  }
  return g;
}
