// Prediction gradients for many query rows and the device-resident optimum search.
//
// With G_i = d k(x, X_i) / dx = cf fac(r_i) (x - X_i) / l^2  (cf = c in the product form, 1 in the sum form; fac(r) = (dS/dr) / r in
// the closed forms of _posterior.CanonicalPosterior.grad_x, 0 at r = 0 for Matern 1/2; the constant and white terms add nothing):
//   mean = sum_i alpha_i k_i            dmean = sum_i alpha_i G_i
//   v    = K^-1 k                       var   = max(0, k_** - k^T v)            dvar = -2 sum_i v_i G_i
// ONE __device__ function, pg_eval, evaluates all of it for one query point with one workgroup of PG_NT threads:
//   pass 1  every thread takes a strided share of the training points, writes k_i and g_i = cf fac_i to the workgroup's row
//           buffers (LDS up to PG_NLDS points, a device scratch row beyond) and accumulates the mean; then dmean, lane t of a wave
//           owning dimension t over the wave's share of the points; a fixed butterfly inside every wave, then the wave partials in
//           ascending order;
//   pass 2  (variance wanted) v_j by row-wise dot products of the symmetric resident inverse against k -- one wave per group of four
//           rows, coalesced row reads, n^2 doubles per evaluation out of L2 / the Infinity Cache: that is its floor --, and from v_j at
//           once the sum of k^T v; g_j becomes v_j g_j and dvar is the contraction of dmean once more.
// bgp_predict_grad_batch runs it on one workgroup per (query row, posterior); bgp_minimize_starts on one workgroup per start, which
// carries the whole bounded quasi-Newton iteration itself: no workgroup ever waits for another, every loop has a fixed cap.
// fp64 VALU work throughout (no MFMA shape); every reduction has a fixed order: results are bitwise reproducible and a row / a start
// does not depend on what shares its launch.
#include "bgp_common.h"
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

// one workgroup per (query row, posterior)
template <int STAT, int FORM>
__global__ void __launch_bounds__(PG_NT) pg_rows_kernel(const double* __restrict__ X, int n, int d, int npad,
                                                        const double* __restrict__ alphaB, const double* __restrict__ KinvB,
                                                        const double* __restrict__ H, const double* __restrict__ Xq, int m,
                                                        double* scratch, double* __restrict__ mean, double* __restrict__ var,
                                                        double* __restrict__ dmean, double* __restrict__ dvar) {
  extern __shared__ double pg_dyn[];
  __shared__ PgWork W;
  const int tid = threadIdx.x, i = blockIdx.x, b = blockIdx.y;
  const double* h = H + (size_t)b * (d + 2);
  if (tid < d) {
    W.x[tid] = Xq[(size_t)i * d + tid];
    W.il[tid] = 1.0 / exp(h[1 + tid]);
  }
  const double cst = exp(h[0]);
  const double kdiag = kb_with_constant<FORM>(cst, 1.0) + exp(h[d + 1]);
  double *kb, *gb;
  pg_rows(pg_dyn, scratch, n, npad, b * gridDim.x + i, kb, gb);
  pg_eval<STAT, FORM>(X, n, d, alphaB + (size_t)b * npad, KinvB + (size_t)b * npad * npad, npad, cst, kdiag, true, kb, gb, W);
  const size_t o = (size_t)b * m + i;
  if (tid == 0) {
    mean[o] = W.mean;
    var[o] = W.var;
  }
  if (tid < d) {
    dmean[o * d + tid] = W.dmean[tid];
    if (dvar) dvar[o * d + tid] = W.dvar[tid];
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

// One workgroup per start: the projected BFGS of bgp_bfgs.h on pg_eval.  status 0: |projected gradient|_inf <= gtol; 1: max_iter
// reached; 2: no decrease found, or a non-finite objective / gradient (a NaN start).
template <int STAT, int FORM>
__global__ void __launch_bounds__(PG_NT) pg_min_kernel(const double* __restrict__ X, int n, int d, int npad,
                                                       const double* __restrict__ alpha, const double* __restrict__ Kinv,
                                                       const double* __restrict__ h, double y_mean, double y_std, double kappa,
                                                       const double* __restrict__ X0, const double* __restrict__ lo_,
                                                       const double* __restrict__ hi_, double gtol, int max_iter, double* scratch,
                                                       double* __restrict__ X_out, double* __restrict__ mean_out,
                                                       double* __restrict__ var_out, int* __restrict__ iters,
                                                       int* __restrict__ evals, int* __restrict__ status) {
#pragma clang fp contract(off)
  extern __shared__ double pg_dyn[];
  __shared__ PgWork W;
  __shared__ PgBfgs Bf;
  const int tid = threadIdx.x, s = blockIdx.x;
  const bool wantv = kappa != 0.0;
  if (tid < d) {
    Bf.lo[tid] = lo_[tid];
    Bf.hi[tid] = hi_[tid];
    double v = X0[(size_t)s * d + tid];
    v = v < Bf.lo[tid] ? Bf.lo[tid] : (v > Bf.hi[tid] ? Bf.hi[tid] : v);
    Bf.x[tid] = v;
    W.x[tid] = v;
    W.il[tid] = 1.0 / exp(h[1 + tid]);
  }
  const double cst = exp(h[0]);
  const double kdiag = kb_with_constant<FORM>(cst, 1.0) + exp(h[d + 1]);
  double *kb, *gb;
  pg_rows(pg_dyn, scratch, n, npad, s, kb, gb);
  int it, nev;
  const int st = pg_bfgs(
      Bf, W.x, d, gtol, max_iter, [&] { pg_eval<STAT, FORM>(X, n, d, alpha, Kinv, npad, cst, kdiag, wantv, kb, gb, W); },
      [&] { return pg_objective(W, y_mean, y_std, kappa); }, [&](int t) { return pg_gradient(W, t, y_std, kappa); }, it, nev);
  // the moments at the end point, variance included: the bits bgp_predict_grad_batch returns there
  if (tid < d) W.x[tid] = Bf.x[tid];
  pg_eval<STAT, FORM>(X, n, d, alpha, Kinv, npad, cst, kdiag, true, kb, gb, W);
  nev++;
  if (tid < d) X_out[(size_t)s * d + tid] = Bf.x[tid];
  if (tid == 0) {
    mean_out[s] = W.mean;
    var_out[s] = W.var;
    iters[s] = it;
    evals[s] = nev;
    status[s] = st;
  }
}

static int pg_check(bgp_ctx* c, const char* who) {
  if (c->d > PG_DMAX || c->has_warp) {
    bgp_set_error("%s: %s", who, c->has_warp ? "warped inputs are not supported" : "d > 32 is not supported");
    return BGP_ERR_INVALID;
  }
  return BGP_OK;
}

extern "C" int bgp_predict_grad_batch(bgp_ctx* c, int B, const double* h_kernel, int m, const double* Xq, double* mean,
                                      double* var, double* dmean, double* dvar) {
  BGP_TRY(bgp_guard(c, "bgp_predict_grad_batch", BGP_POST_PLAIN));
  if (!c || !h_kernel || !Xq || !mean || !var || !dmean || m <= 0 || B <= 0) {
    bgp_set_error("bgp_predict_grad_batch: bad argument");
    return BGP_ERR_INVALID;
  }
  BGP_TRY(pg_check(c, "bgp_predict_grad_batch"));
  BGP_TRY(bgp_guard(c, "bgp_predict_grad_batch", BGP_POST_PLAIN, B));
  return post_call(c, [&]() -> int {
    const int n = c->n, d = c->d, npad = c->npad;
    const size_t p = d + 2;
    const bool lds = n <= PG_NLDS;
    // chunks of query rows: outputs of B mc (2 + 2 d) doubles, and B mc scratch rows of 2 npad doubles beyond PG_NLDS points
    size_t mc = std::min<size_t>((size_t)m, 65535);
    mc = std::min(mc, std::max<size_t>(1, ((size_t)1 << 24) / ((size_t)B * (2 + 2 * (size_t)d))));
    if (!lds) mc = std::min(mc, std::max<size_t>(1, ((size_t)1 << 26) / ((size_t)B * 2 * npad)));
    mc = bgp_switch_cap(BGP_SW_ROW_CHUNK, mc);  // (tests: forced row chunks against the default)
    const size_t Bm = (size_t)B * mc;
    double *dXq, *dH, *dm, *dv, *ddm, *ddv, *rows = nullptr;
    BgpScratch live(c);
    int rc = live.carve([&](BgpCarve& s) {
      dXq = s.take<double>(mc * d);
      dH = s.take<double>(B * p);
      dm = s.take<double>(Bm);
      dv = s.take<double>(Bm);
      ddm = s.take<double>(Bm * d);
      ddv = s.take<double>(Bm * d);
      if (!lds) rows = s.take<double>(Bm * 2 * npad);
    });
    if (rc) return rc;
    const size_t shmem = lds ? 2 * (size_t)n * sizeof(double) : 0;
    BGP_HIP(bgp_memcpy_async(dH, h_kernel, B * p * sizeof(double), hipMemcpyHostToDevice, c->stream));
    c->chunk_last[0] = 1, c->chunk_last[1] = 0;
    for (size_t m0 = 0; m0 < (size_t)m; m0 += mc) {
      const int mm = (int)std::min(mc, (size_t)m - m0);
      c->chunk_last[1]++;
      BGP_HIP(bgp_memcpy_async(dXq, Xq + m0 * d, (size_t)mm * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
      KB_DISPATCH(c->ks.stationary, c->ks.form,
                  hipLaunchKernelGGL((pg_rows_kernel<S, F>), dim3(mm, B), dim3(PG_NT), shmem, c->stream, c->dXeff, n, d, npad,
                                     c->dalpha_sol, c->dKinv, dH, dXq, mm, rows, dm, dv, ddm, dvar ? ddv : nullptr));
      BGP_HIP(hipGetLastError());
      const size_t w1 = (size_t)mm * sizeof(double), wd = (size_t)mm * d * sizeof(double);
      BGP_HIP(bgp_memcpy2d_async(mean + m0, (size_t)m * sizeof(double), dm, w1, w1, B, hipMemcpyDeviceToHost, c->stream));
      BGP_HIP(bgp_memcpy2d_async(var + m0, (size_t)m * sizeof(double), dv, w1, w1, B, hipMemcpyDeviceToHost, c->stream));
      BGP_HIP(bgp_memcpy2d_async(dmean + m0 * d, (size_t)m * d * sizeof(double), ddm, wd, wd, B, hipMemcpyDeviceToHost, c->stream));
      if (dvar)
        BGP_HIP(bgp_memcpy2d_async(dvar + m0 * d, (size_t)m * d * sizeof(double), ddv, wd, wd, B, hipMemcpyDeviceToHost, c->stream));
      BGP_HIP(bgp_stream_sync(c->stream));  // (the next chunk reuses the buffers)
    }
    return BGP_OK;
  });
}

extern "C" int bgp_minimize_starts(bgp_ctx* c, int b, const double* h_kernel, double y_mean, double y_std, double kappa, int S_,
                                   const double* X0, const double* lo, const double* hi, double gtol, int max_iter, double* X_out,
                                   double* mean_out, double* var_out, int* iters, int* evals, int* status) {
  BGP_TRY(bgp_guard(c, "bgp_minimize_starts", BGP_POST_PLAIN));
  if (!c || !h_kernel || !X0 || !lo || !hi || !X_out || !mean_out || !var_out || !iters || !evals || !status || S_ <= 0 ||
      S_ > 65535 || b < 0 || max_iter < 0 || !(gtol >= 0.0)) {
    bgp_set_error("bgp_minimize_starts: bad argument");
    return BGP_ERR_INVALID;
  }
  BGP_TRY(pg_check(c, "bgp_minimize_starts"));
  for (int t = 0; t < c->d; t++)
    if (!(lo[t] <= hi[t])) {
      bgp_set_error("bgp_minimize_starts: empty box in dimension %d", t);
      return BGP_ERR_INVALID;
    }
  BGP_TRY(bgp_guard(c, "bgp_minimize_starts", BGP_POST_PLAIN, b + 1));
  return post_call(c, [&]() -> int {
    const int n = c->n, d = c->d, npad = c->npad;
    const size_t p = d + 2, Sd = (size_t)S_ * d;
    const bool lds = n <= PG_NLDS;
    double *dH, *dX0, *dXo, *dlo, *dhi, *dm, *dv, *rows = nullptr;
    int *dit, *dev, *dst;
    BgpScratch live(c);
    int rc = live.carve([&](BgpCarve& s) {
      dH = s.take<double>(p);
      dX0 = s.take<double>(Sd);
      dXo = s.take<double>(Sd);
      dlo = s.take<double>(d);
      dhi = s.take<double>(d);
      dm = s.take<double>(S_);
      dv = s.take<double>(S_);
      dit = s.take<int>(S_);
      dev = s.take<int>(S_);
      dst = s.take<int>(S_);
      if (!lds) rows = s.take<double>((size_t)S_ * 2 * npad);
    });
    if (rc) return rc;
    const size_t shmem = lds ? 2 * (size_t)n * sizeof(double) : 0;
    hipStream_t st = c->stream;
    BGP_HIP(bgp_memcpy_async(dH, h_kernel, p * sizeof(double), hipMemcpyHostToDevice, st));
    BGP_HIP(bgp_memcpy_async(dX0, X0, Sd * sizeof(double), hipMemcpyHostToDevice, st));
    BGP_HIP(bgp_memcpy_async(dlo, lo, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
    BGP_HIP(bgp_memcpy_async(dhi, hi, (size_t)d * sizeof(double), hipMemcpyHostToDevice, st));
    KB_DISPATCH(c->ks.stationary, c->ks.form,
                hipLaunchKernelGGL((pg_min_kernel<S, F>), dim3(S_), dim3(PG_NT), shmem, st, c->dXeff, n, d, npad,
                                   c->dalpha_sol + (size_t)b * npad, c->dKinv + (size_t)b * npad * npad, dH, y_mean, y_std, kappa, dX0,
                                   dlo, dhi, gtol, max_iter, rows, dXo, dm, dv, dit, dev, dst));
    BGP_HIP(hipGetLastError());
    BGP_HIP(bgp_memcpy_async(X_out, dXo, Sd * sizeof(double), hipMemcpyDeviceToHost, st));
    BGP_HIP(bgp_memcpy_async(mean_out, dm, (size_t)S_ * sizeof(double), hipMemcpyDeviceToHost, st));
    BGP_HIP(bgp_memcpy_async(var_out, dv, (size_t)S_ * sizeof(double), hipMemcpyDeviceToHost, st));
    BGP_HIP(bgp_memcpy_async(iters, dit, (size_t)S_ * sizeof(int), hipMemcpyDeviceToHost, st));
    BGP_HIP(bgp_memcpy_async(evals, dev, (size_t)S_ * sizeof(int), hipMemcpyDeviceToHost, st));
    BGP_HIP(bgp_memcpy_async(status, dst, (size_t)S_ * sizeof(int), hipMemcpyDeviceToHost, st));
    BGP_HIP(bgp_stream_sync(st));
    return BGP_OK;
  });
}
