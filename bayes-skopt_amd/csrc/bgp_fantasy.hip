// Batch proposals by fantasy conditioning (Optimizer.ask(n_points > 1)).
//
// The B resident posteriors of the last proposal (K_b^-1, bgp_posterior_batch) are conditioned, one chosen candidate at a
// time, on a fantasy observation (the "lie"); the latent predictive means / variances at the m candidates are updated by
// the rank-1 identities of the bordered inverse instead of refactorising the augmented training set:
//   w_b        = K_b^-1 k_b(X, x_p)
//   c_b(i)     = k_b(x_i, x_p) - sum_k k_b(x_k, x_i) w_b[k] - sum_{l<j} u_{b,l}(i) u_{b,l}(p)     (latent covariance)
//   s_b        = c_b(p) + noise_b                                                                 (noisy variance of x_p)
//   u_{b,j}(i) = c_b(i) / sqrt(s_b) ;  var_b(i) -= u_{b,j}(i)^2 ;  mu_b(i) += u_{b,j}(i) (lie_b - mu_b(p)) / sqrt(s_b)
// The sum over the training points is a GEMV against the cross-kernel matrix K_b(X, cand) GENERATED on the fly, tile by
// tile from LDS (that matrix is B n m doubles: 10 GB at 128 draws x 974 points x 10 000 candidates, it never goes to HBM).
// The acquisition closed forms and the fixed-order average over the draws are bgp_acq_batch's kernels (bgp_post.hip),
// the argmax over the candidates not yet chosen is one workgroup: only the index (and optionally the m averaged values)
// comes back.  Every reduction has a fixed order; the only atomics are bgp_acq_batch's integer "row not finite" flags.
#include <memory>

#include "bgp_common.h"
#include "bgp_device.h"

#define FT_TP 64       // training points per LDS tile of the generated GEMV
#define FT_DMAX 32     // input dimensions the generated GEMV stages (larger d: the caller's fallback path)

struct bgp_fantasy_state {
  int B = 0, m = 0, mpad = 0, qmax = 0, j = 0, n_acq = 0, n_samples = 1, post_gen = 0;
  double y_mean = 0.0, y_std = 1.0;
  int kinds[BGP_ACQ_MAX] = {0};
  double params[BGP_ACQ_MAX] = {0};
  BgpDev<char> mem;  // one allocation, carved by bgp_fantasy_begin
  double *dXc, *dH, *dnoise, *dmu, *dvar, *dU, *dkp, *dw, *dc, *dpv, *dT, *dacc, *dmumin, *dparams;
  int *dbad, *dkinds, *dchosen, *dnext;
};

static void fantasy_free(bgp_ctx* c) {
  if (!c->fantasy) return;
  if (c->fantasy->mem) (void)hipStreamSynchronize(c->stream);
  delete c->fantasy;
  c->fantasy = nullptr;
}

void bgp_fantasy_abandon(bgp_ctx* c) { fantasy_free(c); }

// kp_b[k] = k_b(x_k, x_p) for the n training points (zero padding up to npad): x / l, (a - b)^2 accumulated with fma in
// ascending dimension, kb_value (bgp_device.h) -- the cross kernel's entries
template <int STAT, int FORM>
__global__ void __launch_bounds__(256) fant_kp_kernel(const double* __restrict__ X, int n, int npad, int d,
                                                      const double* __restrict__ Xc, int p, const double* __restrict__ H,
                                                      double* __restrict__ kp) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (k >= npad) return;
  const double* h = H + (size_t)b * (d + 2);
  double v = 0.0;
  if (k < n) {
    double r2 = 0.0;
    for (int t = 0; t < d; t++) {
      const double l = exp(h[1 + t]);
      const double df = Xc[(size_t)p * d + t] / l - X[(size_t)k * d + t] / l;
      r2 = fma(df, df, r2);
    }
    v = kb_value<STAT, FORM>(r2, exp(h[0]));
  }
  kp[(size_t)b * npad + k] = v;
}

// w_b = K_b^-1 kp_b: one wave per row (rows of the symmetric inverse are contiguous), lanes over the columns in a fixed
// stride, the 64 partial sums reduced by a fixed butterfly
__global__ void __launch_bounds__(256) fant_w_kernel(const double* __restrict__ Kinv, int n, int npad,
                                                     const double* __restrict__ kp, double* __restrict__ w) {
#pragma clang fp contract(off)
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, b = blockIdx.y;
  if (row >= npad) return;
  const double* K = Kinv + ((size_t)b * npad + row) * npad;
  const double* v = kp + (size_t)b * npad;
  double s = 0.0;
  if (row < n)
    for (int k = lane; k < n; k += 64) s = fma(K[k], v[k], s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) w[(size_t)b * npad + row] = (row < n) ? s : 0.0;
}

// c_b(i), one candidate per thread, 256 candidates of draw b per workgroup.  The candidate's scaled inputs live in
// registers (the loops over FT_DMAX are unrolled, the guard t < d keeps them register-indexed); each tile of FT_TP scaled
// training points and their w entries is staged in LDS once and read by every thread as a broadcast.  fp64 VALU work only
// (no MFMA shape: one GEMV per draw), sized for occupancy: 16 KB of LDS and no spills at 256 threads.  The sum over the
// training points runs in ascending order.
template <int STAT, int FORM>
__global__ void __launch_bounds__(256) fant_col_kernel(const double* __restrict__ X, int n, int npad, int d,
                                                       const double* __restrict__ Xc, int m, int mpad, int p,
                                                       const double* __restrict__ H, const double* __restrict__ w,
                                                       const double* __restrict__ U, int j, int B,
                                                       double* __restrict__ cout) {
#pragma clang fp contract(off)
  __shared__ double xt[FT_TP * FT_DMAX];
  __shared__ double wt[FT_TP];
  __shared__ double ell[FT_DMAX];
  const int tid = threadIdx.x, b = blockIdx.y, i = blockIdx.x * 256 + tid;
  const double* h = H + (size_t)b * (d + 2);
  const double cst = exp(h[0]);
  if (tid < d) ell[tid] = exp(h[1 + tid]);
  __syncthreads();
  const int ii = (i < m) ? i : m - 1;  // (threads past the end compute a duplicate and store nothing)
  double xi[FT_DMAX];
  double r2 = 0.0;
#pragma unroll
  for (int t = 0; t < FT_DMAX; t++)
    if (t < d) {
      xi[t] = Xc[(size_t)ii * d + t] / ell[t];
      const double df = xi[t] - Xc[(size_t)p * d + t] / ell[t];
      r2 = fma(df, df, r2);
    }
  // k_b(x_i, x_p)
  const double kip = kb_value<STAT, FORM>(r2, cst);
  // sum_k k_b(x_k, x_i) w_b[k], generated tile by tile
  double acc = 0.0;
  const double* wb = w + (size_t)b * npad;
  for (int k0 = 0; k0 < n; k0 += FT_TP) {
    const int kc = min(FT_TP, n - k0);
    __syncthreads();
    for (int idx = tid; idx < kc * d; idx += 256) {
      const int r = idx / d, t = idx - r * d;
      xt[r * FT_DMAX + t] = X[(size_t)(k0 + r) * d + t] / ell[t];
    }
    if (tid < kc) wt[tid] = wb[k0 + tid];
    __syncthreads();
    for (int r = 0; r < kc; r++) {
      double q = 0.0;
#pragma unroll
      for (int t = 0; t < FT_DMAX; t++)
        if (t < d) {
          const double df = xi[t] - xt[r * FT_DMAX + t];
          q = fma(df, df, q);
        }
      acc = fma(kb_value<STAT, FORM>(q, cst), wt[r], acc);
    }
  }
  if (i >= m) return;
  // earlier fantasies: sum_{l<j} u_{b,l}(i) u_{b,l}(p), in order
  double prev = 0.0;
  for (int l = 0; l < j; l++) {
    const double* ul = U + ((size_t)l * B + b) * mpad;
    prev = fma(ul[i], ul[p], prev);
  }
  cout[(size_t)b * mpad + i] = (kip - acc) - prev;
}

// the pivot values every thread of the update needs, read before anyone writes: pv[b] = {c_b(p), mu_b(p)}
__global__ void fant_pivot_kernel(const double* __restrict__ cvals, const double* __restrict__ mu, int mpad, int p, int B,
                                  double* __restrict__ pv, int* __restrict__ chosen) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b == 0) chosen[p] = 1;
  if (b >= B) return;
  pv[2 * b] = cvals[(size_t)b * mpad + p];
  pv[2 * b + 1] = mu[(size_t)b * mpad + p];
}

// rank-1 update of draw b's latent means / variances; lie_kb != 0: kriging believer (lie = the draw's own mean, the
// means are left as they are)
__global__ void __launch_bounds__(256) fant_update_kernel(const double* __restrict__ cvals, const double* __restrict__ pv,
                                                          const double* __restrict__ noise, int m, int mpad, int B, int j,
                                                          int lie_kb, double lie, double* __restrict__ U,
                                                          double* __restrict__ mu, double* __restrict__ var) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= mpad) return;
  const double rs = sqrt(pv[2 * b] + noise[b]);
  const double u = (i < m) ? cvals[(size_t)b * mpad + i] / rs : 0.0;
  U[((size_t)j * B + b) * mpad + i] = u;
  if (i >= m) return;
  const size_t o = (size_t)b * mpad + i;
  const double v = var[o] - u * u;
  var[o] = v > 0.0 ? v : 0.0;  // (clipped at 0 as bgp_predict_batch clips)
  if (!lie_kb) mu[o] = mu[o] + u * ((lie - pv[2 * b + 1]) / rs);
}

// argmax over the candidates not chosen yet (np.argmax order: NaN wins, then the larger value, ties to the lower index)
static __device__ __forceinline__ bool ft_better(double a, int ia, double b, int ib) {
  const bool na = isnan(a), nb = isnan(b);
  if (ib < 0) return ia >= 0;
  if (ia < 0) return false;
  if (na != nb) return na;
  if (!na && a != b) return a > b;
  return ia < ib;
}
__global__ void __launch_bounds__(1024) fant_argmax_kernel(const double* __restrict__ acc, const int* __restrict__ chosen, int m,
                                                           int* __restrict__ next) {
  __shared__ double sv[1024];
  __shared__ int si[1024];
  const int tid = threadIdx.x;
  double best = 0.0;
  int bi = -1;
  for (int i = tid; i < m; i += 1024)
    if (!chosen[i] && ft_better(acc[i], i, best, bi)) best = acc[i], bi = i;
  sv[tid] = best, si[tid] = bi;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o && ft_better(sv[tid + o], si[tid + o], sv[tid], si[tid])) sv[tid] = sv[tid + o], si[tid] = si[tid + o];
    __syncthreads();
  }
  if (tid == 0) *next = si[0];
}

extern "C" int bgp_fantasy_begin(bgp_ctx* c, int B, const double* h_kernel, const double* noise, int m, const double* Xcand,
                                 double y_mean, double y_std, int n_acq, const int* kinds, const double* params, int n_samples,
                                 int qmax) {
  BGP_TRY(bgp_guard(c, "bgp_fantasy_begin", BGP_POST_PLAIN));
  if (!c || !h_kernel || !noise || !Xcand || !kinds || !params || B <= 0 || m <= 0 || qmax <= 0 || n_samples <= 0 ||
      n_acq <= 0 || n_acq > BGP_ACQ_MAX) {
    bgp_set_error("bgp_fantasy_begin: bad argument");
    return BGP_ERR_INVALID;
  }
  for (int k = 0; k < n_acq; k++)
    if (kinds[k] < BGP_ACQ_EI || kinds[k] > BGP_ACQ_STD) {
      bgp_set_error("bgp_fantasy_begin: unknown acquisition kind %d", kinds[k]);
      return BGP_ERR_INVALID;
    }
  if (qmax >= m) {  // (every step chooses a candidate not chosen before: at most m - 1 steps after the first point)
    bgp_set_error("bgp_fantasy_begin: qmax = %d steps need more than %d candidates", qmax, m);
    return BGP_ERR_INVALID;
  }
  if (c->d > FT_DMAX || c->has_warp) {
    bgp_set_error("bgp_fantasy_begin: %s", c->has_warp ? "warped inputs are not supported" : "d > 32 is not supported");
    return BGP_ERR_INVALID;
  }
  BGP_TRY(bgp_guard(c, "bgp_fantasy_begin", BGP_POST_PLAIN, B));
  fantasy_free(c);  // (whatever happens below, the previous batch is over)
  return post_call(c, [&]() -> int {
    // the starting means / variances: bgp_predict_batch itself (the same bits as the proposal's bgp_acq_batch saw); a complete call
    // of its own, outside this body's carve
    std::vector<double> mean((size_t)B * m), var((size_t)B * m);
    BGP_TRY(bgp_predict_batch(c, B, h_kernel, m, Xcand, mean.data(), var.data(), nullptr));
    std::unique_ptr<bgp_fantasy_state> st(new bgp_fantasy_state());
    bgp_fantasy_state* f = st.get();
    const int d = c->d, npad = c->npad, mpad = ((m + 255) / 256) * 256;
    f->B = B, f->m = m, f->mpad = mpad, f->qmax = qmax, f->j = 0, f->n_acq = n_acq, f->n_samples = n_samples;
    f->y_mean = y_mean, f->y_std = y_std, f->post_gen = c->post.gen();
    for (int k = 0; k < n_acq; k++) f->kinds[k] = kinds[k], f->params[k] = params[k];
    const size_t Bm = (size_t)B * mpad;
    BGP_TRY(bgp_carve(f->mem, 16, [&](BgpCarve& s) {
      f->dXc = s.take<double>((size_t)m * d);
      f->dH = s.take<double>((size_t)B * (d + 2));
      f->dnoise = s.take<double>(B);
      f->dmu = s.take<double>(Bm);
      f->dvar = s.take<double>(Bm);
      f->dU = s.take<double>((size_t)qmax * Bm);
      f->dkp = s.take<double>((size_t)B * npad);
      f->dw = s.take<double>((size_t)B * npad);
      f->dc = s.take<double>(Bm);
      f->dpv = s.take<double>(2 * (size_t)B);
      f->dT = s.take<double>((size_t)n_acq * Bm);
      f->dacc = s.take<double>((size_t)n_acq * mpad);
      f->dmumin = s.take<double>((size_t)B + BGP_ACQ_MAX);
      f->dparams = s.take<double>(BGP_ACQ_MAX);
      f->dbad = s.take<int>((size_t)n_acq * B + BGP_ACQ_MAX);
      f->dkinds = s.take<int>(BGP_ACQ_MAX);
      f->dchosen = s.take<int>(mpad);
      f->dnext = s.take<int>(1);
    }));
    BGP_HIP(hipMemsetAsync(f->mem, 0, f->mem.cap, c->stream));  // (a fresh block: exactly the layout's bytes)
    BGP_HIP(bgp_memcpy_async(f->dXc, Xcand, (size_t)m * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BGP_HIP(bgp_memcpy_async(f->dH, h_kernel, (size_t)B * (d + 2) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BGP_HIP(bgp_memcpy_async(f->dnoise, noise, (size_t)B * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BGP_HIP(bgp_memcpy_async(f->dparams, params, (size_t)n_acq * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BGP_HIP(bgp_memcpy_async(f->dkinds, kinds, (size_t)n_acq * sizeof(int), hipMemcpyHostToDevice, c->stream));
    BGP_HIP(bgp_memcpy2d_async(f->dmu, (size_t)mpad * sizeof(double), mean.data(), (size_t)m * sizeof(double),
                               (size_t)m * sizeof(double), B, hipMemcpyHostToDevice, c->stream));
    BGP_HIP(bgp_memcpy2d_async(f->dvar, (size_t)mpad * sizeof(double), var.data(), (size_t)m * sizeof(double),
                               (size_t)m * sizeof(double), B, hipMemcpyHostToDevice, c->stream));
    BGP_HIP(bgp_stream_sync(c->stream));  // (the host vectors above are staged; the state is complete)
    c->fantasy = st.release();
    c->fant_stats[0]++;
    return BGP_OK;
  });
}

extern "C" int bgp_fantasy_step(bgp_ctx* c, int p, int lie_kind, double lie_value, int* next, double* values) {
  BGP_TRY(bgp_guard(c, "bgp_fantasy_step"));
  if (!c || !next) {
    bgp_set_error("bgp_fantasy_step: bad argument");
    return BGP_ERR_INVALID;
  }
  bgp_fantasy_state* f = c->fantasy;
  if (!f) {
    bgp_set_error("bgp_fantasy_step: no fantasy state (call bgp_fantasy_begin first)");
    return BGP_ERR_STATE;
  }
  if (f->post_gen != c->post.gen() || f->B > c->post.B()) {
    bgp_set_error("bgp_fantasy_step: the resident posteriors changed since bgp_fantasy_begin");
    return BGP_ERR_STATE;
  }
  if (p < 0 || p >= f->m || f->j >= f->qmax || (lie_kind != BGP_LIE_VALUE && lie_kind != BGP_LIE_KB)) {
    bgp_set_error("bgp_fantasy_step: bad argument (p = %d of %d, step %d of %d, lie_kind %d)", p, f->m, f->j, f->qmax,
                  lie_kind);
    return BGP_ERR_INVALID;
  }
  return post_call(c, [&]() -> int {
    const int B = f->B, m = f->m, mpad = f->mpad, n = c->n, npad = c->npad, d = c->d;
    hipStream_t st = c->stream;
    KB_DISPATCH(c->ks.stationary, c->ks.form,
                hipLaunchKernelGGL((fant_kp_kernel<S, F>), dim3((npad + 255) / 256, B), dim3(256), 0, st, c->dXeff, n, npad, d,
                                   f->dXc, p, f->dH, f->dkp));
    hipLaunchKernelGGL(fant_w_kernel, dim3((npad + 3) / 4, B), dim3(256), 0, st, c->dKinv, n, npad, f->dkp, f->dw);
    KB_DISPATCH(c->ks.stationary, c->ks.form,
                hipLaunchKernelGGL((fant_col_kernel<S, F>), dim3(mpad / 256, B), dim3(256), 0, st, c->dXeff, n, npad, d, f->dXc,
                                   m, mpad, p, f->dH, f->dw, f->dU, f->j, B, f->dc));
    hipLaunchKernelGGL(fant_pivot_kernel, dim3((B + 255) / 256), dim3(256), 0, st, f->dc, f->dmu, mpad, p, B, f->dpv,
                       f->dchosen);
    hipLaunchKernelGGL(fant_update_kernel, dim3(mpad / 256, B), dim3(256), 0, st, f->dc, f->dpv, f->dnoise, m, mpad, B, f->j,
                       lie_kind == BGP_LIE_KB ? 1 : 0, lie_value, f->dU, f->dmu, f->dvar);
    // closed forms + average over the draws (bgp_acq_batch's kernels), then the argmax of the first acquisition
    BGP_HIP(hipMemsetAsync(f->dbad, 0, (size_t)f->n_acq * B * sizeof(int), st));
    hipLaunchKernelGGL(acq_mumin_kernel, dim3(B), dim3(256), 0, st, f->dmu, (size_t)mpad, m, f->y_mean, f->y_std, f->dmumin);
    hipLaunchKernelGGL(acq_values_kernel, dim3((m + 255) / 256, B), dim3(256), 0, st, f->dmu, f->dvar, (size_t)mpad, m, B,
                       f->y_mean, f->y_std, f->n_acq, f->dkinds, f->dparams, f->dmumin, f->dT, f->dbad);
    hipLaunchKernelGGL(acq_sum_kernel, dim3((m + 255) / 256, f->n_acq), dim3(256), 0, st, f->dT, f->dbad, (size_t)mpad, m, B,
                       f->n_samples, f->dacc);
    hipLaunchKernelGGL(fant_argmax_kernel, dim3(1), dim3(1024), 0, st, f->dacc, f->dchosen, m, f->dnext);
    BGP_HIP(hipGetLastError());
    BGP_HIP(bgp_memcpy_async(next, f->dnext, sizeof(int), hipMemcpyDeviceToHost, st));
    if (values)
      BGP_HIP(bgp_memcpy2d_async(values, (size_t)m * sizeof(double), f->dacc, (size_t)mpad * sizeof(double),
                                 (size_t)m * sizeof(double), f->n_acq, hipMemcpyDeviceToHost, st));
    BGP_HIP(bgp_stream_sync(st));
    f->j++;
    c->fant_stats[1]++;
    return BGP_OK;
  });
}

extern "C" int bgp_fantasy_moments(bgp_ctx* c, double* mean, double* var) {
  BGP_TRY(bgp_guard(c, "bgp_fantasy_moments"));
  if (!c || !mean || !var) {
    bgp_set_error("bgp_fantasy_moments: bad argument");
    return BGP_ERR_INVALID;
  }
  bgp_fantasy_state* f = c->fantasy;
  if (!f) {
    bgp_set_error("bgp_fantasy_moments: no fantasy state (call bgp_fantasy_begin first)");
    return BGP_ERR_STATE;
  }
  return post_call(c, [&]() -> int {
    const size_t row = (size_t)f->m * sizeof(double), pitch = (size_t)f->mpad * sizeof(double);
    BGP_HIP(bgp_memcpy2d_async(mean, row, f->dmu, pitch, row, f->B, hipMemcpyDeviceToHost, c->stream));
    BGP_HIP(bgp_memcpy2d_async(var, row, f->dvar, pitch, row, f->B, hipMemcpyDeviceToHost, c->stream));
    BGP_HIP(bgp_stream_sync(c->stream));
    return BGP_OK;
  });
}

extern "C" int bgp_fantasy_end(bgp_ctx* c) {
  if (!c) {
    bgp_set_error("bgp_fantasy_end: NULL ctx");
    return BGP_ERR_INVALID;
  }
  fantasy_free(c);
  return BGP_OK;
}

extern "C" int bgp_fantasy_stats(bgp_ctx* c, long long* out) {
  if (!c || !out) {
    bgp_set_error("bgp_fantasy_stats: bad argument");
    return BGP_ERR_INVALID;
  }
  out[0] = c->fant_stats[0];
  out[1] = c->fant_stats[1];
  return BGP_OK;
}
