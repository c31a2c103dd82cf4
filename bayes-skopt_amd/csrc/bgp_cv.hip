// Cross-validation of the surrogate from the resident inverses: the predictive of held-out OBSERVATIONS
// y_F given the remaining ones, for any index set F, without a refit.  With A = K^-1 (K with its alpha diagonal and white level, as
// every posterior build leaves it in dKinv) and a = A y (dalpha_sol):
//   Sigma_F = (A_FF)^-1,   r_F = Sigma_F a_F,   mu_F = y_F - r_F,   var_i = (Sigma_F)_ii
//   lpd_F   = -1/2 a_F^T r_F + sum_k log C_kk - (s / 2) log 2 pi,    A_FF = C C^T,  s = |F|
// Neither X nor the kernel is read: plain, per-row-warped and host-Gram posteriors alike.
//
// cv_fold_kernel: one workgroup per (posterior, fold).  A_FF (lower triangle) and a_F are gathered into LDS, A_FF is factorised
// there column by column (right-looking; the pivot's root and reciprocal root by pf_pivot_root), M = C^-1 is formed column by column
// -- one thread per column, which nobody else reads or writes -- into the unused strict upper triangle of the same array
// (M[k][c], k > c, at S[c][k]; its diagonal is the reciprocal roots), then w = M a_F, r_F = M^T w and var_i = sum_k M[k][i]^2, one
// thread per entry, every sum in ascending index order.  The leading dimension is the call's largest fold rounded up to an odd number:
// a column walk (stride ld) touches every bank pair once per 32 lanes, the walk along M's columns (stride ld + 1) costs two LDS cycles.
// LDS: smax ld + 5 smax doubles + smax ints (dynamic; 137.7 KB at 128 points), so folds of 100 points do not pay for 128.
// cv_loo_kernel: every fold has one point -- one THREAD per (posterior, point) on the inverse's diagonal, the same operations.
// Plain launches, no workgroup waits for another, no atomics; a (posterior, fold) result depends on that posterior and that fold alone.
#include "bgp_common.h"
#include "bgp_device.h"
#include "bgp_pf.h"

#include <algorithm>

#define CV_SMAX 128                        // points per fold (one workgroup's LDS holds A_FF and C^-1)
#define CV_HALF_LOG_2PI 0.9189385332046727  // log(2 pi) / 2

// the strict upper triangle of the fold's LDS array holds M = C^-1 transposed
static __device__ __forceinline__ bool cv_pivot_ok(double p) { return p > 0.0 && p < INFINITY; }

__global__ void __launch_bounds__(256) cv_fold_kernel(const double* __restrict__ Kinv, const double* __restrict__ alpha,
                                                      const double* __restrict__ y, const int* __restrict__ fold_ptr,
                                                      const int* __restrict__ fold_idx, int n, int npad, int n_folds, int smax,
                                                      double* __restrict__ mean, double* __restrict__ var, double* __restrict__ lpd,
                                                      int* __restrict__ status) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char cv_dyn[];
  const int ld = smax | 1;
  double* S = (double*)cv_dyn;       // smax x ld: A_FF -> C in the lower triangle, M^T in the strict upper one
  double* av = S + (size_t)smax * ld;  // a_F
  double* dd = av + smax;              // C_kk, later log C_kk
  double* di = dd + smax;              // 1 / C_kk = M_kk
  double* w = di + smax;               // M a_F
  double* r = w + smax;                // r_F
  int* ix = (int*)(r + smax);          // the fold's indices
  const int tid = threadIdx.x, f = blockIdx.x, b = blockIdx.y;
  const int p0 = fold_ptr[f], s = fold_ptr[f + 1] - p0;
  const double* A = Kinv + (size_t)b * npad * npad;
  const double* ab = alpha + (size_t)b * npad;
  for (int i = tid; i < s; i += 256) {
    const int g = fold_idx[p0 + i];
    ix[i] = g;
    av[i] = ab[g];
  }
  __syncthreads();
  for (int i = tid >> 5; i < s; i += 8) {
    const double* Ai = A + (size_t)ix[i] * npad;
    for (int k = tid & 31; k <= i; k += 32) S[i * ld + k] = Ai[ix[k]];
  }
  __syncthreads();
  // A_FF = C C^T, right-looking: every thread reads the same pivot, so the exit at a failed one is uniform
  int fail = 0;
  for (int j = 0; j < s; j++) {
    const double p = S[j * ld + j];
    if (!cv_pivot_ok(p)) {
      fail = j + 1;
      break;
    }
    double dj, inv;
    pf_pivot_root(p, dj, inv);
    if (tid == 0) dd[j] = dj, di[j] = inv;
    for (int i = j + 1 + tid; i < s; i += 256) S[i * ld + j] *= inv;
    __syncthreads();
    for (int i = j + 1 + (tid >> 5); i < s; i += 8) {
      const double nl = -S[i * ld + j];
      for (int k = j + 1 + (tid & 31); k <= i; k += 32) S[i * ld + k] = fma(nl, S[k * ld + j], S[i * ld + k]);
    }
    __syncthreads();
  }
  if (fail) {  // (mean and var of the fold's points keep the NaN they were filled with)
    if (tid == 0) {
      lpd[(size_t)b * n_folds + f] = NAN;
      status[(size_t)b * n_folds + f] = fail;
    }
    return;
  }
  // column c of M = C^-1 by forward substitution: M[i][c] = -(sum_{c <= k < i} C[i][k] M[k][c]) / C[i][i]
  if (tid < s) {
    const int c = tid;
    const double mcc = di[c];
    for (int i = c + 1; i < s; i++) {
      double acc = S[i * ld + c] * mcc;
      for (int k = c + 1; k < i; k++) acc = fma(S[i * ld + k], S[c * ld + k], acc);
      S[c * ld + i] = -(acc * di[i]);
    }
  }
  __syncthreads();
  if (tid < s) {  // w_k = sum_{c <= k} M[k][c] a_c
    const int k = tid;
    double acc = 0.0;
    for (int c = 0; c < k; c++) acc = fma(S[c * ld + k], av[c], acc);
    w[k] = fma(di[k], av[k], acc);
  }
  __syncthreads();
  if (tid < s) {  // r_i = sum_{k >= i} M[k][i] w_k,  var_i = sum_{k >= i} M[k][i]^2
    const int i = tid, g = ix[i];
    double acc = di[i] * w[i], v = di[i] * di[i];
    for (int k = i + 1; k < s; k++) {
      const double m = S[i * ld + k];
      acc = fma(m, w[k], acc);
      v = fma(m, m, v);
    }
    r[i] = acc;
    dd[i] = log(dd[i]);
    mean[(size_t)b * n + g] = y[g] - acc;
    var[(size_t)b * n + g] = v;
  }
  __syncthreads();
  if (tid == 0) {
    double q = 0.0, ldet = 0.0;
    for (int i = 0; i < s; i++) {
      q = fma(av[i], r[i], q);
      ldet += dd[i];
    }
    lpd[(size_t)b * n_folds + f] = (-0.5 * q + ldet) - (double)s * CV_HALF_LOG_2PI;
    status[(size_t)b * n_folds + f] = 0;
  }
}

// Every fold is one point: thread (b, f) on A_ii alone, with the operations the fold kernel applies to a 1 x 1 block.
__global__ void __launch_bounds__(256) cv_loo_kernel(const double* __restrict__ Kinv, const double* __restrict__ alpha,
                                                     const double* __restrict__ y, const int* __restrict__ fold_idx, int n, int npad,
                                                     int n_folds, double* __restrict__ mean, double* __restrict__ var,
                                                     double* __restrict__ lpd, int* __restrict__ status) {
#pragma clang fp contract(off)
  const int f = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (f >= n_folds) return;
  const int g = fold_idx[f];
  const double p = Kinv[(size_t)b * npad * npad + (size_t)g * npad + g], a = alpha[(size_t)b * npad + g];
  const size_t o = (size_t)b * n_folds + f;
  if (!cv_pivot_ok(p)) {
    lpd[o] = NAN;
    status[o] = 1;
    return;
  }
  double dj, inv;
  pf_pivot_root(p, dj, inv);
  const double w = inv * a, r = inv * w;
  mean[(size_t)b * n + g] = y[g] - r;
  var[(size_t)b * n + g] = inv * inv;
  lpd[o] = (-0.5 * (a * r) + log(dj)) - CV_HALF_LOG_2PI;
  status[o] = 0;
}

static size_t cv_lds_bytes(int smax) { return ((size_t)smax * (smax | 1) + 5 * (size_t)smax) * sizeof(double) + (size_t)smax * sizeof(int); }

static int cv_run(bgp_ctx* c, int B, int n_folds, const int* fold_ptr, const int* fold_idx, int smax, double* mean, double* var,
                  double* fold_lpd, int* status) {
  const int n = c->n, npad = c->npad, total = fold_ptr[n_folds];
  int *dptr, *didx, *dst;
  double *dmean, *dvar, *dlpd;
  BgpScratch live(c);
  BGP_TRY(live.carve([&](BgpCarve& s) {
    dptr = s.take<int>((size_t)n_folds + 1);
    didx = s.take<int>((size_t)total);
    dmean = s.take<double>((size_t)B * n);
    dvar = s.take<double>((size_t)B * n);
    dlpd = s.take<double>((size_t)B * n_folds);
    dst = s.take<int>((size_t)B * n_folds);
  }));
  hipStream_t st = c->stream;
  const double *Kinv = c->dKinv, *al = c->dalpha_sol, *dy = c->dy;
  BGP_HIP(bgp_memcpy_async(dptr, fold_ptr, ((size_t)n_folds + 1) * sizeof(int), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(didx, fold_idx, (size_t)total * sizeof(int), hipMemcpyHostToDevice, st));
  // points that no fold covers, and the points of a fold that fails, stay NaN (every byte 0xff is one)
  BGP_HIP(hipMemsetAsync(dmean, 0xff, (size_t)B * n * sizeof(double), st));
  BGP_HIP(hipMemsetAsync(dvar, 0xff, (size_t)B * n * sizeof(double), st));
  if (smax == 1) {
    hipLaunchKernelGGL(cv_loo_kernel, dim3((n_folds + 255) / 256, B), dim3(256), 0, st, Kinv, al, dy, didx, n, npad, n_folds, dmean,
                       dvar, dlpd, dst);
  } else {
    const size_t lds = cv_lds_bytes(smax);
    if (lds > 64 * 1024)  // (more dynamic LDS than the default limit has to be asked for)
      BGP_HIP(hipFuncSetAttribute((const void*)cv_fold_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(cv_fold_kernel, dim3(n_folds, B), dim3(256), lds, st, Kinv, al, dy, dptr, didx, n, npad, n_folds, smax, dmean,
                       dvar, dlpd, dst);
  }
  BGP_HIP(hipGetLastError());
  BGP_HIP(bgp_memcpy_async(mean, dmean, (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_memcpy_async(var, dvar, (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_memcpy_async(fold_lpd, dlpd, (size_t)B * n_folds * sizeof(double), hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_memcpy_async(status, dst, (size_t)B * n_folds * sizeof(int), hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_stream_sync(st));
  return BGP_OK;
}

extern "C" int bgp_cross_validate(bgp_ctx* c, int B, int n_folds, const int* fold_ptr, const int* fold_idx, double* mean, double* var,
                                  double* fold_lpd, int* status) {
  BGP_TRY(bgp_guard(c, "bgp_cross_validate", BGP_POST_ANY));
  if (!fold_ptr || !fold_idx || !mean || !var || !fold_lpd || !status || B < 1 || B > 65535 || n_folds < 1) {
    bgp_set_error("bgp_cross_validate: bad argument (1 <= B <= 65535 posteriors, n_folds >= 1, no NULL array)");
    return BGP_ERR_INVALID;
  }
  const int n = c->n;
  if (fold_ptr[0] != 0) {
    bgp_set_error("bgp_cross_validate: fold_ptr[0] = %d, not 0", fold_ptr[0]);
    return BGP_ERR_INVALID;
  }
  int smax = 0;
  std::vector<int> owner(n, -1);
  for (int f = 0; f < n_folds; f++) {
    const long long s = (long long)fold_ptr[f + 1] - fold_ptr[f];
    if (s < 1) {
      bgp_set_error("bgp_cross_validate: fold %d is empty (fold_ptr must ascend strictly)", f);
      return BGP_ERR_INVALID;
    }
    if (s > CV_SMAX) {
      bgp_set_error("bgp_cross_validate: fold %d has %lld points, more than the limit of %d per fold", f, s, CV_SMAX);
      return BGP_ERR_INVALID;
    }
    for (int q = fold_ptr[f]; q < fold_ptr[f + 1]; q++) {
      const int g = fold_idx[q];
      if (g < 0 || g >= n) {
        bgp_set_error("bgp_cross_validate: fold %d holds index %d, out of range [0, %d)", f, g, n);
        return BGP_ERR_INVALID;
      }
      if (owner[g] >= 0) {
        bgp_set_error("bgp_cross_validate: index %d is in two folds (%d and %d), or twice in one", g, owner[g], f);
        return BGP_ERR_INVALID;
      }
      owner[g] = f;
    }
    smax = std::max(smax, (int)s);
  }
  BGP_TRY(bgp_guard(c, "bgp_cross_validate", BGP_POST_ANY, B));
  return post_call(c, [&] { return cv_run(c, B, n_folds, fold_ptr, fold_idx, smax, mean, var, fold_lpd, status); });
}
