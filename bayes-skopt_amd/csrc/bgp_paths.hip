// Pathwise posterior function draws (BayesGPR.sample_paths, mvn="pathwise").
//
// Matheron's rule: a posterior draw is a prior draw plus a data-dependent update,
//   f(x) = f0(x) + k(x, X) K^-1 (y - f0(X) - e),   e ~ N(0, diag(alpha_diag + s2))
// with f0 a random-Fourier-feature draw of the prior, every path with its OWN features (E f0 = 0 and Cov f0 = k exactly for any F):
//   A     = sqrt(2 cS / F)   (cS = c in the product form, 1 in the sum form)
//   f0(x) = A sum_{j < F, ascending} w_j cos(phase_j + sum_k (x_k / l_k) omega_jk)  [+ sqrt(c) w_F in the sum form]
//   r     = y - f0(X) - sqrt(alpha_diag + s2) eps ;  v = K^-1 r  (the resident inverse of posterior pidx[p])
//   f(x)  = f0(x) + sum_{i, ascending} k(x, X_i) v_i ;  df/dx_k = -A sum_j w_j sin(arg_j) omega_jk / l_k + sum_i v_i G_ik
// (G: the closed forms of the prediction gradients, bgp_predgrad.hip).  No m x m object exists: a path costs O(F + n) per query
// row, and it is a FUNCTION -- bgp_paths_eval may be called any number of times, at any rows, with consistent values.
// bgp_paths_begin builds the state (omega / l, phase, A w, the constant term, v, and copies of the training inputs and the kernel
// parameters) in ONE owned allocation; after it the paths do not read the resident posteriors any more.
// fp64 VALU work in the shape of fant_col_kernel (bgp_fantasy.hip): one query row per thread, its inputs in registers, tiles of 64
// features / 64 training points staged in LDS and read as broadcasts.  Every sum has a fixed ascending order, no atomics: the value
// at (path, row) does not depend on which rows or paths share the call.
// bgp_paths_minimize minimises every path from its own starts: one workgroup per (start, path) evaluates ONE
// path at ONE point with all its threads (pm_eval) and carries the projected BFGS of bgp_bfgs.h itself.
#include <memory>

#include "bgp_common.h"
#include "bgp_device.h"
#include "bgp_bfgs.h"
#include "bgp_paths_int.h"

#define PT_TF 64       // features per LDS tile of the feature kernel
#define PT_TP 64       // training points per LDS tile of the update kernel
#define PT_DMAX 32     // input dimensions held in registers
#define PT_FMAX 65536  // features per path
#define PT_PMAX 65535  // paths per state (a grid dimension)

static void paths_free(bgp_ctx* c) {
  if (!c->paths) return;
  if (c->paths->mem && c->stream) (void)hipStreamSynchronize(c->stream);
  delete c->paths;
  c->paths = nullptr;
}

void bgp_paths_abandon(bgp_ctx* c) {
  if (c) paths_free(c);
}

// f0 (and, GRAD, its gradient) of path blockIdx.y at 256 rows of Xq.  The row's inputs live in registers (the loops over PT_DMAX
// are unrolled, the guard t < d keeps them register-indexed); each tile of PT_TF scaled feature rows omega / l with their phases
// and weights A w is staged in LDS once and read by every thread as a broadcast.  16.5 KB of LDS.  The same function serves
// bgp_paths_begin (Xq = the training inputs) and bgp_paths_eval: f0(X) and f0(x) are one function.
template <int GRAD>
__global__ void __launch_bounds__(256) paths_feat_kernel(const double* __restrict__ Xq, int m, int d, int F,
                                                         const double* __restrict__ Om, const double* __restrict__ Ph,
                                                         const double* __restrict__ Aw, const double* __restrict__ C0,
                                                         double* __restrict__ out, size_t so, double* __restrict__ dout) {
#pragma clang fp contract(off)
  __shared__ double om[PT_TF * PT_DMAX];
  __shared__ double ph[PT_TF];
  __shared__ double aw[PT_TF];
  const int tid = threadIdx.x, p = blockIdx.y, i = blockIdx.x * 256 + tid;
  const int ii = (i < m) ? i : m - 1;  // (threads past the end compute a duplicate and store nothing)
  double x[PT_DMAX], g[GRAD ? PT_DMAX : 1];
#pragma unroll
  for (int t = 0; t < PT_DMAX; t++) {
    if (t < d) x[t] = Xq[(size_t)ii * d + t];
    if constexpr (GRAD != 0) g[t] = 0.0;
  }
  const double* Omp = Om + (size_t)p * F * d;
  const double* Php = Ph + (size_t)p * F;
  const double* Awp = Aw + (size_t)p * F;
  double acc = 0.0;
  for (int j0 = 0; j0 < F; j0 += PT_TF) {
    const int jc = min(PT_TF, F - j0);
    __syncthreads();
    for (int idx = tid; idx < jc * d; idx += 256) {
      const int r = idx / d, t = idx - r * d;
      om[r * PT_DMAX + t] = Omp[(size_t)(j0 + r) * d + t];
    }
    if (tid < jc) {
      ph[tid] = Php[j0 + tid];
      aw[tid] = Awp[j0 + tid];
    }
    __syncthreads();
    for (int r = 0; r < jc; r++) {
      double a = ph[r];
#pragma unroll
      for (int t = 0; t < PT_DMAX; t++)
        if (t < d) a = fma(x[t], om[r * PT_DMAX + t], a);
      acc = fma(aw[r], cos(a), acc);
      if constexpr (GRAD != 0) {
        const double s = aw[r] * sin(a);
#pragma unroll
        for (int t = 0; t < PT_DMAX; t++)
          if (t < d) g[t] = fma(s, om[r * PT_DMAX + t], g[t]);
      }
    }
  }
  if (i >= m) return;
  const size_t o = (size_t)p * so + i;
  out[o] = acc + C0[p];
  if constexpr (GRAD != 0) {
#pragma unroll
    for (int t = 0; t < PT_DMAX; t++)
      if (t < d) dout[o * d + t] = -g[t];
  }
}

// r_p = (y - f0_p(X)) - sqrt(alpha_diag + s2_p) eps_p
__global__ void __launch_bounds__(256) paths_resid_kernel(const double* __restrict__ y, const double* __restrict__ alpha,
                                                          const double* __restrict__ ls2, const double* __restrict__ f0X,
                                                          const double* __restrict__ eps, int n, double* __restrict__ r) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x, p = blockIdx.y;
  if (i >= n) return;
  const size_t o = (size_t)p * n + i;
  r[o] = (y[i] - f0X[o]) - sqrt(alpha[i] + exp(ls2[p])) * eps[o];
}

// v_p = K^-1 r_p with the resident inverse of posterior pidx[p] (bgp_posterior_batch stores K^-1 itself, both triangles): one wave
// per row (rows of the symmetric inverse are contiguous), lanes over the columns in a fixed stride, the 64 partial sums reduced
// by a fixed butterfly -- fant_w_kernel's loop with a posterior index per item
__global__ void __launch_bounds__(256) paths_v_kernel(const double* __restrict__ Kinv, const int* __restrict__ pidx, int n,
                                                      int npad, const double* __restrict__ r, double* __restrict__ v) {
#pragma clang fp contract(off)
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, p = blockIdx.y;
  if (row >= n) return;
  const double* K = Kinv + ((size_t)pidx[p] * npad + row) * npad;
  const double* rp = r + (size_t)p * n;
  double s = 0.0;
  for (int k = lane; k < n; k += 64) s = fma(K[k], rp[k], s);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane == 0) v[(size_t)p * n + row] = s;
}

// out += sum_i k_p(x, X_i) v_p[i] (and, GRAD, dout += sum_i v_p[i] G_i): the generated GEMV of fant_col_kernel against v, PT_TP
// scaled training points and their v entries per LDS tile.  G_ik = cf fac(r_i) (x_k - X_ik) / l_k^2 (bgp_predgrad.hip).
template <int STAT, int FORM, int GRAD>
__global__ void __launch_bounds__(256) paths_upd_kernel(const double* __restrict__ X, int n, int d, const double* __restrict__ Xq,
                                                        int m, const double* __restrict__ H, const double* __restrict__ V,
                                                        double* __restrict__ out, size_t so, double* __restrict__ dout) {
#pragma clang fp contract(off)
  __shared__ double xt[PT_TP * PT_DMAX];
  __shared__ double vt[PT_TP];
  __shared__ double ell[PT_DMAX];
  const int tid = threadIdx.x, p = blockIdx.y, i = blockIdx.x * 256 + tid;
  const double* h = H + (size_t)p * (d + 2);
  const double cst = exp(h[0]);
  if (tid < d) ell[tid] = exp(h[1 + tid]);
  __syncthreads();
  const int ii = (i < m) ? i : m - 1;
  double xi[PT_DMAX], g[GRAD ? PT_DMAX : 1];
#pragma unroll
  for (int t = 0; t < PT_DMAX; t++) {
    if (t < d) xi[t] = Xq[(size_t)ii * d + t] / ell[t];
    if constexpr (GRAD != 0) g[t] = 0.0;
  }
  double acc = 0.0;
  const double* vp = V + (size_t)p * n;
  for (int k0 = 0; k0 < n; k0 += PT_TP) {
    const int kc = min(PT_TP, n - k0);
    __syncthreads();
    for (int idx = tid; idx < kc * d; idx += 256) {
      const int r = idx / d, t = idx - r * d;
      xt[r * PT_DMAX + t] = X[(size_t)(k0 + r) * d + t] / ell[t];
    }
    if (tid < kc) vt[tid] = vp[k0 + tid];
    __syncthreads();
    for (int r = 0; r < kc; r++) {
      double q = 0.0;
#pragma unroll
      for (int t = 0; t < PT_DMAX; t++)
        if (t < d) {
          const double df = xi[t] - xt[r * PT_DMAX + t];
          q = fma(df, df, q);
        }
      if constexpr (GRAD != 0) {
        double S, fac;
        kb_stationary_fac<STAT>(q, S, fac);
        acc = fma(kb_with_constant<FORM>(cst, S), vt[r], acc);
        const double wg = vt[r] * ((FORM == BGP_FORM_PRODUCT) ? cst * fac : fac);
#pragma unroll
        for (int t = 0; t < PT_DMAX; t++)
          if (t < d) g[t] = fma(wg, xi[t] - xt[r * PT_DMAX + t], g[t]);
      } else {
        acc = fma(kb_value<STAT, FORM>(q, cst), vt[r], acc);
      }
    }
  }
  if (i >= m) return;
  const size_t o = (size_t)p * so + i;
  out[o] = out[o] + acc;
  if constexpr (GRAD != 0) {
#pragma unroll
    for (int t = 0; t < PT_DMAX; t++)
      if (t < d) dout[o * d + t] = dout[o * d + t] + g[t] / ell[t];
  }
}

// ---- the minimiser of a path ----------------------------------------------------------------------------
#define PM_RS (PG_DMAX + 1)  // stride of a wave's partial sums

struct PmWork {               // LDS of one evaluation
  double x[PG_DMAX];          // the query point
  double il[PG_DMAX];         // 1 / length scale
  double ell[PG_DMAX];        // length scale
  double tile[PG_NT];         // A w_j sin(arg_j) of a tile of features, then v_i cf fac_i of a tile of training points
  double red[PG_NW * PM_RS];  // wave partials of the value (column 0) and of the update's gradient (columns 1 ..)
  double redf[PG_NW * PM_RS]; // wave partials of the feature gradient (columns 1 ..)
  double f, df[PG_DMAX];
};

// The path at W.x: f into W.f, df/dx into W.df, by the whole workgroup of PG_NT threads.  Features and training points are taken in
// tiles of PG_NT: thread j of a tile forms its term of the value (arg_j as paths_feat_kernel forms it: from the phase, fma in
// ascending k) and leaves the gradient's weight in W.tile; after a barrier lane (t, half) of wave wv owns dimension t over the tile's
// entries 2 wv + half, + 2 PG_NW, ... (pg_wsum's split), in registers that live across the tiles.  Value: a butterfly inside every
// wave, then the wave partials in ascending order; gradient: the two halves, then the waves in ascending order.  No atomics, no F- or
// n-sized row.  Called by every thread; starts with a barrier (W.x may have been written just before); W.f / W.df are visible to
// every thread on return.
template <int STAT, int FORM>
static __device__ __forceinline__ void pm_eval(const double* __restrict__ X, int n, int d, int F, const double* __restrict__ Om,
                                            const double* __restrict__ Ph, const double* __restrict__ Aw, double c0,
                                            const double* __restrict__ V, double cst, PmWork& W) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, t = lane & 31, r0 = 2 * wv + (lane >> 5);
  const bool own = t < d;
  __syncthreads();
  const double xl = own ? W.x[t] : 0.0, ill = own ? W.il[t] : 0.0;
  double val = 0.0, gf = 0.0, gu = 0.0;
  for (int j0 = 0; j0 < F; j0 += PG_NT) {
    const int jc = min(PG_NT, F - j0), j = j0 + tid;
    if (tid < jc) {
      const double* om = Om + (size_t)j * d;
      double a = Ph[j];
      for (int k = 0; k < d; k++) a = fma(W.x[k], om[k], a);
      const double aw = Aw[j];
      val = fma(aw, cos(a), val);
      W.tile[tid] = aw * sin(a);
    }
    __syncthreads();
    if (own)
      for (int r = r0; r < jc; r += 2 * PG_NW) gf = fma(W.tile[r], Om[(size_t)(j0 + r) * d + t], gf);
    __syncthreads();  // (the tile is rewritten next)
  }
  for (int i0 = 0; i0 < n; i0 += PG_NT) {
    const int ic = min(PG_NT, n - i0), i = i0 + tid;
    if (tid < ic) {
      const double* xi = X + (size_t)i * d;
      double r2 = 0.0;
      for (int k = 0; k < d; k++) {
        const double df = (W.x[k] - xi[k]) * W.il[k];
        r2 = fma(df, df, r2);
      }
      double S, fac;
      kb_stationary_fac<STAT>(r2, S, fac);
      const double v = V[i];
      val = fma(kb_with_constant<FORM>(cst, S), v, val);
      W.tile[tid] = v * ((FORM == BGP_FORM_PRODUCT) ? cst * fac : fac);
    }
    __syncthreads();
    if (own)
      for (int r = r0; r < ic; r += 2 * PG_NW) gu = fma(W.tile[r], (xl - X[(size_t)(i0 + r) * d + t]) * ill, gu);
    __syncthreads();  // (the tile is rewritten next)
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) val += __shfl_xor(val, o, 64);
  gf += __shfl_xor(gf, 32, 64);
  gu += __shfl_xor(gu, 32, 64);
  if (lane == 0) W.red[wv * PM_RS] = val;
  if (lane < d) {
    W.redf[wv * PM_RS + 1 + lane] = gf;
    W.red[wv * PM_RS + 1 + lane] = gu;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int w = 0; w < PG_NW; w++) s += W.red[w * PM_RS];
    W.f = s + c0;
  }
  if (tid < d) {
    double sf = 0.0, su = 0.0;
    for (int w = 0; w < PG_NW; w++) sf += W.redf[w * PM_RS + 1 + tid], su += W.red[w * PM_RS + 1 + tid];
    W.df[tid] = -sf + su / W.ell[tid];
  }
  __syncthreads();
}

// One workgroup per (start, path): blockIdx.x = start, blockIdx.y = path; item o = path * S + start of every array.  The objective
// is the path itself (normalised-y units).  f_out / g_out: the evaluator's own values at X_out; where the search's last evaluation
// was not at X_out (a failed line search) one closing evaluation is made and counted.
template <int STAT, int FORM>
__global__ void __launch_bounds__(PG_NT) pm_min_kernel(const double* __restrict__ X, int n, int d, int F,
                                                       const double* __restrict__ H, const double* __restrict__ Om,
                                                       const double* __restrict__ Ph, const double* __restrict__ Aw,
                                                       const double* __restrict__ C0, const double* __restrict__ V,
                                                       const double* __restrict__ X0, const double* __restrict__ lo_,
                                                       const double* __restrict__ hi_, double gtol, int max_iter,
                                                       double* __restrict__ X_out, double* __restrict__ f_out,
                                                       double* __restrict__ g_out, int* __restrict__ iters, int* __restrict__ evals,
                                                       int* __restrict__ status) {
#pragma clang fp contract(off)
  __shared__ PmWork W;
  __shared__ PgBfgs Bf;
  const int tid = threadIdx.x, p = blockIdx.y;
  const size_t o = (size_t)p * gridDim.x + blockIdx.x;
  const double* h = H + (size_t)p * (d + 2);
  if (tid < d) {
    Bf.lo[tid] = lo_[tid];
    Bf.hi[tid] = hi_[tid];
    double v = X0[o * d + tid];
    v = v < Bf.lo[tid] ? Bf.lo[tid] : (v > Bf.hi[tid] ? Bf.hi[tid] : v);
    Bf.x[tid] = v;
    W.x[tid] = v;
    W.ell[tid] = exp(h[1 + tid]);
    W.il[tid] = 1.0 / W.ell[tid];
  }
  const double cst = exp(h[0]), c0 = C0[p];
  const double *Omp = Om + (size_t)p * F * d, *Php = Ph + (size_t)p * F, *Awp = Aw + (size_t)p * F, *Vp = V + (size_t)p * n;
  auto eval = [&] { pm_eval<STAT, FORM>(X, n, d, F, Omp, Php, Awp, c0, Vp, cst, W); };
  int it, nev;
  const int st = pg_bfgs(Bf, W.x, d, gtol, max_iter, eval, [&] { return W.f; }, [&](int t) { return W.df[t]; }, it, nev);
  bool there = true;  // the last evaluation was made at the end point
  for (int t = 0; t < d; t++) there = there && W.x[t] == Bf.x[t];
  if (!there) {
    __syncthreads();
    if (tid < d) W.x[tid] = Bf.x[tid];
    eval();
    nev++;
  }
  if (tid < d) {
    X_out[o * d + tid] = Bf.x[tid];
    if (g_out) g_out[o * d + tid] = W.df[tid];
  }
  if (tid == 0) {
    f_out[o] = W.f;
    iters[o] = it;
    evals[o] = nev;
    status[o] = st;
  }
}

static int paths_launch_feat(bgp_ctx* c, const bgp_paths_state* s, const double* dXq, int m, double* out, size_t so, double* dout) {
  const dim3 grid((m + 255) / 256, s->P);
  if (dout)
    hipLaunchKernelGGL(paths_feat_kernel<1>, grid, dim3(256), 0, c->stream, dXq, m, s->d, s->F, s->dOm, s->dPh, s->dAw, s->dC0, out,
                       so, dout);
  else
    hipLaunchKernelGGL(paths_feat_kernel<0>, grid, dim3(256), 0, c->stream, dXq, m, s->d, s->F, s->dOm, s->dPh, s->dAw, s->dC0, out,
                       so, dout);
  BGP_HIP(hipGetLastError());
  return BGP_OK;
}

static int paths_begin_run(bgp_ctx* c, int P, const int* pidx, const double* h_kernel, const double* ls2, int F,
                           const double* omega, const double* phase, const double* w, const double* eps) {
  paths_free(c);
  const int n = c->n, d = c->d, npad = c->npad;
  const size_t p2 = d + 2, PF = (size_t)P * F, Pn = (size_t)P * n;
  // the host side of the state: omega / l, A w, the constant term
  std::vector<double> oms(PF * d), aws(PF), c0(P);
  const bool sum = c->ks.form == BGP_FORM_SUM;
  for (int p = 0; p < P; p++) {
    const double* h = h_kernel + (size_t)p * p2;
    const double cst = std::exp(h[0]);
    const double A = std::sqrt(2.0 * (sum ? 1.0 : cst) / (double)F);
    const double *op = omega + (size_t)p * F * d, *wp = w + (size_t)p * (F + 1);
    double* od = oms.data() + (size_t)p * F * d;
    for (int j = 0; j < F; j++) {
      for (int t = 0; t < d; t++) od[(size_t)j * d + t] = op[(size_t)j * d + t] / std::exp(h[1 + t]);
      aws[(size_t)p * F + j] = A * wp[j];
    }
    c0[p] = (sum && cst > 0.0) ? std::sqrt(cst) * wp[F] : 0.0;
  }
  std::unique_ptr<bgp_paths_state> st(new bgp_paths_state());
  bgp_paths_state* s = st.get();
  s->P = P, s->F = F, s->n = n, s->d = d;
  int rc = bgp_carve(s->mem, 16, [&](BgpCarve& k) {
    s->dX = k.take<double>((size_t)n * d);
    s->dH = k.take<double>((size_t)P * p2);
    s->dOm = k.take<double>(PF * d);
    s->dPh = k.take<double>(PF);
    s->dAw = k.take<double>(PF);
    s->dC0 = k.take<double>(P);
    s->dV = k.take<double>(Pn);
  });
  if (rc) return rc;
  double *df0, *deps, *dr, *dls2;
  int* dpidx;
  BgpScratch live(c);
  rc = live.carve([&](BgpCarve& k) {
    df0 = k.take<double>(Pn);
    deps = k.take<double>(Pn);
    dr = k.take<double>(Pn);
    dls2 = k.take<double>(P);
    dpidx = k.take<int>(P);
  });
  if (rc) return rc;
  hipStream_t q = c->stream;
  BGP_HIP(hipMemcpyAsync(s->dX, c->dXeff, (size_t)n * d * sizeof(double), hipMemcpyDeviceToDevice, q));
  BGP_HIP(bgp_memcpy_async(s->dH, h_kernel, (size_t)P * p2 * sizeof(double), hipMemcpyHostToDevice, q));
  BGP_HIP(bgp_memcpy_async(s->dOm, oms.data(), PF * d * sizeof(double), hipMemcpyHostToDevice, q));
  BGP_HIP(bgp_memcpy_async(s->dPh, phase, PF * sizeof(double), hipMemcpyHostToDevice, q));
  BGP_HIP(bgp_memcpy_async(s->dAw, aws.data(), PF * sizeof(double), hipMemcpyHostToDevice, q));
  BGP_HIP(bgp_memcpy_async(s->dC0, c0.data(), (size_t)P * sizeof(double), hipMemcpyHostToDevice, q));
  BGP_HIP(bgp_memcpy_async(deps, eps, Pn * sizeof(double), hipMemcpyHostToDevice, q));
  BGP_HIP(bgp_memcpy_async(dls2, ls2, (size_t)P * sizeof(double), hipMemcpyHostToDevice, q));
  BGP_HIP(bgp_memcpy_async(dpidx, pidx, (size_t)P * sizeof(int), hipMemcpyHostToDevice, q));
  BGP_TRY(paths_launch_feat(c, s, s->dX, n, df0, (size_t)n, nullptr));
  hipLaunchKernelGGL(paths_resid_kernel, dim3((n + 255) / 256, P), dim3(256), 0, q, c->dy, c->dalpha, dls2, df0, deps, n, dr);
  hipLaunchKernelGGL(paths_v_kernel, dim3((n + 3) / 4, P), dim3(256), 0, q, c->dKinv, dpidx, n, npad, dr, s->dV);
  BGP_HIP(hipGetLastError());
  BGP_HIP(bgp_stream_sync(q));  // (the host vectors above are staged; the state is complete)
  c->paths = st.release();
  c->paths_stats[0]++;
  return BGP_OK;
}

extern "C" int bgp_paths_begin(bgp_ctx* c, int P, const int* pidx, const double* h_kernel, const double* s2, int F,
                               const double* omega, const double* phase, const double* w, const double* eps) {
  BGP_TRY(bgp_guard(c, "bgp_paths_begin", BGP_POST_PLAIN));
  if (c && (P < 1 || P > PT_PMAX || F < 1 || F > PT_FMAX)) {
    bgp_set_error("bgp_paths_begin: %d paths of %d features (1 .. %d paths, 1 .. %d features)", P, F, PT_PMAX, PT_FMAX);
    return BGP_ERR_INVALID;
  }
  if (!c || !pidx || !h_kernel || !s2 || !omega || !phase || !w || !eps) {
    bgp_set_error("bgp_paths_begin: bad argument");
    return BGP_ERR_INVALID;
  }
  if (c->d > PT_DMAX || c->has_warp) {
    bgp_set_error("bgp_paths_begin: %s", c->has_warp ? "warped inputs are not supported" : "d > 32 is not supported");
    return BGP_ERR_INVALID;
  }
  BGP_TRY(bgp_guard(c, "bgp_paths_begin", BGP_POST_PLAIN, 0, pidx, P));
  return post_call(c, [&] { return paths_begin_run(c, P, pidx, h_kernel, s2, F, omega, phase, w, eps); });
}

// f0 + the update at device rows (bgp_paths_int.h): what bgp_paths_eval launches per chunk, and bgp_paths_select for its matrix
int bgp_paths_launch_eval(bgp_ctx* c, const bgp_paths_state* s, const double* dXq, int m, double* out, size_t so, double* dout) {
  BGP_TRY(paths_launch_feat(c, s, dXq, m, out, so, dout));
  const int n = s->n, d = s->d;
  const dim3 grid((m + 255) / 256, s->P);
  hipStream_t q = c->stream;
  if (dout)
    KB_DISPATCH(c->ks.stationary, c->ks.form,
                hipLaunchKernelGGL((paths_upd_kernel<S, F, 1>), grid, dim3(256), 0, q, s->dX, n, d, dXq, m, s->dH, s->dV, out, so,
                                   dout));
  else
    KB_DISPATCH(c->ks.stationary, c->ks.form,
                hipLaunchKernelGGL((paths_upd_kernel<S, F, 0>), grid, dim3(256), 0, q, s->dX, n, d, dXq, m, s->dH, s->dV, out, so,
                                   dout));
  BGP_HIP(hipGetLastError());
  return BGP_OK;
}

static int paths_eval_run(bgp_ctx* c, int m, const double* Xq, double* out, double* dout) {
  const bgp_paths_state* s = c->paths;
  const int P = s->P, d = s->d;
  // chunks of query rows: staged outputs of P mc (1 + d) doubles under the budget of the prediction gradients (2^24 doubles)
  size_t mc = std::max<size_t>(1, ((size_t)1 << 24) / ((size_t)P * (1 + (size_t)d)));
  mc = bgp_switch_cap(BGP_SW_ROW_CHUNK, mc);  // (tests: forced row chunks against the default; the rounding below still applies)
  if (mc >= 256) mc &= ~(size_t)255;
  mc = std::min(mc, (size_t)m);
  double *dXq, *dO, *dG = nullptr;
  BgpScratch live(c);
  int rc = live.carve([&](BgpCarve& k) {
    dXq = k.take<double>(mc * d);
    dO = k.take<double>((size_t)P * mc);
    if (dout) dG = k.take<double>((size_t)P * mc * d);
  });
  if (rc) return rc;
  hipStream_t q = c->stream;
  c->chunk_last[0] = 1, c->chunk_last[1] = 0;
  for (size_t m0 = 0; m0 < (size_t)m; m0 += mc) {
    const int mm = (int)std::min(mc, (size_t)m - m0);
    c->chunk_last[1]++;
    BGP_HIP(bgp_memcpy_async(dXq, Xq + m0 * d, (size_t)mm * d * sizeof(double), hipMemcpyHostToDevice, q));
    BGP_TRY(bgp_paths_launch_eval(c, s, dXq, mm, dO, mc, dG));
    const size_t w1 = (size_t)mm * sizeof(double), wd = w1 * d;
    BGP_HIP(bgp_memcpy2d_async(out + m0, (size_t)m * sizeof(double), dO, mc * sizeof(double), w1, P, hipMemcpyDeviceToHost, q));
    if (dout)
      BGP_HIP(bgp_memcpy2d_async(dout + m0 * d, (size_t)m * d * sizeof(double), dG, mc * d * sizeof(double), wd, P,
                                 hipMemcpyDeviceToHost, q));
    BGP_HIP(bgp_stream_sync(q));  // (the next chunk reuses the buffers)
  }
  c->paths_stats[1]++;
  return BGP_OK;
}

extern "C" int bgp_paths_eval(bgp_ctx* c, int m, const double* Xq, double* out, double* dout) {
  BGP_TRY(bgp_guard(c, "bgp_paths_eval"));
  if (!c->paths) {
    bgp_set_error("bgp_paths_eval: no paths state (call bgp_paths_begin first)");
    return BGP_ERR_STATE;
  }
  if (!Xq || !out || m <= 0) {
    bgp_set_error("bgp_paths_eval: bad argument");
    return BGP_ERR_INVALID;
  }
  return post_call(c, [&] { return paths_eval_run(c, m, Xq, out, dout); });
}

static int paths_min_run(bgp_ctx* c, int S, const double* X0, const double* lo, const double* hi, double gtol, int max_iter,
                         double* X_out, double* f_out, double* g_out, int* iters, int* evals, int* status) {
  const bgp_paths_state* s = c->paths;
  const int P = s->P, d = s->d, n = s->n;
  // chunks of starts: staged starts, end points, values, gradients and counters of P sc items under the budget of bgp_paths_eval
  size_t sc = std::max<size_t>(1, ((size_t)1 << 24) / ((size_t)P * (3 + 3 * (size_t)d)));
  sc = std::min(bgp_switch_cap(BGP_SW_ROW_CHUNK, sc), (size_t)S);  // (tests: forced chunks of starts against the default)
  const size_t Ps = (size_t)P * sc;
  double *dX0, *dXo, *dlo, *dhi, *df, *dg = nullptr;
  int *dit, *dev, *dst;
  BgpScratch live(c);
  int rc = live.carve([&](BgpCarve& k) {
    dX0 = k.take<double>(Ps * d);
    dXo = k.take<double>(Ps * d);
    dlo = k.take<double>(d);
    dhi = k.take<double>(d);
    df = k.take<double>(Ps);
    if (g_out) dg = k.take<double>(Ps * d);
    dit = k.take<int>(Ps);
    dev = k.take<int>(Ps);
    dst = k.take<int>(Ps);
  });
  if (rc) return rc;
  hipStream_t q = c->stream;
  BGP_HIP(bgp_memcpy_async(dlo, lo, (size_t)d * sizeof(double), hipMemcpyHostToDevice, q));
  BGP_HIP(bgp_memcpy_async(dhi, hi, (size_t)d * sizeof(double), hipMemcpyHostToDevice, q));
  c->chunk_last[0] = 1, c->chunk_last[1] = 0;
  for (size_t s0 = 0; s0 < (size_t)S; s0 += sc) {
    c->chunk_last[1]++;
    const int ss = (int)std::min(sc, (size_t)S - s0);  // (the chunk's items are packed: item = path * ss + start)
    const size_t w1 = (size_t)ss * sizeof(double), wd = w1 * d, wi = (size_t)ss * sizeof(int);
    BGP_HIP(bgp_memcpy2d_async(dX0, wd, X0 + s0 * d, (size_t)S * d * sizeof(double), wd, P, hipMemcpyHostToDevice, q));
    KB_DISPATCH(c->ks.stationary, c->ks.form,
                hipLaunchKernelGGL((pm_min_kernel<S, F>), dim3(ss, P), dim3(PG_NT), 0, q, s->dX, n, d, s->F, s->dH, s->dOm, s->dPh,
                                   s->dAw, s->dC0, s->dV, dX0, dlo, dhi, gtol, max_iter, dXo, df, dg, dit, dev, dst));
    BGP_HIP(hipGetLastError());
    BGP_HIP(bgp_memcpy2d_async(X_out + s0 * d, (size_t)S * d * sizeof(double), dXo, wd, wd, P, hipMemcpyDeviceToHost, q));
    BGP_HIP(bgp_memcpy2d_async(f_out + s0, (size_t)S * sizeof(double), df, w1, w1, P, hipMemcpyDeviceToHost, q));
    if (g_out) BGP_HIP(bgp_memcpy2d_async(g_out + s0 * d, (size_t)S * d * sizeof(double), dg, wd, wd, P, hipMemcpyDeviceToHost, q));
    BGP_HIP(bgp_memcpy2d_async(iters + s0, (size_t)S * sizeof(int), dit, wi, wi, P, hipMemcpyDeviceToHost, q));
    BGP_HIP(bgp_memcpy2d_async(evals + s0, (size_t)S * sizeof(int), dev, wi, wi, P, hipMemcpyDeviceToHost, q));
    BGP_HIP(bgp_memcpy2d_async(status + s0, (size_t)S * sizeof(int), dst, wi, wi, P, hipMemcpyDeviceToHost, q));
    BGP_HIP(bgp_stream_sync(q));  // (the next chunk reuses the buffers)
  }
  return BGP_OK;
}

extern "C" int bgp_paths_minimize(bgp_ctx* c, int S, const double* X0, const double* lo, const double* hi, double gtol,
                                  int max_iter, double* X_out, double* f_out, double* g_out, int* iters, int* evals, int* status) {
  BGP_TRY(bgp_guard(c, "bgp_paths_minimize"));
  if (!c->paths) {
    bgp_set_error("bgp_paths_minimize: no paths state (call bgp_paths_begin first)");
    return BGP_ERR_STATE;
  }
  if (!X0 || !lo || !hi || !X_out || !f_out || !iters || !evals || !status || S < 1 || max_iter < 0 || !(gtol >= 0.0)) {
    bgp_set_error("bgp_paths_minimize: bad argument (S >= 1, max_iter >= 0, gtol >= 0)");
    return BGP_ERR_INVALID;
  }
  for (int t = 0; t < c->paths->d; t++)
    if (!(lo[t] <= hi[t])) {
      bgp_set_error("bgp_paths_minimize: empty box in dimension %d", t);
      return BGP_ERR_INVALID;
    }
  return post_call(c, [&] { return paths_min_run(c, S, X0, lo, hi, gtol, max_iter, X_out, f_out, g_out, iters, evals, status); });
}

extern "C" int bgp_paths_end(bgp_ctx* c) {
  if (!c) {
    bgp_set_error("bgp_paths_end: NULL ctx");
    return BGP_ERR_INVALID;
  }
  paths_free(c);
  return BGP_OK;
}

extern "C" int bgp_chunk_stats(bgp_ctx* c, long long* out) {
  if (!c || !out) {
    bgp_set_error("bgp_chunk_stats: bad argument");
    return BGP_ERR_INVALID;
  }
  out[0] = c->chunk_last[0];
  out[1] = c->chunk_last[1];
  return BGP_OK;
}

extern "C" int bgp_paths_stats(bgp_ctx* c, long long* out) {
  if (!c || !out) {
    bgp_set_error("bgp_paths_stats: bad argument");
    return BGP_ERR_INVALID;
  }
  out[0] = c->paths_stats[0];
  out[1] = c->paths_stats[1];
  return BGP_OK;
}
