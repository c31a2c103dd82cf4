// Posterior build, predict, LML gradient, PVRS and sample_y.
//
// Posterior build (the BayesGPR.theta setter, bask/bayesgpr.py:200-217): the batched Cholesky of
// bgp_chol.hip is run on the augmented matrix [[K, .], [I, 0]] for nblk steps, which leaves
//   top-left      L                      -> BayesGPR.L_
//   bottom-right  -K^-1 (Schur complement)-> BayesGPR.K_inv_   (the reference forms the explicit
//                                            inverse too: L_inv.dot(L_inv.T), :207-208)
//   rhs, lower    -alpha = -(K^-1 y)      -> BayesGPR.alpha_
// K^-1 and alpha of every posterior stay resident in HBM for the predict / pvrs / gradient calls.
//
// Predict (bask/bayesgpr.py:622-635 -> skopt predict), per resident posterior:
//   K_* = k(Xq, X)  (tiled cross-kernel build);  mean = K_* alpha;
//   var = k_** - rowsum((K_* K^-1) o K_*)   -- one NT tile GEMM on the fp64 MFMA with the row-dot
//   fused into its epilogue (K^-1 symmetric, so K_* K^-1 = K_* (K^-1)^T is an NT product);
//   cov = K_** - (K_* K^-1) K_*^T for predict(return_cov); K_** - (K_* L^-T)(K_* L^-T)^T where a Cholesky reads it (the draws).
#include "bgp_common.h"
#include "bgp_device.h"
#include "bgp_gemm.h"

// ------------------------------------------------------------------------------------------
// small helpers
// ------------------------------------------------------------------------------------------
__global__ void aug_init_kernel(double* __restrict__ Kbuf, double* __restrict__ yw, int npad, int B) {
  // identity into the bottom-left block of every augmented matrix, zero the lower half of the rhs
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (i >= npad || b >= B) return;
  const size_t ld = 2 * (size_t)npad;
  Kbuf[(size_t)b * ld * ld + (size_t)(npad + i) * ld + i] = 1.0;
  yw[(size_t)b * ld + npad + i] = 0.0;
}

// K^-1 (full symmetric npad x npad) and alpha out of the augmented workspace.
__global__ void __launch_bounds__(256) extract_kinv_kernel(const double* __restrict__ Kbuf,
                                                            const double* __restrict__ yw,
                                                            double* __restrict__ Kinv, double* __restrict__ Linv,
                                                            double* __restrict__ alpha, int npad, int boff) {
  const int b = blockIdx.y;
  const size_t ld = 2 * (size_t)npad;
  const double* M = Kbuf + (size_t)b * ld * ld;
  double* out = Kinv + (size_t)(boff + b) * npad * npad;
  double* outL = Linv ? Linv + (size_t)(boff + b) * npad * npad : nullptr;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < (size_t)npad * npad;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(idx / npad), j = (int)(idx - (size_t)i * npad);
    const int hi = i > j ? i : j, lo = i > j ? j : i;
    out[idx] = -M[(size_t)(npad + hi) * ld + npad + lo];
    // the bottom-left block of the augmented factor is [I] L^-T: its transpose is L^-1
    if (outL) outL[idx] = j <= i ? M[(size_t)(npad + j) * ld + i] : 0.0;
  }
  if (blockIdx.x == 0)
    for (int i = threadIdx.x; i < npad; i += blockDim.x)
      alpha[(size_t)(boff + b) * npad + i] = -yw[(size_t)b * ld + npad + i];
}

// compact n x n lower factor (zeros above the diagonal) of matrix b into scratch
__global__ void extract_L_kernel(const double* __restrict__ Kbuf, double* __restrict__ out, int n, int ld,
                                 size_t mstride, int b) {
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < (size_t)n * n;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(idx / n), j = (int)(idx - (size_t)i * n);
    out[idx] = (j <= i) ? Kbuf[(size_t)b * mstride + (size_t)i * ld + j] : 0.0;
  }
}

// Batched launches below run item b = blockIdx.y of a chunk; operands that live in the resident posterior arrays
// (K^-1, alpha) are addressed through `pidx[b]` (NULL: item b is posterior b0 + b ... callers pass explicit maps).
// mean_i = sum_j Ks[i][j] alpha[j]   (one wave per row)
__global__ void __launch_bounds__(256) matvec_rows_kernel(const double* __restrict__ Ks, int lds, size_t sK,
                                                           const double* __restrict__ v, size_t sv,
                                                           const int* __restrict__ pidx, int n, int m,
                                                           double* __restrict__ out, size_t so) {
  const int b = blockIdx.y;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= m) return;
  const double* K = Ks + (size_t)b * sK;
  const double* vb = v + (size_t)(pidx ? pidx[b] : b) * sv;
  double s = 0.0;
  for (int j = lane; j < n; j += 64) s += K[(size_t)row * lds + j] * vb[j];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) out[(size_t)b * so + row] = s;
}

// kernel_.diag(X) incl. the white level (sklearn/kernels.py:868-884, 968-984) from a canonical vector on the device
static __device__ __forceinline__ double dev_kernel_diag(const double* hk, int d, int form) {
  const double cst = exp(hk[0]), s2 = exp(hk[d + 1]);
  return ((form == BGP_FORM_PRODUCT) ? cst * 1.0 : cst + 1.0) + s2;
}

// var_i = max(0, diag_b - q_i)
__global__ void finish_var_kernel(const double* __restrict__ q, size_t sq, const double* __restrict__ H, int d, int form,
                                  int m, double* __restrict__ var, size_t so) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (i >= m) return;
  const double v = dev_kernel_diag(H + (size_t)b * (d + 2), d, form) - q[(size_t)b * sq + i];
  var[(size_t)b * so + i] = v < 0.0 ? 0.0 : v;
}

// Ordered sum of the column-tile partials of a batched row reduction (row dots of rowquad4_kernel, means of
// kbuild_cross_kernel): out[b][i] = sum_t part[(b tn + t) M + i], t ascending -- no floating-point atomics.
__global__ void rowdot_reduce_kernel(const double* __restrict__ part, int tn, int M, double* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (i >= M) return;
  double s = 0.0;
  for (int t = 0; t < tn; t++) s += part[((size_t)b * tn + t) * M + i];
  out[(size_t)b * M + i] = s;  // (batched row dots are packed with stride M)
}

// out[b][i] = a_i^T S_b a_i for the rows of A_b (M x n, zero padded; S symmetric): half-product on the LDS-DMA ring
// (rowquad4_kernel, bgp_syrk4.hip) + ordered reduction of the column-tile partials.  out is packed with stride M.
static int launch_rowquad(bgp_ctx* c, const double* A, int lda, size_t sA, const double* S, int lds_, size_t sS,
                          const int* pidx, int M, int n, int nb, double* out) {
  const int tn = n / bgp_rowquad_tile();
  // (column-tile partials of the row dots in a buffer of their own: the callers' scratch layouts stay as they are)
  int rc = c->drowpart.ensure((size_t)nb * tn * M);
  if (rc) return rc;
  bgp_launch_rowquad(c->stream, A, lda, sA, S, lds_, sS, pidx, M, n, nb, c->drowpart);
  BGP_HIP(hipGetLastError());
  hipLaunchKernelGGL(rowdot_reduce_kernel, dim3((M + 255) / 256, nb), dim3(256), 0, c->stream, c->drowpart, tn, M, out);
  BGP_HIP(hipGetLastError());
  return BGP_OK;
}

static inline int pad128(int v) { return pad_to(v, 128); }

// The latent moments of `rows` query rows for nb items (contract: bgp_common.h).  mean = K_* alpha comes out of the cross build's
// registers as column-tile partials, added in tile order; q_i = k_i^T K^-1 k_i (= rowsum((K_* K^-1) o K_*), evaluated on the lower
// block triangle of K^-1) becomes the variance in place.
int bgp_launch_moments(bgp_ctx* c, int nb, const double* dH, int rows, const double* dXq, size_t qstride, const double* dXt,
                       size_t xstride, const double* alpha, const double* Kinv, double* dKs, int ldk, size_t sKs, double* dmpart,
                       double* dmean, double* dvar) {
  const int npad = c->npad, rp = pad128(rows);
  BGP_TRY(bgp_launch_kcross_matvec_x(c, nb, dH, rows, dXq, qstride, c->n, dXt, xstride, dKs, ldk, sKs, alpha, (size_t)npad, dmpart));
  hipLaunchKernelGGL(rowdot_reduce_kernel, dim3((rp + 255) / 256, nb), dim3(256), 0, c->stream, dmpart, npad / 128, rp, dmean);
  if (dvar) {
    BGP_TRY(launch_rowquad(c, dKs, ldk, sKs, Kinv, npad, (size_t)npad * npad, nullptr, rp, npad, nb, dvar));
    hipLaunchKernelGGL(finish_var_kernel, dim3((rows + 255) / 256, nb), dim3(256), 0, c->stream, dvar, (size_t)rp, dH, c->d,
                       c->ks.form, rows, dvar, (size_t)rp);
  }
  BGP_HIP(hipGetLastError());
  return BGP_OK;
}

// (bgp_guard and post_call, the ONE guard and the ONE exit path of the entry points of this file: bgp_common.h)

// `rows` rows of `w` doubles between a packed host array and device rows of stride `ld`
static hipError_t rows_up(bgp_ctx* c, double* dev, const double* host, int w, int ld, int rows) {
  return bgp_memcpy2d_async(dev, (size_t)ld * sizeof(double), host, (size_t)w * sizeof(double), (size_t)w * sizeof(double), rows,
                            hipMemcpyHostToDevice, c->stream);
}
static hipError_t rows_down(bgp_ctx* c, double* host, const double* dev, int w, int ld, int rows) {
  return bgp_memcpy2d_async(host, (size_t)w * sizeof(double), dev, (size_t)ld * sizeof(double), (size_t)w * sizeof(double), rows,
                            hipMemcpyDeviceToHost, c->stream);
}

// Items per chunk of a batched call: what `budget` doubles of scratch hold at `per_item` each; round8: whole rounds of the
// item -> XCD pinning (rowquad4_kernel) when the batch takes more than one chunk.  BGP_ITEM_CHUNK (tests: forced chunks against the
// default) bounds the budget's answer from above, in front of the rounding.
static int post_chunk(int B, size_t per_item, size_t budget, bool round8) {
  int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, budget / per_item));
  chunk = (int)bgp_switch_cap(BGP_SW_ITEM_CHUNK, (size_t)chunk);
  if (round8 && chunk >= 8 && chunk < B) chunk &= ~7;
  return chunk;
}

// Query points to the device, through the context-level warp when one is set: BayesGPR.predict warps them with the current warpers
// (bask/bayesgpr.py:630-632), PVRS compares candidates and Thompson points in the warped space (bask/acquisition.py:324-327).
int post_stage_queries(bgp_ctx* c, double* dst, const double* src, int rows) {
  BGP_HIP(bgp_memcpy_async(dst, src, (size_t)rows * c->d * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return c->has_warp ? bgp_launch_warp(c, c->stream, dst, c->dwarp, dst, rows, 1, 0) : BGP_OK;
}

// ------------------------------------------------------------------------------------------
// posterior build
// ------------------------------------------------------------------------------------------
static int ensure_resident(bgp_ctx* c, int B, bool want_Linv, bool rowwarp) {
  // K^-1 needs B npad^2 doubles, alpha B npad: the two capacities are tracked separately (a context reused through
  // bgp_ctx_update_data may see n shrink and B grow: B=1 at npad=1024 and B=64 at npad=128 need the same K^-1
  // bytes but 8x the alpha bytes)
  int rc = c->dKinv.ensure((size_t)B * c->npad * c->npad);
  if (!rc && want_Linv) rc = c->dLinv.ensure((size_t)B * c->npad * c->npad);
  // (per-row-warped posteriors keep their warped training inputs and warp parameters beside K^-1)
  if (!rc && rowwarp) rc = c->dXwP.ensure((size_t)B * c->n * c->d);
  if (!rc && rowwarp) rc = c->dwarpP.ensure((size_t)B * 2 * c->d);
  return rc ? rc : c->dalpha_sol.ensure((size_t)B * c->npad);
}

int bgp_posterior_build(bgp_ctx* c, int B, const double* h, int use_alpha, double* L, double* alpha, double* K_inv,
                        double* lml, int* status, const double* Kgram, bool want_Linv, const double* warp) {
  const int npad = c->npad, n = c->n;
  const size_t p = c->d + 2, nd = (size_t)n * c->d, w2 = 2 * (size_t)c->d;
  const size_t ld = 2 * (size_t)npad;
  c->post.drop();  // (whatever was resident is gone before the buffers are touched; commit() below when the build is through)
  int rc = ensure_resident(c, B, want_Linv, warp != nullptr);
  if (rc) return rc;
  if (warp) {
    // every item's own Beta-CDF warp of the un-warped training inputs, all B in one launch; they stay resident for the predict
    BGP_HIP(bgp_memcpy_async(c->dwarpP, warp, (size_t)B * w2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
    rc = bgp_launch_warp(c, c->stream, c->dX, c->dwarpP, c->dXwP, n, B, nd);
    if (rc) return rc;
  }
  // augmented matrices are 4x the LML workspace per item
  int chunk = (int)(c->dK.cap / (ld * ld));
  if (chunk < 1) {
    rc = bgp_grow_workspace(c, ld * ld);
    if (rc) return rc;
    chunk = 1;
  }
  chunk = std::min(chunk, c->max_batch);
  for (int off = 0; off < B; off += chunk) {
    const int nb = std::min(chunk, B - off);
    if (!Kgram)
      BGP_HIP(bgp_memcpy_async(c->dh, h + (size_t)off * p, nb * p * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BGP_HIP(hipMemsetAsync(c->dstatus, 0, nb * sizeof(int), c->stream));
    // zero the bottom halves ([I | 0] rows), then K into the top-left, identity, rhs
    for (int b = 0; b < nb; b++)
      BGP_HIP(hipMemsetAsync(c->dK + (size_t)b * ld * ld + (size_t)npad * ld, 0, (size_t)npad * ld * sizeof(double),
                             c->stream));
    // (no kernel of the augmented factorisation reads c->dXeff: bgp_launch_cholesky generates nothing there)
    rc = Kgram  ? bgp_gram_load(c, nb, Kgram + (size_t)off * n * n, 1, use_alpha)
         : warp ? bgp_launch_kbuild_x(c, 0, nb, c->stream, 0, 1, use_alpha, c->dXwP + (size_t)off * nd, nd)
                : bgp_launch_kbuild(c, nb, 0, 1, use_alpha);
    if (rc) return rc;
    hipLaunchKernelGGL(aug_init_kernel, dim3((npad + 255) / 256, nb), dim3(256), 0, c->stream, c->dK, c->dyw, npad, nb);
    rc = bgp_launch_cholesky(c, nb, 1);
    if (rc) return rc;
    hipLaunchKernelGGL(extract_kinv_kernel, dim3(256, nb), dim3(256), 0, c->stream, c->dK, c->dyw, c->dKinv,
                       want_Linv ? (double*)c->dLinv : nullptr, c->dalpha_sol, npad, off);
    BGP_HIP(hipGetLastError());
    if (lml) BGP_HIP(bgp_memcpy_async(lml + off, c->dlml, nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (status) BGP_HIP(bgp_memcpy_async(status + off, c->dstatus, nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (alpha)
      BGP_HIP(bgp_memcpy2d_async(alpha + (size_t)off * n, (size_t)n * sizeof(double),
                               c->dalpha_sol + (size_t)off * npad, (size_t)npad * sizeof(double),
                               (size_t)n * sizeof(double), nb, hipMemcpyDeviceToHost, c->stream));
    if (K_inv)
      for (int b = 0; b < nb; b++)
        BGP_HIP(bgp_memcpy2d_async(K_inv + (size_t)(off + b) * n * n, (size_t)n * sizeof(double),
                                 c->dKinv + (size_t)(off + b) * npad * npad, (size_t)npad * sizeof(double),
                                 (size_t)n * sizeof(double), n, hipMemcpyDeviceToHost, c->stream));
    if (L) {
      BgpScratch live(c);
      double* dL = nullptr;
      rc = live.carve([&](BgpCarve& s) { dL = s.take<double>((size_t)n * n); });
      if (rc) return rc;
      for (int b = 0; b < nb; b++) {
        hipLaunchKernelGGL(extract_L_kernel, dim3(512), dim3(256), 0, c->stream, c->dK, dL, n, (int)ld,
                           ld * ld, b);
        BGP_HIP(bgp_memcpy_async(L + (size_t)(off + b) * n * n, dL, (size_t)n * n * sizeof(double),
                               hipMemcpyDeviceToHost, c->stream));
        BGP_HIP(bgp_stream_sync(c->stream));
      }
    }
    BGP_HIP(bgp_stream_sync(c->stream));
  }
  c->post.commit(B, warp != nullptr);
  return BGP_OK;
}

// ... as an entry point runs it
static int post_build(bgp_ctx* c, int B, const double* h, int use_alpha, double* L, double* alpha, double* K_inv, double* lml,
                      int* status, const double* Kgram = nullptr, const double* warp = nullptr) {
  return post_call(c, [&] { return bgp_posterior_build(c, B, h, use_alpha, L, alpha, K_inv, lml, status, Kgram, true, warp); });
}

extern "C" int bgp_posterior_batch(bgp_ctx* c, int B, const double* h, double* L, double* alpha, double* K_inv,
                                   double* lml, int* status) {
  BGP_TRY(bgp_guard(c, "bgp_posterior_batch"));
  if (!c || !h || B <= 0) {
    bgp_set_error("bgp_posterior_batch: bad argument");
    return BGP_ERR_INVALID;
  }
  return post_build(c, B, h, 1, L, alpha, K_inv, lml, status);
}

// The same posterior build with item b's training inputs passed through ITS OWN Beta-CDF warp, warp[b * 2d .. (b + 1) * 2d) (log
// space, [wa_1..wa_d, wb_1..wb_d], as bgp_lml_batch_warped lays them out): the hyper-posterior draws of warp_inputs=True, every one
// with its own warped design matrix.  A context-level warp is replaced for this call, not composed with it.  The warped inputs stay
// resident beside K^-1 / alpha for bgp_predict_batch_warped, the only reader of these posteriors (bgp_guard, BGP_POST_ROWWARP).
extern "C" int bgp_posterior_batch_warped(bgp_ctx* c, int B, const double* h, const double* warp, double* L, double* alpha,
                                          double* K_inv, double* lml, int* status) {
  BGP_TRY(bgp_guard(c, "bgp_posterior_batch_warped"));
  if (!c || !h || !warp || B <= 0) {
    bgp_set_error("bgp_posterior_batch_warped: bad argument");
    return BGP_ERR_INVALID;
  }
  return post_build(c, B, h, 1, L, alpha, K_inv, lml, status, nullptr, warp);
}

// The same posterior build from HOST-evaluated kernel matrices (generic kernel expression trees, bgp_gram.hip): K is B
// matrices of n x n (kernel_(X_train) without the alpha term), everything behind it as bgp_posterior_batch.
extern "C" int bgp_posterior_batch_gram(bgp_ctx* c, int B, const double* K, int use_alpha, double* L, double* alpha,
                                        double* K_inv, double* lml, int* status) {
  BGP_TRY(bgp_guard(c, "bgp_posterior_batch_gram"));
  if (!c || !K || B <= 0) {
    bgp_set_error("bgp_posterior_batch_gram: bad argument");
    return BGP_ERR_INVALID;
  }
  return post_build(c, B, nullptr, use_alpha, L, alpha, K_inv, lml, status, K);
}

// ------------------------------------------------------------------------------------------
// predict
// ------------------------------------------------------------------------------------------
static double kernel_diag_value(const bgp_ctx* c, const double* hk) {
  // kernel_.diag(X) incl. the white level: sklearn/kernels.py:868-884, 968-984
  const double cst = std::exp(hk[0]), s2 = std::exp(hk[c->d + 1]);
  const double base = (c->ks.form == BGP_FORM_PRODUCT) ? cst * 1.0 : cst + 1.0;
  return base + s2;
}

__global__ void add_diag_batch_kernel(double* __restrict__ C, int ld, size_t sC, int m, const double* __restrict__ H,
                                      int d) {
  // + white level of item b on the diagonal of its m x m block (kernel_(X) of a Sum with WhiteKernel)
  const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (i < m) C[(size_t)b * sC + (size_t)i * ld + i] += exp(H[(size_t)b * (d + 2) + d + 1]);
}

// Posteriors are processed in chunks of `nb` items whose scratch slices sit side by side: every launch covers the
// whole chunk (grid.y = item), nothing synchronises inside a chunk, and the host waits once at the end of the call.
// Results per item are the same bits as an item-by-item loop (each item's tiles are reduced in the same order).
struct AcqPlan {  // closed-form acquisitions evaluated on the device-resident mean / variance (bgp_acq_batch)
  int n_acq = 0;
  const int* kinds = nullptr;
  const double* params = nullptr;
  double y_mean = 0.0, y_std = 1.0;
  int n_samples = 1;
  double* out = nullptr;  // host, n_acq * m
};
struct AcqScratch {  // device regions of acq_run
  double *dT = nullptr, *dacc = nullptr, *dmumin = nullptr, *dparams = nullptr;
  int *dbad = nullptr, *dkinds = nullptr;
  void take(BgpCarve& s, int n_acq, int B, int mpad) {
    dT = s.take<double>((size_t)n_acq * B * mpad);  // every acquisition of every draw
    dacc = s.take<double>((size_t)n_acq * mpad);    // ... averaged over the draws
    dmumin = s.take<double>(B);                     // lowest mean of every draw
    dbad = s.take<int>((size_t)n_acq * B);          // draw has a non-finite value
    dkinds = s.take<int>(n_acq);
    dparams = s.take<double>(n_acq);
  }
};
static int acq_run(bgp_ctx* c, int B, int m, int mpad, const double* dmean, const double* dvar, const AcqPlan& ap,
                   const AcqScratch& as);

// Where post_cov takes K_** = kernel_(Xq) from: generated by the cross kernel from the staged queries, with the white level of
// the items' hyper-vectors on the diagonal (no white noise off it) -- or uploaded.
struct PostKss {
  const double *dH = nullptr, *dXq = nullptr;  // generated for the device hyper-vectors dH (nb x (d + 2)); white level: exp on the device,
  const double* hk = nullptr;                  // ... or, for ONE item, std::exp of this host copy (bgp_sample_y: not the same bits)
  const double* host = nullptr;                // uploaded: nb host matrices of m x m with their diagonal, zero padded here
};
// The predictive covariance of nb items: P = K_* K^-1 (item b's K^-1 is Kinv[pidxB ? pidxB[b] : b]), K_** into dC, then
// dC -= P K_*^T -- or, with ``factor``, Kinv holds L^-1 instead: P = K_* L^-T, dC -= P P^T.  The product with the explicit
// inverse carries kappa(K) eps |K^-1| into the covariance, which a Cholesky factorisation of it then amplifies by the
// covariance's own condition number (16 tol on the draws at kappa 7e4 / 2e5); the factor's inverse carries sqrt(kappa) and
// the subtraction is a difference of squares.  The draws use the factor; predict(return_cov) keeps the inverse, so that its
// diagonal stays the variance's own arithmetic.  Mode 2: the whole square (every element is read and written by the same lane), mode 1: the lower tiles only (all a
// factorisation reads).  Both products on the LDS-DMA ring (gemm4_kernel).  cov != NULL: the nb matrices go back to the host.
static int post_cov(bgp_ctx* c, int nb, int m, const double* dKs, const double* Kinv, const int* pidxB, double* dP,
                    const PostKss& kss, int mode, double* dC, double* cov = nullptr, bool factor = false) {
  const int npad = c->npad, d = c->d, mpad = pad128(m);
  const size_t sKs = (size_t)mpad * npad, sC = (size_t)mpad * mpad;
  bgp_launch_gemm4(c->stream, 0, dKs, Kinv, npad, mpad, npad, npad, dP, npad, nb, sKs, (size_t)npad * npad, sKs, pidxB);
  if (kss.host) {
    BGP_HIP(hipMemsetAsync(dC, 0, (size_t)nb * sC * sizeof(double), c->stream));
    for (int b = 0; b < nb; b++) BGP_HIP(rows_up(c, dC + (size_t)b * sC, kss.host + (size_t)b * m * m, m, mpad, m));
  } else {
    BGP_TRY(bgp_launch_kcross_batch(c, nb, kss.dH, m, kss.dXq, m, kss.dXq, dC, mpad, sC));
    if (kss.hk)
      hipLaunchKernelGGL(add_diag_kernel, dim3((m + 255) / 256), dim3(256), 0, c->stream, dC, mpad, m, std::exp(kss.hk[d + 1]));
    else
      hipLaunchKernelGGL(add_diag_batch_kernel, dim3((m + 255) / 256, nb), dim3(256), 0, c->stream, dC, mpad, sC, m, kss.dH, d);
  }
  bgp_launch_gemm4(c->stream, mode, dP, factor ? dP : dKs, npad, mpad, mpad, npad, dC, mpad, nb, sKs, sKs, sC, nullptr);
  BGP_HIP(hipGetLastError());
  for (int b = 0; cov && b < nb; b++) BGP_HIP(rows_down(c, cov + (size_t)b * m * m, dC + (size_t)b * sC, m, mpad, m));
  return BGP_OK;
}

// rowwarp: the resident posteriors are per-row warped -- item b reads its own training inputs (c->dXwP) and its own warped copy of
// the queries (one upload of the m rows, ONE warp launch over the B parameter sets in c->dwarpP); no cov there.
static int predict_run(bgp_ctx* c, int B, const double* h_kernel, int m, const double* Xq, double* mean, double* var,
                       double* cov, const AcqPlan* ap, bool rowwarp = false, const BgpMixPlan* mp = nullptr) {
  const int npad = c->npad, n = c->n, d = c->d, mpad = pad128(m);
  const size_t p = d + 2, sKs = (size_t)mpad * npad, sCv = (size_t)mpad * mpad;
  const size_t qs = rowwarp ? (size_t)m * d : 0, xs = rowwarp ? (size_t)n * d : 0;  // per-item strides of queries / training inputs
  // (1 << 30 doubles of scratch per chunk: 8 GiB of the 288 GB)
  const int chunk = post_chunk(B, sKs + 2 * (size_t)mpad + (cov ? sKs + sCv : 0), (size_t)1 << 30, true);
  const int n_acq = ap ? ap->n_acq : 0;
  double *dXq, *dXq0 = nullptr, *dH, *dKs, *dmpart, *dqB, *doutB, *dP = nullptr, *dCov = nullptr;
  AcqScratch as;
  BgpMixScratch ms;
  BgpScratch live(c);
  BGP_TRY(live.carve([&](BgpCarve& s) {
    dXq = s.take<double>(rowwarp ? (size_t)B * qs : (size_t)m * d);  // (every item's warped queries: all B, as dqB / doutB)
    if (rowwarp) dXq0 = s.take<double>((size_t)m * d);              // the un-warped rows they are made from
    dH = s.take<double>((size_t)B * p);
    dKs = s.take<double>((size_t)chunk * sKs);
    dmpart = s.take<double>((size_t)chunk * (npad / 128) * mpad);  // column-tile partials of the means
    dqB = s.take<double>((size_t)B * mpad);    // variance of every item (stays on the device for the acquisitions)
    doutB = s.take<double>((size_t)B * mpad);  // mean of every item
    if (cov) {
      dP = s.take<double>((size_t)chunk * sKs);
      dCov = s.take<double>((size_t)chunk * sCv);
    }
    if (n_acq) as.take(s, n_acq, B, mpad);
    if (mp) ms.take(s, B, mpad, mp->Q);
  }));
  if (rowwarp) {
    BGP_HIP(bgp_memcpy_async(dXq0, Xq, (size_t)m * d * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BGP_TRY(bgp_launch_warp(c, c->stream, dXq0, c->dwarpP, dXq, m, B, qs));
  } else {
    BGP_TRY(post_stage_queries(c, dXq, Xq, m));
  }
  const double* dXt = rowwarp ? (const double*)c->dXwP : (const double*)c->dXeff;
  BGP_HIP(bgp_memcpy_async(dH, h_kernel, (size_t)B * p * sizeof(double), hipMemcpyHostToDevice, c->stream));
  c->chunk_last[0] = 0, c->chunk_last[1] = 1;
  for (int off = 0; off < B; off += chunk) {
    const int nb = std::min(chunk, B - off);
    c->chunk_last[0]++;
    const double* dHc = dH + (size_t)off * p;
    const double* Kinv = c->dKinv + (size_t)off * npad * npad;  // items off .. off+nb-1 are posteriors off .. off+nb-1
    const double* al = c->dalpha_sol + (size_t)off * npad;
    double *dq = dqB + (size_t)off * mpad, *dout = doutB + (size_t)off * mpad;
    BGP_TRY(bgp_launch_moments(c, nb, dHc, m, dXq + (size_t)off * qs, qs, dXt + (size_t)off * xs, xs, al, Kinv, dKs, npad, sKs, dmpart,
                               dout, dq));
    if (mean) BGP_HIP(rows_down(c, mean + (size_t)off * m, dout, m, mpad, nb));
    // (the covariance reads K_* and K^-1 and writes dP / dCov, never dq: behind the moments it leaves their bits alone)
    if (cov) BGP_TRY(post_cov(c, nb, m, dKs, Kinv, nullptr, dP, PostKss{dHc, dXq}, 2, dCov, cov + (size_t)off * m * m));  // (never rowwarp)
    if (var) BGP_HIP(rows_down(c, var + (size_t)off * m, dq, m, mpad, nb));
    // (the next chunk reuses the scratch slices: stream order keeps its launches behind these copies)
  }
  if (n_acq) BGP_TRY(acq_run(c, B, m, mpad, doutB, dqB, *ap, as));
  if (mp) BGP_TRY(bgp_mix_run(c, B, m, mpad, doutB, dqB, *mp, ms));  // the hyper-posterior mixture of the B rows (bgp_mix.hip)
  BGP_HIP(bgp_stream_sync(c->stream));
  return BGP_OK;
}

int bgp_predict_run_mix(bgp_ctx* c, int B, const double* h_kernel, int m, const double* Xq, const BgpMixPlan& mp, bool rowwarp) {
  return predict_run(c, B, h_kernel, m, Xq, nullptr, nullptr, nullptr, nullptr, rowwarp, &mp);
}

extern "C" int bgp_predict_batch(bgp_ctx* c, int B, const double* h_kernel, int m, const double* Xq, double* mean,
                                 double* var, double* cov) {
  BGP_TRY(bgp_guard(c, "bgp_predict_batch", BGP_POST_PLAIN));
  if (!c || !h_kernel || !Xq || !mean || !var || m <= 0 || B <= 0) {
    bgp_set_error("bgp_predict_batch: bad argument");
    return BGP_ERR_INVALID;
  }
  BGP_TRY(bgp_guard(c, "bgp_predict_batch", BGP_POST_PLAIN, B));
  return post_call(c, [&] { return predict_run(c, B, h_kernel, m, Xq, mean, var, cov, nullptr); });
}

// Predict for per-row-warped resident posteriors (bgp_posterior_batch_warped): item b sees the m query rows through ITS warp and
// its own warped training inputs; everything behind the cross build is bgp_predict_batch's (predict_run).  Mean and variance only.
extern "C" int bgp_predict_batch_warped(bgp_ctx* c, int B, const double* h_kernel, int m, const double* Xq, double* mean,
                                        double* var) {
  BGP_TRY(bgp_guard(c, "bgp_predict_batch_warped"));
  if (!c || !h_kernel || !Xq || !mean || !var || m <= 0 || B <= 0) {
    bgp_set_error("bgp_predict_batch_warped: bad argument");
    return BGP_ERR_INVALID;
  }
  BGP_TRY(bgp_guard(c, "bgp_predict_batch_warped", BGP_POST_ROWWARP, B));
  return post_call(c, [&] { return predict_run(c, B, h_kernel, m, Xq, mean, var, nullptr, nullptr, true); });
}

// var_i = max(0, kss_i - q_i) with the prior variances kernel_.diag(Xq) supplied by the host (generic kernels)
__global__ void finish_var_gram_kernel(const double* __restrict__ q, const double* __restrict__ kss, size_t sq, int m,
                                       double* __restrict__ var) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
  if (i >= m) return;
  const double v = kss[(size_t)b * sq + i] - q[(size_t)b * sq + i];
  var[(size_t)b * sq + i] = v < 0.0 ? 0.0 : v;
}

// Predict with HOST-evaluated cross covariances for the B resident posteriors (generic kernel expression trees): Ks is B x m x n
// (kernel_(Xq, X_train) per item), kss B x m (kernel_.diag(Xq)), Kss B x m x m (kernel_(Xq); only with cov).  The products --
// mean = K_* alpha, var = kss - rowsum((K_* K^-1) o K_*), cov = K_** - (K_* K^-1) K_*^T -- are the kernels of bgp_predict_batch.
extern "C" int bgp_predict_batch_gram(bgp_ctx* c, int B, int m, const double* Ks, const double* kss, const double* Kss,
                                      double* mean, double* var, double* cov) {
  BGP_TRY(bgp_guard(c, "bgp_predict_batch_gram"));
  if (!c || !Ks || !kss || !mean || !var || m <= 0 || B <= 0 || (cov && !Kss)) {
    bgp_set_error("bgp_predict_batch_gram: bad argument");
    return BGP_ERR_INVALID;
  }
  BGP_TRY(bgp_guard(c, "bgp_predict_batch_gram", BGP_POST_ANY, B));
  return post_call(c, [&]() -> int {
    const int npad = c->npad, n = c->n, mpad = pad128(m);
    const size_t sKs = (size_t)mpad * npad, sCv = (size_t)mpad * mpad;
    const int chunk = post_chunk(B, sKs + 3 * (size_t)mpad + (cov ? sKs + sCv : 0), (size_t)1 << 29, true);
    double *dKs, *dq, *dout, *dkss, *dP = nullptr, *dCov = nullptr;
    BgpScratch live(c);
    BGP_TRY(live.carve([&](BgpCarve& s) {
      dKs = s.take<double>((size_t)chunk * sKs);
      dq = s.take<double>((size_t)chunk * mpad);
      dout = s.take<double>((size_t)chunk * mpad);
      dkss = s.take<double>((size_t)chunk * mpad);
      if (cov) {
        dP = s.take<double>((size_t)chunk * sKs);
        dCov = s.take<double>((size_t)chunk * sCv);
      }
    }));
    c->chunk_last[0] = 0, c->chunk_last[1] = 1;
    for (int off = 0; off < B; off += chunk) {
      const int nb = std::min(chunk, B - off);
      c->chunk_last[0]++;
      const double* Kinv = c->dKinv + (size_t)off * npad * npad;
      const double* al = c->dalpha_sol + (size_t)off * npad;
      // K_* with its zero padding (rows m .. mpad, columns n .. npad)
      BGP_HIP(hipMemsetAsync(dKs, 0, (size_t)nb * sKs * sizeof(double), c->stream));
      for (int b = 0; b < nb; b++) BGP_HIP(rows_up(c, dKs + (size_t)b * sKs, Ks + (size_t)(off + b) * m * n, n, npad, m));
      BGP_HIP(rows_up(c, dkss, kss + (size_t)off * m, m, mpad, nb));
      hipLaunchKernelGGL(matvec_rows_kernel, dim3((m + 3) / 4, nb), dim3(256), 0, c->stream, dKs, npad, sKs, al, (size_t)npad,
                         (const int*)nullptr, npad, m, dout, (size_t)mpad);
      BGP_HIP(rows_down(c, mean + (size_t)off * m, dout, m, mpad, nb));
      BGP_TRY(launch_rowquad(c, dKs, npad, sKs, Kinv, npad, (size_t)npad * npad, nullptr, mpad, npad, nb, dq));
      if (cov) {
        PostKss src;
        src.host = Kss + (size_t)off * m * m;
        BGP_TRY(post_cov(c, nb, m, dKs, Kinv, nullptr, dP, src, 2, dCov, cov + (size_t)off * m * m));
      }
      hipLaunchKernelGGL(finish_var_gram_kernel, dim3((m + 255) / 256, nb), dim3(256), 0, c->stream, dq, dkss, (size_t)mpad, m, dq);
      BGP_HIP(hipGetLastError());
      BGP_HIP(rows_down(c, var + (size_t)off * m, dq, m, mpad, nb));
      BGP_HIP(bgp_stream_sync(c->stream));  // (the next chunk reuses the staged host slices' arena and the scratch)
    }
    return BGP_OK;
  });
}

// ------------------------------------------------------------------------------------------
// Closed-form acquisition functions on the device (bask/acquisition.py:154-172 ExpectedImprovement, :197-201
// Expectation, :204-216 LCB), averaged over the hyper-posterior draws exactly like evaluate_acquisitions
// (:112-139): per draw b  tmp = acq(mu_b, std_b);  a draw whose values are not all finite contributes nothing;
// out = sum_b tmp_b / n_samples in draw order (one thread per candidate walks the draws: no atomics on doubles).
// mu = y_std * mean + y_mean, std = sqrt(var * y_std^2) as BayesGPR.predict returns them (skopt predict).
// ------------------------------------------------------------------------------------------
static __device__ __forceinline__ double acq_ndtr(double a) {
  // Phi(a) the way scipy.special.ndtr (cephes) evaluates it: erf near 0, erfc in the tails
  const double x = a * 0.70710678118654752440, z = fabs(x);
  if (z < 0.70710678118654752440) return 0.5 + 0.5 * erf(x);
  double y = 0.5 * erfc(z);
  if (x > 0) y = 1.0 - y;
  return y;
}

static __device__ __forceinline__ double acq_value(int kind, double param, double mu, double sd, double mumin) {
#pragma clang fp contract(off)
  if (kind == BGP_ACQ_MEAN) return -mu;
  if (kind == BGP_ACQ_STD) return sd;
  if (kind == BGP_ACQ_LCB) return param * sd - mu;
  // expected improvement over y_opt (default: this draw's lowest mean); zero where std is not positive
  if (!(sd > 0.0)) return 0.0;
  const double y_opt = isnan(param) ? mumin : param;
  const double x = (y_opt - mu) / sd;
  const double f = x * acq_ndtr(x) + exp(-(x * x) / 2.0) / 2.5066282746310002;  // sqrt(2 pi)
  return f * sd;
}

// np.min over one draw's means (NaN if any is NaN)
__global__ void __launch_bounds__(256) acq_mumin_kernel(const double* __restrict__ mean, size_t smean, int m,
                                                         double y_mean, double y_std, double* __restrict__ mumin) {
#pragma clang fp contract(off)
  const int b = blockIdx.x, tid = threadIdx.x;
  double best = INFINITY;
  int nan = 0;
  for (int i = tid; i < m; i += 256) {
    const double mu = y_std * mean[(size_t)b * smean + i] + y_mean;
    if (isnan(mu)) nan = 1;
    best = fmin(best, mu);
  }
  __shared__ double sb[256];
  __shared__ int sn[256];
  sb[tid] = best, sn[tid] = nan;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sb[tid] = fmin(sb[tid], sb[tid + o]), sn[tid] |= sn[tid + o];
    __syncthreads();
  }
  if (tid == 0) mumin[b] = sn[0] ? NAN : sb[0];
}

__global__ void __launch_bounds__(256) acq_values_kernel(const double* __restrict__ mean, const double* __restrict__ var,
                                                          size_t sm, int m, int B, double y_mean, double y_std, int n_acq,
                                                          const int* __restrict__ kinds,
                                                          const double* __restrict__ params,
                                                          const double* __restrict__ mumin, double* __restrict__ T,
                                                          int* __restrict__ bad) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= m) return;
  const double mu = y_std * mean[(size_t)b * sm + i] + y_mean;
  const double sd = sqrt(var[(size_t)b * sm + i] * (y_std * y_std));
  for (int k = 0; k < n_acq; k++) {
    const double v = acq_value(kinds[k], params[k], mu, sd, mumin[b]);
    T[((size_t)k * B + b) * sm + i] = v;
    if (!isfinite(v)) atomicOr(&bad[k * B + b], 1);
  }
}

__global__ void __launch_bounds__(256) acq_sum_kernel(const double* __restrict__ T, const int* __restrict__ bad, size_t sm,
                                                       int m, int B, int n_samples, double* __restrict__ acc) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
  if (i >= m) return;
  double s = 0.0;
  const double ns = (double)n_samples;
  for (int b = 0; b < B; b++)
    if (!bad[k * B + b]) s += T[((size_t)k * B + b) * sm + i] / ns;
  acc[(size_t)k * sm + i] = s;
}

__global__ void acq_square_kernel(double* __restrict__ v, size_t sv, int m) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i < m) v[(size_t)b * sv + i] *= v[(size_t)b * sv + i];
}

static int acq_run(bgp_ctx* c, int B, int m, int mpad, const double* dmean, const double* dvar, const AcqPlan& ap,
                   const AcqScratch& as) {
  hipStream_t st = c->stream;
  BGP_HIP(bgp_memcpy_async(as.dkinds, ap.kinds, (size_t)ap.n_acq * sizeof(int), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(as.dparams, ap.params, (size_t)ap.n_acq * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(hipMemsetAsync(as.dbad, 0, (size_t)ap.n_acq * B * sizeof(int), st));
  hipLaunchKernelGGL(acq_mumin_kernel, dim3(B), dim3(256), 0, st, dmean, (size_t)mpad, m, ap.y_mean, ap.y_std, as.dmumin);
  hipLaunchKernelGGL(acq_values_kernel, dim3((m + 255) / 256, B), dim3(256), 0, st, dmean, dvar, (size_t)mpad, m, B,
                     ap.y_mean, ap.y_std, ap.n_acq, as.dkinds, as.dparams, as.dmumin, as.dT, as.dbad);
  hipLaunchKernelGGL(acq_sum_kernel, dim3((m + 255) / 256, ap.n_acq), dim3(256), 0, st, as.dT, as.dbad, (size_t)mpad, m, B,
                     ap.n_samples, as.dacc);
  BGP_HIP(hipGetLastError());
  BGP_HIP(rows_down(c, ap.out, as.dacc, m, mpad, ap.n_acq));
  return BGP_OK;
}

static int acq_check(const char* who, int n_acq, const int* kinds, const double* params, int n_samples, const double* out) {
  if (n_acq <= 0 || n_acq > BGP_ACQ_MAX || !kinds || !params || !out || n_samples <= 0) {
    bgp_set_error("%s: bad argument (1 <= n_acq <= %d)", who, BGP_ACQ_MAX);
    return BGP_ERR_INVALID;
  }
  for (int k = 0; k < n_acq; k++)
    if (kinds[k] < BGP_ACQ_EI || kinds[k] > BGP_ACQ_STD) {
      bgp_set_error("%s: unknown acquisition kind %d", who, kinds[k]);
      return BGP_ERR_INVALID;
    }
  return BGP_OK;
}

extern "C" int bgp_acq_batch(bgp_ctx* c, int B, const double* h_kernel, int m, const double* Xq, double y_mean,
                             double y_std, int n_acq, const int* kinds, const double* params, int n_samples,
                             double* out) {
  BGP_TRY(bgp_guard(c, "bgp_acq_batch", BGP_POST_PLAIN));
  if (!c || !h_kernel || !Xq || m <= 0 || B <= 0) {
    bgp_set_error("bgp_acq_batch: bad argument");
    return BGP_ERR_INVALID;
  }
  BGP_TRY(acq_check("bgp_acq_batch", n_acq, kinds, params, n_samples, out));
  AcqPlan ap;
  ap.n_acq = n_acq, ap.kinds = kinds, ap.params = params, ap.y_mean = y_mean, ap.y_std = y_std, ap.n_samples = n_samples;
  ap.out = out;
  BGP_TRY(bgp_guard(c, "bgp_acq_batch", BGP_POST_PLAIN, B));
  return post_call(c, [&] { return predict_run(c, B, h_kernel, m, Xq, nullptr, nullptr, nullptr, &ap); });
}

// The same closed forms on caller-supplied (mu, std) rows: B x m each, already in y units (y_mean = 0, y_std = 1).
extern "C" int bgp_acq_values(bgp_ctx* c, int B, int m, const double* mu, const double* std_, int n_acq, const int* kinds,
                              const double* params, int n_samples, double* out) {
  BGP_TRY(bgp_guard(c, "bgp_acq_values"));
  if (!c || !mu || !std_ || m <= 0 || B <= 0) {
    bgp_set_error("bgp_acq_values: bad argument");
    return BGP_ERR_INVALID;
  }
  BGP_TRY(acq_check("bgp_acq_values", n_acq, kinds, params, n_samples, out));
  return post_call(c, [&]() -> int {
    const int mpad = pad128(m);
    double *dmu, *dvar;
    AcqScratch as;
    BgpScratch live(c);
    BGP_TRY(live.carve([&](BgpCarve& s) {
      dmu = s.take<double>((size_t)B * mpad);
      dvar = s.take<double>((size_t)B * mpad);
      as.take(s, n_acq, B, mpad);
    }));
    BGP_HIP(rows_up(c, dmu, mu, m, mpad, B));
    BGP_HIP(rows_up(c, dvar, std_, m, mpad, B));
    hipLaunchKernelGGL(acq_square_kernel, dim3((m + 255) / 256, B), dim3(256), 0, c->stream, dvar, (size_t)mpad, m);
    AcqPlan ap;
    ap.n_acq = n_acq, ap.kinds = kinds, ap.params = params, ap.n_samples = n_samples, ap.out = out;
    BGP_TRY(acq_run(c, B, m, mpad, dmu, dvar, ap, as));
    BGP_HIP(bgp_stream_sync(c->stream));
    return BGP_OK;
  });
}

// ------------------------------------------------------------------------------------------
// LML gradient:  g_k = 1/2 sum_ij (alpha_i alpha_j - Kinv_ij) dK_ij/dh_k   (sklearn/_gpr.py:615-647)
// One workgroup per lower-triangular 128x128 tile (off-diagonal tiles count twice); per-dimension
// sums are reduced in the workgroup and stored to gpart[b][tile][k]; grad_reduce_kernel adds the tiles in a
// fixed order (bitwise reproducible gradients: no floating-point atomics).
// ------------------------------------------------------------------------------------------
#define GR_DK 16
__global__ void __launch_bounds__(256) lml_grad_kernel(const double* __restrict__ X,
                                                        const double* __restrict__ H,
                                                        const double* __restrict__ Kinv,
                                                        const double* __restrict__ alpha_sol,
                                                        double* __restrict__ gpart, int n, int d, int npad, int nblk,
                                                        int form, int stat, int B) {
  const int ntiles = nblk * (nblk + 1) / 2;
  int b, t;
  bgp_map_block(blockIdx.x, ntiles, B, b, t);
  if (b >= B) return;
  double* gp = gpart + ((size_t)b * ntiles + t) * (d + 2);
  int ti, tj;
  bgp_tri_decode(t, ti, tj);
  __shared__ double xi[GR_DK][BGP_TILE_LD];
  __shared__ double xj[GR_DK][BGP_TILE_LD];
  __shared__ double ell[GR_DK];
  __shared__ double red[4][GR_DK + 2];
  const double* h = H + (size_t)b * (d + 2);
  const double* Ki = Kinv + (size_t)b * npad * npad;
  const double* al = alpha_sol + (size_t)b * npad;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63, w = tid >> 6;
  const int i0 = ti * 128, j0 = tj * 128;
  const double wtile = (ti == tj) ? 1.0 : 2.0;
  double F[8][8];
#pragma unroll
  for (int r = 0; r < 8; r++)
#pragma unroll
    for (int c = 0; c < 8; c++) F[r][c] = 0.0;
  // pass 1: squared scaled distances
  for (int k0 = 0; k0 < d; k0 += GR_DK) {
    const int kc = min(GR_DK, d - k0);
    __syncthreads();
    if (tid < kc) ell[tid] = exp(h[1 + k0 + tid]);
    __syncthreads();
    for (int idx = tid; idx < kc * 128; idx += 256) {
      int row = idx / kc, k = idx - row * kc;
      int gi = i0 + row, gj = j0 + row;
      xi[k][row] = (gi < n) ? X[(size_t)gi * d + k0 + k] / ell[k] : 0.0;
      xj[k][row] = (gj < n) ? X[(size_t)gj * d + k0 + k] / ell[k] : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < kc; k++) {
      double a[8], bb[8];
#pragma unroll
      for (int r = 0; r < 8; r++) a[r] = xi[k][ty + 16 * r];
#pragma unroll
      for (int c = 0; c < 8; c++) bb[c] = xj[k][tx + 16 * c];
#pragma unroll
      for (int r = 0; r < 8; r++)
#pragma unroll
        for (int c = 0; c < 8; c++) {
          double df = a[r] - bb[c];
          F[r][c] += df * df;
        }
    }
  }
  // F_ij = W_ij * f(r_ij);   constant / noise terms on the fly
  const double cst = exp(h[0]), s2 = exp(h[d + 1]);
  const double cf = (form == BGP_FORM_PRODUCT) ? cst : 1.0;
  double g_const = 0.0, g_noise = 0.0;
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const int gi = i0 + ty + 16 * r;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const int gj = j0 + tx + 16 * c;
      double f = 0.0;
      if (gi < n && gj < n) {
        const double Wij = al[gi] * al[gj] - Ki[(size_t)gi * npad + gj];
        if (gi == gj) {
          g_const += Wij * ((form == BGP_FORM_PRODUCT) ? cst * 1.0 : cst);
          g_noise += Wij * s2;
        } else {
          const double r2 = F[r][c];
          double S, fr;  // (not kb_stationary_fac: runtime stat, libm exp / sqrt, default contraction -- moving would change gradient bits)
          if (stat == BGP_RBF) {
            S = exp(-0.5 * r2);
            fr = S;
          } else if (stat == BGP_MATERN12) {
            const double rr = sqrt(r2);
            S = exp(-rr);
            fr = (rr > 0.0) ? S / rr : 0.0;
          } else if (stat == BGP_MATERN32) {
            const double tt = sqrt(r2) * 1.7320508075688772;
            const double e = exp(-tt);
            S = (1.0 + tt) * e;
            fr = 3.0 * e;
          } else {
            const double tt = sqrt(r2) * 2.23606797749979;
            const double e = exp(-tt);
            S = (1.0 + tt + tt * tt / 3.0) * e;
            fr = (5.0 / 3.0) * (tt + 1.0) * e;
          }
          g_const += wtile * Wij * ((form == BGP_FORM_PRODUCT) ? cst * S : cst);
          f = wtile * Wij * cf * fr;
        }
      }
      F[r][c] = f;
    }
  }
  // pass 2: per-dimension sums  sum_ij F_ij (x_ik - x_jk)^2 / l_k^2
  for (int k0 = 0; k0 < d; k0 += GR_DK) {
    const int kc = min(GR_DK, d - k0);
    __syncthreads();
    if (tid < kc) ell[tid] = exp(h[1 + k0 + tid]);
    __syncthreads();
    if (d > GR_DK) {  // tiles still staged from pass 1 when d fits in one chunk
      for (int idx = tid; idx < kc * 128; idx += 256) {
        int row = idx / kc, k = idx - row * kc;
        int gi = i0 + row, gj = j0 + row;
        xi[k][row] = (gi < n) ? X[(size_t)gi * d + k0 + k] / ell[k] : 0.0;
        xj[k][row] = (gj < n) ? X[(size_t)gj * d + k0 + k] / ell[k] : 0.0;
      }
      __syncthreads();
    }
    for (int k = 0; k < kc; k++) {
      double a[8], bb[8];
#pragma unroll
      for (int r = 0; r < 8; r++) a[r] = xi[k][ty + 16 * r];
#pragma unroll
      for (int c = 0; c < 8; c++) bb[c] = xj[k][tx + 16 * c];
      double sk = 0.0;
#pragma unroll
      for (int r = 0; r < 8; r++)
#pragma unroll
        for (int c = 0; c < 8; c++) {
          double df = a[r] - bb[c];
          sk += F[r][c] * df * df;
        }
      for (int o = 32; o > 0; o >>= 1) sk += __shfl_xor(sk, o);
      if (lane == 0) red[w][k] = sk;
    }
    __syncthreads();
    if (tid < kc) gp[1 + k0 + tid] = 0.5 * (red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid]);
  }
  for (int o = 32; o > 0; o >>= 1) {
    g_const += __shfl_xor(g_const, o);
    g_noise += __shfl_xor(g_noise, o);
  }
  __syncthreads();
  if (lane == 0) {
    red[w][0] = g_const;
    red[w][1] = g_noise;
  }
  __syncthreads();
  if (tid == 0) {
    gp[0] = 0.5 * (red[0][0] + red[1][0] + red[2][0] + red[3][0]);
    gp[d + 1] = 0.5 * (red[0][1] + red[1][1] + red[2][1] + red[3][1]);
  }
}

__global__ void grad_reduce_kernel(const double* __restrict__ gpart, double* __restrict__ grad, int ntiles, int p) {
  const int b = blockIdx.x, k = threadIdx.x;
  if (k >= p) return;
  double s = 0.0;
  for (int t = 0; t < ntiles; t++) s += gpart[((size_t)b * ntiles + t) * p + k];
  grad[(size_t)b * p + k] = s;
}

extern "C" int bgp_lml_grad_batch(bgp_ctx* c, int B, const double* h, double* lml, double* grad, int* status) {
  BGP_TRY(bgp_guard(c, "bgp_lml_grad_batch"));
  if (!c || !h || !lml || !grad || B <= 0) {
    bgp_set_error("bgp_lml_grad_batch: bad argument");
    return BGP_ERR_INVALID;
  }
  return post_call(c, [&]() -> int {
    const size_t p = c->d + 2;
    std::vector<int> st(B, 0);
    BGP_TRY(bgp_posterior_build(c, B, h, 1, nullptr, nullptr, nullptr, lml, st.data(), nullptr, false));
    c->post.drop();  // the resident K^-1 belong to a gradient evaluation, not to a posterior (the build has counted a generation)
    const int ntiles = c->nblk * (c->nblk + 1) / 2;
    double *dgrad, *dH, *dgpart;
    BgpScratch live(c);
    BGP_TRY(live.carve([&](BgpCarve& s) {
      dgrad = s.take<double>((size_t)B * p);
      dH = s.take<double>((size_t)B * p);
      dgpart = s.take<double>((size_t)B * p * ntiles);
    }));
    BGP_HIP(hipMemsetAsync(dgpart, 0, (size_t)B * p * ntiles * sizeof(double), c->stream));
    BGP_HIP(bgp_memcpy_async(dH, h, (size_t)B * p * sizeof(double), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(lml_grad_kernel, dim3(8 * ((B + 7) / 8) * ntiles), dim3(256), 0, c->stream, c->dXeff, dH, c->dKinv,
                       c->dalpha_sol, dgpart, c->n, c->d, c->npad, c->nblk, c->ks.form, c->ks.stationary, B);
    BGP_HIP(hipGetLastError());
    hipLaunchKernelGGL(grad_reduce_kernel, dim3(B), dim3(((int)p + 63) / 64 * 64), 0, c->stream, dgpart, dgrad, ntiles,
                       (int)p);
    BGP_HIP(hipGetLastError());
    BGP_HIP(bgp_memcpy_async(grad, dgrad, (size_t)B * p * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BGP_HIP(bgp_stream_sync(c->stream));
    for (int b = 0; b < B; b++) {
      if (st[b] != 0)
        for (size_t k = 0; k < p; k++) grad[(size_t)b * p + k] = 0.0;  // sklearn/_gpr.py:589: (-inf, zeros)
      if (status) status[b] = st[b];
    }
    return BGP_OK;
  });
}

// ------------------------------------------------------------------------------------------
// PVRS (bask/acquisition.py:328-338) through the bordered-inverse identity:
//   covs[i] = sum_t [ k_t^T Kinv k_t + (k(x_t, x_i) - k_i^T Kinv k_t)^2 / (kappa - k_i^T Kinv k_i) ]
// ------------------------------------------------------------------------------------------
__global__ void pvrs_combine_kernel(const double* __restrict__ G, int ldg, const double* __restrict__ Kti, int ldk,
                                    const double* __restrict__ u, const double* __restrict__ st, double kappa, int m,
                                    int T, double* __restrict__ covs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const double lam2 = kappa - u[i];
  double s = 0.0;
  for (int t = 0; t < T; t++) {
    const double e = Kti[(size_t)i * ldk + t] - G[(size_t)i * ldg + t];
    s += st[t] + e * e / lam2;
  }
  covs[i] = s;
}

extern "C" int bgp_pvrs(bgp_ctx* c, const double* h_kernel, int m, const double* Xcand, int T,
                        const double* Xthompson, double* covs) {
  BGP_TRY(bgp_guard(c, "bgp_pvrs", BGP_POST_PLAIN));
  if (!c || !h_kernel || !Xcand || !Xthompson || !covs || m <= 0 || T <= 0) {
    bgp_set_error("bgp_pvrs: bad argument");
    return BGP_ERR_INVALID;
  }
  BGP_TRY(bgp_guard(c, "bgp_pvrs", BGP_POST_PLAIN, 1));
  return post_call(c, [&]() -> int {
    const int npad = c->npad, n = c->n, d = c->d, mpad = pad128(m), Tpad = pad128(T);
    const size_t p = d + 2;
    double *dXc, *dXt, *dhk, *dKc, *dKT, *dPT, *dG, *dKti, *du, *dcov, *dst, *dend;
    BgpScratch live(c);
    BGP_TRY(live.carve([&](BgpCarve& s) {
      dXc = s.take<double>((size_t)m * d);
      dXt = s.take<double>((size_t)T * d);
      dhk = s.take<double>(p);
      dKc = s.take<double>((size_t)mpad * npad);   // k(cand, train)
      dKT = s.take<double>((size_t)Tpad * npad);   // k(thompson, train)
      dPT = s.take<double>((size_t)Tpad * npad);   // K_T Kinv
      dG = s.take<double>((size_t)mpad * Tpad);    // K_c Kinv K_T^T
      dKti = s.take<double>((size_t)mpad * Tpad);  // k(cand, thompson)
      du = s.take<double>(mpad);
      dcov = s.take<double>(mpad);
      dst = s.take<double>(Tpad);
      dend = s.take<double>(0);
    }));
    const double* Kinv = c->dKinv;
    BGP_TRY(post_stage_queries(c, dXc, Xcand, m));
    BGP_TRY(post_stage_queries(c, dXt, Xthompson, T));
    BGP_HIP(bgp_memcpy_async(dhk, h_kernel, p * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BGP_HIP(hipMemsetAsync(dKc, 0, (size_t)(dend - dKc) * sizeof(double), c->stream));  // (zero padding of every matrix and vector)
    BGP_TRY(bgp_launch_kcross(c, dhk, m, dXc, n, c->dXeff, dKc, npad));
    BGP_TRY(bgp_launch_kcross(c, dhk, T, dXt, n, c->dXeff, dKT, npad));
    BGP_TRY(bgp_launch_kcross(c, dhk, m, dXc, T, dXt, dKti, Tpad));
    // P_T = K_T Kinv ; s_t = rowsum(P_T o K_T) ; u_i = rowsum((K_c Kinv) o K_c) ; G = K_c P_T^T
    bgp_launch_gemm4(c->stream, 0, dKT, Kinv, npad, Tpad, npad, npad, dPT, npad, 1, 0, 0, 0, nullptr);
    BGP_TRY(launch_rowquad(c, dKT, npad, 0, Kinv, npad, 0, nullptr, Tpad, npad, 1, dst));
    BGP_TRY(launch_rowquad(c, dKc, npad, 0, Kinv, npad, 0, nullptr, mpad, npad, 1, du));
    bgp_launch_gemm4(c->stream, 0, dKc, dPT, npad, mpad, Tpad, npad, dG, Tpad, 1, 0, 0, 0, nullptr);
    hipLaunchKernelGGL(pvrs_combine_kernel, dim3((m + 255) / 256), dim3(256), 0, c->stream, dG, Tpad, dKti, Tpad, du,
                       dst, kernel_diag_value(c, h_kernel), m, T, dcov);
    BGP_HIP(hipGetLastError());
    BGP_HIP(bgp_memcpy_async(covs, dcov, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    BGP_HIP(bgp_stream_sync(c->stream));
    return BGP_OK;
  });
}

extern "C" int bgp_pvrs_prepare(bgp_ctx* c, const double* h_kernel, int has_alpha_vec, int* status) {
  BGP_TRY(bgp_guard(c, "bgp_pvrs_prepare"));
  // K_aug's leading block: kernel_(X_train) + alpha only when alpha is a vector
  // (bask/acquisition.py:332-333)
  if (!c || !h_kernel) {
    bgp_set_error("bgp_pvrs_prepare: bad argument");
    return BGP_ERR_INVALID;
  }
  return post_build(c, 1, h_kernel, has_alpha_vec ? 1 : 0, nullptr, nullptr, nullptr, nullptr, status);
}

// ------------------------------------------------------------------------------------------
// sample_y:  f = mean + L_cov z  with  L_cov = chol(cov + jitter I)  (same batched Cholesky, B = 1)
// ------------------------------------------------------------------------------------------
__global__ void cov_prepare_kernel(double* __restrict__ C, int m, int mpad, double jitter) {
  // jitter on the diagonal, identity padding, zero rhs handled by the caller; blockIdx.y = matrix of a batch
  C += (size_t)blockIdx.y * mpad * mpad;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < (size_t)mpad * mpad;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(idx / mpad), j = (int)(idx - (size_t)i * mpad);
    if (i >= m || j >= m)
      C[idx] = (i == j) ? 1.0 : 0.0;
    else if (i == j)
      C[idx] += jitter;
  }
}

__global__ void zero_upper_kernel(double* __restrict__ C, int mpad) {
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < (size_t)mpad * mpad;
       idx += (size_t)gridDim.x * blockDim.x) {
    const int i = (int)(idx / mpad), j = (int)(idx - (size_t)i * mpad);
    if (j > i) C[idx] = 0.0;
  }
}

__global__ void add_diag_kernel(double* __restrict__ C, int ld, int m, double v) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) C[(size_t)i * ld + i] += v;
}

__global__ void add_mean_rows_kernel(double* __restrict__ out, int ldo, const double* __restrict__ mean, int m,
                                     int rows) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = blockIdx.y;
  if (j < m && i < rows) out[(size_t)i * ldo + j] += mean[j];
}

static int ensure_child(bgp_ctx* c, int mpad, int nb, bgp_ctx** out);

// Child workspace for the Cholesky of nb covariance matrices of m x m (it shares the stream); cached on the context and grown on demand
// (an m = 10 000 candidate grid needs 0.8 GB: re-allocating it per call costs more than the factorisation)
static int post_child(bgp_ctx* c, int m, int nb, bgp_ctx** out) {
  const int mpad = pad128(m);
  BGP_TRY(ensure_child(c, mpad, nb, out));
  (*out)->n = m;
  (*out)->npad = mpad;
  (*out)->nblk = mpad / 128;
  return BGP_OK;
}

// Cholesky of the child's nb matrices in place (rhs and statuses cleared in front of it), the statuses on their way to the host right
// behind it.  allow_launch_free: where the planner (bgp_plan.h) takes the shape, ONE launch-free kernel (a single covariance of 79
// block columns at 10 000 candidates is the longest launch chain of a tell: 12.6 -> 10.9 ms per call, same draws) -- then the call waits
// for it, and should a wait inside it have timed out, `rebuild` restores the matrices, they are factorised by launches, and the context
// stays on them (bgp_ps_note_timeout).
template <class Rebuild>
static int post_factor_child(bgp_ctx* c, bgp_ctx* w, int nb, bool allow_launch_free, int* status, Rebuild&& rebuild) {
  for (;;) {
    BGP_HIP(hipMemsetAsync(w->dyw, 0, (size_t)nb * w->npad * sizeof(double), c->stream));
    BGP_HIP(hipMemsetAsync(w->dstatus, 0, (size_t)nb * sizeof(int), c->stream));
    // the child's shape under the parent's mode; the cool-down and the call count are the parent's (after a time-out bgp_ps_allowed
    // refuses, and the redo counts as one eligible call of the cool-down)
    BgpLmlShape shape = bgp_lml_shape(w, nb, 0, 1);
    shape.persist = c->persist;
    const BgpLmlPlan plan = bgp_plan_for(c, shape, allow_launch_free);
    const bool ps = plan.path == BGP_PATH_LAUNCH_FREE;
    if (ps) w->persist = 1;
    BGP_TRY(ps ? bgp_launch_cholesky_persist(w, plan) : bgp_launch_lml_group(w, plan, 0, c->stream));
    BGP_HIP(bgp_memcpy_async(status, w->dstatus, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (!ps) return BGP_OK;
    BGP_HIP(bgp_stream_sync(c->stream));
    if (!bgp_ps_timed_out(c, w, "the covariance is rebuilt and factorised")) return BGP_OK;
    BGP_TRY(rebuild());
  }
}

// out[r] = mean + L z[r] for ALL draws r of one posterior: one wave per row of the lower factor, which is read once
// (the draws' normal vectors stay in L2); rows of z / out have stride ldz.  Fixed order: bitwise reproducible.
#define TRI_MAXD 16
__global__ void __launch_bounds__(256) tri_matmul_draws_kernel(const double* __restrict__ L, int mpad,
                                                                const double* __restrict__ z, int ldz, int n_draws,
                                                                const double* __restrict__ mean, int m,
                                                                double* __restrict__ out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= m) return;
  const double* Lr = L + (size_t)row * mpad;
  for (int r0 = 0; r0 < n_draws; r0 += TRI_MAXD) {
    const int nd = min(TRI_MAXD, n_draws - r0);
    double acc[TRI_MAXD];
#pragma unroll
    for (int r = 0; r < TRI_MAXD; r++) acc[r] = 0.0;
    for (int j = lane; j <= row; j += 64) {
      const double l = Lr[j];
#pragma unroll
      for (int r = 0; r < TRI_MAXD; r++)
        if (r < nd) acc[r] += l * z[(size_t)(r0 + r) * ldz + j];
    }
#pragma unroll
    for (int r = 0; r < TRI_MAXD; r++) {
      double s = acc[r];
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if (r < nd && lane == 0) out[(size_t)(r0 + r) * ldz + row] = s + mean[row];
    }
  }
}

extern "C" int bgp_sample_y(bgp_ctx* c, int b, const double* h_kernel, int m, const double* Xq, int n_draws,
                            const double* z, double jitter, double* out) {
  BGP_TRY(bgp_guard(c, "bgp_sample_y", BGP_POST_PLAIN));
  if (!c || !h_kernel || !Xq || !z || !out || m <= 0 || n_draws <= 0 || b < 0) {
    bgp_set_error("bgp_sample_y: bad argument");
    return BGP_ERR_INVALID;
  }
  BGP_TRY(bgp_guard(c, "bgp_sample_y", BGP_POST_PLAIN, b + 1));
  return post_call(c, [&]() -> int {
    const int npad = c->npad, n = c->n, d = c->d, mpad = pad128(m), rpad = pad128(n_draws);
    const size_t p = d + 2;
    bgp_ctx* w = nullptr;
    BGP_TRY(post_child(c, m, 1, &w));
    double *dXq, *dhk, *dKs, *dP, *dmean, *dZ, *dO;
    BgpScratch live(c);
    BGP_TRY(live.carve([&](BgpCarve& s) {
      dXq = s.take<double>((size_t)m * d);
      dhk = s.take<double>(p);
      dKs = s.take<double>((size_t)mpad * npad);
      dP = s.take<double>((size_t)mpad * npad);
      dmean = s.take<double>(mpad);
      dZ = s.take<double>((size_t)rpad * mpad);
      dO = s.take<double>((size_t)rpad * mpad);
    }));
    const double* Linv = c->dLinv + (size_t)b * npad * npad;
    const double* al = c->dalpha_sol + (size_t)b * npad;
    BGP_TRY(post_stage_queries(c, dXq, Xq, m));
    BGP_HIP(bgp_memcpy_async(dhk, h_kernel, p * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BGP_HIP(hipMemsetAsync(dKs, 0, (size_t)mpad * npad * sizeof(double), c->stream));
    BGP_HIP(hipMemsetAsync(dZ, 0, (size_t)rpad * mpad * sizeof(double), c->stream));
    BGP_HIP(rows_up(c, dZ, z, m, mpad, n_draws));
    BGP_TRY(bgp_launch_kcross(c, dhk, m, dXq, n, c->dXeff, dKs, npad));
    hipLaunchKernelGGL(matvec_rows_kernel, dim3((m + 3) / 4, 1), dim3(256), 0, c->stream, dKs, npad, (size_t)0, al,
                       (size_t)0, (const int*)nullptr, n, m, dmean, (size_t)0);
    // cov = K_** - P P^T, P = K_* L^-T, in the child's matrix (white level from the host's exp), + jitter, identity padding
    auto build_cov = [&]() -> int {
      BGP_TRY(post_cov(c, 1, m, dKs, Linv, nullptr, dP, PostKss{dhk, dXq, h_kernel}, 1, w->dK, nullptr, true));
      hipLaunchKernelGGL(cov_prepare_kernel, dim3(1024), dim3(256), 0, c->stream, w->dK, m, mpad, jitter);
      return BGP_OK;
    };
    int st = 0;
    BGP_TRY(build_cov());
    BGP_TRY(post_factor_child(c, w, 1, true, &st, build_cov));
    BGP_HIP(bgp_stream_sync(c->stream));
    if (st != 0) {
      bgp_set_error("bgp_sample_y: predictive covariance not positive definite at pivot %d (jitter %.3g)", st, jitter);
      return BGP_ERR_NOTPD;
    }
    // out = mean + L z for every draw (the factor's strict upper triangle is never read)
    hipLaunchKernelGGL(tri_matmul_draws_kernel, dim3((m + 3) / 4), dim3(256), 0, c->stream, w->dK, mpad, dZ, mpad, n_draws,
                       dmean, m, dO);
    BGP_HIP(hipGetLastError());
    BGP_HIP(rows_down(c, out, dO, m, mpad, n_draws));
    BGP_HIP(bgp_stream_sync(c->stream));
    return BGP_OK;
  });
}

// out_b = mean_b + L_b z_b for the lower factors left by the batched Cholesky (one wave per row, fixed order)
__global__ void __launch_bounds__(256) tri_matvec_kernel(const double* __restrict__ Lb, int mpad, const double* __restrict__ z,
                                                          const double* __restrict__ mean, int m,
                                                          double* __restrict__ out) {
  const int b = blockIdx.y, row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= m) return;
  const double* L = Lb + (size_t)b * mpad * mpad + (size_t)row * mpad;
  const double* zb = z + (size_t)b * mpad;
  double s = 0.0;
  for (int j = lane; j <= row; j += 64) s += L[j] * zb[j];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) out[(size_t)b * mpad + row] = s + mean[(size_t)b * mpad + row];
}

// workspace of the m x m covariance factorisations: a child context sharing the parent's stream, cached on the
// parent and grown on demand (rows mpad, nb matrices side by side)
static int ensure_child(bgp_ctx* c, int mpad, int nb, bgp_ctx** out) {
  bgp_ctx* w = c->child;
  if (w && (w->dyw.cap < (size_t)w->max_batch * mpad || w->max_batch < nb)) {  // (dyw holds max_batch x its row capacity)
    bgp_free_child(c);
    w = nullptr;
  }
  if (!w) {
    w = new bgp_ctx();
    w->device = c->device;
    w->stream = c->stream;
    w->ncu = c->ncu;
    w->d = c->d;
    w->max_batch = nb;
    const size_t B8 = 8 * ((size_t)(nb + 7) / 8);
    c->child = w;
    int rc = w->dK.ensure((size_t)nb * mpad * mpad);
    if (!rc) rc = w->dW.ensure((size_t)nb * (mpad / 128) * 128 * 128);
    if (!rc) rc = w->dyw.ensure((size_t)nb * mpad);
    if (!rc) rc = w->dacc.ensure(B8 * 4);
    if (!rc) rc = w->dlml.ensure(B8);
    if (!rc) rc = w->dstatus.ensure(B8);
    if (rc) {
      bgp_free_child(c);
      return rc;
    }
  }
  w->panels = c->panels;
  w->panels_auto = c->panels_auto;
  *out = w;
  return BGP_OK;
}

// One function draw per resident posterior (the hyper-posterior branch of BayesGPR.sample_y, bask/bayesgpr.py:679-718,
// and the Thompson-sampling acquisition): item i uses posterior pidx[i] with the kernel parameters h_kernel[i] (noise
// already switched off by the caller where the reference does), its own standard-normal vector z[i] and returns
// out[i] = mean_i + chol(cov_i + jitter I) z[i].  All items of a chunk share every launch (grid.y = item), including
// ONE batched Cholesky of their covariance matrices.  status[i] != 0: covariance i not positive definite at that
// jitter (out[i] undefined) -- the caller retries those items with a larger jitter.
extern "C" int bgp_sample_y_batch(bgp_ctx* c, int B, const int* pidx, const double* h_kernel, int m, const double* Xq,
                                  const double* z, double jitter, double* out, int* status) {
  BGP_TRY(bgp_guard(c, "bgp_sample_y_batch", BGP_POST_PLAIN));
  if (!c || !pidx || !h_kernel || !Xq || !z || !out || !status || m <= 0 || B <= 0) {
    bgp_set_error("bgp_sample_y_batch: bad argument");
    return BGP_ERR_INVALID;
  }
  BGP_TRY(bgp_guard(c, "bgp_sample_y_batch", BGP_POST_PLAIN, 0, pidx, B));
  return post_call(c, [&]() -> int {
    const int npad = c->npad, n = c->n, d = c->d, mpad = pad128(m);
    const size_t p = d + 2, sKs = (size_t)mpad * npad, sCv = (size_t)mpad * mpad;
    // per item: K_*, P, cov (child), mean / z / out; 1 << 30 doubles per chunk (8 GiB)
    const int chunk = post_chunk(B, 2 * sKs + sCv + 3 * (size_t)mpad, (size_t)1 << 30, false);
    bgp_ctx* w = nullptr;
    BGP_TRY(post_child(c, m, chunk, &w));
    double *dXq, *dH, *dKs, *dP, *dmean, *dZ, *dO;
    int* dpidx;
    BgpScratch live(c);
    BGP_TRY(live.carve([&](BgpCarve& s) {
      dXq = s.take<double>((size_t)m * d);
      dH = s.take<double>((size_t)B * p);
      dKs = s.take<double>((size_t)chunk * sKs);
      dP = s.take<double>((size_t)chunk * sKs);
      dmean = s.take<double>((size_t)chunk * mpad);
      dZ = s.take<double>((size_t)chunk * mpad);
      dO = s.take<double>((size_t)chunk * mpad);
      dpidx = s.take<int>(B);
    }));
    BGP_TRY(post_stage_queries(c, dXq, Xq, m));
    BGP_HIP(bgp_memcpy_async(dH, h_kernel, (size_t)B * p * sizeof(double), hipMemcpyHostToDevice, c->stream));
    BGP_HIP(bgp_memcpy_async(dpidx, pidx, (size_t)B * sizeof(int), hipMemcpyHostToDevice, c->stream));
    c->chunk_last[0] = 0, c->chunk_last[1] = 1;
    for (int off = 0; off < B; off += chunk) {
      const int nb = std::min(chunk, B - off);
      c->chunk_last[0]++;
      const double* dHc = dH + (size_t)off * p;
      const int* dpc = dpidx + off;
      BGP_HIP(hipMemsetAsync(dZ, 0, (size_t)nb * mpad * sizeof(double), c->stream));
      BGP_HIP(rows_up(c, dZ, z + (size_t)off * m, m, mpad, nb));
      BGP_TRY(bgp_launch_kcross_batch(c, nb, dHc, m, dXq, n, c->dXeff, dKs, npad, sKs));
      hipLaunchKernelGGL(matvec_rows_kernel, dim3((m + 3) / 4, nb), dim3(256), 0, c->stream, dKs, npad, sKs, c->dalpha_sol,
                         (size_t)npad, dpc, n, m, dmean, (size_t)mpad);
      // cov = K_** - P P^T, P = K_* L^-T, in place in the child's matrices, + jitter, identity padding
      BGP_TRY(post_cov(c, nb, m, dKs, c->dLinv, dpc, dP, PostKss{dHc, dXq}, 1, w->dK, nullptr, true));
      hipLaunchKernelGGL(cov_prepare_kernel, dim3(256, nb), dim3(256), 0, c->stream, w->dK, m, mpad, jitter);
      // (by launches: nothing waits inside a chunk, so there is nothing to rebuild)
      BGP_TRY(post_factor_child(c, w, nb, false, status + off, [] { return (int)BGP_OK; }));
      hipLaunchKernelGGL(tri_matvec_kernel, dim3((m + 3) / 4, nb), dim3(256), 0, c->stream, w->dK, mpad, dZ, dmean, m, dO);
      BGP_HIP(hipGetLastError());
      BGP_HIP(rows_down(c, out + (size_t)off * m, dO, m, mpad, nb));
    }
    BGP_HIP(bgp_stream_sync(c->stream));
    return BGP_OK;
  });
}

// (the child owns its buffers and BORROWS the parent's stream: it is deleted, never passed to bgp_ctx_destroy)
void bgp_free_child(bgp_ctx* c) {
  if (!c) return;
  delete c->child;
  c->child = nullptr;
}
