// Shapley attribution of the surrogate mean at a point against a background.
//
// For resident posterior b with mean mu_b, P points x_p to explain and N background rows z_s, over the dimensions D = {0 .. d-1}:
//   v_bp(S)    = (1 / N) sum_s mu_b(z_s with the columns in S taken from x_p)                    all 2^d coalitions S, d <= 16
//   phi_bpk    = sum over S in D \ {k}    |S|! (d - |S| - 1)! / d!        [v(S + k) - v(S)]
//   inter_bpkl = sum over S in D \ {k, l} |S|! (d - |S| - 2)! / (d - 1)!  [(v(S + k + l) - v(S + k)) - (v(S + l) - v(S))]
// Phase 1, shap_value_kernel: the 2^d rows of one (background row s, training point j) pair share almost all of their squared
// distance, so it is built by meet-in-the-middle.  With a_k = (x_pk / l_k - X_jk / l_k)^2, z_k = (z_sk / l_k - X_jk / l_k)^2, the low
// half of the dimensions dl = ceil(d / 2) and the high half dh = d - dl:
//   TL[m] = sum over k < dl, ascending, of (bit k of m ? a_k : z_k)       TH[m] likewise over the dimensions dl + k, k < dh
//   r2(S) = TL[S mod 2^dl] + TH[S >> dl]
// Every table entry is a sum of non-negative squares; nothing is obtained by taking a swapped term off (section 21).  A thread owns
// one low sub-mask and keeps its TL entry in a register; a workgroup owns a block of HB = min(16, 2^dh) high sub-masks whose TH
// entries for the current tile of pairs lie in LDS beside the tile's alpha_j, read as broadcasts; the thread carries HB
// accumulators.  One value then costs one addition in front of kb_value instead of a d-term distance.  With fewer than 256 low
// sub-masks the workgroup's 256 / 2^dl pair slots take the tile's pairs in turn and their sums are added in ascending slot order.
// The pairs (s-major, j fastest) are cut into chunks of SH_PC, a compile-time constant: the grid is (chunks, coalition blocks,
// B P) and a workgroup writes its partial v(S) per chunk.
// Phase 2, shap_reduce_kernel: chunk partials in ascending order, one division by N.
// Phase 3, shap_weight_kernel: one workgroup per (b, p, k) and per (b, p, k < l): the weighted differences over the subsets in
// ascending index, chunks of 256 in a fixed tree, chunk partials in ascending order; base and value are v(0) and v(2^d - 1).
// fp64 VALU work (the Matern families do not factorise over the halves: no MFMA shape).  Plain launches; no workgroup waits for
// another; no floating-point atomics; every loop is bounded by an argument.  The bits of (b, p) depend on posterior b, x_p and Z alone.
#include "bgp_common.h"
#include "bgp_device.h"

#define SH_DMAX 16                     // dimensions: 2^d coalitions are enumerated (larger d: the caller's sampling route)
#define SH_PC 1024                     // (s, j) pairs per chunk (fixed: the order of accumulation must not depend on the device)
#define SH_RC 256                      // subsets per chunk of the weighted sum
#define SH_NMAX (1 << 24)              // background rows per call
#define SH_PARTMAX ((size_t)1 << 26)   // doubles of chunk partials per call: B P 2^d chunks

// out[b][r][k] = in[r][k] / l_bk
__global__ void __launch_bounds__(256) shap_scale_kernel(const double* __restrict__ in, int rows, int d,
                                                         const double* __restrict__ H, double* __restrict__ out) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int b = blockIdx.y;
  if (idx >= (size_t)rows * d) return;
  const int k = (int)(idx % d);
  out[(size_t)b * rows * d + idx] = in[idx] / exp(H[(size_t)b * (d + 2) + 1 + k]);
}

// Workgroup (chunk, block of HB high sub-masks, b P + p); thread tid: low sub-mask tid mod 2^dl, pair slot tid >> dl.
// LDS per tile of TP pairs: the squares (z_k, a_k) of every dimension, the block's TH entries, alpha_j (HB = 16: 24.5 KB).
template <int STAT, int FORM, int HB>
__global__ void __launch_bounds__(256) shap_value_kernel(const double* __restrict__ Us, const double* __restrict__ xs,
                                                         const double* __restrict__ zs, const double* __restrict__ H,
                                                         const double* __restrict__ alpha, int n, int npad, int d, int P, int N,
                                                         int nchunk, double* __restrict__ part) {
#pragma clang fp contract(off)
  constexpr int TP = HB == 16 ? 64 : 128;  // pairs per tile: at least one per pair slot (HB < 16 is d <= 7: up to 128 slots)
  constexpr int DT = HB == 16 ? 16 : 7;    // dimensions a tile row holds
  __shared__ double az[TP * DT * 2];
  __shared__ double th[TP * HB];
  __shared__ double al[TP];
  __shared__ double red[256];
  const int tid = threadIdx.x, chunk = blockIdx.x, blk = blockIdx.y, bp = blockIdx.z, b = bp / P;
  const int dl = (d + 1) / 2, dh = d - dl, nlow = 1 << dl, slots = 256 >> dl;
  const int ml = tid & (nlow - 1), slot = tid >> dl;
  const double cst = exp(H[(size_t)b * (d + 2)]);
  const double* Ub = Us + (size_t)b * n * d;
  const double* zb = zs + (size_t)b * N * d;
  const double* xp = xs + (size_t)bp * d;
  const double* ab = alpha + (size_t)b * npad;
  const long long q0 = (long long)chunk * SH_PC;
  const long long left = (long long)n * N - q0;
  const int pc = left < SH_PC ? (int)left : SH_PC;
  double acc[HB];
#pragma unroll
  for (int h = 0; h < HB; h++) acc[h] = 0.0;
  for (int t0 = 0; t0 < pc; t0 += TP) {
    const int tc = min(TP, pc - t0);
    __syncthreads();
    for (int idx = tid; idx < tc * d; idx += 256) {
      const int t = idx / d, k = idx - t * d;
      const long long q = q0 + t0 + t;
      const int s = (int)(q / n), j = (int)(q - (long long)s * n);
      const double u = Ub[(size_t)j * d + k];
      const double dz = zb[(size_t)s * d + k] - u, da = xp[k] - u;
      az[(t * DT + k) * 2] = dz * dz;
      az[(t * DT + k) * 2 + 1] = da * da;
    }
    if (tid < tc) al[tid] = ab[(int)((q0 + t0 + tid) % n)];
    __syncthreads();
    for (int idx = tid; idx < tc * HB; idx += 256) {
      const int t = idx / HB, mh = blk * HB + (idx - t * HB);
      double q = 0.0;
      for (int k = 0; k < dh; k++) q = q + az[(t * DT + dl + k) * 2 + ((mh >> k) & 1)];
      th[idx] = q;
    }
    __syncthreads();
    for (int t = slot; t < tc; t += slots) {
      double tl = 0.0;
      for (int k = 0; k < dl; k++) tl = tl + az[(t * DT + k) * 2 + ((ml >> k) & 1)];
      const double a = al[t];
#pragma unroll
      for (int h = 0; h < HB; h++) acc[h] = fma(kb_value<STAT, FORM>(tl + th[t * HB + h], cst), a, acc[h]);
    }
  }
  double* out = part + (((size_t)bp * nchunk + chunk) << d);
#pragma unroll
  for (int h = 0; h < HB; h++) {
    double s = acc[h];
    if (slots > 1) {  // (uniform over the workgroup: the pair slots' sums in ascending slot order)
      __syncthreads();
      red[tid] = s;
      __syncthreads();
      if (tid < nlow)
        for (int g = 1; g < slots; g++) s = s + red[g * nlow + tid];
    }
    if (tid < nlow) out[((size_t)(blk * HB + h) << dl) + ml] = s;
  }
}

// v[bp][S] = (sum of part[bp][0 .. nchunk)[S], ascending chunk) / N
__global__ void __launch_bounds__(256) shap_reduce_kernel(const double* __restrict__ part, int nchunk, int d, double den,
                                                          double* __restrict__ v) {
#pragma clang fp contract(off)
  const size_t S = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t bp = blockIdx.y;
  if (S >> d) return;
  double s = 0.0;
  for (int c = 0; c < nchunk; c++) s += part[((bp * nchunk + c) << d) + S];
  v[(bp << d) + S] = s / den;
}

// the sum of the workgroup's 256 values in a fixed tree; the result is in every thread
static __device__ __forceinline__ double shap_tree(double x, double* sh) {
#pragma clang fp contract(off)
  const int tid = threadIdx.x;
  __syncthreads();
  sh[tid] = x;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sh[tid] = sh[tid] + sh[tid + o];
    __syncthreads();
  }
  return sh[0];
}

// i with a zero bit put in at position k
static __device__ __forceinline__ unsigned shap_spread(unsigned i, int k) {
  return ((i >> k) << (k + 1)) | (i & ((1u << k) - 1u));
}

// Workgroup (item, b P + p): item k < d is phi_k (and base, value, the diagonal of inter from item 0's kin); item d + r is the
// r-th pair k < l in row-major order.  W: the d weights of phi, then from W + SH_DMAX the d - 1 weights of inter, by |S|.
__global__ void __launch_bounds__(SH_RC) shap_weight_kernel(const double* __restrict__ v, const double* __restrict__ W, int d,
                                                            int P, double* __restrict__ phi, double* __restrict__ inter,
                                                            double* __restrict__ base, double* __restrict__ value) {
#pragma clang fp contract(off)
  __shared__ double sh[SH_RC];
  const int tid = threadIdx.x, item = blockIdx.x, bp = blockIdx.y;
  const double* vb = v + ((size_t)bp << d);
  int k = item, l = -1;
  if (item >= d) {
    int r = item - d;
    k = 0;
    while (k < d - 2 && r >= d - 1 - k) {
      r -= d - 1 - k;
      k++;
    }
    l = k + 1 + r;
  }
  const unsigned cnt = 1u << (l < 0 ? d - 1 : d - 2), kb = 1u << k, lb = l < 0 ? 0u : 1u << l;
  const double* w = W + (l < 0 ? 0 : SH_DMAX);
  double total = 0.0;
  for (unsigned i0 = 0; i0 < cnt; i0 += SH_RC) {
    const unsigned i = i0 + tid;
    double term = 0.0;
    if (i < cnt) {
      unsigned S = shap_spread(i, k);
      if (l >= 0) S = shap_spread(S, l);
      const double wt = w[__popc(S)];
      term = l < 0 ? wt * (vb[S | kb] - vb[S]) : wt * ((vb[S | kb | lb] - vb[S | kb]) - (vb[S | lb] - vb[S]));
    }
    total = total + shap_tree(term, sh);
  }
  if (tid != 0) return;
  if (l < 0) {
    phi[(size_t)bp * d + k] = total;
    if (inter) inter[((size_t)bp * d + k) * d + k] = 0.0;
    if (k == 0) {
      value[bp] = vb[(1u << d) - 1u];
      if (bp % P == 0) base[bp / P] = vb[0];  // (v of the empty coalition does not read x_p: the same bits for every p)
    }
  } else {
    inter[((size_t)bp * d + k) * d + l] = total;
    inter[((size_t)bp * d + l) * d + k] = total;
  }
}

template <int HB>
static void shap_launch_values(bgp_ctx* c, int B, int P, int N, int nchunk, const double* dUs, const double* dxs,
                               const double* dzs, const double* dH, double* dpart) {
  const int dh = c->d - (c->d + 1) / 2;
  const dim3 grid(nchunk, (1 << dh) / HB, B * P);
  KB_DISPATCH(c->ks.stationary, c->ks.form,
              hipLaunchKernelGGL((shap_value_kernel<S, F, HB>), grid, dim3(256), 0, c->stream, dUs, dxs, dzs, dH, c->dalpha_sol,
                                 c->n, c->npad, c->d, P, N, nchunk, dpart));
}

static int shap_chunks(const bgp_ctx* c, int N) { return (int)(((long long)c->n * N + SH_PC - 1) / SH_PC); }

static int shap_run(bgp_ctx* c, int B, const double* h_kernel, int P, const double* Xp, int N, const double* Z, double* phi,
                    double* base, double* value, double* inter) {
  const int n = c->n, d = c->d, nchunk = shap_chunks(c, N), BP = B * P;
  const size_t p = d + 2, nco = (size_t)1 << d;
  double *dXp, *dZ, *dH, *dUs, *dxs, *dzs, *dW, *dpart, *dv, *dphi, *dbase, *dvalue, *dinter;
  BgpScratch live(c);
  BGP_TRY(live.carve([&](BgpCarve& s) {
    dXp = s.take<double>((size_t)P * d);
    dZ = s.take<double>((size_t)N * d);
    dH = s.take<double>((size_t)B * p);
    dUs = s.take<double>((size_t)B * n * d);
    dxs = s.take<double>((size_t)BP * d);
    dzs = s.take<double>((size_t)B * N * d);
    dW = s.take<double>(2 * SH_DMAX);
    dpart = s.take<double>((size_t)BP * nchunk * nco);  // the chunk partials: all the scratch that grows with n N 2^d
    dv = s.take<double>((size_t)BP * nco);
    dphi = s.take<double>((size_t)BP * d);
    dbase = s.take<double>((size_t)B);
    dvalue = s.take<double>((size_t)BP);
    dinter = s.take<double>(inter ? (size_t)BP * d * d : 0);
  }));
  hipStream_t st = c->stream;
  // the weights by |S|: the factorials and their products are exact in fp64 for d <= 16, one rounding in the division
  double fact[SH_DMAX + 1], W[2 * SH_DMAX] = {0.0};
  fact[0] = 1.0;
  for (int i = 1; i <= d; i++) fact[i] = fact[i - 1] * (double)i;
  for (int s = 0; s < d; s++) W[s] = fact[s] * fact[d - s - 1] / fact[d];
  for (int s = 0; s + 1 < d; s++) W[SH_DMAX + s] = fact[s] * fact[d - s - 2] / fact[d - 1];
  // points and background the way predict's queries go up: through the context-level warp when one is set
  BGP_TRY(post_stage_queries(c, dXp, Xp, P));
  BGP_TRY(post_stage_queries(c, dZ, Z, N));
  BGP_HIP(bgp_memcpy_async(dH, h_kernel, (size_t)B * p * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(dW, W, sizeof(W), hipMemcpyHostToDevice, st));
  const auto blocks = [](size_t items) { return (unsigned)((items + 255) / 256); };
  hipLaunchKernelGGL(shap_scale_kernel, dim3(blocks((size_t)n * d), B), dim3(256), 0, st, c->dXeff, n, d, dH, dUs);
  hipLaunchKernelGGL(shap_scale_kernel, dim3(blocks((size_t)P * d), B), dim3(256), 0, st, dXp, P, d, dH, dxs);
  hipLaunchKernelGGL(shap_scale_kernel, dim3(blocks((size_t)N * d), B), dim3(256), 0, st, dZ, N, d, dH, dzs);
  switch (d - (d + 1) / 2) {  // dh: the coalition block holds min(16, 2^dh) high sub-masks
    case 0: shap_launch_values<1>(c, B, P, N, nchunk, dUs, dxs, dzs, dH, dpart); break;
    case 1: shap_launch_values<2>(c, B, P, N, nchunk, dUs, dxs, dzs, dH, dpart); break;
    case 2: shap_launch_values<4>(c, B, P, N, nchunk, dUs, dxs, dzs, dH, dpart); break;
    case 3: shap_launch_values<8>(c, B, P, N, nchunk, dUs, dxs, dzs, dH, dpart); break;
    default: shap_launch_values<16>(c, B, P, N, nchunk, dUs, dxs, dzs, dH, dpart); break;
  }
  hipLaunchKernelGGL(shap_reduce_kernel, dim3(blocks(nco), BP), dim3(256), 0, st, dpart, nchunk, d, (double)N, dv);
  const int items = d + (inter ? d * (d - 1) / 2 : 0);
  hipLaunchKernelGGL(shap_weight_kernel, dim3(items, BP), dim3(SH_RC), 0, st, dv, dW, d, P, dphi, inter ? dinter : nullptr, dbase,
                     dvalue);
  BGP_HIP(hipGetLastError());
  BGP_HIP(bgp_memcpy_async(phi, dphi, (size_t)BP * d * sizeof(double), hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_memcpy_async(base, dbase, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_memcpy_async(value, dvalue, (size_t)BP * sizeof(double), hipMemcpyDeviceToHost, st));
  if (inter) BGP_HIP(bgp_memcpy_async(inter, dinter, (size_t)BP * d * d * sizeof(double), hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_stream_sync(st));
  return BGP_OK;
}

extern "C" int bgp_shapley(bgp_ctx* c, int B, const double* h_kernel, int P, const double* Xp, int N, const double* Z,
                           double* phi, double* base, double* value, double* inter) {
  BGP_TRY(bgp_guard(c, "bgp_shapley", BGP_POST_PLAIN));
  if (!h_kernel || !Xp || !Z || !phi || !base || !value || B <= 0 || P <= 0 || N <= 0 || N > SH_NMAX ||
      (long long)B * P > 65535) {
    bgp_set_error("bgp_shapley: bad argument (1 <= B, 1 <= P, B P <= 65535, 1 <= N <= %d)", SH_NMAX);
    return BGP_ERR_INVALID;
  }
  if (c->d > SH_DMAX) {
    bgp_set_error("bgp_shapley: d > %d is not supported (2^d coalitions are enumerated)", SH_DMAX);
    return BGP_ERR_INVALID;
  }
  if ((double)B * (double)P * (double)shap_chunks(c, N) * (double)((size_t)1 << c->d) > (double)SH_PARTMAX) {
    bgp_set_error("bgp_shapley: more than 2^26 chunk partials (B P 2^d ceil(n N / %d)) in one call", SH_PC);
    return BGP_ERR_INVALID;
  }
  BGP_TRY(bgp_guard(c, "bgp_shapley", BGP_POST_PLAIN, B));
  return post_call(c, [&] { return shap_run(c, B, h_kernel, P, Xp, N, Z, phi, base, value, inter); });
}
