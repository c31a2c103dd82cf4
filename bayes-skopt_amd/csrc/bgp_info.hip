// The information an observation carries about the kernel hyper-parameters (BALD): the mutual information
// between y(x) and the chain row under the hyper-posterior mixture  p(.|x) = sum_b w^_b N(mu_b(x), sd_b(x)^2)  of bgp_mix.hip,
//   I(x) = H[p(.|x)] - sum_b w^_b H[N(mu_b, sd_b^2)] = sum_b w^_b KL(N(mu_b, sd_b^2) || p(.|x))     (nats, 0 <= I <= H[w^]),
// and the entropy of the mixture itself.  Neither has a closed form: every component's KL is a Q-node Gauss-Hermite sum, and every
// node needs a log-sum-exp over all components -- B Q B exponentials per point.  ONE pass serves the three entry points:
// bgp_hyper_information and bgp_hyper_information_warped run it behind the batched predict on the B x mpad moments that predict_run
// keeps on the device (bgp_post.hip, next to the mixture pass), bgp_information_values on caller-supplied ones.
//
// Definitions.  mu, sd (y units), the USED rows and the normalised weights w^_b are those of bgp_mix.hip (mix_prep_kernel,
// mix_norm_kernel: the same launches).  The host passes the rule (t_q, omega_q), q < Q <= 64 (numpy's hermgauss): no table here.
// Per point, over the used rows (in ascending b; k, c number them):
//   y_bq   = mu_b + (sqrt(2) sd_b) t_q
//   own_bq = (log w^_b - log sd_b) - t_q^2                                   component b's weighted log density at its own node
//   a_c(y) = (log w^_c - log sd_c) - ((y - mu_c) (1 / sd_c))^2 / 2  for c != b,   a_b(y_bq) = own_bq
//   lse    = A + log sum_c exp(a_c - A),  A = max_c a_c: two passes over c ascending, the first one max only (no exp)
//   g_bq   = own_bq - lse
//   information = max(0, sum_{b,q} w^_b ((omega_q / sqrt(pi)) (g_bq - log w^_b)))
//   entropy     = -sum_{b,q} w^_b ((omega_q / sqrt(pi)) lse) + log(2 pi) / 2
// With ONE used row a_b = A, the sum is exp(0) = 1, lse = own and every term of the information is exactly 0.  A used row whose sd is
// not > 0 (an atom) makes the point's entropy -inf and its information NaN; no used row: both NaN (BGP_OK, as the mixture pass).
//
// Work split (not the mixture pass's thread per point): ONE WAVE per point, four points per 256-thread workgroup.  A wave stages its
// point's column as triples (mu_c, 1 / sd_c, log w^_c - log sd_c), 24 bytes a row, into its own LDS slice of BGP_INFO_TILE = 256
// rows: 24 KB per workgroup, room for six workgroups in a CU's 160 KB (the registers allow four, below).  Lane l owns the node pairs (b, q) of flat
// index b Q + q = l, l + 64, ..., two at a time (the two exp chains overlap); for each it walks the components in ascending c, every
// lane reading the SAME triple at the same time -- an LDS broadcast, no bank conflict -- with y, own, A and the running sum in
// registers.  More than 256 used rows: the component loop runs tile by tile, re-staged per pass (1 / 64 of the walk's work).  Lane
// partials (pairs in ascending flat index) are added by a fixed xor butterfly.  No floating-point atomics, no contraction: a point's
// two outputs are a function of its column, the weights and the rule only -- the same bits whatever m and its neighbours are.
//
// Instruction mix: fp64 VALU and transcendental work (one exp per (b, q, c), one log per (b, q)); there is no matrix product in it,
// so no MFMA.  The compiler's report for info_kernel on gfx950: 121 VGPRs, no AGPRs, no scratch, 24 576 bytes of LDS, occupancy 4
// waves per SIMD (the two inlined exp chains' registers bound it, not the LDS).
#include "bgp_common.h"

#include <climits>
#include <cmath>

#define BGP_INFO_TILE 256

void BgpInfoScratch::take(BgpCarve& s, int B, int mpad) {
  dmu = s.take<double>((size_t)B * mpad);
  dsd = s.take<double>((size_t)B * mpad);
  dw = s.take<double>(B);
  dwn = s.take<double>(B);
  dlw = s.take<double>(B);
  dwu = s.take<double>(B);
  drule = s.take<double>(2 * BGP_INFO_QMAX);
  dout = s.take<double>((size_t)2 * mpad);
  dbad = s.take<int>(B);
  dused = s.take<int>(B);
  didx = s.take<int>(B);
  dstat = s.take<int>(4);
}

// The used rows in ascending b: idx[k] = b, wu[k] = w^_b, lw[k] = log w^_b (exactly 0 for one row).  One thread.
__global__ void info_rows_kernel(const int* __restrict__ used, const double* __restrict__ wn, int B, int* __restrict__ idx,
                                 double* __restrict__ wu, double* __restrict__ lw) {
  if (blockIdx.x || threadIdx.x) return;
  int k = 0;
  for (int b = 0; b < B; b++)
    if (used[b]) idx[k] = b, wu[k] = wn[b], lw[k] = log(wn[b]), k++;
}

struct InfoTriple {
  double mu, rinv, L;
};

// grid ceil(m / 4); rule = Q nodes, then Q weights.  stat[0] = the number of used rows (mix_norm_kernel).
__global__ void __launch_bounds__(256) info_kernel(const double* __restrict__ mu, const double* __restrict__ sd, size_t sm, int m,
                                                    const int* __restrict__ stat, const int* __restrict__ idx,
                                                    const double* __restrict__ wu, const double* __restrict__ lw, int Q,
                                                    const double* __restrict__ rule, double* __restrict__ info,
                                                    double* __restrict__ ent) {
#pragma clang fp contract(off)
  __shared__ InfoTriple tiles[4][BGP_INFO_TILE];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 4 + wv;
  const bool live = i < m;  // (a wave without a point still takes part in the barriers)
  const int nu = stat[0];
  if (nu == 0) {  // (the same for the whole grid)
    if (live && lane == 0) info[i] = NAN, ent[i] = NAN;
    return;
  }
  InfoTriple* T = tiles[wv];
  const double *cmu = mu + (live ? i : 0), *csd = sd + (live ? i : 0);
  const int ntile = (nu + BGP_INFO_TILE - 1) / BGP_INFO_TILE, npairs = nu * Q;
  bool atom = false;
  auto stage = [&](int tl) {
    __syncthreads();  // (every wave has left the previous tile)
    const int c0 = tl * BGP_INFO_TILE, cn = min(BGP_INFO_TILE, nu - c0);
    for (int k = lane; live && k < cn; k += 64) {
      const size_t o = (size_t)idx[c0 + k] * sm;
      const double s_ = csd[o];
      T[k].mu = cmu[o], T[k].rinv = 1.0 / s_, T[k].L = lw[c0 + k] - log(s_);
      if (!(s_ > 0.0)) atom = true;
    }
    __syncthreads();
  };
  if (ntile == 1) stage(0);
  double accI = 0.0, accH = 0.0;
  for (int base = 0; base < npairs; base += 128) {
    double y[2], own[2], A[2], s[2], wq[2], lwb[2];
    int kb[2];
    bool ok[2];
#pragma unroll
    for (int u = 0; u < 2; u++) {
      const int p = base + u * 64 + lane;
      ok[u] = live && p < npairs;
      kb[u] = ok[u] ? p / Q : -1;
      const int k = ok[u] ? kb[u] : 0, q = ok[u] ? p - kb[u] * Q : 0;
      const size_t o = (size_t)idx[k] * sm;
      const double mb = cmu[o], sb = csd[o], t = rule[q];
      y[u] = mb + (1.4142135623730951 * sb) * t;
      lwb[u] = lw[k];
      own[u] = (lwb[u] - log(sb)) - t * t;
      wq[u] = rule[Q + q] / 1.7724538509055159;  // sqrt(pi)
      A[u] = own[u], s[u] = 0.0;
    }
    for (int tl = 0; tl < ntile; tl++) {  // pass 1: the largest exponent
      if (ntile > 1) stage(tl);
      const int c0 = tl * BGP_INFO_TILE, cn = live ? min(BGP_INFO_TILE, nu - c0) : 0;
      for (int k = 0; k < cn; k++) {
        const InfoTriple tr = T[k];
#pragma unroll
        for (int u = 0; u < 2; u++) {
          const double z = (y[u] - tr.mu) * tr.rinv;
          const double a = tr.L - (z * z) / 2.0;
          if (c0 + k != kb[u]) A[u] = fmax(A[u], a);
        }
      }
    }
    for (int tl = 0; tl < ntile; tl++) {  // pass 2: the shifted sum, c ascending
      if (ntile > 1) stage(tl);
      const int c0 = tl * BGP_INFO_TILE, cn = live ? min(BGP_INFO_TILE, nu - c0) : 0;
      for (int k = 0; k < cn; k++) {
        const InfoTriple tr = T[k];
#pragma unroll
        for (int u = 0; u < 2; u++) {
          const double z = (y[u] - tr.mu) * tr.rinv;
          const double a = (c0 + k != kb[u]) ? tr.L - (z * z) / 2.0 : own[u];
          s[u] += exp(a - A[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; u++) {
      if (!ok[u]) continue;
      const double lse = A[u] + log(s[u]);
      const double w = wu[kb[u]];
      accI += w * (wq[u] * ((own[u] - lse) - lwb[u]));
      accH += w * (wq[u] * lse);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {  // the fixed butterfly: every lane ends with the same two sums
    accI += __shfl_xor(accI, off, 64);
    accH += __shfl_xor(accH, off, 64);
  }
  const bool any_atom = __any(atom ? 1 : 0) != 0;
  if (live && lane == 0) {
    info[i] = any_atom ? NAN : fmax(accI, 0.0);
    ent[i] = any_atom ? -INFINITY : 0.91893853320467274178 - accH;  // log(2 pi) / 2
  }
}

int bgp_info_check(const char* who, int B, const BgpInfoPlan& ip) {
  if (B <= 0 || ip.Q < 1 || ip.Q > BGP_INFO_QMAX || !ip.nodes || !ip.wts || !ip.information || !ip.entropy || !ip.n_used ||
      (long long)B * ip.Q > INT_MAX) {
    bgp_set_error("%s: bad argument (1 <= Q <= %d nodes and weights, information, entropy, n_used)", who, BGP_INFO_QMAX);
    return BGP_ERR_INVALID;
  }
  for (int q = 0; q < ip.Q; q++)
    if (!std::isfinite(ip.nodes[q]) || !std::isfinite(ip.wts[q])) {
      bgp_set_error("%s: node %d of the rule is not finite", who, q);
      return BGP_ERR_INVALID;
    }
  const BgpMixPlan mp{ip.weights, ip.y_mean, ip.y_std, 0, nullptr, nullptr, nullptr, nullptr, nullptr, ip.n_used};
  return bgp_mix_check(who, B, mp);  // (the weights' rules are the mixture's)
}

// The pass on dmean / dvar (B rows of stride mpad, on the device): uploads, five launches and the downloads on the context's
// stream; the caller waits (bgp_stream_sync) before it reads the outputs and c->info_last.
int bgp_info_run(bgp_ctx* c, int B, int m, int mpad, const double* dmean, const double* dvar, const BgpInfoPlan& ip,
                 const BgpInfoScratch& is) {
  hipStream_t st = c->stream;
  const size_t row = (size_t)m * sizeof(double);
  const std::vector<double> ones(ip.weights ? 0 : B, 1.0);
  BGP_HIP(bgp_memcpy_async(is.dw, ip.weights ? ip.weights : ones.data(), (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(is.drule, ip.nodes, (size_t)ip.Q * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(is.drule + ip.Q, ip.wts, (size_t)ip.Q * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(hipMemsetAsync(is.dbad, 0, (size_t)B * sizeof(int), st));
  hipLaunchKernelGGL(mix_prep_kernel, dim3((m + 255) / 256, B), dim3(256), 0, st, dmean, dvar, (size_t)mpad, m, ip.y_mean,
                     ip.y_std, is.dmu, is.dsd, is.dbad);
  hipLaunchKernelGGL(mix_norm_kernel, dim3(1), dim3(64), 0, st, (const double*)is.dw, (const int*)is.dbad, B, is.dwn, is.dused,
                     is.dstat);
  hipLaunchKernelGGL(info_rows_kernel, dim3(1), dim3(64), 0, st, (const int*)is.dused, (const double*)is.dwn, B, is.didx, is.dwu,
                     is.dlw);
  hipLaunchKernelGGL(info_kernel, dim3((m + 3) / 4), dim3(256), 0, st, (const double*)is.dmu, (const double*)is.dsd, (size_t)mpad,
                     m, (const int*)is.dstat, (const int*)is.didx, (const double*)is.dwu, (const double*)is.dlw, ip.Q,
                     (const double*)is.drule, is.dout, is.dout + mpad);
  BGP_HIP(hipGetLastError());
  BGP_HIP(bgp_memcpy_async(ip.information, is.dout, row, hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_memcpy_async(ip.entropy, is.dout + mpad, row, hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_memcpy_async(c->info_last, is.dstat, 4 * sizeof(int), hipMemcpyDeviceToHost, st));
  return BGP_OK;
}

static int info_resident(bgp_ctx* c, const char* who, bool rowwarp, int B, const double* h_kernel, const double* weights, int m,
                         const double* Xq, double y_mean, double y_std, int Q, const double* nodes, const double* wts,
                         double* information, double* entropy, int* n_used) {
  const BgpPostKind kind = rowwarp ? BGP_POST_ROWWARP : BGP_POST_PLAIN;
  BGP_TRY(bgp_guard(c, who, kind));
  if (!h_kernel || !Xq || m <= 0 || B <= 0) {
    bgp_set_error("%s: bad argument", who);
    return BGP_ERR_INVALID;
  }
  const BgpInfoPlan ip{weights, y_mean, y_std, Q, nodes, wts, information, entropy, n_used};
  BGP_TRY(bgp_info_check(who, B, ip));
  BGP_TRY(bgp_guard(c, who, kind, B));
  const int rc = post_call(c, [&] { return bgp_predict_run_info(c, B, h_kernel, m, Xq, ip, rowwarp); });
  if (rc == BGP_OK) *n_used = c->info_last[0];
  return rc;
}

extern "C" int bgp_hyper_information(bgp_ctx* c, int B, const double* h_kernel, const double* weights, int m, const double* Xq,
                                     double y_mean, double y_std, int Q, const double* nodes, const double* wts,
                                     double* information, double* entropy, int* n_used) {
  return info_resident(c, "bgp_hyper_information", false, B, h_kernel, weights, m, Xq, y_mean, y_std, Q, nodes, wts, information,
                       entropy, n_used);
}

extern "C" int bgp_hyper_information_warped(bgp_ctx* c, int B, const double* h_kernel, const double* weights, int m,
                                            const double* Xq, double y_mean, double y_std, int Q, const double* nodes,
                                            const double* wts, double* information, double* entropy, int* n_used) {
  return info_resident(c, "bgp_hyper_information_warped", true, B, h_kernel, weights, m, Xq, y_mean, y_std, Q, nodes, wts,
                       information, entropy, n_used);
}

extern "C" int bgp_information_values(bgp_ctx* c, int B, int m, const double* mean, const double* var, const double* weights,
                                      double y_mean, double y_std, int Q, const double* nodes, const double* wts,
                                      double* information, double* entropy, int* n_used) {
  BGP_TRY(bgp_guard(c, "bgp_information_values"));
  if (!mean || !var || m <= 0 || B <= 0) {
    bgp_set_error("bgp_information_values: bad argument");
    return BGP_ERR_INVALID;
  }
  const BgpInfoPlan ip{weights, y_mean, y_std, Q, nodes, wts, information, entropy, n_used};
  BGP_TRY(bgp_info_check("bgp_information_values", B, ip));
  const int rc = post_call(c, [&]() -> int {
    const int mpad = pad_to(m, 128);
    const size_t row = (size_t)m * sizeof(double), pitch = (size_t)mpad * sizeof(double);
    double *dmean, *dvar;
    BgpInfoScratch is;
    BgpScratch live(c);
    BGP_TRY(live.carve([&](BgpCarve& s) {
      dmean = s.take<double>((size_t)B * mpad);
      dvar = s.take<double>((size_t)B * mpad);
      is.take(s, B, mpad);
    }));
    BGP_HIP(bgp_memcpy2d_async(dmean, pitch, mean, row, row, B, hipMemcpyHostToDevice, c->stream));
    BGP_HIP(bgp_memcpy2d_async(dvar, pitch, var, row, row, B, hipMemcpyHostToDevice, c->stream));
    BGP_TRY(bgp_info_run(c, B, m, mpad, dmean, dvar, ip, is));
    BGP_HIP(bgp_stream_sync(c->stream));
    return BGP_OK;
  });
  if (rc == BGP_OK) *n_used = c->info_last[0];
  return rc;
}
