// Case-deletion influence of every observation on the surrogate: how far the latent posterior at m query rows
// moves when observation i is taken out, for all n observations of each of the first B resident posteriors, without a refit.  With
// P = K^-1 (the resident inverse: white level and alpha / noise_vector included), a = alpha_sol, k_*(x) the latent cross kernel,
// mu / var the latent moments and s_b the variance of an observation (all in normalised units; hyper-parameters, warps and the y
// normalisation held fixed under deletion, as bgp_cross_validate holds them):
//   c_i(x)    = [k_*(x)^T P]_i
//   dmu_i(x)  = mu_{-i}(x) - mu(x)   = -c_i(x) (a_i / P_ii)
//   dvar_i(x) = var_{-i}(x) - var(x) = +c_i(x)^2 (1 / P_ii)
//   v = var(x) + s_b,  t = dvar_i(x) / v,  v_i = v (1 + t)
//   cook_i(x) = dmu_i(x)^2 / v
//   kl_i(x)   = 1/2 [log1p(t) - t / (1 + t) + dmu_i(x)^2 / v_i]         = KL(N(mu, v) || N(mu_{-i}, v_i))
// (v / v_i - 1 + log(v_i / v) of the definition, written without its cancellation); a row with v <= 0 gives 0 to cook and kl.
//
// Per chunk of posteriors and chunk of query rows (a multiple of 128):
//   1  K_* = k_b(chunk, X), mu and var of the chunk: bgp_launch_moments, the launches -- and the bits -- of bgp_predict_batch.
//   2  infl_kernel: V = K_* P on v_mfma_f64_16x16x4_f64, never stored.  A workgroup owns a strip of 128 query rows x 64 observations;
//      its four waves are stacked along the rows (32 rows x 64 columns each: 2 x 4 accumulator tiles, 64 accumulator registers), so
//      a column's 128 entries lie in four waves and, inside a wave, in the four row groups lane >> 4 of the GK_ROW layout.  The
//      operands (128 rows of K_*, 64 rows of the symmetric P, 16 k at a time) come in on the two-stage LDS-DMA ring of bgp_s4.h:
//      48 KB, plus 3 KB holding a_i / P_ii and 1 / P_ii of the strip's columns (P_ii from the inverse's diagonal) and v, 1 / v of
//      its rows, staged once under the first chunk's flight.
//      Epilogue: every lane forms dmu, dvar, cook and kl of its 32 entries and reduces per column -- its 8 rows in ascending row,
//      then the 4 row groups by shfl_xor 16 then 32, then the 4 waves through LDS (the ring, free by then) in ascending wave.
//      max |dmu| goes with its row; ties keep the lower row.  One partial per (row strip, posterior, column); the rows below n_focus
//      also write their signed dmu / dvar straight to the focus outputs.  Pad rows (x >= m) and pad columns (i >= n) are left out.
//   3  infl_reduce_kernel: one thread per (posterior, observation) adds the chunk's strip partials, ascending, onto the running
//      result (the chunks of rows come in ascending order: ((p_0 + p_1) + p_2) ... whatever the chunk size is).
// Strips start at multiples of 128 of the call's rows whatever the chunk is, nothing is added atomically in floating point, no
// workgroup waits for another, and no product is contracted: an output is the same bits whatever B is, whatever shares the call and
// however it is chunked (BGP_ITEM_CHUNK, BGP_ROW_CHUNK).
#include "bgp_s4.h"

#include <cmath>

#define IF_TM 128    // query rows of a strip
#define IF_TN 64     // observations of a strip
#define IF_DMAX 32
#define IF_FMAX 64   // focus rows

// grid (column panels x S4_PW x tm, posteriors of the chunk).  Ks: the chunk's K_* (row stride npad, item stride sKs); Kinv, alpha,
// noise, fdmu, fdvar: those of the chunk's first posterior; var: the chunk's latent variances (item stride sv); mm rows in the
// chunk, the first of them row m0 of the call.  Partials at [(ti nb + b) npad + i].
__global__ void __launch_bounds__(256, 2)
    infl_kernel(const double* __restrict__ Ks, size_t sKs, const double* __restrict__ Kinv, const double* __restrict__ alpha,
                const double* __restrict__ var, size_t sv, const double* __restrict__ noise, int npad, int n, int mm, int m0,
                int n_focus, int tm, double* __restrict__ pdm2, double* __restrict__ pcook, double* __restrict__ pkl,
                double* __restrict__ pmax, int* __restrict__ parg, double* __restrict__ fdmu, double* __restrict__ fdvar) {
#pragma clang fp contract(off)
  constexpr unsigned AOPB = IF_TM * S4_ROWB, STAGEB = (IF_TM + IF_TN) * S4_ROWB;
  __shared__ __attribute__((aligned(1024))) char smem[2 * STAGEB];
  __shared__ double epi[2 * IF_TN + 2 * IF_TM];  // a_i / P_ii, 1 / P_ii of the columns; v, 1 / v of the rows
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)smem;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, nb = gridDim.y, tn = npad / IF_TN;
  int ti, tj;
  {  // column panels of S4_PW strips, row strip by row strip inside (gemm4_kernel's order: placement only)
    const int t = blockIdx.x, per = S4_PW * tm, p = t / per, r = t - p * per;
    const int wdt = min(S4_PW, tn - p * S4_PW);
    ti = r / wdt;
    tj = p * S4_PW + (r - ti * wdt);
    if (ti >= tm) return;
  }
  const double* A = Ks + (size_t)b * sKs + (size_t)(ti * IF_TM) * npad;
  const double* Pb = Kinv + (size_t)b * npad * npad;
  const double* Bm = Pb + (size_t)(tj * IF_TN) * npad;
  unsigned voffA[IF_TM / 32], voffB[IF_TN / 32];
  s4_src<IF_TM>(voffA, npad, w, lane);
  s4_src<IF_TN>(voffB, npad, w, lane);
  const int r0 = w * 32;
  unsigned pa[4], pb[4];
  s4_frag_addr(pa, lds0, r0, lane);
  s4_frag_addr(pb, lds0 + AOPB, 0, lane);
  d4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
  s4_issue<IF_TM>(A, voffA, 0, lds0, w);
  s4_issue<IF_TN>(Bm, voffB, 0, lds0 + AOPB, w);
  if (tid < IF_TN) {
    const int gi = tj * IF_TN + tid;
    double ca = 0.0, cp = 0.0;
    if (gi < n) {
      const double pii = Pb[(size_t)gi * npad + gi];
      cp = 1.0 / pii;
      ca = alpha[(size_t)b * npad + gi] / pii;
    }
    epi[tid] = ca, epi[IF_TN + tid] = cp;
  } else if (tid < IF_TN + IF_TM) {
    const int row = tid - IF_TN, g = ti * IF_TM + row;
    const double v = (g < mm) ? var[(size_t)b * sv + g] + noise[b] : 0.0;
    epi[2 * IF_TN + row] = v, epi[2 * IF_TN + IF_TM + row] = (v > 0.0) ? 1.0 / v : 0.0;
  }
  const int nch = npad / S4_KC;  // (npad is a multiple of 128: an even number of chunks)
  for (int c = 0; c < nch; c += 2) {
#pragma unroll
    for (int s = 0; s < 2; s++) {
      S4_WAIT_VM0();
      __builtin_amdgcn_s_barrier();
      if (c + s + 1 < nch) {
        const unsigned nbuf = lds0 + (unsigned)((s ^ 1) * STAGEB);
        s4_issue<IF_TM>(A, voffA, (c + s + 1) * S4_KC, nbuf, w);
        s4_issue<IF_TN>(Bm, voffB, (c + s + 1) * S4_KC, nbuf + AOPB, w);
      }
      s4_mma<2, 4, -64, 0, 0>(pa, pb, s * STAGEB, acc);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  __syncthreads();  // every wave is past its last fragment read: the ring is free (and epi was written before the first barrier)
  double* red = reinterpret_cast<double*>(smem);  // [quantity 0 .. 3][wave][column], then the rows of the maxima
  int* redarg = reinterpret_cast<int*>(red + 4 * 4 * IF_TN);
  const int lq = lane >> 4, lc = lane & 15;
  const double *vv = epi + 2 * IF_TN, *rvv = vv + IF_TM;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int col = 16 * j + lc, gi = tj * IF_TN + col;
    const bool cok = gi < n;
    const double ca = epi[col], cp = epi[IF_TN + col];
    double s2 = 0.0, sc = 0.0, sk = 0.0, best = -1.0;
    int arg = 0;
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
      for (int r = 0; r < 4; r++) {  // (ascending row for this lane)
        const int row = GK_ROWB(r0, i, lane, r), g = ti * IF_TM + row;
        const double cx = acc[i][j][r];
        const double dmu = -(cx * ca), dvar = (cx * cx) * cp;
        const double d2 = dmu * dmu;
        const double v = vv[row], rv = rvv[row];
        double ck = 0.0, kl = 0.0;
        if (v > 0.0) {
          const double t = dvar * rv, ri = 1.0 / (1.0 + t);
          ck = d2 * rv;
          kl = 0.5 * ((log1p(t) - t * ri) + ck * ri);
        }
        if (cok && g < mm) {
          s2 += d2, sc += ck, sk += kl;
          const double a = fabs(dmu);
          if (a > best) best = a, arg = m0 + g;
          if (m0 + g < n_focus) {
            const size_t o = ((size_t)b * n_focus + (m0 + g)) * n + gi;
            fdmu[o] = dmu, fdvar[o] = dvar;
          }
        }
      }
#pragma unroll
    for (int off = 16; off <= 32; off <<= 1) {  // the four row groups of the wave
      s2 += __shfl_xor(s2, off);
      sc += __shfl_xor(sc, off);
      sk += __shfl_xor(sk, off);
      const double ob = __shfl_xor(best, off);
      const int oa = __shfl_xor(arg, off);
      if (ob > best || (ob == best && oa < arg)) best = ob, arg = oa;
    }
    if (lq == 0) {
      red[(0 * 4 + w) * IF_TN + col] = s2;
      red[(1 * 4 + w) * IF_TN + col] = sc;
      red[(2 * 4 + w) * IF_TN + col] = sk;
      red[(3 * 4 + w) * IF_TN + col] = best;
      redarg[w * IF_TN + col] = arg;
    }
  }
  __syncthreads();
  if (tid < IF_TN && tj * IF_TN + tid < n) {
    double s2 = red[tid], sc = red[4 * IF_TN + tid], sk = red[8 * IF_TN + tid], best = red[12 * IF_TN + tid];
    int arg = redarg[tid];
    for (int u = 1; u < 4; u++) {  // ascending wave = ascending row: a tie keeps the earlier one
      s2 += red[(0 * 4 + u) * IF_TN + tid];
      sc += red[(1 * 4 + u) * IF_TN + tid];
      sk += red[(2 * 4 + u) * IF_TN + tid];
      const double ob = red[(3 * 4 + u) * IF_TN + tid];
      if (ob > best) best = ob, arg = redarg[u * IF_TN + tid];
    }
    const size_t o = ((size_t)ti * nb + b) * npad + tj * IF_TN + tid;
    pdm2[o] = s2, pcook[o] = sc, pkl[o] = sk, pmax[o] = best, parg[o] = arg;
  }
}

// grid (ceil(n / 256), posteriors of the chunk): the tm strip partials of the chunk onto the running result of (b, i), ascending.
// first: the chunk holds the call's first rows (the result starts from them); last: its last ones -- a sum that is not finite, or a
// column without one comparable |dmu|, raises status[b] and the maximum becomes NaN (a NaN |dmu| is skipped by the maximum and by
// nothing else: it is in sum_dm2; the focus outputs are not inspected themselves).
__global__ void __launch_bounds__(256)
    infl_reduce_kernel(const double* __restrict__ pdm2, const double* __restrict__ pcook, const double* __restrict__ pkl,
                       const double* __restrict__ pmax, const int* __restrict__ parg, int tm, int npad, int n, int first, int last,
                       double* __restrict__ odm2, double* __restrict__ ocook, double* __restrict__ okl, double* __restrict__ omax,
                       int* __restrict__ oarg, int* __restrict__ status) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, nb = gridDim.y;
  if (i >= n) return;
  const size_t o = (size_t)b * n + i;
  double s2 = first ? 0.0 : odm2[o], sc = first ? 0.0 : ocook[o], sk = first ? 0.0 : okl[o], best = first ? -1.0 : omax[o];
  int arg = first ? 0 : oarg[o];
  for (int t = 0; t < tm; t++) {
    const size_t p = ((size_t)t * nb + b) * npad + i;
    s2 += pdm2[p], sc += pcook[p], sk += pkl[p];
    const double ob = pmax[p];
    if (ob > best) best = ob, arg = parg[p];
  }
  if (last) {
    const bool bad = !(s2 < INFINITY) || !(sc < INFINITY) || !(sk < INFINITY) || !(best >= 0.0 && best < INFINITY);
    if (bad) atomicOr(&status[b], 1);
    if (!(best >= 0.0)) best = NAN;
  }
  odm2[o] = s2, ocook[o] = sc, okl[o] = sk, omax[o] = best, oarg[o] = arg;
}

struct InflOut {
  double *sum_dm2, *sum_cook, *sum_kl, *max_abs;
  int* arg_max;
  double *dmu_focus, *dvar_focus;
  int* status;
};

static int infl_run(bgp_ctx* c, int B, const double* h_kernel, const double* noise, int m, const double* Xq, int n_focus,
                    const InflOut& out) {
  const int d = c->d, n = c->n, npad = c->npad;
  const size_t hp = d + 2;
  // rows per chunk: a multiple of 128 that keeps a posterior's K_* within 2^24 doubles (BGP_ROW_CHUNK: an upper bound, rounded up
  // to 128); posteriors per chunk: the K_* of a chunk within 2^29 doubles (BGP_ITEM_CHUNK)
  size_t mc = std::max<size_t>((((size_t)1 << 24) / (size_t)npad) / 128 * 128, 128);
  mc = (bgp_switch_cap(BGP_SW_ROW_CHUNK, mc) + 127) / 128 * 128;
  mc = std::min(mc, (size_t)pad_to(m, 128));
  const size_t sKs = mc * npad;
  const int Bc = (int)bgp_switch_cap(BGP_SW_ITEM_CHUNK, std::max<size_t>(1, std::min<size_t>((size_t)B, ((size_t)1 << 29) / sKs)));
  const int tmc = (int)(mc / IF_TM), tn = npad / IF_TN, npanel = (tn + S4_PW - 1) / S4_PW;
  const size_t np = (size_t)tmc * Bc * npad, Bn = (size_t)B * n, nF = (size_t)B * n_focus * n;
  double *dXq, *dH, *dnoise, *dKs, *dmpart, *dmean, *dvar, *ppart[4], *dres[4], *dfm = nullptr, *dfv = nullptr;
  int *parg, *darg, *dst;
  BgpScratch live(c);
  BGP_TRY(live.carve([&](BgpCarve& s) {
    dXq = s.take<double>((size_t)m * d);
    dH = s.take<double>((size_t)B * hp);
    dnoise = s.take<double>(B);
    dKs = s.take<double>((size_t)Bc * sKs);
    dmpart = s.take<double>((size_t)Bc * (npad / 128) * mc);
    dmean = s.take<double>((size_t)Bc * mc);
    dvar = s.take<double>((size_t)Bc * mc);
    for (int k = 0; k < 4; k++) ppart[k] = s.take<double>(np);
    parg = s.take<int>(np);
    for (int k = 0; k < 4; k++) dres[k] = s.take<double>(Bn);
    darg = s.take<int>(Bn);
    if (n_focus) dfm = s.take<double>(nF), dfv = s.take<double>(nF);
    dst = s.take<int>(B);
  }));
  BGP_TRY(c->drowpart.ensure((size_t)Bc * (npad / bgp_rowquad_tile()) * mc));
  hipStream_t st = c->stream;
  BGP_HIP(bgp_memcpy_async(dXq, Xq, (size_t)m * d * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(dH, h_kernel, (size_t)B * hp * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(dnoise, noise, (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(hipMemsetAsync(dst, 0, (size_t)B * sizeof(int), st));
  c->chunk_last[0] = c->chunk_last[1] = 0;
  for (int b0 = 0; b0 < B; b0 += Bc) {
    c->chunk_last[0]++;
    const int nb = std::min(Bc, B - b0);
    const double* Kinv = c->dKinv + (size_t)b0 * npad * npad;
    const double* al = c->dalpha_sol + (size_t)b0 * npad;
    for (int m0 = 0; m0 < m; m0 += (int)mc) {
      if (b0 == 0) c->chunk_last[1]++;
      const int mm = std::min((int)mc, m - m0), mmp = pad_to(mm, 128), tm = mmp / IF_TM;
      BGP_TRY(bgp_launch_moments(c, nb, dH + (size_t)b0 * hp, mm, dXq + (size_t)m0 * d, 0, c->dXeff, 0, al, Kinv, dKs, npad, sKs,
                                 dmpart, dmean, dvar));
      hipLaunchKernelGGL(infl_kernel, dim3(npanel * S4_PW * tm, nb), dim3(256), 0, st, (const double*)dKs, sKs, Kinv, al,
                         (const double*)dvar, (size_t)mmp, (const double*)(dnoise + b0), npad, n, mm, m0, n_focus, tm, ppart[0],
                         ppart[1], ppart[2], ppart[3], parg, n_focus ? dfm + (size_t)b0 * n_focus * n : nullptr,
                         n_focus ? dfv + (size_t)b0 * n_focus * n : nullptr);
      BGP_HIP(hipGetLastError());
      const size_t ob = (size_t)b0 * n;
      hipLaunchKernelGGL(infl_reduce_kernel, dim3((n + 255) / 256, nb), dim3(256), 0, st, (const double*)ppart[0],
                         (const double*)ppart[1], (const double*)ppart[2], (const double*)ppart[3], (const int*)parg, tm, npad, n,
                         m0 == 0 ? 1 : 0, m0 + mm == m ? 1 : 0, dres[0] + ob, dres[1] + ob, dres[2] + ob, dres[3] + ob, darg + ob,
                         dst + b0);
      BGP_HIP(hipGetLastError());
    }
  }
  double* host[4] = {out.sum_dm2, out.sum_cook, out.sum_kl, out.max_abs};
  for (int k = 0; k < 4; k++) BGP_HIP(bgp_memcpy_async(host[k], dres[k], Bn * sizeof(double), hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_memcpy_async(out.arg_max, darg, Bn * sizeof(int), hipMemcpyDeviceToHost, st));
  if (n_focus) {
    BGP_HIP(bgp_memcpy_async(out.dmu_focus, dfm, nF * sizeof(double), hipMemcpyDeviceToHost, st));
    BGP_HIP(bgp_memcpy_async(out.dvar_focus, dfv, nF * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  BGP_HIP(bgp_memcpy_async(out.status, dst, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_stream_sync(st));
  return BGP_OK;
}

extern "C" int bgp_influence(bgp_ctx* c, int B, const double* h_kernel, const double* noise, int m, const double* Xq, int n_focus,
                             double* sum_dm2, double* sum_cook, double* sum_kl, double* max_abs, int* arg_max, double* dmu_focus,
                             double* dvar_focus, int* status) {
  BGP_TRY(bgp_guard(c, "bgp_influence", BGP_POST_PLAIN));
  if (!h_kernel || !noise || !Xq || !sum_dm2 || !sum_cook || !sum_kl || !max_abs || !arg_max || !status || B < 1 || B > 65535 ||
      m < 1 || m > (1 << 24) || n_focus < 0 || n_focus > std::min(m, IF_FMAX) || (n_focus > 0 && (!dmu_focus || !dvar_focus))) {
    bgp_set_error("bgp_influence: bad argument (1 <= B <= 65535 posteriors, 1 <= m <= 2^24 rows, 0 <= n_focus <= min(m, %d), no NULL "
                  "array but the focus outputs at n_focus = 0)", IF_FMAX);
    return BGP_ERR_INVALID;
  }
  if (c->d > IF_DMAX || c->has_warp) {
    bgp_set_error("bgp_influence: %s", c->has_warp ? "warped inputs are not supported" : "d > 32 is not supported");
    return BGP_ERR_INVALID;
  }
  for (int b = 0; b < B; b++)
    if (!(noise[b] >= 0.0) || !std::isfinite(noise[b])) {
      bgp_set_error("bgp_influence: noise[%d] is not a finite variance >= 0", b);
      return BGP_ERR_INVALID;
    }
  BGP_TRY(bgp_guard(c, "bgp_influence", BGP_POST_PLAIN, B));
  const InflOut out{sum_dm2, sum_cook, sum_kl, max_abs, arg_max, dmu_focus, dvar_focus, status};
  return post_call(c, [&] { return infl_run(c, B, h_kernel, noise, m, Xq, n_focus, out); });
}
