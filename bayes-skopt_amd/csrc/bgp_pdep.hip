// Partial dependence of the surrogate mean on one or two input dimensions.
//
// For resident posterior b, S sample rows x_s and a panel D = {k1} or {k1, k2} with grid values g:
//   pd_b(D, g) = (1 / S) sum_s sum_j alpha_bj k_b(x_s[D <- g], X_j)                       (normalised-y units)
// In coordinates scaled by the length scales (u = x / l, U = X / l) the squared distance of a synthetic row splits into
//   Q_sj   = sum_{k not in D} (u_sk - U_jk)^2      the sample part: one value per (sample, training point), whatever the cell
//   T_j(g) = sum_{k in D} (g_k / l_k - U_jk)^2     the grid part:   one value per (cell, training point), whatever the sample
// and k = kb_value(Q_sj + T_j(g), c).  Both parts are sums of squares (fma, ascending dimension); Q is never formed as "full
// distance minus the panel's terms".  The sum over the training points is a GEMV against cross-kernel values GENERATED from the
// two parts, tile by tile in LDS: nothing of size samples x cells x n exists.  fp64 VALU work, no MFMA shape.  Plain launches; no
// workgroup waits for another; no floating-point atomics (chunk partials, added in ascending chunk order by a second kernel); every
// loop is bounded by an argument.  A panel's values depend on the posterior, the samples, the grids and the panel alone -- its
// tiles, their order of accumulation and the chunks are the same whatever else shares the call.
#include "bgp_common.h"
#include "bgp_device.h"

#define PD_TJ 32      // training points per LDS tile
#define PD_SC 16      // samples per chunk (fixed: the order of accumulation must not depend on S, P or B)
#define PD_GT 16      // edge of a grid tile: 16 x 16 cells, one per thread
#define PD_DMAX 32    // input dimensions (larger d: the caller's route over predict)
#define PD_GMAX 256   // grid values per dimension
#define PD_XLD (PD_DMAX + 1)  // LDS row of a scaled sample (odd: lanes over the samples read distinct banks)

// out[b][r][k] = in[r][k] / l_bk: the scaled training inputs, samples and grid rows of posterior b (x / l as the cross kernel forms it)
__global__ void __launch_bounds__(256) pdep_scale_kernel(const double* __restrict__ in, int rows, int d, const double* __restrict__ H,
                                                         double* __restrict__ out) {
  const int idx = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (idx >= rows * d) return;
  const int k = idx % d;
  out[(size_t)b * rows * d + idx] = in[idx] / exp(H[(size_t)b * (d + 2) + 1 + k]);
}

// One workgroup: posterior b = blockIdx.z, sample chunk blockIdx.y, grid tile blockIdx.x (tile record: ka, kb, Ga, Gb, a0, b0, off, -;
// axis a is the slow one of the panel's block, ka = -1 and Ga = 1 for a 1-D panel, whose grid lies on axis b).  Thread (ta, tb) owns
// cell (a0 + ta, b0 + tb).  Per tile of PD_TJ training points the workgroup writes once Q[j][s], Ta[j][ga], Tb[j][gb] and alpha[j]; a
// thread then forms t = Ta + Tb once per j and runs over the chunk's samples.  LDS reads of the inner loops: Q and alpha are
// broadcasts, Tb is 16 consecutive doubles per 16 lanes, Ta one address per 16 lanes.  16.6 KB of LDS.
template <int STAT, int FORM>
__global__ void __launch_bounds__(256) pdep_kernel(const double* __restrict__ Us, const double* __restrict__ us,
                                                   const double* __restrict__ gs, const double* __restrict__ H,
                                                   const double* __restrict__ alpha, const int* __restrict__ tiles, int n, int npad,
                                                   int d, int S, int gmax, int total, int nchunk, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double Qs[PD_TJ * PD_SC];
  __shared__ double Ta[PD_TJ * PD_GT];
  __shared__ double Tb[PD_TJ * PD_GT];
  __shared__ double al[PD_TJ];
  __shared__ double xs[PD_SC * PD_XLD];
  const int tid = threadIdx.x, b = blockIdx.z, ch = blockIdx.y;
  const int* tl = tiles + 8 * (size_t)blockIdx.x;
  const int ka = tl[0], kb = tl[1], Ga = tl[2], Gb = tl[3], a0 = tl[4], b0 = tl[5], off = tl[6];
  const int s0 = ch * PD_SC, sc = min(PD_SC, S - s0);
  const double cst = exp(H[(size_t)b * (d + 2)]);
  const double* Ub = Us + (size_t)b * n * d;
  const double* ub = us + ((size_t)b * S + s0) * d;
  const double* gb = gs + (size_t)b * gmax * d;
  const double* ab = alpha + (size_t)b * npad;
  for (int idx = tid; idx < sc * d; idx += 256) {
    const int s = idx / d, k = idx - s * d;
    xs[s * PD_XLD + k] = ub[idx];
  }
  const int ta = tid >> 4, tb = tid & 15, ia = a0 + ta, ib = b0 + tb;
  const bool live = ia < Ga && ib < Gb;  // (a 1-D panel: the first 16 threads, one wave)
  double acc = 0.0;
  for (int j0 = 0; j0 < n; j0 += PD_TJ) {
    const int jc = min(PD_TJ, n - j0);
    __syncthreads();
    // the sample part
    for (int idx = tid; idx < jc * PD_SC; idx += 256) {
      const int j = idx >> 4, s = idx & 15;
      if (s < sc) {
        const double* Uj = Ub + (size_t)(j0 + j) * d;
        double q = 0.0;
        for (int k = 0; k < d; k++)
          if (k != ka && k != kb) {
            const double df = xs[s * PD_XLD + k] - Uj[k];
            q = fma(df, df, q);
          }
        Qs[j * PD_SC + s] = q;
      }
    }
    // the grid parts of the tile's 16 + 16 grid values (cells past the grid, and axis a of a 1-D panel: 0)
    for (int idx = tid; idx < jc * 2 * PD_GT; idx += 256) {
      const int j = idx >> 5, g = idx & 15, axis = (idx >> 4) & 1;
      const int k = axis ? kb : ka, cell = (axis ? b0 : a0) + g;
      double v = 0.0;
      if (k >= 0 && cell < (axis ? Gb : Ga)) {
        const double df = gb[(size_t)cell * d + k] - Ub[(size_t)(j0 + j) * d + k];
        v = df * df;
      }
      (axis ? Tb : Ta)[j * PD_GT + g] = v;
    }
    if (tid < jc) al[tid] = ab[j0 + tid];
    __syncthreads();
    if (live)
      for (int j = 0; j < jc; j++) {
        const double t = Ta[j * PD_GT + ta] + Tb[j * PD_GT + tb], a = al[j];
        for (int s = 0; s < sc; s++) acc = fma(kb_value<STAT, FORM>(Qs[j * PD_SC + s] + t, cst), a, acc);
      }
  }
  if (live) part[((size_t)b * nchunk + ch) * total + off + (size_t)ia * Gb + ib] = acc;
}

// out[b][i] = (sum of the chunk partials, ascending chunk) / S
__global__ void __launch_bounds__(256) pdep_reduce_kernel(const double* __restrict__ part, int nchunk, int total, int S,
                                                          double* __restrict__ out) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= total) return;
  double s = 0.0;
  for (int c = 0; c < nchunk; c++) s += part[((size_t)b * nchunk + c) * total + i];
  out[(size_t)b * total + i] = s / (double)S;
}

static int pdep_run(bgp_ctx* c, int B, const double* h_kernel, int ns, const double* Xs, int gmax, const double* grid,
                    const std::vector<int>& tiles, int total, double* out) {
  const int n = c->n, d = c->d, npad = c->npad, nchunk = (ns + PD_SC - 1) / PD_SC, ntiles = (int)(tiles.size() / 8);
  const size_t p = d + 2;
  double *dXs, *dG, *dH, *dUs, *dus, *dgs, *dpart, *dout;
  int* dtiles;
  BgpScratch live(c);
  BGP_TRY(live.carve([&](BgpCarve& s) {
    dXs = s.take<double>((size_t)ns * d);
    dG = s.take<double>((size_t)gmax * d);
    dH = s.take<double>((size_t)B * p);
    dUs = s.take<double>((size_t)B * n * d);
    dus = s.take<double>((size_t)B * ns * d);
    dgs = s.take<double>((size_t)B * gmax * d);
    dtiles = s.take<int>(tiles.size());
    dpart = s.take<double>((size_t)B * nchunk * total);  // the chunk partials: all the scratch that grows with the cells
    dout = s.take<double>((size_t)B * total);
  }));
  hipStream_t st = c->stream;
  // samples and grid rows the way predict's queries go up: through the context-level warp when one is set
  BGP_TRY(post_stage_queries(c, dXs, Xs, ns));
  BGP_TRY(post_stage_queries(c, dG, grid, gmax));
  BGP_HIP(bgp_memcpy_async(dH, h_kernel, (size_t)B * p * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(dtiles, tiles.data(), tiles.size() * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(pdep_scale_kernel, dim3((n * d + 255) / 256, B), dim3(256), 0, st, c->dXeff, n, d, dH, dUs);
  hipLaunchKernelGGL(pdep_scale_kernel, dim3((ns * d + 255) / 256, B), dim3(256), 0, st, dXs, ns, d, dH, dus);
  hipLaunchKernelGGL(pdep_scale_kernel, dim3((gmax * d + 255) / 256, B), dim3(256), 0, st, dG, gmax, d, dH, dgs);
  KB_DISPATCH(c->ks.stationary, c->ks.form,
              hipLaunchKernelGGL((pdep_kernel<S, F>), dim3(ntiles, nchunk, B), dim3(256), 0, st, dUs, dus, dgs, dH, c->dalpha_sol,
                                 dtiles, n, npad, d, ns, gmax, total, nchunk, dpart));
  hipLaunchKernelGGL(pdep_reduce_kernel, dim3((total + 255) / 256, B), dim3(256), 0, st, dpart, nchunk, total, ns, dout);
  BGP_HIP(hipGetLastError());
  BGP_HIP(bgp_memcpy_async(out, dout, (size_t)B * total * sizeof(double), hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_stream_sync(st));
  return BGP_OK;
}

extern "C" int bgp_partial_dependence(bgp_ctx* c, int B, const double* h_kernel, int S, const double* Xs, int gmax, const int* ng,
                                      const double* grid, int P, const int* panels, double* out) {
  BGP_TRY(bgp_guard(c, "bgp_partial_dependence", BGP_POST_PLAIN));
  if (!c || !h_kernel || !Xs || !ng || !grid || !panels || !out || B <= 0 || S <= 0 || P <= 0 || gmax <= 0 || gmax > PD_GMAX) {
    bgp_set_error("bgp_partial_dependence: bad argument (B, S, P >= 1, 1 <= gmax <= %d)", PD_GMAX);
    return BGP_ERR_INVALID;
  }
  const int d = c->d;
  if (d > PD_DMAX) {
    bgp_set_error("bgp_partial_dependence: d > %d is not supported", PD_DMAX);
    return BGP_ERR_INVALID;
  }
  for (int k = 0; k < d; k++)
    if (ng[k] < 1 || ng[k] > gmax) {
      bgp_set_error("bgp_partial_dependence: ng[%d] = %d outside 1 .. gmax = %d", k, ng[k], gmax);
      return BGP_ERR_INVALID;
    }
  // the grid tiles of every panel, in panel order: ka, kb, Ga, Gb, a0, b0, offset of the panel's block, -
  std::vector<int> tiles;
  long long total = 0;
  for (int p = 0; p < P; p++) {
    const int k1 = panels[2 * p], k2 = panels[2 * p + 1];
    if (k1 < 0 || k1 >= d || k2 < -1 || k2 >= d || k1 == k2) {
      bgp_set_error("bgp_partial_dependence: panel %d = (%d, %d) is not (k, -1) or (k1, k2), k1 != k2, inside [0, %d)", p, k1, k2, d);
      return BGP_ERR_INVALID;
    }
    const int ka = k2 < 0 ? -1 : k1, kb = k2 < 0 ? k1 : k2, Ga = ka < 0 ? 1 : ng[ka], Gb = ng[kb];
    for (int a0 = 0; a0 < Ga; a0 += PD_GT)
      for (int b0 = 0; b0 < Gb; b0 += PD_GT) tiles.insert(tiles.end(), {ka, kb, Ga, Gb, a0, b0, (int)total, 0});
    total += (long long)Ga * Gb;
    if (total > (1ll << 30) || tiles.size() / 8 > (size_t)1 << 30) {
      bgp_set_error("bgp_partial_dependence: more than 2^30 grid cells in one call");
      return BGP_ERR_INVALID;
    }
  }
  if ((S + PD_SC - 1) / PD_SC > 65535 || B > 65535) {  // (launch grid: chunks on y, posteriors on z)
    bgp_set_error("bgp_partial_dependence: at most %d samples and 65535 posteriors per call", 65535 * PD_SC);
    return BGP_ERR_INVALID;
  }
  BGP_TRY(bgp_guard(c, "bgp_partial_dependence", BGP_POST_PLAIN, B));
  return post_call(c, [&] { return pdep_run(c, B, h_kernel, S, Xs, gmax, grid, tiles, (int)total, out); });
}
