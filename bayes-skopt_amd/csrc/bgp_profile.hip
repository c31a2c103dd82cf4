// Profile curves and maps of the surrogate mean: the best the mean can be with one or two coordinates held
// at a grid value and every other coordinate re-optimised inside the box,
//   prof_b(D, g) = min over x in [lo, hi] with x_D = g of mean_b(x)        xarg_b(D, g) = the minimiser found.
// Thousands of small bounded searches whose neighbours are excellent starting points: the continuation lives on the device.
//   line       the cells swept along the LAST panel dimension: a 1-D panel is one line of ng[k1] cells, a 2-D panel ng[k1] lines of
//              ng[k2] cells with x[k1] fixed for the line
//   workgroup  one per (line, chain s, posterior b), PG_NT threads: chain s starts from X0[s] clipped into the box, the line's fixed
//              coordinate overwritten; its anchor is the cell whose grid value is nearest the start's swept coordinate (ties: the
//              lower index).  It minimises at the anchor, walks forward to the last cell, restarts from the anchor's end point and
//              walks backward to cell 0.  At every cell: swept coordinate = lo = hi = grid value, free coordinates kept from the
//              previous cell, pg_bfgs (bgp_bfgs.h) on pg_eval (bgp_pg.h) with kappa = 0 -- the mean alone: no second pass, the
//              resident inverse is never read --, one closing evaluation where the last trial point was not the end point.
// pg_bfgs resets its matrix on entry, so a (chain, cell) result is bit for bit what bgp_minimize_starts returns from the cell's
// start in the cell's degenerate box.  Kernel parameters, 1 / l, the box and the swept grid column are staged once per workgroup;
// the k / g rows live in dynamic LDS up to PG_NLDS points and in per-workgroup scratch rows beyond.  A second kernel, one thread per
// (posterior, cell), takes the lowest value over the chains in ascending chain order.  Plain launches; no workgroup waits for
// another; every loop is bounded by an argument; no floating-point atomics.
#include "bgp_common.h"
#include "bgp_device.h"
#include "bgp_bfgs.h"
#include "bgp_pg.h"

#define PF_GMAX 256        // grid values per dimension (bgp_partial_dependence's limit)
#define PF_MAX_CELLS (1 << 24)

struct PfLine {            // one line: the fixed coordinate (kf = -1: none) and its value's grid row, the swept one, cells, offset
  int kf, jf, ks, ns, off, pad[3];
};

// the workgroup's LDS at the largest n served from LDS: W, Bf, the grid column, the anchor's end point and the k / g rows
static_assert(sizeof(PgWork) + sizeof(PgBfgs) + (PF_GMAX + PG_DMAX) * sizeof(double) + 2 * PG_NLDS * sizeof(double) <= 65536,
              "pf_line_kernel: more than 64 KB of LDS at n = PG_NLDS");

// One workgroup per (line of the chunk, chain, posterior).  Staging layout: item = (b * cells + cell - c0) * S + s.
template <int STAT, int FORM>
__global__ void __launch_bounds__(PG_NT) pf_line_kernel(const double* __restrict__ X, int n, int d, int npad,
                                                        const double* __restrict__ alphaB, const double* __restrict__ H,
                                                        double y_mean, double y_std, const double* __restrict__ X0,
                                                        const double* __restrict__ lo_, const double* __restrict__ hi_,
                                                        const double* __restrict__ grid, const PfLine* __restrict__ lines, int c0,
                                                        int cells, double gtol, int max_iter, double* scratch,
                                                        double* __restrict__ cval, double* __restrict__ cx, int* __restrict__ cst,
                                                        int* __restrict__ cev) {
#pragma clang fp contract(off)
  extern __shared__ double pg_dyn[];
  __shared__ PgWork W;
  __shared__ PgBfgs Bf;
  __shared__ double gcol[PF_GMAX];  // the swept dimension's grid values
  __shared__ double xa[PG_DMAX];    // the anchor's end point
  const int tid = threadIdx.x, s = blockIdx.y, b = blockIdx.z, S = gridDim.y;
  const PfLine ln = lines[blockIdx.x];
  const int ks = ln.ks, ns = ln.ns;
  const double* h = H + (size_t)b * (d + 2);
  const double* alpha = alphaB + (size_t)b * npad;
  if (tid < d) {
    double l = lo_[tid], u = hi_[tid];
    if (tid == ln.kf) l = u = grid[(size_t)ln.jf * d + tid];
    double v = X0[(size_t)s * d + tid];
    v = v < l ? l : (v > u ? u : v);
    if (tid == ln.kf) v = l;  // (overwritten, not clipped: a NaN there does not survive)
    Bf.lo[tid] = l;
    Bf.hi[tid] = u;
    Bf.x[tid] = v;
    W.il[tid] = 1.0 / exp(h[1 + tid]);
  }
  for (int j = tid; j < ns; j += PG_NT) gcol[j] = grid[(size_t)j * d + ks];
  const double cst_ = exp(h[0]);
  double *kb, *gb;
  pg_rows(pg_dyn, scratch, n, npad, (b * (int)S + s) * (int)gridDim.x + (int)blockIdx.x, kb, gb);
  __syncthreads();
  // the anchor: nearest grid value to the clipped start's swept coordinate, ties (and a NaN coordinate) to the lower index
  int anchor = 0;
  {
    const double xs = Bf.x[ks];
    double best = fabs(gcol[0] - xs);
    for (int j = 1; j < ns; j++) {
      const double dj = fabs(gcol[j] - xs);
      if (dj < best) best = dj, anchor = j;
    }
  }
  auto eval = [&] { pg_eval<STAT, FORM>(X, n, d, alpha, nullptr, npad, cst_, 0.0, false, kb, gb, W); };
  // anchor, forward to ns - 1, then from the anchor's end point backward to 0: at most ns cells
  for (int step = 0; step < ns; step++) {
    const int cell = step <= ns - 1 - anchor ? anchor + step : ns - 1 - step;
    __syncthreads();
    if (tid < d) {
      if (step == ns - anchor) Bf.x[tid] = xa[tid];  // the backward sweep restarts from the anchor's end point
      if (tid == ks) Bf.x[tid] = Bf.lo[tid] = Bf.hi[tid] = gcol[cell];
      W.x[tid] = Bf.x[tid];
    }
    __syncthreads();
    int it, nev;
    const int st = pg_bfgs(
        Bf, W.x, d, gtol, max_iter, eval, [&] { return pg_objective(W, y_mean, y_std, 0.0); },
        [&](int t) { return pg_gradient(W, t, y_std, 0.0); }, it, nev);
    bool there = true;  // the last evaluation was made at the end point
    for (int t = 0; t < d; t++) there = there && W.x[t] == Bf.x[t];
    if (!there) {
      __syncthreads();
      if (tid < d) W.x[tid] = Bf.x[tid];
      eval();
      nev++;
    }
    const size_t o = ((size_t)b * cells + (size_t)(ln.off - c0 + cell)) * S + s;
    if (tid < d) {
      cx[o * d + tid] = Bf.x[tid];
      if (step == 0) xa[tid] = Bf.x[tid];
    }
    if (tid == 0) {
      cval[o] = W.mean;
      cst[o] = st;
      cev[o] = nev;
    }
  }
}

// One thread per (posterior, cell of the chunk): the lowest value over the chains in ascending chain order -- a tie keeps the lower
// chain, a non-finite value never wins against a finite one --, that chain's point, the chains with status 0, and the evaluations
// spent (an integer sum: its order does not matter).
__global__ void __launch_bounds__(256) pf_reduce_kernel(const double* __restrict__ cval, const double* __restrict__ cx,
                                                        const int* __restrict__ cst, const int* __restrict__ cev, int cells, int S,
                                                        int d, double* __restrict__ val, double* __restrict__ xarg,
                                                        int* __restrict__ best_chain, int* __restrict__ n_conv,
                                                        unsigned long long* __restrict__ evals) {
  const int i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (i >= cells) return;
  const size_t o = ((size_t)b * cells + i) * S;
  int best = 0, nc = 0;
  double vb = cval[o];
  unsigned long long ev = 0;
  for (int s = 0; s < S; s++) {
    const double v = cval[o + s];
    if (s > 0 && isfinite(v) && (!isfinite(vb) || v < vb)) vb = v, best = s;
    nc += cst[o + s] == 0;
    ev += (unsigned long long)cev[o + s];
  }
  const size_t r = (size_t)b * cells + i;
  val[r] = vb;
  best_chain[r] = best;
  n_conv[r] = nc;
  for (int t = 0; t < d; t++) xarg[r * d + t] = cx[(o + best) * d + t];
  atomicAdd(evals + b, ev);
}

__global__ void pf_zero_kernel(unsigned long long* p, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = 0ull;
}

static int pf_run(bgp_ctx* c, int B, const double* h_kernel, double y_mean, double y_std, int S, const double* X0, const double* lo,
                  const double* hi, int gmax, const double* grid, const std::vector<PfLine>& lines, int total, double gtol,
                  int max_iter, double* val, double* xarg, int* best_chain, int* n_conv, double* chain_val, double* chain_x,
                  int* chain_status, long long* evals) {
  const int n = c->n, d = c->d, npad = c->npad, nl = (int)lines.size();
  const size_t p = d + 2, BS = (size_t)B * S;
  const bool lds = n <= PG_NLDS;
  int gm = 1;  // cells of the longest line
  for (const PfLine& l : lines) gm = std::max(gm, l.ns);
  // chunks of lines: the staging block of B S cells (2 + d) doubles, and B S scratch rows of 2 npad doubles
  // per line beyond PG_NLDS points
  size_t lc = std::max<size_t>(1, ((size_t)1 << 24) / (BS * gm * (2 + (size_t)d)));
  if (!lds) lc = std::min(lc, std::max<size_t>(1, ((size_t)1 << 26) / (BS * 2 * npad)));
  lc = std::min(bgp_switch_cap(BGP_SW_ROW_CHUNK, lc), (size_t)nl);  // (tests: one line per chunk against the default)
  size_t cc = 0;  // cells of the largest chunk
  for (size_t l0 = 0; l0 < (size_t)nl; l0 += lc) {
    const PfLine& last = lines[std::min(l0 + lc, (size_t)nl) - 1];
    cc = std::max(cc, (size_t)(last.off + last.ns - lines[l0].off));
  }
  double *dH, *dX0, *dlo, *dhi, *dG, *dcv, *dcx, *dval, *dxa, *rows = nullptr;
  int *dcs, *dce, *dbest, *dnc;
  unsigned long long* dev;
  PfLine* dlines;
  BgpScratch live(c);
  BGP_TRY(live.carve([&](BgpCarve& k) {
    dH = k.take<double>(B * p);
    dX0 = k.take<double>((size_t)S * d);
    dlo = k.take<double>(d);
    dhi = k.take<double>(d);
    dG = k.take<double>((size_t)gmax * d);
    dlines = k.take<PfLine>(nl);
    dev = k.take<unsigned long long>(B);
    dcv = k.take<double>(BS * cc);
    dcx = k.take<double>(BS * cc * d);
    dcs = k.take<int>(BS * cc);
    dce = k.take<int>(BS * cc);
    dval = k.take<double>((size_t)B * cc);
    dxa = k.take<double>((size_t)B * cc * d);
    dbest = k.take<int>((size_t)B * cc);
    dnc = k.take<int>((size_t)B * cc);
    if (!lds) rows = k.take<double>(BS * lc * 2 * npad);
  }));
  const size_t shmem = lds ? 2 * (size_t)n * sizeof(double) : 0;
  hipStream_t q = c->stream;
  BGP_HIP(bgp_memcpy_async(dH, h_kernel, B * p * sizeof(double), hipMemcpyHostToDevice, q));
  BGP_HIP(bgp_memcpy_async(dX0, X0, (size_t)S * d * sizeof(double), hipMemcpyHostToDevice, q));
  BGP_HIP(bgp_memcpy_async(dlo, lo, (size_t)d * sizeof(double), hipMemcpyHostToDevice, q));
  BGP_HIP(bgp_memcpy_async(dhi, hi, (size_t)d * sizeof(double), hipMemcpyHostToDevice, q));
  BGP_HIP(bgp_memcpy_async(dG, grid, (size_t)gmax * d * sizeof(double), hipMemcpyHostToDevice, q));
  BGP_HIP(bgp_memcpy_async(dlines, lines.data(), (size_t)nl * sizeof(PfLine), hipMemcpyHostToDevice, q));
  hipLaunchKernelGGL(pf_zero_kernel, dim3((B + 255) / 256), dim3(256), 0, q, dev, B);
  c->chunk_last[0] = 1, c->chunk_last[1] = 0;
  const size_t T = (size_t)total;
  for (size_t l0 = 0; l0 < (size_t)nl; l0 += lc) {
    c->chunk_last[1]++;
    const int ll = (int)std::min(lc, (size_t)nl - l0), c0 = lines[l0].off;
    const int cells = lines[l0 + ll - 1].off + lines[l0 + ll - 1].ns - c0;
    const dim3 wgs(ll, S, B);  // (inside KB_DISPATCH S and F are the kernel's template arguments)
    KB_DISPATCH(c->ks.stationary, c->ks.form,
                hipLaunchKernelGGL((pf_line_kernel<S, F>), wgs, dim3(PG_NT), shmem, q, c->dXeff, n, d, npad, c->dalpha_sol,
                                   dH, y_mean, y_std, dX0, dlo, dhi, dG, dlines + l0, c0, cells, gtol, max_iter, rows, dcv, dcx, dcs,
                                   dce));
    hipLaunchKernelGGL(pf_reduce_kernel, dim3((cells + 255) / 256, B), dim3(256), 0, q, dcv, dcx, dcs, dce, cells, S, d, dval, dxa,
                       dbest, dnc, dev);
    BGP_HIP(hipGetLastError());
    // per posterior one contiguous run of the chunk's cells
    const size_t w1 = (size_t)cells * sizeof(double), wi = (size_t)cells * sizeof(int);
    BGP_HIP(bgp_memcpy2d_async(val + c0, T * sizeof(double), dval, w1, w1, B, hipMemcpyDeviceToHost, q));
    BGP_HIP(bgp_memcpy2d_async(xarg + (size_t)c0 * d, T * d * sizeof(double), dxa, w1 * d, w1 * d, B, hipMemcpyDeviceToHost, q));
    BGP_HIP(bgp_memcpy2d_async(best_chain + c0, T * sizeof(int), dbest, wi, wi, B, hipMemcpyDeviceToHost, q));
    BGP_HIP(bgp_memcpy2d_async(n_conv + c0, T * sizeof(int), dnc, wi, wi, B, hipMemcpyDeviceToHost, q));
    if (chain_val)
      BGP_HIP(bgp_memcpy2d_async(chain_val + (size_t)c0 * S, T * S * sizeof(double), dcv, w1 * S, w1 * S, B, hipMemcpyDeviceToHost, q));
    if (chain_x)
      BGP_HIP(bgp_memcpy2d_async(chain_x + (size_t)c0 * S * d, T * S * d * sizeof(double), dcx, w1 * S * d, w1 * S * d, B,
                                 hipMemcpyDeviceToHost, q));
    if (chain_status)
      BGP_HIP(bgp_memcpy2d_async(chain_status + (size_t)c0 * S, T * S * sizeof(int), dcs, wi * S, wi * S, B, hipMemcpyDeviceToHost, q));
    if (l0 + lc >= (size_t)nl)
      BGP_HIP(bgp_memcpy_async(evals, dev, (size_t)B * sizeof(long long), hipMemcpyDeviceToHost, q));
    BGP_HIP(bgp_stream_sync(q));  // (the next chunk reuses the buffers)
  }
  return BGP_OK;
}

extern "C" int bgp_profile_dependence(bgp_ctx* c, int B, const double* h_kernel, double y_mean, double y_std, int S, const double* X0,
                                      const double* lo, const double* hi, int gmax, const int* ng, const double* grid, int P,
                                      const int* panels, double gtol, int max_iter, double* val, double* xarg, int* best_chain,
                                      int* n_converged, double* chain_val, double* chain_x, int* chain_status, long long* evals) {
  const char* who = "bgp_profile_dependence";
  BGP_TRY(bgp_guard(c, who, BGP_POST_PLAIN));
  if (!h_kernel || !X0 || !lo || !hi || !ng || !grid || !panels || !val || !xarg || !best_chain || !n_converged || !evals || B < 1 ||
      B > 65535 || S < 1 || S > 65535 || P < 1 || gmax < 1 || gmax > PF_GMAX || max_iter < 0 || !(gtol >= 0.0)) {
    bgp_set_error("%s: bad argument (1 <= B, S <= 65535, P >= 1, 1 <= gmax <= %d, max_iter >= 0, gtol >= 0, no NULL among the "
                  "required arrays)", who, PF_GMAX);
    return BGP_ERR_INVALID;
  }
  const int d = c->d;
  if (d > PG_DMAX || c->has_warp) {
    bgp_set_error("%s: %s", who, c->has_warp ? "warped inputs are not supported" : "d > 32 is not supported");
    return BGP_ERR_INVALID;
  }
  for (int k = 0; k < d; k++) {
    if (ng[k] < 1 || ng[k] > gmax) {
      bgp_set_error("%s: ng[%d] = %d outside 1 .. gmax = %d", who, k, ng[k], gmax);
      return BGP_ERR_INVALID;
    }
    if (!(lo[k] <= hi[k])) {
      bgp_set_error("%s: empty box in dimension %d", who, k);
      return BGP_ERR_INVALID;
    }
  }
  // the lines of every panel, in panel order
  std::vector<PfLine> lines;
  long long total = 0;
  for (int p = 0; p < P; p++) {
    const int k1 = panels[2 * p], k2 = panels[2 * p + 1];
    if (k1 < 0 || k1 >= d || k2 < -1 || k2 >= d || k1 == k2) {
      bgp_set_error("%s: panel %d = (%d, %d) is not (k, -1) or (k1, k2), k1 != k2, inside [0, %d)", who, p, k1, k2, d);
      return BGP_ERR_INVALID;
    }
    for (int k : {k1, k2})
      for (int j = 0; k >= 0 && j < ng[k]; j++) {
        const double g = grid[(size_t)j * d + k];
        if (!(g >= lo[k] && g <= hi[k])) {
          bgp_set_error("%s: grid value %d of panel dimension %d lies outside [lo, hi]", who, j, k);
          return BGP_ERR_INVALID;
        }
      }
    const int kf = k2 < 0 ? -1 : k1, ks = k2 < 0 ? k1 : k2, nf = kf < 0 ? 1 : ng[kf];
    if (total + (long long)nf * ng[ks] > PF_MAX_CELLS) {
      bgp_set_error("%s: more than 2^24 grid cells in one call", who);
      return BGP_ERR_INVALID;
    }
    for (int j = 0; j < nf; j++) {
      lines.push_back(PfLine{kf, j, ks, ng[ks], (int)total, {0, 0, 0}});
      total += ng[ks];
    }
  }
  BGP_TRY(bgp_guard(c, who, BGP_POST_PLAIN, B));
  return post_call(c, [&] {
    return pf_run(c, B, h_kernel, y_mean, y_std, S, X0, lo, hi, gmax, grid, lines, (int)total, gtol, max_iter, val, xarg, best_chain,
                  n_converged, chain_val, chain_x, chain_status, evals);
  });
}
