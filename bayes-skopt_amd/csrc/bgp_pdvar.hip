// Partial dependence with its posterior variance and the cell covariance of the curves.
//
// For resident posterior b, S sample rows x_s, a panel D = {k1} or {k1, k2} and cells g, g' of it, with z_gs = x_s[D <- g], for the
// LATENT function (no white term; the constant of the sum form included), normalised-y units:
//   kbar_b(g)_j            = sum_s k_b(z_gs, X_j)                                    mean_b(g) = kbar_b(g)^T alpha_b / S
//   prior_b(D; g, g')      = sum_s sum_s' k_b(Qss' + T(g, g'))     Qss' = sum_{k not in D} (u_sk - u_s'k)^2,  T = sum_{k in D} (g_k / l_k - g'_k / l_k)^2
//   Cov[pd_b(g), pd_b(g')] = (prior_b(D; g, g') - kbar_b(g)^T K_b^-1 kbar_b(g')) / S^2
// Two synthesised rows of one cell differ only outside the panel: the variance's prior term (T = 0) is ONE number per (panel,
// posterior).  Stages, plain launches on the context's stream:
//   1  pdvar_kbar_kernel      Kbar (rows: the cells of a chunk in output order, padded to 128 with zero rows; columns: the npad
//                             training points, n .. npad zero) -- the layout bgp_launch_gemm4 mode 0 reads.  A workgroup owns 64
//                             training points (LDS tile, k-major) and four groups of at most 16 cells of one panel each; a wave takes
//                             a group, a lane a training point: 16 accumulators and 16 T_j(g) in registers, the samples wave-uniform;
//                             Q_sj once per sample (fma, ascending dimension over the dimensions outside the panel), spent on the 16
//                             cells; s ascending inside ONE thread.
//   2  bgp_launch_gemm4       Pm = Kbar K^-1 on the LDS-DMA ring (fp64 MFMA), 2 npad^2 flop per cell; not with `mean` alone.
//   3  pdvar_contract_kernel  a wave per cell: q_g = sum_j Pm_gj Kbar_gj and mean_g = sum_j alpha_j Kbar_gj / S (a lane its columns in
//                             ascending j, then the xor butterfly); with `cov` the same kernel per (g, g'), g > g', of a 1-D panel.
//   4  pdvar_prior_kernel     pairs s <= s' by GLOBAL pair index, 1024 per wave, off-diagonal pairs counted twice; Qss' once per pair,
//                             reused for every T(g, g') of the panel; wave partials, added in ascending order by pdvar_prior_reduce_kernel.
//   5  pdvar_finish_kernel / pdvar_cov_finish_kernel   (prior - q) / S^2, the variance clipped at 0; cov mirrored, its diagonal the variance.
// No workgroup waits for another; no floating-point atomics; every loop is bounded by an argument.  A cell's mean and variance and a
// 1-D panel's covariance depend on the posterior, the samples, the grids and the panel alone -- not on the other panels, on B, on
// the chunking or on which outputs are asked for.
#include "bgp_common.h"
#include "bgp_device.h"

#define PV_DMAX 32            // input dimensions
#define PV_GMAX 256           // grid values per dimension
#define PV_SMAX 16384         // samples (the prior is a pair sum)
#define PV_TJ 64              // training points per workgroup of the build
#define PV_CW 16              // cells per wave of the build
#define PV_PW 16              // pairs per lane of the prior: 1024 per wave (fixed: the order of accumulation must not depend on P or B)
#define PV_TB 32               // T values (cell pairs of a curve) per workgroup of the prior
#define PV_GRPMAX (4 * 65535)  // cell groups per chunk: four per workgroup on the build's grid y
#define PV_PARTMAX ((size_t)1 << 24)  // doubles of pair partials per launch of the prior

// t = r (r + 1) / 2 + c, 0 <= c <= r (t < 2^31; the two corrections run at most a step or two)
static __device__ __forceinline__ void pv_tri(int t, int& r, int& c) {
  int rr = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
  while ((long long)rr * (rr + 1) / 2 > t) rr--;
  while ((long long)(rr + 1) * (rr + 2) / 2 <= t) rr++;
  r = rr;
  c = t - (int)((long long)rr * (rr + 1) / 2);
}

static __device__ __forceinline__ double pv_wave_sum(double v) {
#pragma unroll
  for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w, 64);
  return v;
}

// Kbar[b][(row0 + i) npad + j] for the cell groups of a chunk (group record: panel, first cell, cells, first row; panel record: ka, kb,
// Gb, -; axis a the slow one, ka = -1 for a curve, whose grid lies on axis b).  grid (npad / 64, groups / 4, posteriors)
template <int STAT, int FORM>
__global__ void __launch_bounds__(256) pdvar_kbar_kernel(const double* __restrict__ Us, const double* __restrict__ us,
                                                         const double* __restrict__ gs, const double* __restrict__ H,
                                                         const int* __restrict__ pan, const int* __restrict__ grp, int ngrp, int n,
                                                         int npad, int d, int S, int gmax, size_t sR, double* __restrict__ Kbar) {
#pragma clang fp contract(off)
  __shared__ double Xt[PV_DMAX * PV_TJ];
  const int tid = threadIdx.x, lane = tid & 63;
  const int j0 = blockIdx.x * PV_TJ, b = blockIdx.z;
  const double* Ub = Us + (size_t)b * n * d;
  for (int idx = tid; idx < PV_TJ * d; idx += 256) {
    const int jj = idx / d, k = idx - jj * d;
    Xt[k * PV_TJ + jj] = (j0 + jj < n) ? Ub[(size_t)(j0 + jj) * d + k] : 0.0;
  }
  __syncthreads();
  const int g = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + (tid >> 6));
  if (g >= ngrp) return;
  const int p = __builtin_amdgcn_readfirstlane(grp[4 * g]), c0 = __builtin_amdgcn_readfirstlane(grp[4 * g + 1]);
  const int cnt = __builtin_amdgcn_readfirstlane(grp[4 * g + 2]), row0 = __builtin_amdgcn_readfirstlane(grp[4 * g + 3]);
  const int ka = __builtin_amdgcn_readfirstlane(pan[4 * p]), kb = __builtin_amdgcn_readfirstlane(pan[4 * p + 1]);
  const int Gb = __builtin_amdgcn_readfirstlane(pan[4 * p + 2]);
  const int j = j0 + lane;
  double* Kb = Kbar + (size_t)b * sR + (size_t)row0 * npad + j;
  if (j0 >= n) {  // (a tile of padding columns)
    for (int i = 0; i < cnt; i++) Kb[(size_t)i * npad] = 0.0;
    return;
  }
  const double cst = exp(H[(size_t)b * (d + 2)]);
  const double* ub = us + (size_t)b * S * d;
  const double* gb = gs + (size_t)b * gmax * d;
  double t[PV_CW], acc[PV_CW];
#pragma unroll
  for (int i = 0; i < PV_CW; i++) {  // (a slot past the group: the group's last cell, not written)
    const int c = c0 + (i < cnt ? i : cnt - 1), ia = c / Gb, ib = c - ia * Gb;
    const double dfb = gb[(size_t)ib * d + kb] - Xt[kb * PV_TJ + lane];
    double ta = 0.0;
    if (ka >= 0) {
      const double dfa = gb[(size_t)ia * d + ka] - Xt[ka * PV_TJ + lane];
      ta = dfa * dfa;
    }
    t[i] = ta + dfb * dfb;
    acc[i] = 0.0;
  }
  for (int s = 0; s < S; s++) {
    const double* x = ub + (size_t)s * d;  // (wave-uniform)
    double q = 0.0;
    for (int k = 0; k < d; k++)
      if (k != ka && k != kb) {
        const double df = x[k] - Xt[k * PV_TJ + lane];
        q = fma(df, df, q);
      }
#pragma unroll
    for (int i = 0; i < PV_CW; i++) acc[i] += kb_value<STAT, FORM>(q + t[i], cst);
  }
#pragma unroll
  for (int i = 0; i < PV_CW; i++)
    if (i < cnt) Kb[(size_t)i * npad] = (j < n) ? acc[i] : 0.0;
}

// rows [r0, r1) of every posterior's Kbar: zeros (the 128-row padding that the product reads)
__global__ void __launch_bounds__(256) pdvar_zero_rows_kernel(double* __restrict__ R, size_t sR, int r0, int r1, int npad) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx < (size_t)(r1 - r0) * npad) R[(size_t)blockIdx.y * sR + (size_t)r0 * npad + idx] = 0.0;
}

// A wave per unit u.  pairs == 0: unit = row u: q[u] = Pm_u . Kbar_u (with Pm) and mean[u] = alpha . Kbar_u / S (with mean).
// pairs != 0: unit u = g (g - 1) / 2 + g', g > g', of the panel whose rows start at row0: q[u] = Pm_(row0 + g) . Kbar_(row0 + g').
// grid (units / 4, posteriors)
__global__ void __launch_bounds__(256) pdvar_contract_kernel(const double* __restrict__ Kbar, const double* __restrict__ Pm, size_t sR,
                                                             const double* __restrict__ alphaB, int n, int npad, int S, int row0,
                                                             int nunit, int pairs, double* __restrict__ q, size_t sq,
                                                             double* __restrict__ mean) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int u = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (u >= nunit) return;
  int ra = row0 + u, rb = ra;
  if (pairs) {
    int r, c;
    pv_tri(u, r, c);
    ra = row0 + r + 1, rb = row0 + c;
  }
  const double* Kr = Kbar + (size_t)b * sR + (size_t)rb * npad;
  const double* Pr = Pm ? Pm + (size_t)b * sR + (size_t)ra * npad : nullptr;
  const double* ab = alphaB + (size_t)b * npad;
  double aq = 0.0, am = 0.0;
  for (int j = lane; j < n; j += 64) {
    const double kv = Kr[j];
    if (Pr) aq = fma(Pr[j], kv, aq);
    if (mean) am = fma(ab[j], kv, am);
  }
  aq = pv_wave_sum(aq);
  am = pv_wave_sum(am);
  if (lane == 0) {
    if (Pr) q[(size_t)b * sq + u] = aq;
    if (mean) mean[(size_t)b * sq + u] = am / (double)S;
  }
}

// part[((b ny + y) nchunk + chunk)] = sum over the 1024 pairs of wave chunk `chunk` of w k_b(Qss' + T_y), w = 1 (s = s') or 2.
// G == 0: the variance's prior, T = 0, of panel p0 + blockIdx.y (y = blockIdx.y, ny = gridDim.y).  G > 0: the 1-D panel p0, y = 0 ..
// nT: T of the cell pair t0 + y = g (g - 1) / 2 + g', g > g' (ny = nT), PV_TB of them per workgroup: blockIdx.y is the slice, and
// every slice forms the Q of its pairs again (d fused multiply-adds against PV_TB kernel values).  grid (chunks / 4, ., posteriors)
template <int STAT, int FORM>
__global__ void __launch_bounds__(256) pdvar_prior_kernel(const double* __restrict__ us, const double* __restrict__ gs,
                                                          const double* __restrict__ H, const int* __restrict__ pan, int S, int d,
                                                          int gmax, int Np, int nchunk, int p0, int G, int t0, int nT,
                                                          double* __restrict__ part) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, b = blockIdx.z;
  const int chunk = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (chunk >= nchunk) return;
  const int p = p0 + (G ? 0 : blockIdx.y), ny = G ? nT : gridDim.y, y0 = G ? 0 : blockIdx.y;
  const int ka = pan[4 * p], kb = pan[4 * p + 1];
  const double cst = exp(H[(size_t)b * (d + 2)]);
  const double* ub = us + (size_t)b * S * d;
  const double* gb = gs + (size_t)b * gmax * d;
  double Q[PV_PW], w[PV_PW];
#pragma unroll
  for (int i = 0; i < PV_PW; i++) {
    const long long e = (long long)chunk * (64 * PV_PW) + i * 64 + lane;
    Q[i] = 0.0, w[i] = 0.0;
    if (e < Np) {
      int sp, s;
      pv_tri((int)e, sp, s);
      w[i] = (s == sp) ? 1.0 : 2.0;
      double qv = 0.0;
      for (int k = 0; k < d; k++)
        if (k != ka && k != kb) {
          const double df = ub[(size_t)s * d + k] - ub[(size_t)sp * d + k];
          qv = fma(df, df, qv);
        }
      Q[i] = qv;
    }
  }
  const int ya = G ? blockIdx.y * PV_TB : 0, yb = G ? min(nT, ya + PV_TB) : 1;
  for (int y = ya; y < yb; y++) {
    double T = 0.0;
    if (G) {
      int r, c;
      pv_tri(t0 + y, r, c);
      const double df = gb[(size_t)(r + 1) * d + kb] - gb[(size_t)c * d + kb];
      T = df * df;
    }
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < PV_PW; i++) sum = fma(w[i], kb_value<STAT, FORM>(Q[i] + T, cst), sum);
    sum = pv_wave_sum(sum);
    if (lane == 0) part[((size_t)b * ny + y0 + y) * nchunk + chunk] = sum;
  }
}

// out[b so + o0 + y] = sum of the wave partials, ascending chunk; grid (ny / 256, posteriors)
__global__ void __launch_bounds__(256) pdvar_prior_reduce_kernel(const double* __restrict__ part, int nchunk, int ny,
                                                                 double* __restrict__ out, size_t so, int o0) {
#pragma clang fp contract(off)
  const int y = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (y >= ny) return;
  const double* pp = part + ((size_t)b * ny + y) * nchunk;
  double s = 0.0;
  for (int c = 0; c < nchunk; c++) s += pp[c];
  out[(size_t)b * so + o0 + y] = s;
}

// var[b][row] = max(0, (prior[b][panel of the row] - q[b][row]) / S^2); 16 groups per workgroup; grid (groups / 16, posteriors)
__global__ void __launch_bounds__(256) pdvar_finish_kernel(const int* __restrict__ grp, int ngrp, const double* __restrict__ prior,
                                                           size_t sp, const double* __restrict__ q, size_t sq, double S2,
                                                           double* __restrict__ var) {
#pragma clang fp contract(off)
  const int g = blockIdx.x * 16 + (threadIdx.x >> 4), i = threadIdx.x & 15, b = blockIdx.y;
  if (g >= ngrp || i >= grp[4 * g + 2]) return;
  const size_t o = (size_t)b * sq + grp[4 * g + 3] + i;
  const double v = (prior[(size_t)b * sp + grp[4 * g]] - q[o]) / S2;
  var[o] = v > 0.0 ? v : 0.0;  // (clipped at 0 as the predictive variance is)
}

// cov[b][g G + g'] of a 1-D panel whose rows start at row0: the variance on the diagonal, (priorT - qc) / S^2 of the pair beside it
__global__ void __launch_bounds__(256) pdvar_cov_finish_kernel(const double* __restrict__ priorT, const double* __restrict__ qc, int nT,
                                                               const double* __restrict__ var, size_t sq, int row0, int G, double S2,
                                                               double* __restrict__ cov) {
#pragma clang fp contract(off)
  const int idx = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (idx >= G * G) return;
  const int g = idx / G, h = idx - g * G;
  double v;
  if (g == h) {
    v = var[(size_t)b * sq + row0 + g];
  } else {
    const int hi = g > h ? g : h, lo = g > h ? h : g;
    const size_t t = (size_t)b * nT + hi * (hi - 1) / 2 + lo;
    v = (priorT[t] - qc[t]) / S2;
  }
  cov[(size_t)b * G * G + idx] = v;
}

// Cells per chunk: a multiple of 128 that depends on n alone, so that a posterior's Kbar stays within 2^25 doubles.  BGP_PDVAR_CHUNK
// (tests): another size, rounded up to 128.
static size_t pdvar_cell_chunk(int npad) {
  size_t mc = (((size_t)1 << 25) / (size_t)npad) / 128 * 128;
  if (const char* e = bgp_switch(BGP_SW_PDVAR_CHUNK)) {
    const long v = atol(e);
    if (v > 0) mc = ((size_t)v + 127) / 128 * 128;
  }
  return std::min<size_t>(std::max<size_t>(mc, 128), (size_t)1 << 20);  // (the groups of a chunk are bounded by the planner)
}

struct PdvarPanel {
  int ka, kb, Gb, cells;
  long long off;  // of the panel's block in mean / var
  long long coff;  // of its block in cov (curves)
};
struct PdvarChunk {
  long long cell0 = 0;
  int rows = 0;
  std::vector<int> grp;                     // panel, first cell, cells, first row
  std::vector<std::pair<int, int>> curves;  // (panel, first row) of the curves whose covariance this chunk serves
};
// The chunks in output order, one at a time: a panel is cut wherever the chunk is full (of rows, or of PV_GRPMAX cell groups), but a
// curve with `cov` never is (a chunk that holds nothing else takes it whole, whatever the chunk size: at most 256 rows).
struct PdvarPlanner {
  const std::vector<PdvarPanel>& pans;
  int cap;
  bool cov;
  size_t p = 0;
  int c = 0;
  long long cell = 0;
  bool next(PdvarChunk& ch) {
    ch = PdvarChunk();
    ch.cell0 = cell;
    while (p < pans.size()) {
      const PdvarPanel& pn = pans[p];
      const bool whole = cov && pn.ka < 0;
      if (ch.rows >= cap || (whole && ch.rows > 0 && ch.rows + pn.cells > cap)) break;
      const int take = whole ? pn.cells : std::min(pn.cells - c, cap - ch.rows);
      // (many short panels: a chunk also ends where its groups would pass the build's grid; a first take has at most 2^16 + 1)
      if (ch.rows > 0 && ch.grp.size() / 4 + (size_t)take / PV_CW + 1 > PV_GRPMAX) break;
      if (whole) ch.curves.push_back({(int)p, ch.rows});
      for (int o = 0; o < take; o += PV_CW) ch.grp.insert(ch.grp.end(), {(int)p, c + o, std::min(PV_CW, take - o), ch.rows + o});
      ch.rows += take, cell += take, c += take;
      if (c >= pn.cells) p++, c = 0;
    }
    return ch.rows > 0;
  }
};

static int pdvar_run(bgp_ctx* c, int B, const double* h_kernel, int ns, const double* Xs, int gmax, const double* grid,
                     const std::vector<PdvarPanel>& pans, long long total, long long covtotal, double* mean, double* var, double* cov) {
  const int n = c->n, d = c->d, npad = c->npad, P = (int)pans.size();
  const size_t p = d + 2;
  const bool wantP = var || cov;
  const int cap = (int)std::min<size_t>(pdvar_cell_chunk(npad), (size_t)((total + 127) / 128 * 128));
  const int capA = std::max(cap, cov ? PV_GMAX : 0);  // (a curve with cov alone in a smaller chunk)
  const size_t sR = (size_t)capA * npad;              // a posterior's Kbar (and Pm) of one chunk
  // posteriors per chunk: Kbar and Pm of a chunk within 2^29 doubles together
  // (BGP_ITEM_CHUNK, tests: forced posterior chunks against the default)
  const int Bc = (int)bgp_switch_cap(BGP_SW_ITEM_CHUNK, std::max<size_t>(1, std::min<size_t>((size_t)B, ((size_t)1 << 28) / sR)));
  const int Np = (int)((long long)ns * (ns + 1) / 2), nchunkP = (Np + 64 * PV_PW - 1) / (64 * PV_PW);
  int Gm = 0;
  if (cov)
    for (const PdvarPanel& pn : pans)
      if (pn.ka < 0) Gm = std::max(Gm, pn.Gb);
  const int nTm = Gm * (Gm - 1) / 2;
  // units (panels of the variance's prior, cell pairs of a curve) per launch of the prior: the partials within PV_PARTMAX doubles
  const int ub = (int)std::max<size_t>(1, std::min<size_t>(65535, PV_PARTMAX / ((size_t)Bc * nchunkP)));
  const size_t maxgrp = std::min<size_t>((size_t)capA / PV_CW + std::min<size_t>((size_t)P + 1, (size_t)capA) + 1, PV_GRPMAX);
  double *dXs, *dG, *dH, *dUs, *dus, *dgs, *dK, *dP = nullptr, *dq = nullptr, *dmean = nullptr, *dvar = nullptr, *dprior = nullptr,
         *dpart = nullptr, *dqc = nullptr, *dpriorT = nullptr, *dcov = nullptr;
  int *dpan, *dgrp;
  BgpScratch live(c);
  BGP_TRY(live.carve([&](BgpCarve& s) {
    dXs = s.take<double>((size_t)ns * d);
    dG = s.take<double>((size_t)gmax * d);
    dH = s.take<double>((size_t)B * p);
    dUs = s.take<double>((size_t)B * n * d);
    dus = s.take<double>((size_t)B * ns * d);
    dgs = s.take<double>((size_t)B * gmax * d);
    dpan = s.take<int>((size_t)P * 4);
    dgrp = s.take<int>(maxgrp * 4);
    dK = s.take<double>((size_t)Bc * sR);
    if (mean) dmean = s.take<double>((size_t)Bc * capA);
    if (wantP) {
      dP = s.take<double>((size_t)Bc * sR);
      dq = s.take<double>((size_t)Bc * capA);
      dvar = s.take<double>((size_t)Bc * capA);
      dprior = s.take<double>((size_t)Bc * P);
      dpart = s.take<double>((size_t)Bc * nchunkP * std::min(ub, std::max(P, std::max(nTm, 1))));
    }
    if (cov && nTm > 0) {
      dqc = s.take<double>((size_t)Bc * nTm);
      dpriorT = s.take<double>((size_t)Bc * nTm);
    }
    if (cov) dcov = s.take<double>((size_t)Bc * std::max(Gm * Gm, 1));
  }));
  hipStream_t st = c->stream;
  const auto blocks = [](size_t items) { return (unsigned)((items + 255) / 256); };
  const double S2 = (double)ns * (double)ns;
  std::vector<int> hpan((size_t)P * 4);
  for (int i = 0; i < P; i++) hpan[4 * i] = pans[i].ka, hpan[4 * i + 1] = pans[i].kb, hpan[4 * i + 2] = pans[i].Gb, hpan[4 * i + 3] = 0;
  // samples and grid rows the way predict's queries go up: through the context-level warp when one is set
  BGP_TRY(post_stage_queries(c, dXs, Xs, ns));
  BGP_TRY(post_stage_queries(c, dG, grid, gmax));
  BGP_HIP(bgp_memcpy_async(dH, h_kernel, (size_t)B * p * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(dpan, hpan.data(), hpan.size() * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(pdep_scale_kernel, dim3(blocks((size_t)n * d), B), dim3(256), 0, st, c->dXeff, n, d, dH, dUs);
  hipLaunchKernelGGL(pdep_scale_kernel, dim3(blocks((size_t)ns * d), B), dim3(256), 0, st, dXs, ns, d, dH, dus);
  hipLaunchKernelGGL(pdep_scale_kernel, dim3(blocks((size_t)gmax * d), B), dim3(256), 0, st, dG, gmax, d, dH, dgs);
  BGP_HIP(hipGetLastError());
  c->chunk_last[0] = c->chunk_last[1] = 0;
  for (int b0 = 0; b0 < B; b0 += Bc) {
    const int nb = std::min(Bc, B - b0);
    const double *dHb = dH + (size_t)b0 * p, *dusb = dus + (size_t)b0 * ns * d, *dgsb = dgs + (size_t)b0 * gmax * d;
    c->chunk_last[0]++;
    // the prior of pd's variance: the pair sum of stage 4 with T = 0 for `nu` panels per launch
    if (wantP)
      for (int p0 = 0; p0 < P; p0 += ub) {
        const int nu = std::min(ub, P - p0);
        KB_DISPATCH(c->ks.stationary, c->ks.form,
                    hipLaunchKernelGGL((pdvar_prior_kernel<S, F>), dim3((nchunkP + 3) / 4, nu, nb), dim3(256), 0, st, dusb, dgsb, dHb,
                                       dpan, ns, d, gmax, Np, nchunkP, p0, 0, 0, 1, dpart));
        hipLaunchKernelGGL(pdvar_prior_reduce_kernel, dim3(blocks(nu), nb), dim3(256), 0, st, dpart, nchunkP, nu, dprior, (size_t)P, p0);
      }
    PdvarPlanner plan{pans, cap, cov != nullptr};
    PdvarChunk ch;
    while (plan.next(ch)) {
      if (b0 == 0) c->chunk_last[1]++;
      const int rows = ch.rows, rpad = (rows + 127) / 128 * 128, ngrp = (int)(ch.grp.size() / 4);
      BGP_HIP(bgp_memcpy_async(dgrp, ch.grp.data(), ch.grp.size() * sizeof(int), hipMemcpyHostToDevice, st));
      KB_DISPATCH(c->ks.stationary, c->ks.form,
                  hipLaunchKernelGGL((pdvar_kbar_kernel<S, F>), dim3(npad / PV_TJ, (ngrp + 3) / 4, nb), dim3(256), 0, st,
                                     dUs + (size_t)b0 * n * d, dusb, dgsb, dHb, dpan, dgrp, ngrp, n, npad, d, ns, gmax, sR, dK));
      if (wantP) {
        if (rpad > rows)
          hipLaunchKernelGGL(pdvar_zero_rows_kernel, dim3(blocks((size_t)(rpad - rows) * npad), nb), dim3(256), 0, st, dK, sR, rows,
                             rpad, npad);
        bgp_launch_gemm4(st, 0, dK, c->dKinv + (size_t)b0 * npad * npad, npad, rpad, npad, npad, dP, npad, nb, sR,
                         (size_t)npad * npad, sR, nullptr);
      }
      hipLaunchKernelGGL(pdvar_contract_kernel, dim3((rows + 3) / 4, nb), dim3(256), 0, st, dK, dP, sR,
                         c->dalpha_sol + (size_t)b0 * npad, n, npad, ns, 0, rows, 0, dq, (size_t)capA, dmean);
      if (wantP)
        hipLaunchKernelGGL(pdvar_finish_kernel, dim3((ngrp + 15) / 16, nb), dim3(256), 0, st, dgrp, ngrp, dprior, (size_t)P, dq,
                           (size_t)capA, S2, dvar);
      BGP_HIP(hipGetLastError());
      const size_t wr = (size_t)rows * sizeof(double), sp = (size_t)capA * sizeof(double), dp = (size_t)total * sizeof(double);
      if (mean) BGP_HIP(bgp_memcpy2d_async(mean + (size_t)b0 * total + ch.cell0, dp, dmean, sp, wr, nb, hipMemcpyDeviceToHost, st));
      if (var) BGP_HIP(bgp_memcpy2d_async(var + (size_t)b0 * total + ch.cell0, dp, dvar, sp, wr, nb, hipMemcpyDeviceToHost, st));
      for (const auto& cv : ch.curves) {  // (only with cov)
        const PdvarPanel& pn = pans[cv.first];
        const int G = pn.Gb, nT = G * (G - 1) / 2;
        if (nT > 0) {
          hipLaunchKernelGGL(pdvar_contract_kernel, dim3((nT + 3) / 4, nb), dim3(256), 0, st, dK, dP, sR,
                             c->dalpha_sol + (size_t)b0 * npad, n, npad, ns, cv.second, nT, 1, dqc, (size_t)nT, (double*)nullptr);
          for (int t0 = 0; t0 < nT; t0 += ub) {
            const int nu = std::min(ub, nT - t0);
            KB_DISPATCH(c->ks.stationary, c->ks.form,
                        hipLaunchKernelGGL((pdvar_prior_kernel<S, F>), dim3((nchunkP + 3) / 4, (nu + PV_TB - 1) / PV_TB, nb), dim3(256), 0, st,
                                           dusb, dgsb,
                                           dHb, dpan, ns, d, gmax, Np, nchunkP, cv.first, G, t0, nu, dpart));
            hipLaunchKernelGGL(pdvar_prior_reduce_kernel, dim3(blocks(nu), nb), dim3(256), 0, st, dpart, nchunkP, nu, dpriorT,
                               (size_t)nT, t0);
          }
        }
        hipLaunchKernelGGL(pdvar_cov_finish_kernel, dim3(blocks((size_t)G * G), nb), dim3(256), 0, st, dpriorT, dqc, nT, dvar,
                           (size_t)capA, cv.second, G, S2, dcov);
        BGP_HIP(hipGetLastError());
        const size_t wc = (size_t)G * G * sizeof(double);
        BGP_HIP(bgp_memcpy2d_async(cov + (size_t)b0 * covtotal + pn.coff, (size_t)covtotal * sizeof(double), dcov, wc, wc, nb,
                                   hipMemcpyDeviceToHost, st));
        // (the next curve reuses dqc, dpriorT and dcov behind this download, in stream order)
      }
      BGP_HIP(bgp_stream_sync(st));  // (the next chunk reuses the buffers)
    }
  }
  return BGP_OK;
}

extern "C" int bgp_partial_dependence_var(bgp_ctx* c, int B, const double* h_kernel, int S, const double* Xs, int gmax, const int* ng,
                                          const double* grid, int P, const int* panels, double* mean, double* var, double* cov) {
  const char* who = "bgp_partial_dependence_var";
  BGP_TRY(bgp_guard(c, who, BGP_POST_PLAIN));
  if (!h_kernel || !Xs || !ng || !grid || !panels || (!mean && !var && !cov) || B <= 0 || B > 65535 || S <= 0 || P <= 0 || gmax <= 0 ||
      gmax > PV_GMAX) {
    bgp_set_error("%s: bad argument (1 <= B <= 65535, S, P >= 1, 1 <= gmax <= %d, at least one output)", who, PV_GMAX);
    return BGP_ERR_INVALID;
  }
  const int d = c->d;
  if (d > PV_DMAX) {
    bgp_set_error("%s: d > %d is not supported", who, PV_DMAX);
    return BGP_ERR_INVALID;
  }
  if (S > PV_SMAX) {
    bgp_set_error("%s: S = %d exceeds %d samples (the prior is a pair sum)", who, S, PV_SMAX);
    return BGP_ERR_INVALID;
  }
  for (int k = 0; k < d; k++)
    if (ng[k] < 1 || ng[k] > gmax) {
      bgp_set_error("%s: ng[%d] = %d outside 1 .. gmax = %d", who, k, ng[k], gmax);
      return BGP_ERR_INVALID;
    }
  std::vector<PdvarPanel> pans;
  long long total = 0, covtotal = 0;
  const long long Np = (long long)S * (S + 1) / 2;
  for (int p = 0; p < P; p++) {
    const int k1 = panels[2 * p], k2 = panels[2 * p + 1];
    if (k1 < 0 || k1 >= d || k2 < -1 || k2 >= d || k1 == k2) {
      bgp_set_error("%s: panel %d = (%d, %d) is not (k, -1) or (k1, k2), k1 != k2, inside [0, %d)", who, p, k1, k2, d);
      return BGP_ERR_INVALID;
    }
    const int ka = k2 < 0 ? -1 : k1, kb = k2 < 0 ? k1 : k2, Ga = ka < 0 ? 1 : ng[ka], Gb = ng[kb];
    if (cov && ka < 0 && (long long)Gb * (Gb + 1) / 2 * Np > (1ll << 38)) {
      bgp_set_error("%s: panel %d: ng (ng + 1) / 2 * S (S + 1) / 2 exceeds 2^38 with cov", who, p);
      return BGP_ERR_INVALID;
    }
    pans.push_back({ka, kb, Gb, Ga * Gb, total, covtotal});
    total += (long long)Ga * Gb;
    if (ka < 0) covtotal += (long long)Gb * Gb;
    if (total > (1ll << 30)) {
      bgp_set_error("%s: more than 2^30 grid cells in one call", who);
      return BGP_ERR_INVALID;
    }
  }
  BGP_TRY(bgp_guard(c, who, BGP_POST_PLAIN, B));
  return post_call(c, [&] { return pdvar_run(c, B, h_kernel, S, Xs, gmax, grid, pans, total, covtotal, mean, var, cov); });
}
