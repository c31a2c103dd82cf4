// Generic kernel expression trees evaluated on the device.  The host compiles a scikit-learn kernel tree
// once into a postfix program (kernels.compile_tree; the format: bgp_tree.h) and sends a (B, P) block of log-space parameters per
// call; tree_tile_kernel evaluates the tree for every pair of points of a 64 x 64 tile, and the factorisation, the solves, the
// inverse and the predictive products run behind it as they do behind the canonical Gram build.  Trees the compiler does not cover
// (Matern with a general nu, ...) keep the host path of bgp_gram.hip.
#include "bgp_tree.h"
#include "bgp_device.h"

#define TREE_TILE 64
#define TREE_LD 65  // LDS leading dimension of a staged operand (odd: the staging writes of one row do not meet on a bank)

// ---- the interpreter ----
// One program step for NP pairs at once.  The value stack lives in registers and is indexed statically: its top is always s[0],
// a push moves the entries down, a binary op moves them up.  Every branch depends on the program alone, so all lanes of all waves
// take it together.  No implicit contraction: the tile kernel and the diagonal kernel must produce the same bits.
template <int NP>
static __device__ __forceinline__ double tree_pick(int a, const double (&met)[BGP_TREE_MAXMET][NP], int q) {
  // (all four read first, then selected by value: a conditional read becomes a register array indexed through scratch)
  const double v0 = met[0][q], v1 = met[1][q], v2 = met[2][q], v3 = met[3][q];
  double v = v0;
  v = (a == 1) ? v1 : v;
  v = (a == 2) ? v2 : v;
  v = (a == 3) ? v3 : v;
  return v;
}

template <int NP>
static __device__ __forceinline__ void tree_walk(const BgpTreeProg& pg, const double* __restrict__ pe,
                                                 const double (&met)[BGP_TREE_MAXMET][NP], const bool (&ondiag)[NP],
                                                 double (&res)[NP]) {
#pragma clang fp contract(off)
  double s[BGP_TREE_STACK][NP];
#pragma unroll
  for (int l = 0; l < BGP_TREE_STACK; l++)
#pragma unroll
    for (int q = 0; q < NP; q++) s[l][q] = 0.0;
  for (int it = 0; it < pg.n_ins; it++) {
    const int code = pg.ins[it][0], a = pg.ins[it][1], b = pg.ins[it][2], c = pg.ins[it][3];
    if (code == BGP_TO_ADD || code == BGP_TO_MUL) {
#pragma unroll
      for (int q = 0; q < NP; q++) s[0][q] = (code == BGP_TO_ADD) ? s[1][q] + s[0][q] : s[1][q] * s[0][q];
#pragma unroll
      for (int l = 1; l < BGP_TREE_STACK - 1; l++)
#pragma unroll
        for (int q = 0; q < NP; q++) s[l][q] = s[l + 1][q];
      continue;
    }
    if (code == BGP_TO_POW) {
      const double e = pg.imm[a];
#pragma unroll
      for (int q = 0; q < NP; q++) s[0][q] = pow(s[0][q], e);
      continue;
    }
    // a leaf: its value for every pair, then the push
    double v[NP];
    switch (code) {
      case BGP_TO_CONST: {
        const double cst = pe[a];
#pragma unroll
        for (int q = 0; q < NP; q++) v[q] = cst;
      } break;
      case BGP_TO_WHITE: {
        const double lvl = pe[a];
#pragma unroll
        for (int q = 0; q < NP; q++) v[q] = ondiag[q] ? lvl : 0.0;
      } break;
      case BGP_TO_RBF:
#pragma unroll
        for (int q = 0; q < NP; q++) v[q] = kb_stationary<BGP_RBF>(tree_pick<NP>(a, met, q));
        break;
      case BGP_TO_M12:
#pragma unroll
        for (int q = 0; q < NP; q++) v[q] = kb_stationary<BGP_MATERN12>(tree_pick<NP>(a, met, q));
        break;
      case BGP_TO_M32:
#pragma unroll
        for (int q = 0; q < NP; q++) v[q] = kb_stationary<BGP_MATERN32>(tree_pick<NP>(a, met, q));
        break;
      case BGP_TO_M52:
#pragma unroll
        for (int q = 0; q < NP; q++) v[q] = kb_stationary<BGP_MATERN52>(tree_pick<NP>(a, met, q));
        break;
      case BGP_TO_RQ: {
        // (1 + r^2 / (2 alpha l^2))^-alpha (sklearn/kernels.py RationalQuadratic.__call__); the metric carries 1 / l^2
        const double al = pe[b], two_al = 2.0 * al;
#pragma unroll
        for (int q = 0; q < NP; q++) v[q] = pow(1.0 + tree_pick<NP>(a, met, q) / two_al, -al);
      } break;
      case BGP_TO_ESS: {
        // exp(-2 (sin(pi r / p) / l)^2) on the unscaled distance (ExpSineSquared.__call__)
        const double ell = pe[b], per = pe[c];
#pragma unroll
        for (int q = 0; q < NP; q++) {
          const double sn = sin(3.141592653589793 * sqrt(tree_pick<NP>(a, met, q)) / per) / ell;
          v[q] = kb_exp_neg(2.0 * (sn * sn));
        }
      } break;
      default: {  // BGP_TO_DOT: sigma_0^2 + x . y (DotProduct.__call__)
        const double s0 = pe[b], s02 = s0 * s0;
#pragma unroll
        for (int q = 0; q < NP; q++) v[q] = tree_pick<NP>(a, met, q) + s02;
      } break;
    }
#pragma unroll
    for (int l = BGP_TREE_STACK - 1; l > 0; l--)
#pragma unroll
      for (int q = 0; q < NP; q++) s[l][q] = s[l - 1][q];
#pragma unroll
    for (int q = 0; q < NP; q++) s[0][q] = v[q];
  }
#pragma unroll
  for (int q = 0; q < NP; q++) res[q] = s[0][q];
}

// One dimension of NP pairs: x against y[q].  Direct differences, scaled by the inverse length scale, accumulated with fma in the
// caller's ascending dimension order (never |x|^2 + |y|^2 - 2 x.y: the small distances are where Matern and RQ are read).
// (x - y) w and (y - x) w differ in sign alone, and fma(x, y, .) is fma(y, x, .): every metric is bit-symmetric.
template <int NP>
static __device__ __forceinline__ void tree_accum(const BgpTreeProg& pg, const double* __restrict__ w, int k, double x,
                                                  const double (&y)[NP], double (&met)[BGP_TREE_MAXMET][NP]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int m = 0; m < BGP_TREE_MAXMET; m++) {
    if (m >= pg.n_met) continue;  // (uniform; metrics the program does not have stay 0 and are never picked)
    if (pg.met[m][0] == BGP_TM_DOT) {
#pragma unroll
      for (int q = 0; q < NP; q++) met[m][q] = __builtin_fma(x, y[q], met[m][q]);
    } else {
      const double wk = w[m * BGP_TREE_MAXD + k];
#pragma unroll
      for (int q = 0; q < NP; q++) {
        const double t = (x - y[q]) * wk;
        met[m][q] = __builtin_fma(t, t, met[m][q]);
      }
    }
  }
}

// The item's parameter row, exponentiated once: pe[s] = exp(p_s) (levels, constants, alpha, periodicity, sigma_0; exp(-inf) = 0)
// and w[m][k] = exp(-p) = 1 / l of metric m in dimension k (1 for the unscaled metrics).  The caller synchronises.
static __device__ __forceinline__ void tree_fill_params(const BgpTreeProg& pg, const double* __restrict__ prow, int d,
                                                        double* __restrict__ pe, double* __restrict__ w, int tid) {
  if (tid < pg.P) pe[tid] = exp(prow[tid]);
  if (tid < BGP_TREE_MAXMET * BGP_TREE_MAXD) {
    const int m = tid / BGP_TREE_MAXD, k = tid - m * BGP_TREE_MAXD;
    double v = 1.0;
    if (m < pg.n_met && k < d) {
      const int kind = pg.met[m][0], slot = pg.met[m][1];
      if (kind == BGP_TM_ISO) v = exp(-prow[slot]);
      if (kind == BGP_TM_ARD) v = exp(-prow[slot + k]);
    }
    w[tid] = v;
  }
}

// ---- the tile kernel ----
// A workgroup of 256 threads owns one 64 x 64 tile of one item; thread (tx, ty) of a 16 x 16 grid owns the 4 x 4 block of rows
// ty + 16 r and columns tx + 16 c.  The 64 rows of each operand are staged in LDS dimension-major (xs[k][row]): the row reads of a
// wave are four broadcast addresses, the column reads sixteen consecutive doubles -- no bank conflict.  The block is walked one row
// of four pairs at a time (metrics and value stack of four pairs: 8 + 64 VGPRs; all sixteen at once would hold 4 * 32 + 8 * 32).
// Self mode: only tiles with tj <= ti are launched; an off-diagonal tile is stored a second time, transposed through LDS so that
// the mirrored store is as coalesced as the direct one.  The mirror is exactly symmetric with the tile, and a diagonal tile is
// exactly symmetric in itself because every metric is (tree_accum).  Nothing here depends on the grid or on the other items.
__global__ void __launch_bounds__(256) tree_tile_kernel(BgpTreeProg pg, const double* __restrict__ params, int d,
                                                        const double* __restrict__ A, size_t sA, int na,
                                                        const double* __restrict__ Bm, size_t sB, int nbm, int self,
                                                        double* __restrict__ out, int ldo, size_t sO, int out_rows, int out_cols,
                                                        int tiles_j) {
  __shared__ double buf[2 * BGP_TREE_MAXD * TREE_LD];  // xs | ys, later the transposed tile (64 x 65)
  __shared__ double pe[BGP_TREE_MAXP];
  __shared__ double w[BGP_TREE_MAXMET * BGP_TREE_MAXD];
  double* xs = buf;
  double* ys = buf + BGP_TREE_MAXD * TREE_LD;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int b = blockIdx.y;
  int ti, tj;
  if (self) {
    bgp_tri_decode(blockIdx.x, ti, tj);
  } else {
    ti = blockIdx.x / tiles_j;
    tj = blockIdx.x - ti * tiles_j;
  }
  const int i0 = ti * TREE_TILE, j0 = tj * TREE_TILE;
  const double* Ab = A + (size_t)b * sA;
  const double* Bb = Bm + (size_t)b * sB;
  double* ob = out + (size_t)b * sO;
  tree_fill_params(pg, params + (size_t)b * pg.P, d, pe, w, tid);
  for (int idx = tid; idx < d * TREE_TILE; idx += 256) {
    const int row = idx / d, k = idx - row * d;
    const int gi = i0 + row, gj = j0 + row;
    xs[k * TREE_LD + row] = (gi < na) ? Ab[(size_t)gi * d + k] : 0.0;
    ys[k * TREE_LD + row] = (gj < nbm) ? Bb[(size_t)gj * d + k] : 0.0;
  }
  __syncthreads();
  double val[4][4];
  for (int r = 0; r < 4; r++) {
    double met[BGP_TREE_MAXMET][4];
#pragma unroll
    for (int m = 0; m < BGP_TREE_MAXMET; m++)
#pragma unroll
      for (int q = 0; q < 4; q++) met[m][q] = 0.0;
    for (int k = 0; k < d; k++) {
      const double x = xs[k * TREE_LD + ty + 16 * r];
      double y[4];
#pragma unroll
      for (int q = 0; q < 4; q++) y[q] = ys[k * TREE_LD + tx + 16 * q];
      tree_accum<4>(pg, w, k, x, y, met);
    }
    bool ondiag[4];
#pragma unroll
    for (int q = 0; q < 4; q++) ondiag[q] = self && (i0 + ty + 16 * r == j0 + tx + 16 * q);
    double res[4];
    tree_walk<4>(pg, pe, met, ondiag, res);
    // (r is a loop counter, not a constant: the row goes to its registers through selects, never through scratch)
#pragma unroll
    for (int rr = 0; rr < 4; rr++)
#pragma unroll
      for (int q = 0; q < 4; q++)
        if (rr == r) val[rr][q] = res[q];
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int gi = i0 + ty + 16 * r;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int gj = j0 + tx + 16 * q;
      const bool inside = gi < na && gj < nbm;
      if (self) {
        if (inside) ob[(size_t)gi * ldo + gj] = val[r][q];
      } else if (gi < out_rows && gj < out_cols) {
        ob[(size_t)gi * ldo + gj] = inside ? val[r][q] : 0.0;
      }
    }
  }
  if (!self || ti == tj) return;  // (uniform over the workgroup)
  __syncthreads();                // every thread is through with xs / ys
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int q = 0; q < 4; q++) buf[(tx + 16 * q) * TREE_LD + ty + 16 * r] = val[r][q];
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int gj = j0 + ty + 16 * r;  // row of the mirrored tile
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int gi = i0 + tx + 16 * q;
      if (gi < na && gj < nbm) ob[(size_t)gj * ldo + gi] = buf[(ty + 16 * r) * TREE_LD + tx + 16 * q];
    }
  }
}

// K_b(x_i, x_i) as the self mode of the tile kernel forms it: the same accumulation (every difference is 0, the inner product is
// the row's own) and the same walk, one thread per row.
__global__ void __launch_bounds__(256) tree_diag_kernel(BgpTreeProg pg, const double* __restrict__ params, int d,
                                                        const double* __restrict__ A, size_t sA, int na, double* __restrict__ out,
                                                        size_t sO) {
  __shared__ double pe[BGP_TREE_MAXP];
  __shared__ double w[BGP_TREE_MAXMET * BGP_TREE_MAXD];
  const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  tree_fill_params(pg, params + (size_t)b * pg.P, d, pe, w, threadIdx.x);
  __syncthreads();
  if (i >= na) return;
  const double* xi = A + (size_t)b * sA + (size_t)i * d;
  double met[BGP_TREE_MAXMET][1];
#pragma unroll
  for (int m = 0; m < BGP_TREE_MAXMET; m++) met[m][0] = 0.0;
  for (int k = 0; k < d; k++) {
    const double x = xi[k];
    const double y[1] = {x};
    tree_accum<1>(pg, w, k, x, y, met);
  }
  const bool ondiag[1] = {true};
  double res[1];
  tree_walk<1>(pg, pe, met, ondiag, res);
  out[(size_t)b * sO + i] = res[0];
}

// ---- host side ----
int bgp_tree_check(const char* who, int d, int n_ops, const int* ops, int n_imm, const double* imm, int P, BgpTreeProg* out) {
  auto bad = [&](const char* why) {
    bgp_set_error("%s: kernel program refused: %s", who, why);
    return BGP_ERR_INVALID;
  };
  if (!ops || n_ops < 2 || n_imm < 0 || (n_imm > 0 && !imm)) return bad("no program");
  if (d < 1 || d > BGP_TREE_MAXD) return bad("more than 32 dimensions");
  if (P < 1 || P > BGP_TREE_MAXP) return bad("parameter count outside [1, 256]");
  if (n_imm > BGP_TREE_MAXIMM) return bad("too many immediates");
  const int n_met = ops[0], n_ins = ops[1];
  if (n_met < 0 || n_met > BGP_TREE_MAXMET) return bad("more than 4 metrics");
  if (n_ins < 1 || n_ins > BGP_TREE_MAXINS) return bad("instruction count outside [1, 32]");
  if (n_ops != 2 + 2 * n_met + 4 * n_ins) return bad("the op array's length does not match its header");
  BgpTreeProg pg = {};
  pg.n_met = n_met, pg.n_ins = n_ins, pg.P = P, pg.n_imm = n_imm;
  for (int k = 0; k < n_imm; k++) pg.imm[k] = imm[k];
  const int* q = ops + 2;
  for (int m = 0; m < n_met; m++, q += 2) {
    const int kind = q[0], slot = q[1];
    if (kind < BGP_TM_ISO || kind > BGP_TM_DOT) return bad("unknown metric kind");
    const int width = kind == BGP_TM_ISO ? 1 : kind == BGP_TM_ARD ? d : 0;
    if (width && (slot < 0 || slot + width > P)) return bad("a metric's slots pass P");
    pg.met[m][0] = kind, pg.met[m][1] = width ? slot : 0;
  }
  auto slot_ok = [&](int s) { return s >= 0 && s < P; };
  auto met_is = [&](int m, bool scaled, int kind) {
    if (m < 0 || m >= n_met) return false;
    return scaled ? (pg.met[m][0] == BGP_TM_ISO || pg.met[m][0] == BGP_TM_ARD) : pg.met[m][0] == kind;
  };
  int depth = 0;
  for (int it = 0; it < n_ins; it++, q += 4) {
    const int code = q[0], a = q[1], b = q[2], c = q[3];
    switch (code) {
      case BGP_TO_CONST:
      case BGP_TO_WHITE:
        if (!slot_ok(a)) return bad("a slot index passes P");
        break;
      case BGP_TO_RBF:
      case BGP_TO_M12:
      case BGP_TO_M32:
      case BGP_TO_M52:
        if (!met_is(a, true, 0)) return bad("a stationary leaf without a scaled metric");
        break;
      case BGP_TO_RQ:
        if (!met_is(a, true, 0)) return bad("a stationary leaf without a scaled metric");
        if (!slot_ok(b)) return bad("a slot index passes P");
        break;
      case BGP_TO_ESS:
        if (!met_is(a, false, BGP_TM_EUCL)) return bad("ExpSineSquared without the Euclidean metric");
        if (!slot_ok(b) || !slot_ok(c)) return bad("a slot index passes P");
        break;
      case BGP_TO_DOT:
        if (!met_is(a, false, BGP_TM_DOT)) return bad("DotProduct without the inner-product metric");
        if (!slot_ok(b)) return bad("a slot index passes P");
        break;
      case BGP_TO_ADD:
      case BGP_TO_MUL:
        if (depth < 2) return bad("the stack underflows");
        depth -= 2;
        break;
      case BGP_TO_POW:
        if (depth < 1) return bad("the stack underflows");
        if (a < 0 || a >= n_imm) return bad("an immediate index passes n_imm");
        depth -= 1;
        break;
      default:
        return bad("unknown op");
    }
    if (++depth > BGP_TREE_STACK) return bad("the stack is deeper than 8");
    pg.ins[it][0] = code, pg.ins[it][1] = a, pg.ins[it][2] = b, pg.ins[it][3] = c;
  }
  if (depth != 1) return bad("the program does not leave one value");
  *out = pg;
  return BGP_OK;
}

int bgp_launch_tree(hipStream_t st, const BgpTreeProg& prog, int nb, const double* dparams, int d, const double* A, size_t sA, int na,
                    const double* Bm, size_t sB, int nbm, int self, double* out, int ldo, size_t sO, int out_rows, int out_cols) {
  const int ntr = (self ? na : out_rows) + TREE_TILE - 1, nti = ntr / TREE_TILE, ntj = (out_cols + TREE_TILE - 1) / TREE_TILE;
  const int tiles = self ? nti * (nti + 1) / 2 : nti * ntj;
  hipLaunchKernelGGL(tree_tile_kernel, dim3(tiles, nb), dim3(256), 0, st, prog, dparams, d, A, sA, na, Bm, sB, nbm, self, out, ldo, sO,
                     out_rows, out_cols, ntj);
  BGP_HIP(hipGetLastError());
  return BGP_OK;
}

int bgp_launch_tree_diag(hipStream_t st, const BgpTreeProg& prog, int nb, const double* dparams, int d, const double* A, size_t sA,
                         int na, double* out, size_t sO) {
  hipLaunchKernelGGL(tree_diag_kernel, dim3((na + 255) / 256, nb), dim3(256), 0, st, prog, dparams, d, A, sA, na, out, sO);
  BGP_HIP(hipGetLastError());
  return BGP_OK;
}

// The matrices themselves: B n x n (Xq == NULL: kernel_(X_train), WhiteKernel on the diagonal, no alpha) or B m x n (kernel_(Xq,
// X_train)), items in chunks of the scratch budget.  The training inputs are the context's (warped under a context-level warp) and
// the query rows are warped as bgp_predict_batch warps them.
extern "C" int bgp_tree_gram(bgp_ctx* c, int n_ops, const int* ops, int n_imm, const double* imm, int P, int B, const double* params,
                             int m, const double* Xq, double* out) {
  BGP_TRY(bgp_guard(c, "bgp_tree_gram"));
  if (!params || !out || B <= 0 || (Xq && m <= 0)) {
    bgp_set_error("bgp_tree_gram: bad argument");
    return BGP_ERR_INVALID;
  }
  BgpTreeProg pg;
  BGP_TRY(bgp_tree_check("bgp_tree_gram", c->d, n_ops, ops, n_imm, imm, P, &pg));
  return post_call(c, [&]() -> int {
    const int n = c->n, d = c->d, rows = Xq ? m : n;
    const size_t per = (size_t)rows * n;
    const int chunk = (int)std::max<size_t>(1, std::min<size_t>((size_t)B, ((size_t)1 << 28) / per));
    double *dP, *dXq = nullptr, *dOut;
    BgpScratch live(c);
    BGP_TRY(live.carve([&](BgpCarve& s) {
      dP = s.take<double>((size_t)B * P);
      if (Xq) dXq = s.take<double>((size_t)m * d);
      dOut = s.take<double>((size_t)chunk * per);
    }));
    BGP_HIP(bgp_memcpy_async(dP, params, (size_t)B * P * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (Xq) BGP_TRY(post_stage_queries(c, dXq, Xq, m));
    for (int off = 0; off < B; off += chunk) {
      const int nb = std::min(chunk, B - off);
      BGP_TRY(bgp_launch_tree(c->stream, pg, nb, dP + (size_t)off * P, d, Xq ? dXq : c->dXeff, 0, rows, c->dXeff, 0, n, Xq ? 0 : 1, dOut, n,
                              per, rows, n));
      BGP_HIP(bgp_memcpy_async(out + (size_t)off * per, dOut, (size_t)nb * per * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      BGP_HIP(bgp_stream_sync(c->stream));  // (the next chunk writes the same scratch)
    }
    return BGP_OK;
  });
}

// bgp_lml_batch_gram with the matrices built straight into the working matrices: no host kernel evaluation, no B n^2 upload.
// warp (B x 2d, log space, as bgp_lml_batch_warped lays it out): item b is built from its own Beta-CDF warp of the un-warped
// training inputs, which replaces a context-level warp for this call.
extern "C" int bgp_lml_batch_tree(bgp_ctx* c, int n_ops, const int* ops, int n_imm, const double* imm, int P, int B,
                                  const double* params, const double* warp, int use_alpha, double* lml, int* status) {
  BGP_TRY(bgp_guard(c, "bgp_lml_batch_tree"));
  if (!params || !lml || B <= 0) {
    bgp_set_error("bgp_lml_batch_tree: bad argument");
    return BGP_ERR_INVALID;
  }
  BgpTreeProg pg;
  BGP_TRY(bgp_tree_check("bgp_lml_batch_tree", c->d, n_ops, ops, n_imm, imm, P, &pg));
  return post_call(c, [&]() -> int {
    const int n = c->n, d = c->d, npad = c->npad;
    const size_t nd = (size_t)n * d, w2 = 2 * (size_t)d, ld = (size_t)npad;
    if (warp) BGP_TRY(bgp_ensure_warp_buffers(c));
    BGP_TRY(c->dtreep.ensure((size_t)B * P));
    BGP_HIP(bgp_memcpy_async(c->dtreep, params, (size_t)B * P * sizeof(double), hipMemcpyHostToDevice, c->stream));
    for (int off = 0; off < B; off += c->max_batch) {
      const int nb = std::min(c->max_batch, B - off);
      BGP_HIP(hipMemsetAsync(c->dstatus, 0, nb * sizeof(int), c->stream));
      if (warp) {
        BGP_HIP(bgp_memcpy_async(c->dwarpB, warp + (size_t)off * w2, (size_t)nb * w2 * sizeof(double), hipMemcpyHostToDevice, c->stream));
        BGP_TRY(bgp_launch_warp(c, c->stream, c->dX, c->dwarpB, c->dXwB, n, nb, nd));
      }
      const double* X = warp ? (const double*)c->dXwB : (const double*)c->dXeff;
      const size_t xs = warp ? nd : 0;
      BGP_TRY(bgp_launch_tree(c->stream, pg, nb, c->dtreep + (size_t)off * P, d, X, xs, n, X, xs, n, 1, c->dK, (int)ld, ld * ld, n, n));
      BGP_TRY(bgp_gram_fixup(c, nb, 0, use_alpha));
      BGP_TRY(bgp_launch_cholesky(c, nb, 0));
      BGP_HIP(bgp_memcpy_async(lml + off, c->dlml, nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
      if (status) BGP_HIP(bgp_memcpy_async(status + off, c->dstatus, nb * sizeof(int), hipMemcpyDeviceToHost, c->stream));
      BGP_HIP(bgp_stream_sync(c->stream));
    }
    return BGP_OK;
  });
}
