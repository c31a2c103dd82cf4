// Hessian of the log marginal likelihood with respect to the canonical vector.
//
// h = [log c, log l_1 .. l_d, log s2], p = d + 2; alpha = K^-1 y, W = alpha alpha^T - K^-1, D_k = dK / dh_k, D_kl = d2K / dh_k dh_l:
//   H_kl = 1/2 tr(W D_kl) - (D_k alpha)^T K^-1 (D_l alpha) + 1/2 tr(K^-1 D_k K^-1 D_l)
// Length scales, u_k = (x_ik - x_jk)^2 / l_k^2, fr = -2 dS / dr^2 as lml_grad_kernel has it, fr2 = -2 dfr / dr^2, cf = c (product
// form) or 1 (sum form):
//   D_k = cf fr u_k            D_kl = cf (fr2 u_k u_l - 2 delta_kl fr u_k)
//   fr2:  RBF exp(-r^2 / 2);  Matern 1/2 e^-r (1 + r) / r^3;  Matern 3/2 9 e^-t / t, t = sqrt3 r;  Matern 5/2 (25 / 3) e^-t, t = sqrt5 r
//   (Matern 1/2 and 3/2: singular at r = 0 where u_k u_l = 0; coincident points contribute exactly 0, as the gradient's rr > 0 guard)
// Constant and noise (never through the product):
//   D_n = s2 I = D_nn, D_n. = 0 otherwise;  D_0 = D_00 = c S (product; diagonal c) or c 1 1^T (sum);  D_0k = D_k (product) or 0 (sum)
//   P_n = D_n K^-1 = s2 K^-1;  P_0 = D_0 K^-1 = I - diag(s2 + alpha_diag) K^-1 (product: D_0 = K - s2 I - diag(alpha_diag)) or
//   c 1 w^T, w = K^-1 1 (sum)
// so that, with g the gradient (lml_grad_kernel's bits), S1_kl = sum_ij W_ij cf fr2 u_k u_l, P_k = D_k K^-1, T_kl = tr(P_k P_l),
// v_k = D_k alpha, z_l = P_l^T alpha (= K^-1 v_l) and q_kl = v_k . z_l:
//   H_kl = [1/2 S1_kl - 2 delta_kl g_k | g_0 | g_l or 0 | g_n | 0] - q_kl + 1/2 T_kl
// Stages per chunk of matrices, plain launches on the context's stream:
//   1  lmlhess_build_kernel   one workgroup per 64 x 128 tile of the n x n index square: r^2 once, one exp per element; the d
//                             matrices D_k into the stacked (d npad) x npad operand (zero padding written here), the tile's share
//                             of S1_kl for the d (d + 1) / 2 pairs and of v_0 .. v_d for its rows.
//   2  bgp_launch_gemm4       P = D K^-1 for the whole stack on the LDS-DMA ring (fp64 MFMA): 2 d npad^3 flops per matrix.
//   3  lmlhess_pair_kernel    T_kl for all p (p + 1) / 2 pairs: a workgroup owns a 16-row strip of a tile pair (I, J) / (J, I) of the
//                             lower triangle.  A wave owns the columns l = wave, wave + 4, ..; a lane holds its four elements of a
//                             16 x 16 block of P_k[I, J] for ALL k in registers, the wave stages the mirror blocks of its P_l
//                             in LDS (row stride 18: the transposed read of 32 lanes falls on 32 different banks) and reads them
//                             transposed.  The second pass swaps the roles of the two tiles, so k <= l suffices.
//      lmlhess_z_kernel       z_l = P_l^T alpha, a column per thread, ascending rows.
//   4  lmlhess_finish_kernel  a thread per pair: tile partials in ascending order, q_kl ascending, the closed-form first term,
//                             both triangles written from one value.
// No workgroup waits for another; no floating-point atomics; every loop is bounded by an argument.  A matrix's Hessian depends on
// its h alone (not on B, its position in the batch or the chunking).
#include "bgp_common.h"
#include "bgp_device.h"

#define LH_DMAX 16   // input dimensions (a lane's P_k fragments stay in registers)
#define LH_PMAX 18   // LH_DMAX + 2
#define LH_NPAIR 171 // LH_PMAX (LH_PMAX + 1) / 2
#define LH_NL 5      // columns l per wave of the pair kernel: ceil(LH_PMAX / 4)
#define LH_SB 16     // edge of a block of the pair kernel
#define LH_LD 18     // LDS row stride of a staged 16 x 16 block: lane (jj, r) reads word 18 jj + r (+ 4 e); 18 jj mod 32 takes the 16
                     // even values once each, r = 0 / 1 picks even / odd: the 32 lanes of a half wave hit 32 banks

// S, fr = -2 dS / dr^2 and fr2 = -2 dfr / dr^2 from the squared scaled distance (runtime family, libm exp / sqrt as lml_grad_kernel)
static __device__ __forceinline__ void lh_facs(int stat, double r2, double& S, double& fr, double& fr2) {
  if (stat == BGP_RBF) {
    S = exp(-0.5 * r2);
    fr = S;
    fr2 = S;
  } else if (stat == BGP_MATERN12) {
    const double rr = sqrt(r2);
    S = exp(-rr);
    fr = (rr > 0.0) ? S / rr : 0.0;
    fr2 = (rr > 0.0) ? S * (1.0 + rr) / (rr * rr * rr) : 0.0;
  } else if (stat == BGP_MATERN32) {
    const double tt = sqrt(r2) * 1.7320508075688772;
    const double e = exp(-tt);
    S = (1.0 + tt) * e;
    fr = 3.0 * e;
    fr2 = (tt > 0.0) ? 9.0 * e / tt : 0.0;
  } else {
    const double tt = sqrt(r2) * 2.23606797749979;
    const double e = exp(-tt);
    S = (1.0 + tt + tt * tt / 3.0) * e;
    fr = (5.0 / 3.0) * (tt + 1.0) * e;
    fr2 = (25.0 / 3.0) * e;
  }
}

// grid (npad / 64 * nblk, matrices).  Dst: [b][(k npad + i) npad + j]; s1part: [b][tile][pair k (k + 1) / 2 + l, l <= k];
// vpart: [b][k = 0 (constant), 1 .. d][column tile][i]
__global__ void __launch_bounds__(256) lmlhess_build_kernel(const double* __restrict__ X, const double* __restrict__ H,
                                                            const double* __restrict__ Kinv, const double* __restrict__ alpha_sol,
                                                            double* __restrict__ Dst, double* __restrict__ s1part,
                                                            double* __restrict__ vpart, int n, int d, int npad, int nblk, int form,
                                                            int stat) {
  __shared__ double xi[LH_DMAX][65];
  __shared__ double xj[LH_DMAX][BGP_TILE_LD];
  __shared__ double ell[LH_DMAX];
  __shared__ double alj[128];
  __shared__ double red[4][LH_DMAX * (LH_DMAX + 1) / 2];
  const int b = blockIdx.y, tr = blockIdx.x / nblk, tj = blockIdx.x - tr * nblk;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63, w = tid >> 6;
  const int i0 = tr * 64, j0 = tj * 128, npairs = d * (d + 1) / 2;
  const size_t p = d + 2;
  const double* h = H + (size_t)b * p;
  const double* Ki = Kinv + (size_t)b * npad * npad;
  const double* al = alpha_sol + (size_t)b * npad;
  double* Db = Dst + (size_t)b * d * npad * npad;
  double* vp = vpart + (size_t)b * (d + 1) * nblk * npad;
  if (tid < d) ell[tid] = exp(h[1 + tid]);
  if (tid < 128) alj[tid] = (j0 + tid < n) ? al[j0 + tid] : 0.0;
  __syncthreads();
  for (int idx = tid; idx < d * 128; idx += 256) {
    const int row = idx / d, k = idx - row * d;
    const int gi = i0 + row, gj = j0 + row;
    if (row < 64) xi[k][row] = (gi < n) ? X[(size_t)gi * d + k] / ell[k] : 0.0;
    xj[k][row] = (gj < n) ? X[(size_t)gj * d + k] / ell[k] : 0.0;
  }
  __syncthreads();
  double Fr[4][8], G[4][8];
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 8; c++) Fr[r][c] = 0.0;
  for (int k = 0; k < d; k++) {
    double a[4], bb[8];
#pragma unroll
    for (int r = 0; r < 4; r++) a[r] = xi[k][ty + 16 * r];
#pragma unroll
    for (int c = 0; c < 8; c++) bb[c] = xj[k][tx + 16 * c];
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const double df = a[r] - bb[c];
        Fr[r][c] += df * df;
      }
  }
  // Fr = cf fr, G = W cf fr2 off the diagonal inside the matrix, zeros elsewhere; the constant's row sums v_0 on the way
  const double cst = exp(h[0]);
  const double cf = (form == BGP_FORM_PRODUCT) ? cst : 1.0;
  double v0[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int gi = i0 + ty + 16 * r;
    const double ai = (gi < n) ? al[gi] : 0.0;
    v0[r] = 0.0;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const int gj = j0 + tx + 16 * c;
      double f = 0.0, g = 0.0;
      if (gi < n && gj < n) {
        double S = 1.0;
        if (gi != gj) {
          double fr, fr2;
          lh_facs(stat, Fr[r][c], S, fr, fr2);
          const double Wij = ai * alj[tx + 16 * c] - Ki[(size_t)gi * npad + gj];
          f = cf * fr;
          g = Wij * (cf * fr2);
        }
        v0[r] += ((form == BGP_FORM_PRODUCT) ? cst * S : cst) * alj[tx + 16 * c];
      }
      Fr[r][c] = f;
      G[r][c] = g;
    }
  }
#pragma unroll
  for (int r = 0; r < 4; r++) {
    double s = v0[r];
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (tx == 0) vp[(size_t)tj * npad + i0 + ty + 16 * r] = s;
  }
  for (int k = 0; k < d; k++) {
    double a[4], bb[8], wk[4][8];
#pragma unroll
    for (int r = 0; r < 4; r++) a[r] = xi[k][ty + 16 * r];
#pragma unroll
    for (int c = 0; c < 8; c++) bb[c] = xj[k][tx + 16 * c];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int gi = i0 + ty + 16 * r;
      double s = 0.0;
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const double df = a[r] - bb[c];
        const double u = df * df;
        const double dk = Fr[r][c] * u;
        Db[((size_t)k * npad + gi) * npad + j0 + tx + 16 * c] = dk;
        s += dk * alj[tx + 16 * c];
        wk[r][c] = G[r][c] * u;
      }
      for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if (tx == 0) vp[((size_t)(k + 1) * nblk + tj) * npad + gi] = s;
    }
    for (int l = 0; l <= k; l++) {
      double a2[4], b2[8];
#pragma unroll
      for (int r = 0; r < 4; r++) a2[r] = xi[l][ty + 16 * r];
#pragma unroll
      for (int c = 0; c < 8; c++) b2[c] = xj[l][tx + 16 * c];
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 8; c++) {
          const double df = a2[r] - b2[c];
          s += wk[r][c] * (df * df);
        }
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
      if (lane == 0) red[w][k * (k + 1) / 2 + l] = s;
    }
  }
  __syncthreads();
  if (tid < npairs)
    s1part[((size_t)b * gridDim.x + blockIdx.x) * npairs + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// w[b][j] = sum_i K^-1[i][j], ascending i (the sum form's P_0 = c 1 w^T); grid (npad / 256, matrices)
__global__ void __launch_bounds__(256) lmlhess_colsum_kernel(const double* __restrict__ Kinv, int n, int npad,
                                                             double* __restrict__ wout) {
  const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
  if (j >= npad) return;
  const double* Ki = Kinv + (size_t)b * npad * npad;
  double s = 0.0;
  if (j < n)
    for (int i = 0; i < n; i++) s += Ki[(size_t)i * npad + j];
  wout[(size_t)b * npad + j] = s;
}

// v[b][k][i], k = 0 .. p - 1: the column-tile partials added in ascending order; the noise row s2 alpha; grid (npad / 256, p, matrices)
__global__ void __launch_bounds__(256) lmlhess_v_kernel(const double* __restrict__ vpart, const double* __restrict__ alpha_sol,
                                                        const double* __restrict__ H, int n, int d, int npad, int nblk,
                                                        double* __restrict__ v) {
  const int i = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y, b = blockIdx.z;
  if (i >= npad) return;
  const int p = d + 2;
  double s = 0.0;
  if (i < n) {
    if (k == p - 1) {
      s = exp(H[(size_t)b * p + d + 1]) * alpha_sol[(size_t)b * npad + i];
    } else {
      const double* vp = vpart + (((size_t)b * (d + 1) + k) * nblk) * npad;
      for (int t = 0; t < nblk; t++) s += vp[(size_t)t * npad + i];
    }
  }
  v[((size_t)b * p + k) * npad + i] = s;
}

// Element (i, j) of P_k = D_k K^-1: the stack for the length scales, the closed forms for the constant (k = 0) and the noise (k = p - 1)
struct LhMat {
  const double* P;      // d stacked npad x npad products of this matrix
  const double* Ki;     // its K^-1
  const double* adiag;  // the diagonal additions (shared)
  const double* w;      // K^-1 1 (sum form)
  double cst, s2;
  int n, npad, p;
};
template <int FORM>
static __device__ __forceinline__ double lh_elem(const LhMat& m, int k, int i, int j) {
  if (i >= m.n || j >= m.n) return 0.0;
  if (k == 0) {
    if (FORM == BGP_FORM_PRODUCT) return ((i == j) ? 1.0 : 0.0) - (m.s2 + m.adiag[i]) * m.Ki[(size_t)i * m.npad + j];
    return m.cst * m.w[j];
  }
  if (k == m.p - 1) return m.s2 * m.Ki[(size_t)i * m.npad + j];
  return m.P[((size_t)(k - 1) * m.npad + i) * m.npad + j];
}
static __device__ __forceinline__ LhMat lh_mat(const double* P, const double* Kinv, const double* adiag, const double* wv,
                                               const double* H, int b, int n, int npad, int d) {
  LhMat m;
  m.P = P + (size_t)b * d * npad * npad;
  m.Ki = Kinv + (size_t)b * npad * npad;
  m.adiag = adiag;
  m.w = wv + (size_t)b * npad;
  m.cst = exp(H[(size_t)b * (d + 2)]);
  m.s2 = exp(H[(size_t)b * (d + 2) + d + 1]);
  m.n = n, m.npad = npad, m.p = d + 2;
  return m;
}

// z[b][l][j] = sum_i P_l[i][j] alpha_i, ascending i; grid (npad / 256, p, matrices)
template <int FORM>
__global__ void __launch_bounds__(256) lmlhess_z_kernel(const double* __restrict__ P, const double* __restrict__ Kinv,
                                                        const double* __restrict__ adiag, const double* __restrict__ wv,
                                                        const double* __restrict__ alpha_sol, const double* __restrict__ H, int n,
                                                        int d, int npad, double* __restrict__ z) {
  const int j = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y, b = blockIdx.z;
  if (j >= npad) return;
  const LhMat m = lh_mat(P, Kinv, adiag, wv, H, b, n, npad, d);
  const double* al = alpha_sol + (size_t)b * npad;
  double s = 0.0;
  if (j < n)
    for (int i = 0; i < n; i++) s += lh_elem<FORM>(m, l, i, j) * al[i];
  z[((size_t)b * m.p + l) * npad + j] = s;
}

// grid (8 ntiles, matrices): tile pair t = blockIdx.x / 8 of the lower triangle, 16-row strip si = blockIdx.x % 8 of its blocks.
// tpart[b][blockIdx.x][pair l (l + 1) / 2 + k, k <= l] = sum over the strip of P_k[i][j] P_l[j][i], both orientations of the pair.
template <int FORM>
__global__ void __launch_bounds__(256) lmlhess_pair_kernel(const double* __restrict__ P, const double* __restrict__ Kinv,
                                                           const double* __restrict__ adiag, const double* __restrict__ wv,
                                                           const double* __restrict__ H, int n, int d, int npad,
                                                           double* __restrict__ tpart) {
  __shared__ double Ms[4][LH_NL][LH_SB * LH_LD];
  const int b = blockIdx.y, t = blockIdx.x >> 3, si = blockIdx.x & 7;
  const int tid = threadIdx.x, lane = tid & 63, jj = lane & 15, lq = lane >> 4;
  const int wv_ = __builtin_amdgcn_readfirstlane(tid >> 6);
  const LhMat m = lh_mat(P, Kinv, adiag, wv, H, b, n, npad, d);
  const int p = m.p;
  int ti, tj;
  bgp_tri_decode(t, ti, tj);
  double acc[LH_NL][LH_PMAX];
#pragma unroll
  for (int li = 0; li < LH_NL; li++)
#pragma unroll
    for (int k = 0; k < LH_PMAX; k++) acc[li][k] = 0.0;
  const int npass = (ti == tj) ? 1 : 2;
  for (int pass = 0; pass < npass; pass++) {
    const int ia = (pass ? tj : ti) * 128 + si * LH_SB;  // rows of the register operand
    const int jb = (pass ? ti : tj) * 128;               // its columns = rows of the mirror operand
    if (ia >= n || jb >= n) continue;                    // (uniform: every element of the strip lies in the padding)
    for (int sj = 0; sj < 8; sj++) {
      const int j0 = jb + sj * LH_SB;
      if (j0 >= n) break;  // (uniform)
      double A[LH_PMAX][4];
#pragma unroll
      for (int k = 0; k < LH_PMAX; k++)
        if (k < p) {
#pragma unroll
          for (int e = 0; e < 4; e++) A[k][e] = lh_elem<FORM>(m, k, ia + lq + 4 * e, j0 + jj);
        }
      __syncthreads();  // (the previous block's reads of Ms are through)
#pragma unroll
      for (int li = 0; li < LH_NL; li++) {
        const int l = wv_ + 4 * li;
        if (l < p) {
#pragma unroll
          for (int e = 0; e < 4; e++) Ms[wv_][li][(lq + 4 * e) * LH_LD + jj] = lh_elem<FORM>(m, l, j0 + lq + 4 * e, ia + jj);
        }
      }
      __syncthreads();
#pragma unroll
      for (int li = 0; li < LH_NL; li++) {
        const int l = wv_ + 4 * li;
        if (l < p) {
          double bl[4];
#pragma unroll
          for (int e = 0; e < 4; e++) bl[e] = Ms[wv_][li][jj * LH_LD + lq + 4 * e];  // = P_l[j0 + jj][ia + lq + 4 e]
#pragma unroll
          for (int k = 0; k < LH_PMAX; k++)
            if (k <= 4 * li + 3 && k <= l) {
#pragma unroll
              for (int e = 0; e < 4; e++) acc[li][k] += A[k][e] * bl[e];
            }
        }
      }
    }
  }
  double* out = tpart + ((size_t)b * gridDim.x + blockIdx.x) * LH_NPAIR;
#pragma unroll
  for (int li = 0; li < LH_NL; li++) {
    const int l = wv_ + 4 * li;
#pragma unroll
    for (int k = 0; k < LH_PMAX; k++)
      if (k <= 4 * li + 3 && k <= l && l < p) {
        double s = acc[li][k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) out[l * (l + 1) / 2 + k] = s;
      }
  }
}

// grid (matrices), a thread per pair k <= l
__global__ void __launch_bounds__(256) lmlhess_finish_kernel(const double* __restrict__ s1part, int ntile1,
                                                             const double* __restrict__ tpart, int ntile2,
                                                             const double* __restrict__ v, const double* __restrict__ z,
                                                             const double* __restrict__ grad, int n, int d, int npad, int form,
                                                             double* __restrict__ hess) {
  const int b = blockIdx.x, p = d + 2, tid = threadIdx.x;
  if (tid >= p * (p + 1) / 2) return;
  int l = 0;
  while ((l + 1) * (l + 2) / 2 <= tid) l++;  // (at most p steps)
  const int k = tid - l * (l + 1) / 2;       // k <= l
  const double* g = grad + (size_t)b * p;
  double first = 0.0;
  if (k >= 1 && l <= d) {
    const int npairs = d * (d + 1) / 2, pr = (l - 1) * l / 2 + (k - 1);
    double s1 = 0.0;
    for (int t = 0; t < ntile1; t++) s1 += s1part[((size_t)b * ntile1 + t) * npairs + pr];
    first = 0.5 * s1 - ((k == l) ? 2.0 * g[k] : 0.0);
  } else if (k == 0 && l == 0) {
    first = g[0];
  } else if (k == 0 && l <= d) {
    first = (form == BGP_FORM_PRODUCT) ? g[l] : 0.0;
  } else if (k == p - 1) {
    first = g[p - 1];
  }
  double T = 0.0;
  for (int t = 0; t < ntile2; t++) T += tpart[((size_t)b * ntile2 + t) * LH_NPAIR + tid];
  const double* vk = v + ((size_t)b * p + k) * npad;
  const double* zl = z + ((size_t)b * p + l) * npad;
  double q = 0.0;
  for (int j = 0; j < n; j++) q += vk[j] * zl[j];
  const double val = (first - q) + 0.5 * T;
  hess[((size_t)b * p + k) * p + l] = val;
  hess[((size_t)b * p + l) * p + k] = val;
}

extern "C" int bgp_lml_hess_batch(bgp_ctx* c, int B, const double* h, double* lml, double* grad, double* hess, int* status) {
  BGP_TRY(bgp_guard(c, "bgp_lml_hess_batch"));
  if (!h || !lml || !grad || !hess || B <= 0 || B > 65535) {
    bgp_set_error("bgp_lml_hess_batch: bad argument (1 <= B <= 65535)");
    return BGP_ERR_INVALID;
  }
  if (c->d > LH_DMAX) {
    bgp_set_error("bgp_lml_hess_batch: d > 16 is not supported");
    return BGP_ERR_INVALID;
  }
  return post_call(c, [&]() -> int {
    const int n = c->n, d = c->d, npad = c->npad, nblk = c->nblk, form = c->ks.form;
    const size_t p = d + 2, pp = p * p, nn = (size_t)npad * npad;
    std::vector<int> st(B, 0);
    BGP_TRY(bgp_posterior_build(c, B, h, 1, nullptr, nullptr, nullptr, lml, st.data(), nullptr, false));
    c->post.drop();  // the resident K^-1 belong to this evaluation, not to a posterior (the build has counted a generation)
    const int ntiles = nblk * (nblk + 1) / 2, ntile1 = (npad / 64) * nblk, ntile2 = 8 * ntiles, npairs = d * (d + 1) / 2;
    // matrices per chunk: D and P of a chunk within 2^29 doubles together (BGP_LMLHESS_CHUNK, tests: a forced chunk)
    const int Bc = (int)bgp_switch_cap(BGP_SW_LMLHESS_CHUNK,
                                       std::max<size_t>(1, std::min<size_t>((size_t)B, ((size_t)1 << 28) / ((size_t)d * nn))));
    double *dgrad, *dH, *dgpart, *dhess, *dD, *dP, *ds1, *dvp, *dv, *dz, *dw, *dtp;
    BgpScratch live(c);
    BGP_TRY(live.carve([&](BgpCarve& s) {
      dgrad = s.take<double>((size_t)B * p);
      dH = s.take<double>((size_t)B * p);
      dgpart = s.take<double>((size_t)B * p * ntiles);
      dhess = s.take<double>((size_t)B * pp);
      dD = s.take<double>((size_t)Bc * d * nn);
      dP = s.take<double>((size_t)Bc * d * nn);
      ds1 = s.take<double>((size_t)Bc * ntile1 * npairs);
      dvp = s.take<double>((size_t)Bc * (d + 1) * nblk * npad);
      dv = s.take<double>((size_t)Bc * p * npad);
      dz = s.take<double>((size_t)Bc * p * npad);
      dw = s.take<double>((size_t)Bc * npad);
      dtp = s.take<double>((size_t)Bc * ntile2 * LH_NPAIR);
    }));
    hipStream_t sq = c->stream;
    // the gradient: bgp_lml_grad_batch's launches as they are (its bits)
    BGP_HIP(hipMemsetAsync(dgpart, 0, (size_t)B * p * ntiles * sizeof(double), sq));
    BGP_HIP(bgp_memcpy_async(dH, h, (size_t)B * p * sizeof(double), hipMemcpyHostToDevice, sq));
    hipLaunchKernelGGL(lml_grad_kernel, dim3(8 * ((B + 7) / 8) * ntiles), dim3(256), 0, sq, c->dXeff, dH, c->dKinv, c->dalpha_sol,
                       dgpart, n, d, npad, nblk, form, c->ks.stationary, B);
    BGP_HIP(hipGetLastError());
    hipLaunchKernelGGL(grad_reduce_kernel, dim3(B), dim3(((int)p + 63) / 64 * 64), 0, sq, dgpart, dgrad, ntiles, (int)p);
    BGP_HIP(hipGetLastError());
    BGP_HIP(bgp_memcpy_async(grad, dgrad, (size_t)B * p * sizeof(double), hipMemcpyDeviceToHost, sq));
    const unsigned cb = (unsigned)(npad / 256 + (npad % 256 != 0));
    c->chunk_last[0] = c->chunk_last[1] = 0;
    for (int b0 = 0; b0 < B; b0 += Bc) {  // (the stream orders a chunk behind the one whose buffers it reuses)
      const int nb = std::min(Bc, B - b0);
      const double* dHb = dH + (size_t)b0 * p;
      const double* Ki = c->dKinv + (size_t)b0 * nn;
      const double* al = c->dalpha_sol + (size_t)b0 * npad;
      c->chunk_last[0]++;
      hipLaunchKernelGGL(lmlhess_build_kernel, dim3(ntile1, nb), dim3(256), 0, sq, c->dXeff, dHb, Ki, al, dD, ds1, dvp, n, d, npad,
                         nblk, form, c->ks.stationary);
      BGP_HIP(hipGetLastError());
      if (d > 0)
        bgp_launch_gemm4(sq, 0, dD, Ki, npad, d * npad, npad, npad, dP, npad, nb, (size_t)d * nn, nn, (size_t)d * nn, nullptr);
      hipLaunchKernelGGL(lmlhess_v_kernel, dim3(cb, (unsigned)p, nb), dim3(256), 0, sq, dvp, al, dHb, n, d, npad, nblk, dv);
      if (form == BGP_FORM_PRODUCT) {
        hipLaunchKernelGGL((lmlhess_z_kernel<BGP_FORM_PRODUCT>), dim3(cb, (unsigned)p, nb), dim3(256), 0, sq, dP, Ki, c->dalpha, dw,
                           al, dHb, n, d, npad, dz);
        hipLaunchKernelGGL((lmlhess_pair_kernel<BGP_FORM_PRODUCT>), dim3(ntile2, nb), dim3(256), 0, sq, dP, Ki, c->dalpha, dw, dHb,
                           n, d, npad, dtp);
      } else {
        hipLaunchKernelGGL(lmlhess_colsum_kernel, dim3(cb, nb), dim3(256), 0, sq, Ki, n, npad, dw);
        hipLaunchKernelGGL((lmlhess_z_kernel<BGP_FORM_SUM>), dim3(cb, (unsigned)p, nb), dim3(256), 0, sq, dP, Ki, c->dalpha, dw, al,
                           dHb, n, d, npad, dz);
        hipLaunchKernelGGL((lmlhess_pair_kernel<BGP_FORM_SUM>), dim3(ntile2, nb), dim3(256), 0, sq, dP, Ki, c->dalpha, dw, dHb, n,
                           d, npad, dtp);
      }
      BGP_HIP(hipGetLastError());
      hipLaunchKernelGGL(lmlhess_finish_kernel, dim3(nb), dim3(256), 0, sq, ds1, ntile1, dtp, ntile2, dv, dz,
                         dgrad + (size_t)b0 * p, n, d, npad, form, dhess + (size_t)b0 * pp);
      BGP_HIP(hipGetLastError());
    }
    BGP_HIP(bgp_memcpy_async(hess, dhess, (size_t)B * pp * sizeof(double), hipMemcpyDeviceToHost, sq));
    BGP_HIP(bgp_stream_sync(sq));
    for (int b = 0; b < B; b++) {
      if (st[b] != 0) {  // sklearn/_gpr.py:589: (-inf, zeros); the Hessian with them
        for (size_t k = 0; k < p; k++) grad[(size_t)b * p + k] = 0.0;
        for (size_t k = 0; k < pp; k++) hess[(size_t)b * pp + k] = 0.0;
      }
      if (status) status[b] = st[b];
    }
    return BGP_OK;
  });
}
