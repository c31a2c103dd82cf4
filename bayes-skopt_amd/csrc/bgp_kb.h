// Pieces of the kernel-matrix build shared by bgp_kbuild.hip (the Gram / cross kernels) and bgp_ps.hip (the launch-free
// factorisation's tile workers generating the Gram blocks of their own call).  gfx950 only.
#pragma once
#include "bgp_common.h"
#include "bgp_device.h"

#define KB_DK 16  // input dimensions staged per pass

// Epilogue of a 128 x 128 tile whose squared scaled distances sit in acc[r][c] (rows ty + 16 r, columns tx + 16 c):
// stationary kernel, constant, exact diagonal / identity padding (GRAM) or zero padding (cross matrices).
// R = rows per thread (8: 256 threads, rows ty + 16 r; 4: 512 threads, rows ty + 32 r).
template <int GRAM, int STAT, int FORM, int R = 8>
static __device__ __forceinline__ void kb_epilogue(double (&acc)[R][8], int na, int nb, int d,
                                                   const double* __restrict__ h, const double* __restrict__ alpha,
                                                   int i0, int j0, double* __restrict__ out, size_t ldo, int out_rows,
                                                   int out_cols, int tx, int ty) {
#pragma clang fp contract(off)
  const double cst = exp(h[0]);
  const bool interior = (i0 + 128 <= na) && (j0 + 128 <= nb) && (i0 + 128 <= out_rows) && (j0 + 128 <= out_cols) &&
                        !(GRAM && i0 == j0);
  if (interior) {
#pragma unroll
    for (int r = 0; r < R; r++) {
      double* orow = out + (size_t)(i0 + ty + (128 / R) * r) * ldo + j0 + tx;
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const double v = kb_value<STAT, FORM>(acc[r][c], cst);
        orow[16 * c] = v;
        if (!GRAM) acc[r][c] = v;  // (cross builds: the caller may go on with the values, see kbuild_cross_kernel)
      }
    }
    return;
  }
  const double s2 = exp(h[d + 1]);
#pragma unroll
  for (int r = 0; r < R; r++) {
    const int gi = i0 + ty + (128 / R) * r;
    if (!GRAM) {
      // cross matrices are consumed by 128-tiled GEMMs: the tile's padding (rows >= out_rows, columns >= out_cols,
      // inside the 128-padded buffer) is written as zeros here, so no memset pass over the buffer is needed
#pragma unroll
      for (int c = 0; c < 8; c++) {
        const int gj = j0 + tx + 16 * c;
        const double v = (gi < out_rows && gj < out_cols) ? kb_value<STAT, FORM>(acc[r][c], cst) : 0.0;
        out[(size_t)gi * ldo + gj] = v;
        acc[r][c] = v;
      }
      continue;
    }
    if (gi >= out_rows) continue;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      const int gj = j0 + tx + 16 * c;
      if (gj >= out_cols) continue;
      out[(size_t)gi * ldo + gj] = kb_gram_entry<STAT, FORM>(acc[r][c], gi, gj, na, cst, s2, alpha);  // (GRAM: na == nb)
    }
  }
}

// One input dimension of a tile: acc[r][c] = fma(df, df, acc[r][c]), df = xi[ty + (128 / R) r] - xj[tx + 16 c], with xi / xj
// that dimension's row of the staged operands; callers walk the dimensions in ascending order.  The 8 differences of a row
// are batched ahead of their squares (a subtract never feeds the very next instruction: see kbuild2_kernel).
// (Keep the loop over the dimensions in the caller: the register counts of kbuild_gram_kernel and ps_kernel depend on it.)
template <int R>
static __device__ __forceinline__ void kb_accum(const double* xi, const double* xj, int tx, int ty, double (&acc)[R][8]) {
  double a[R], b[8];
#pragma unroll
  for (int r = 0; r < R; r++) a[r] = xi[ty + (128 / R) * r];
#pragma unroll
  for (int c = 0; c < 8; c++) b[c] = xj[tx + 16 * c];
#pragma unroll
  for (int r = 0; r < R; r++) {
    double df[8];
#pragma unroll
    for (int c = 0; c < 8; c++) df[c] = a[r] - b[c];
    __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
#pragma unroll
    for (int c = 0; c < 8; c++) acc[r][c] = fma(df[c], df[c], acc[r][c]);
    __builtin_amdgcn_sched_group_barrier(0x002, 8, 0);
  }
}

// One 128 x 128 tile out[(i0+..)][(j0+..)] = k(A_i, B_j) by a workgroup of THREADS threads: thread (tx, ty) of a
// 16 x THREADS/16 grid owns rows ty + (128 / R) r, r < R = 2048 / THREADS, and columns tx + 16 c, c < 8.  A is (na x d), Bm is
// (nb x d), row-major; the operands are staged, pre-divided by the length scales, in caller-provided LDS (xi, xj:
// KB_DK rows of BGP_TILE_LD doubles each, ell: KB_DK).  GRAM != 0: A == Bm is the training set (kb_gram_entry).  The values stay in
// acc (cross builds go on with them).
template <int THREADS, int GRAM, int STAT, int FORM>
static __device__ __forceinline__ void kb_tile(const double* __restrict__ A, int na, const double* __restrict__ Bm, int nb,
                                               int d, const double* __restrict__ h, const double* __restrict__ alpha, int i0,
                                               int j0, double* __restrict__ out, size_t ldo, int out_rows, int out_cols,
                                               double (*xi)[BGP_TILE_LD], double (*xj)[BGP_TILE_LD], double* ell,
                                               double (&acc)[2048 / THREADS][8]) {
  constexpr int R = 2048 / THREADS;
  const int tid = threadIdx.x;
  const int tx = tid & 15, ty = tid >> 4;
#pragma unroll
  for (int r = 0; r < R; r++)
#pragma unroll
    for (int c = 0; c < 8; c++) acc[r][c] = 0.0;
  for (int k0 = 0; k0 < d; k0 += KB_DK) {
    const int kc = min(KB_DK, d - k0);
    __syncthreads();
    if (tid < kc) ell[tid] = exp(h[1 + k0 + tid]);
    __syncthreads();
    for (int idx = tid; idx < kc * 128; idx += THREADS) {
      const int row = idx / kc, k = idx - row * kc;
      const int gi = i0 + row, gj = j0 + row;
      const double l = ell[k];
      xi[k][row] = (gi < na) ? A[(size_t)gi * d + k0 + k] / l : 0.0;
      xj[k][row] = (gj < nb) ? Bm[(size_t)gj * d + k0 + k] / l : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < kc; k++) kb_accum<R>(xi[k], xj[k], tx, ty, acc);
  }
  kb_epilogue<GRAM, STAT, FORM, R>(acc, na, nb, d, h, alpha, i0, j0, out, ldo, out_rows, out_cols, tx, ty);
}
