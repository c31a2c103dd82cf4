// Generic kernel expression trees on the device (bgp_tree.hip): the program a tree is compiled to on the
// host (kernels.compile_tree), as the entry points receive it and as the tile kernel reads it.
//
// ops (int32 words):  [n_met, n_ins,  n_met x (kind, slot),  n_ins x (code, a, b, c)]
//   metric kinds  BGP_TM_ISO  sum_k ((x_k - y_k) / l)^2,     l   = exp(params[slot])
//                 BGP_TM_ARD  sum_k ((x_k - y_k) / l_k)^2,   l_k = exp(params[slot + k])
//                 BGP_TM_EUCL sum_k (x_k - y_k)^2            (ExpSineSquared)
//                 BGP_TM_DOT  sum_k x_k y_k                  (DotProduct)
//   instructions, postfix over a value stack of BGP_TREE_STACK entries (a, b, c: metric index / parameter slots / immediate index):
//                 CONST(slot)  WHITE(slot)  RBF(met)  M12(met)  M32(met)  M52(met)  RQ(met, slot_alpha)  ESS(met, slot_l, slot_p)
//                 DOT(met, slot_sigma0)  ADD  MUL  POW(imm)
// params: B rows of P log-space values; -inf is legal (a zeroed level exponentiates to 0).
#pragma once
#include "bgp_common.h"

#define BGP_TREE_STACK 8
#define BGP_TREE_MAXMET 4
#define BGP_TREE_MAXINS 32
#define BGP_TREE_MAXIMM 8
#define BGP_TREE_MAXP 256
#define BGP_TREE_MAXD 32

enum { BGP_TM_ISO = 0, BGP_TM_ARD = 1, BGP_TM_EUCL = 2, BGP_TM_DOT = 3 };
enum {
  BGP_TO_CONST = 0, BGP_TO_WHITE, BGP_TO_RBF, BGP_TO_M12, BGP_TO_M32, BGP_TO_M52, BGP_TO_RQ, BGP_TO_ESS, BGP_TO_DOT, BGP_TO_ADD,
  BGP_TO_MUL, BGP_TO_POW, BGP_TO_COUNT
};

// The program as a kernel argument: every lane reads it through scalar loads of the kernel-argument segment.
struct BgpTreeProg {
  int n_met, n_ins, P, n_imm;
  int met[BGP_TREE_MAXMET][2];
  int ins[BGP_TREE_MAXINS][4];
  double imm[BGP_TREE_MAXIMM];
};

// Check a program as the entry points receive it against dimension d and fill `out`; BGP_ERR_INVALID (with the error text set, `who`
// in front) for d > 32, a stack deeper than BGP_TREE_STACK or underflowing, an unknown op or metric, a slot >= P.  Host code only.
int bgp_tree_check(const char* who, int d, int n_ops, const int* ops, int n_imm, const double* imm, int P, BgpTreeProg* out);

// K_b(A_b, Bm_b) for nb items on `st`: item b reads dparams + b P, A + b sA (na x d, row-major) and Bm + b sB (stride 0: shared), and
// writes out + b sO with leading dimension ldo.  self != 0: A == Bm, WhiteKernel counts on i == j, only the tiles on and below the
// diagonal are computed and mirrored; entries outside na x nb are left alone.  self == 0: WhiteKernel counts nothing, the tiles
// cover out_rows x out_cols (multiples of 64, or the matrix's own extents) and entries outside na x nb are written as zeros.
int bgp_launch_tree(hipStream_t st, const BgpTreeProg& prog, int nb, const double* dparams, int d, const double* A, size_t sA, int na,
                    const double* Bm, size_t sB, int nbm, int self, double* out, int ldo, size_t sO, int out_rows, int out_cols);
// diag_b[i] = K_b(x_i, x_i) as self mode gives it (the same bits as the diagonal of that matrix): out + b sO, i < na
int bgp_launch_tree_diag(hipStream_t st, const BgpTreeProg& prog, int nb, const double* dparams, int d, const double* A, size_t sA,
                         int na, double* out, size_t sO);
