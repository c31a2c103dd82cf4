// Joint batch selection on pathwise posterior draws (bgp_paths_select; PosteriorPaths.select_batch, Optimizer.ask(strategy="joint_ei" |
// "thompson")).
//
// The P open paths (bgp_paths.hip) are evaluated ONCE at the m candidates into a device matrix F[s, i] -- the evaluator's own
// launches (bgp_paths_launch_eval): bgp_paths_eval's bits --, and q candidates are picked greedily on it without the matrix or
// anything else crossing to the host between the steps.  With c_s the incumbent of path s (a scalar, or the path's own minimum
// over the training inputs: the "noisy EI" incumbent) lowered by every candidate chosen so far,
//   improvement:  a_j(i) = (sum over s, ascending, of max(0, c_s - F[s, i])) / P         the gain of the Monte-Carlo q-EI of the
//                 chosen set when i joins it; the pick is its argmax, then c_s = min(c_s, F[s, pick])
//   Thompson:     a_j(i) = -F[j mod P, i]                                                 path j's minimiser among the candidates left
// The values kernel is fant_col_kernel's shape turned to a column sum: one candidate per thread, F read coalesced along i, the
// incumbents staged in LDS tiles and read as broadcasts, no atomics, one read of F per step.  The argmax is bgp_fantasy.hip's
// (np.argmax's order: ties to the lower index).
#include "bgp_common.h"
#include "bgp_device.h"
#include "bgp_paths_int.h"

#define SEL_NT 64    // candidates per workgroup of the values kernel (one wave: m = 10 000 is 157 workgroups, not 40)
#define SEL_TC 256   // incumbents per LDS tile of the values kernel

// c_s = min over the n rows of FX[s, .] (FX != nullptr) or y_opt, written to inc[s] (the caller's incumbents) and, lowered by the
// forced candidates in their order, to c[s].  One workgroup per path; min is exact, so the tree's order is free.  Path 0's
// workgroup marks the forced candidates chosen.
__global__ void __launch_bounds__(256) sel_init_kernel(const double* __restrict__ FX, int n, double y_opt,
                                                       const double* __restrict__ Fm, size_t mpad, int n_forced,
                                                       const int* __restrict__ forced, double* __restrict__ inc,
                                                       double* __restrict__ c, int* __restrict__ chosen) {
  __shared__ double sv[256];
  const int tid = threadIdx.x, s = blockIdx.x;
  if (FX) {
    const double* row = FX + (size_t)s * n;
    double best = row[0];
    for (int i = tid; i < n; i += 256) {
      const double v = row[i];
      best = v < best ? v : best;
    }
    sv[tid] = best;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) sv[tid] = sv[tid + o] < sv[tid] ? sv[tid + o] : sv[tid];
      __syncthreads();
    }
  }
  if (s == 0)
    for (int k = tid; k < n_forced; k += 256) chosen[forced[k]] = 1;
  if (tid != 0) return;
  double cs = FX ? sv[0] : y_opt;
  inc[s] = cs;
  for (int k = 0; k < n_forced; k++) {
    const double v = Fm[(size_t)s * mpad + forced[k]];
    cs = v < cs ? v : cs;
  }
  c[s] = cs;
}

// a(i) = (sum over s, ascending, of max(0, c_s - F[s, i])) / P, one candidate per thread: plain ascending s whatever m, q and P
// are, so a value depends on its own column of F and on c alone.  2 KB of LDS.
__global__ void __launch_bounds__(SEL_NT) sel_improve_kernel(const double* __restrict__ Fm, size_t mpad, int m, int P,
                                                             const double* __restrict__ c, double* __restrict__ a) {
#pragma clang fp contract(off)
  __shared__ double ct[SEL_TC];
  const int tid = threadIdx.x, i = blockIdx.x * SEL_NT + tid;
  const int ii = (i < m) ? i : m - 1;  // (threads past the end compute a duplicate and store nothing)
  double acc = 0.0;
  for (int s0 = 0; s0 < P; s0 += SEL_TC) {
    const int sc = min(SEL_TC, P - s0);
    __syncthreads();
    for (int k = tid; k < sc; k += SEL_NT) ct[k] = c[s0 + k];
    __syncthreads();
    const double* col = Fm + (size_t)s0 * mpad + ii;
#pragma unroll 8
    for (int r = 0; r < sc; r++) {
      const double df = ct[r] - col[(size_t)r * mpad];
      acc = acc + (df > 0.0 ? df : 0.0);
    }
  }
  if (i < m) a[i] = acc / (double)P;
}

// a(i) = -F[s, i] of ONE path
__global__ void __launch_bounds__(256) sel_thompson_kernel(const double* __restrict__ Frow, int m, double* __restrict__ a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < m) a[i] = -Frow[i];
}

// after a pick: it is chosen, and (improvement) c_s = min(c_s, F[s, pick])
__global__ void __launch_bounds__(256) sel_update_kernel(const double* __restrict__ Fm, size_t mpad, int P, int lower,
                                                         const int* __restrict__ pick, double* __restrict__ c,
                                                         int* __restrict__ chosen) {
  const int s = blockIdx.x * 256 + threadIdx.x, p = *pick;
  if (p < 0) return;  // (cannot happen: q + n_forced <= m leaves a candidate to every step)
  if (s == 0) chosen[p] = 1;
  if (s >= P || !lower) return;
  const double v = Fm[(size_t)s * mpad + p];
  if (v < c[s]) c[s] = v;
}

// mem: the matrix and everything the steps touch, ONE owned allocation of the entry point (it outlives post_call's wait)
static int paths_select_run(bgp_ctx* c, BgpDev<char>& mem, int m, const double* Xcand, int kind, int incumbent, double y_opt,
                            int n_forced, const int* forced, int q, int* picks, double* values, double* inc_out) {
  const bgp_paths_state* s = c->paths;
  const int P = s->P, d = s->d, n = s->n;
  const size_t mpad = ((size_t)m + 255) / 256 * 256, vrows = values ? (size_t)q : 1;
  double *dXc, *dF, *dFX = nullptr, *dinc, *dc, *dval;
  int *dchosen, *dpicks, *dforced;
  BGP_TRY(bgp_carve(mem, 16, [&](BgpCarve& k) {
    dF = k.take<double>((size_t)P * mpad);
    dXc = k.take<double>((size_t)m * d);
    if (incumbent) dFX = k.take<double>((size_t)P * n);
    dinc = k.take<double>(P);
    dc = k.take<double>(P);
    dval = k.take<double>(vrows * mpad);
    dchosen = k.take<int>(mpad);
    dpicks = k.take<int>(q);
    dforced = k.take<int>(n_forced > 0 ? n_forced : 1);
  }));
  hipStream_t st = c->stream;
  BGP_HIP(hipMemsetAsync(dchosen, 0, mpad * sizeof(int), st));
  BGP_HIP(bgp_memcpy_async(dXc, Xcand, (size_t)m * d * sizeof(double), hipMemcpyHostToDevice, st));
  if (n_forced > 0) BGP_HIP(bgp_memcpy_async(dforced, forced, (size_t)n_forced * sizeof(int), hipMemcpyHostToDevice, st));
  BGP_TRY(bgp_paths_launch_eval(c, s, dXc, m, dF, mpad, nullptr));
  if (incumbent) BGP_TRY(bgp_paths_launch_eval(c, s, s->dX, n, dFX, (size_t)n, nullptr));
  hipLaunchKernelGGL(sel_init_kernel, dim3(P), dim3(256), 0, st, dFX, n, y_opt, dF, mpad, n_forced, dforced, dinc, dc, dchosen);
  for (int j = 0; j < q; j++) {
    double* a = dval + (values ? (size_t)j * mpad : 0);
    if (kind == BGP_SELECT_IMPROVEMENT)
      hipLaunchKernelGGL(sel_improve_kernel, dim3((unsigned)(mpad / SEL_NT)), dim3(SEL_NT), 0, st, dF, mpad, m, P, dc, a);
    else
      hipLaunchKernelGGL(sel_thompson_kernel, dim3((unsigned)(mpad / 256)), dim3(256), 0, st, dF + (size_t)(j % P) * mpad, m, a);
    hipLaunchKernelGGL(fant_argmax_kernel, dim3(1), dim3(1024), 0, st, a, dchosen, m, dpicks + j);
    if (j + 1 < q)
      hipLaunchKernelGGL(sel_update_kernel, dim3((P + 255) / 256), dim3(256), 0, st, dF, mpad, P,
                         kind == BGP_SELECT_IMPROVEMENT ? 1 : 0, dpicks + j, dc, dchosen);
  }
  BGP_HIP(hipGetLastError());
  BGP_HIP(bgp_memcpy_async(picks, dpicks, (size_t)q * sizeof(int), hipMemcpyDeviceToHost, st));
  if (values)
    BGP_HIP(bgp_memcpy2d_async(values, (size_t)m * sizeof(double), dval, mpad * sizeof(double), (size_t)m * sizeof(double), q,
                               hipMemcpyDeviceToHost, st));
  if (inc_out) BGP_HIP(bgp_memcpy_async(inc_out, dinc, (size_t)P * sizeof(double), hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_stream_sync(st));
  return BGP_OK;
}

extern "C" int bgp_paths_select(bgp_ctx* c, int m, const double* Xcand, int kind, int incumbent, double y_opt, int n_forced,
                                const int* forced, int q, int* picks, double* values, double* inc_out) {
  BGP_TRY(bgp_guard(c, "bgp_paths_select"));
  if (!c->paths) {
    bgp_set_error("bgp_paths_select: no paths state (call bgp_paths_begin first)");
    return BGP_ERR_STATE;
  }
  if ((kind != BGP_SELECT_IMPROVEMENT && kind != BGP_SELECT_THOMPSON) || (incumbent != 0 && incumbent != 1) || m < 1 || q < 1 ||
      n_forced < 0 || (long long)q + n_forced > m || !Xcand || !picks || (n_forced > 0 && !forced)) {
    bgp_set_error("bgp_paths_select: bad argument (kind %d, incumbent %d, m = %d, q = %d, %d forced: q + forced <= m)", kind,
                  incumbent, m, q, n_forced);
    return BGP_ERR_INVALID;
  }
  if (incumbent == 0 && !std::isfinite(y_opt)) {
    bgp_set_error("bgp_paths_select: the scalar incumbent is not finite");
    return BGP_ERR_INVALID;
  }
  const size_t mpad = ((size_t)m + 255) / 256 * 256;
  if ((size_t)c->paths->P * mpad > BGP_SELECT_MAX_DOUBLES) {
    bgp_set_error("bgp_paths_select: %d paths x %zu padded candidates exceed the 2^27 doubles of the resident draw matrix", c->paths->P,
                  mpad);
    return BGP_ERR_INVALID;
  }
  std::vector<char> seen(n_forced > 0 ? (size_t)m : 0, 0);
  for (int k = 0; k < n_forced; k++) {
    if (forced[k] < 0 || forced[k] >= m || seen[forced[k]]) {
      bgp_set_error("bgp_paths_select: forced pick %d names candidate %d (of %d, each at most once)", k, forced[k], m);
      return BGP_ERR_INVALID;
    }
    seen[forced[k]] = 1;
  }
  BgpDev<char> mem;  // (freed when the call returns, after post_call has waited for a failed body's launches)
  return post_call(
      c, [&] { return paths_select_run(c, mem, m, Xcand, kind, incumbent, y_opt, n_forced, forced, q, picks, values, inc_out); });
}
