// THE bounded quasi-Newton iteration of the library (DESIGN.md sections 13 and 15): projected BFGS carried by ONE workgroup of PG_NT
// threads -- a dense inverse Hessian in LDS, the active set read off the projected gradient, Armijo backtracking along the projected
// path.  bgp_minimize_starts (bgp_predgrad.hip: the predictive mean / an upper bound) and bgp_paths_minimize (bgp_paths.hip: a
// posterior function draw) run this one function; what differs is the evaluator it is handed.
//   eval()        evaluates the objective at the point wx (d doubles in LDS, written here) with the whole workgroup; starts with a
//                 barrier, and its results are visible to every thread on return
//   objective()   f of that evaluation (the same value in every thread)
//   gradient(t)   df/dx_t of that evaluation
// Every thread follows the same control flow: all decisions are taken on values read from LDS.  Every loop is capped (max_iter
// iterations of at most PG_LS_MAX trial points); no workgroup waits for another.
#pragma once

#define PG_NT 512                 // threads of a workgroup
#define PG_NW (PG_NT / 64)        // its waves
#define PG_DMAX 32                // input dimensions (the limit of the fantasy fast path): a dimension per lane of half a wave
#define PG_LS_MAX 30              // cap of the backtracking line search
#define PG_HS (PG_DMAX + 1)       // row stride of the inverse-Hessian approximation in LDS (32 x 33 doubles: 8.25 KB)

struct PgBfgs {                   // LDS of one search
  double Hm[PG_DMAX * PG_HS];     // the inverse-Hessian approximation
  double x[PG_DMAX], g[PG_DMAX], p[PG_DMAX], sv[PG_DMAX], yv[PG_DMAX], Hy[PG_DMAX], lo[PG_DMAX], hi[PG_DMAX];
  int act[PG_DMAX];
};

// Minimises from B.x (inside [B.lo, B.hi]; wx holds the same point) until the inf-norm of the projected gradient is <= gtol.  On
// return B.x is the end point, it / nev the iterations and evaluations spent, and the status is returned -- 0: converged, 1: max_iter
// reached, 2: no decrease found, or the objective / its gradient is not finite.  The last evaluation need not have been at B.x (a
// failed line search): the caller closes with one.
template <class Eval, class Objective, class Gradient>
static __device__ __forceinline__ int pg_bfgs(PgBfgs& B, double* wx, int d, double gtol, int max_iter, Eval&& eval,
                                              Objective&& objective, Gradient&& gradient, int& it, int& nev) {
#pragma clang fp contract(off)
  double(&Hm)[PG_DMAX * PG_HS] = B.Hm;
  double(&x)[PG_DMAX] = B.x, (&g)[PG_DMAX] = B.g, (&p)[PG_DMAX] = B.p, (&sv)[PG_DMAX] = B.sv, (&yv)[PG_DMAX] = B.yv;
  double(&Hy)[PG_DMAX] = B.Hy, (&lo)[PG_DMAX] = B.lo, (&hi)[PG_DMAX] = B.hi;
  int(&act)[PG_DMAX] = B.act;
  const int tid = threadIdx.x;
  for (int idx = tid; idx < PG_DMAX * PG_HS; idx += PG_NT) Hm[idx] = (idx / PG_HS == idx % PG_HS) ? 1.0 : 0.0;
  eval();
  double f = objective();
  if (tid < d) g[tid] = gradient(tid);
  __syncthreads();
  int st = 1;
  it = 0, nev = 1;
  bool fresh = true;  // Hm is the identity
  for (; it < max_iter; it++) {
    if (tid < d) act[tid] = (x[tid] <= lo[tid] && g[tid] > 0.0) || (x[tid] >= hi[tid] && g[tid] < 0.0);
    __syncthreads();
    double pgn = 0.0;
    bool finite = isfinite(f);
    for (int t = 0; t < d; t++) {
      finite = finite && isfinite(g[t]);
      if (!act[t]) pgn = fmax(pgn, fabs(g[t]));
    }
    if (!finite) {  // (fmax drops a NaN: without this a non-finite iterate would pass for converged)
      st = 2;
      break;
    }
    if (pgn <= gtol) {
      st = 0;
      break;
    }
    if (tid < d) {
      double pt = 0.0;
      if (!act[tid])
        for (int u = 0; u < d; u++)
          if (!act[u]) pt = fma(-Hm[tid * PG_HS + u], g[u], pt);
      p[tid] = pt;
    }
    __syncthreads();
    double gp = 0.0, pn = 0.0;
    for (int t = 0; t < d; t++) gp = fma(g[t], p[t], gp), pn = fma(p[t], p[t], pn);
    if (!(gp < 0.0)) {  // not a descent direction: forget the curvature, steepest descent on the free variables
      __syncthreads();
      for (int idx = tid; idx < PG_DMAX * PG_HS; idx += PG_NT) Hm[idx] = (idx / PG_HS == idx % PG_HS) ? 1.0 : 0.0;
      if (tid < d) p[tid] = act[tid] ? 0.0 : -g[tid];
      fresh = true;
      __syncthreads();
      gp = 0.0, pn = 0.0;
      for (int t = 0; t < d; t++) gp = fma(g[t], p[t], gp), pn = fma(p[t], p[t], pn);
    }
    double a = 1.0;
    if (fresh) {
      const double r = 1.0 / sqrt(pn);
      a = r < 1.0 ? r : 1.0;
    }
    bool accepted = false;
    double fn = f;
    for (int ls = 0; ls < PG_LS_MAX; ls++) {
      if (tid < d) {
        double v = fma(a, p[tid], x[tid]);
        v = v < lo[tid] ? lo[tid] : (v > hi[tid] ? hi[tid] : v);
        wx[tid] = v;
      }
      eval();
      nev++;
      fn = objective();
      double dd = 0.0;  // the decrease the gradient predicts along the projected step
      for (int t = 0; t < d; t++) dd = fma(g[t], wx[t] - x[t], dd);
      if (dd < 0.0 && fn <= f + 1e-4 * dd) {
        accepted = true;
        break;
      }
      a *= 0.5;
      __syncthreads();  // (wx is rewritten next)
    }
    if (!accepted) {
      if (!fresh) {  // once more from this iterate along the steepest descent (counts as an iteration)
        __syncthreads();
        for (int idx = tid; idx < PG_DMAX * PG_HS; idx += PG_NT) Hm[idx] = (idx / PG_HS == idx % PG_HS) ? 1.0 : 0.0;
        fresh = true;
        __syncthreads();
        continue;
      }
      st = 2;
      break;
    }
    __syncthreads();
    if (tid < d) {
      const double gn = gradient(tid);
      sv[tid] = wx[tid] - x[tid];
      yv[tid] = gn - g[tid];
      x[tid] = wx[tid];
      g[tid] = gn;
    }
    f = fn;
    __syncthreads();
    double sy = 0.0, yy = 0.0, ss = 0.0;
    for (int t = 0; t < d; t++) sy = fma(sv[t], yv[t], sy), yy = fma(yv[t], yv[t], yy), ss = fma(sv[t], sv[t], ss);
    if (sy > 1e-10 * sqrt(ss * yy)) {
      if (fresh) {  // the first pair scales the identity
        const double sc = sy / yy;
        for (int idx = tid; idx < PG_DMAX * PG_HS; idx += PG_NT) Hm[idx] = (idx / PG_HS == idx % PG_HS) ? sc : 0.0;
        __syncthreads();
      }
      if (tid < d) {
        double v = 0.0;
        for (int u = 0; u < d; u++) v = fma(Hm[tid * PG_HS + u], yv[u], v);
        Hy[tid] = v;
      }
      __syncthreads();
      double yHy = 0.0;
      for (int t = 0; t < d; t++) yHy = fma(yv[t], Hy[t], yHy);
      const double rho = 1.0 / sy, c2 = (sy + yHy) * rho * rho;
      for (int idx = tid; idx < d * d; idx += PG_NT) {
        const int t = idx / d, u = idx - t * d;
        Hm[t * PG_HS + u] = Hm[t * PG_HS + u] + (c2 * (sv[t] * sv[u]) - rho * (Hy[t] * sv[u] + sv[t] * Hy[u]));
      }
      fresh = false;
      __syncthreads();
    }
  }
  __syncthreads();
  return st;
}
