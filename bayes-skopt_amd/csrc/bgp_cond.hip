// Moments of candidates conditional on point sets, on the resident posteriors: everything of bgp_knowledge_gradient (bgp_kg.hip) and
// bgp_joint_entropy (bgp_jes.hip) but their scoring kernels.
//
// For resident posterior b, its points A_b = (a_0 .. a_{M-1}) -- one set shared by all posteriors, or one set per posterior -- and a
// chunk of candidates x_i:
//   1  once per chunk of posteriors (skipped with M = 0): R_b = k_b(A_b, X) with mu_b(A_b) = R_b alpha_b and, on request, var_b(A_b)
//      (bgp_launch_moments: rows zero padded to 128), then P_b = R_b K_b^-1 on the LDS-DMA ring (bgp_launch_gemm4 mode 0; K^-1
//      symmetric: an NT product).
//   2  once per chunk of candidates: K_* = k_b(chunk, X), mean and variance of the chunk (bgp_launch_moments: the launches of
//      bgp_predict_batch, the same bits); k_b(chunk, A_b) by the cross build into C, then C -= K_* P_b^T on the ring (mode 2 of
//      gemm4_kernel) on the columns 0 .. pad64(M) only: the hot product, 2 n m pad64(M) flops per posterior.
//      C[x][j] = cov_b(a_j, x) = k_b(a_j, x) - k_b(a_j, X) K_b^-1 k_b(X, x)   (latent: no white term)
//   3  the caller's scoring kernel on the chunk, into its slice of the B x pad128(m) value matrix.
//   4  the average over the posteriors: bgp_acq_batch's kernel (acq_sum_kernel: ascending posterior, value / n_samples, a posterior
//      with a non-finite value contributes nothing), the downloads, one stream sync.
// Plain launches on the context's stream; nothing here waits for another workgroup or adds floating-point numbers atomically.
#include "bgp_common.h"

// Candidates per chunk: a multiple of 128 that depends on n alone, so that a posterior's K_* stays within 2^24 doubles.  The
// caller's switch (tests): another size, rounded up to 128.
static size_t cond_cand_chunk(int npad, BgpSwitch sw) {
  size_t mc = (((size_t)1 << 24) / (size_t)npad) / 128 * 128;
  if (const char* e = bgp_switch(sw)) {
    const long v = atol(e);
    if (v > 0) mc = ((size_t)v + 127) / 128 * 128;
  }
  return std::min<size_t>(std::max<size_t>(mc, 128), (size_t)1 << 18);
}

BgpCondPlan bgp_cond_plan(const bgp_ctx* c, const BgpCondReq& q) {
  const int npad = c->npad;
  BgpCondPlan p;
  p.Mp = std::max(pad_to(q.M, 128), 128), p.M64 = pad_to(q.M, 64);
  p.mtot = pad_to(q.m, 128);
  p.mc = (int)std::min<size_t>(cond_cand_chunk(npad, q.chunk_switch), (size_t)p.mtot);
  p.tq = npad / bgp_rowquad_tile();
  p.sKs = (size_t)p.mc * npad, p.sC = (size_t)p.mc * p.Mp, p.sR = (size_t)p.Mp * npad;
  p.sAx = q.per_posterior ? (size_t)q.M * c->d : 0;
  p.Bc = (int)std::max<size_t>(1, std::min<size_t>((size_t)q.B, ((size_t)1 << 29) / (p.sKs + p.sC + 2 * p.sR)));
  p.Bc = (int)bgp_switch_cap(BGP_SW_ITEM_CHUNK, (size_t)p.Bc);  // (tests: forced posterior chunks against the default)
  return p;
}

int bgp_cond_run(bgp_ctx* c, const BgpCondReq& q, const std::function<void(const BgpCondChunk&)>& score) {
  const int d = c->d, npad = c->npad, B = q.B, m = q.m, M = q.M;
  const size_t hp = d + 2;
  const BgpCondPlan p = bgp_cond_plan(c, q);
  const int Bc = p.Bc, Mp = p.Mp, mc = p.mc, mtot = p.mtot;
  const size_t nA = (q.per_posterior ? (size_t)B : 1) * M * d;  // doubles of the point sets
  double *dXc, *dA, *dF = nullptr, *dH, *dnoise, *dR, *dP, *dmuA, *dvA = nullptr, *dpartA, *dKs, *dmpart, *dmean, *dvar, *dCv, *dV,
      *davg;
  int* dbad;
  BgpScratch live(c);
  BGP_TRY(live.carve([&](BgpCarve& s) {
    dXc = s.take<double>((size_t)m * d);
    dA = s.take<double>(std::max<size_t>(nA, d));
    if (q.fpts) dF = s.take<double>((size_t)B * M);
    dH = s.take<double>((size_t)B * hp);
    dnoise = s.take<double>(B);
    dR = s.take<double>((size_t)Bc * p.sR);
    dP = s.take<double>((size_t)Bc * p.sR);
    dmuA = s.take<double>((size_t)Bc * Mp);
    if (q.want_var) dvA = s.take<double>((size_t)Bc * Mp);
    dpartA = s.take<double>((size_t)Bc * (npad / 128) * Mp);
    dKs = s.take<double>((size_t)Bc * p.sKs);
    dmpart = s.take<double>((size_t)Bc * (npad / 128) * mc);
    dmean = s.take<double>((size_t)Bc * mc);
    dvar = s.take<double>((size_t)Bc * mc);
    dCv = s.take<double>((size_t)Bc * p.sC);
    dV = s.take<double>((size_t)B * mtot);
    davg = s.take<double>(mtot);
    dbad = s.take<int>(B);
  }));
  // (the row-dot partials of every moments stage below, sized once: nothing grows inside the loops)
  BGP_TRY(c->drowpart.ensure((size_t)Bc * p.tq * (q.want_var ? std::max(mc, Mp) : mc)));
  hipStream_t st = c->stream;
  BGP_HIP(bgp_memcpy_async(dXc, q.Xcand, (size_t)m * d * sizeof(double), hipMemcpyHostToDevice, st));
  if (M > 0) BGP_HIP(bgp_memcpy_async(dA, q.Xpts, nA * sizeof(double), hipMemcpyHostToDevice, st));
  if (q.fpts) BGP_HIP(bgp_memcpy_async(dF, q.fpts, (size_t)B * M * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(dH, q.h_kernel, (size_t)B * hp * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(bgp_memcpy_async(dnoise, q.noise, (size_t)B * sizeof(double), hipMemcpyHostToDevice, st));
  BGP_HIP(hipMemsetAsync(dbad, 0, (size_t)B * sizeof(int), st));
  c->chunk_last[0] = c->chunk_last[1] = 0;
  for (int b0 = 0; b0 < B; b0 += Bc) {
    c->chunk_last[0]++;
    const int nb = std::min(Bc, B - b0);
    const double* dHb = dH + (size_t)b0 * hp;
    const double* dAb = dA + (size_t)b0 * p.sAx;
    const double* Kinv = c->dKinv + (size_t)b0 * npad * npad;
    const double* al = c->dalpha_sol + (size_t)b0 * npad;
    if (M > 0) {
      BGP_TRY(bgp_launch_moments(c, nb, dHb, M, dAb, p.sAx, c->dXeff, 0, al, Kinv, dR, npad, p.sR, dpartA, dmuA, dvA));
      bgp_launch_gemm4(st, 0, dR, Kinv, npad, p.M64, npad, npad, dP, npad, nb, p.sR, (size_t)npad * npad, p.sR, nullptr);
      BGP_HIP(hipGetLastError());
    }
    for (int m0 = 0; m0 < m; m0 += mc) {
      const int mm = std::min(mc, m - m0), mmp = pad_to(mm, 128);  // (the strides of this chunk's moments: mmp)
      if (b0 == 0) c->chunk_last[1]++;
      const double* dXq = dXc + (size_t)m0 * d;
      BGP_TRY(bgp_launch_moments(c, nb, dHb, mm, dXq, 0, c->dXeff, 0, al, Kinv, dKs, npad, p.sKs, dmpart, dmean, dvar));
      if (M > 0) {
        BGP_TRY(bgp_launch_kcross_matvec_x(c, nb, dHb, mm, dXq, 0, M, dAb, p.sAx, dCv, Mp, p.sC, nullptr, 0, nullptr));
        bgp_launch_gemm4(st, 2, dKs, dP, npad, pad_to(mm, 64), p.M64, npad, dCv, Mp, nb, p.sKs, p.sR, p.sC, nullptr);
      }
      BgpCondChunk k;
      k.b0 = b0, k.nb = nb, k.m0 = m0, k.mm = mm;
      k.muA = dmuA, k.vA = dvA, k.fpts = dF ? dF + (size_t)b0 * M : nullptr;
      k.Cv = dCv, k.Mp = Mp, k.sC = p.sC;
      k.mean = dmean, k.var = dvar, k.sm = (size_t)mmp;
      k.noise = dnoise + b0;
      k.out = dV + (size_t)b0 * mtot + m0, k.so = (size_t)mtot;
      k.bad = dbad + b0;
      score(k);
      BGP_HIP(hipGetLastError());
    }
  }
  if (q.avg) {
    hipLaunchKernelGGL(acq_sum_kernel, dim3((m + 255) / 256, 1), dim3(256), 0, st, dV, dbad, (size_t)mtot, m, B, q.n_samples, davg);
    BGP_HIP(hipGetLastError());
    BGP_HIP(bgp_memcpy_async(q.avg, davg, (size_t)m * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  if (q.rows)
    BGP_HIP(bgp_memcpy2d_async(q.rows, (size_t)m * sizeof(double), dV, (size_t)mtot * sizeof(double), (size_t)m * sizeof(double), B,
                               hipMemcpyDeviceToHost, st));
  BGP_HIP(bgp_stream_sync(st));
  return BGP_OK;
}
