// What bgp_paths.hip shares with the other users of an open paths state (bgp_paths_select.hip): the state itself and the
// evaluator's launches.  Host code only; the kernels stay in bgp_paths.hip.
#pragma once
#include "bgp_common.h"

struct bgp_paths_state {
  int P = 0, F = 0, n = 0, d = 0;
  BgpDev<char> mem;  // one allocation, carved by bgp_paths_begin
  double *dX, *dH, *dOm, *dPh, *dAw, *dC0, *dV;
};

// The P paths at the m rows of dXq (device, m*d) into out[p * so + i] (and, dout != nullptr, the gradients into dout[(p * so + i) * d + k]):
// THE feature and update launches of bgp_paths_eval, enqueued on c->stream -- whoever calls this gets bgp_paths_eval's bits.
int bgp_paths_launch_eval(bgp_ctx* c, const bgp_paths_state* s, const double* dXq, int m, double* out, size_t so, double* dout);
