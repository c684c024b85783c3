// rsim_dyn_grad.h -- kernel argument of the kernels of the dynamics derivatives (rsim_dyn_grad.hip), filled by the C-ABI host code (rsim_api.cpp).  Not part of
// the public boundary.  Everything k_dyn_rne takes (rsim_dyn.h DDyn, unchanged: d.qd, d.qdd the point of linearisation, d.dscr the words k_dyn_rne has left
// there at that point) plus the tangent scratch, the direction and the outputs.
#pragma once
#include "rsim_dyn.h"

struct DDynGrad {
  DDyn d;
  float* tscr;                    // [nslot][RSIM_DYN_TAN_WORDS][NC]: the tangent words of one direction, reused by the next
  const float *dq, *dqd, *dqdd;   // k_dyn_rne_jvp: [B][K][n] each, or null: zeros
  float* dtau;                    // k_dyn_rne_jvp: [B][K][n]
  float *dtau_dq, *dtau_dqd;      // k_dyn_rne_grad: [B][K][n][n] each, entry [i][j] = d tau_i / d q_j (qd_j)
  int negate;                     // k_dyn_rne_grad: write minus both (the right-hand sides of the forward-dynamics chain)
};

extern "C" int rsim_launch_dyn_rne_jvp(const DDynGrad* a, hipStream_t stream);
extern "C" int rsim_launch_dyn_rne_grad(const DDynGrad* a, hipStream_t stream);
