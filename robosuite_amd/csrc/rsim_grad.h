// rsim_grad.h -- kernel argument of the clearance gradient and collision cost kernels (rsim_grad.hip), filled by the C-ABI host code (rsim_api.cpp).  Not part
// of the public boundary.  Everything the clearance kernels take (rsim_clear.h DClear: the body table, the pose scratch, the pair table, the results) plus the
// joint store, the signature table and the new outputs.
#pragma once
#include "rsim_clear.h"

#define RSIM_GRAD_PART 3         /* words per partial result of a pair chunk in front of its n gradient entries: cost, nnear, noverlap */

struct DGrad {
  DClear c;                      // c.dist / c.pair / c.fromto / c.status: what k_clear_dist (k_clear_min) wrote -- the gradient kernel READS them
  float* jscr;                   // [n][6][NC]: world axis and anchor of every controlled column (rsim_grad_core.h JointStore)
  unsigned slide_mask;           // bit c: controlled column c is a slide joint
  const int* sig;                // [nbody]: dof signatures, unheld in the low 16 bits, held in the high 16 (c.body_att [nbody] says of which attachment)
  float* grad;                   // [B][K][n]
  // the collision cost
  float d_safe;
  float* cost;                   // [B][K]
  int *nnear, *nover;            // [B][K] each, or null
  float* cpart;                  // c.chunks > 1: [chunks][RSIM_GRAD_PART + n][NC] partial results (floats and ints share the words)
};

extern "C" int rsim_launch_clear_joints(const DGrad* a, hipStream_t stream);
extern "C" int rsim_launch_clear_grad(const DGrad* a, hipStream_t stream);
extern "C" int rsim_launch_clear_cost(const DGrad* a, hipStream_t stream);
// k_clear_cost_sum alone, behind a pair loop that another code object ran (rsim_pen.hip k_clear_cost_signed); nothing with g.c.chunks <= 1
extern "C" int rsim_launch_clear_cost_sum(const DGrad* a, hipStream_t stream);
