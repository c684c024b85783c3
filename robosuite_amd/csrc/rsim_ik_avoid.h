// rsim_ik_avoid.h -- kernel argument of the collision-aware IK kernels (rsim_ik_avoid.hip), filled by the C-ABI host code (rsim_api.cpp).  Not part of the public
// boundary.  Everything the cost kernels take (rsim_grad.h DGrad on rsim_clear.h DClear: the body table, the pose scratch, the pair table, the joint store, the
// signature table, the chunks' partial results) plus the site, the targets, the options and the problems' state.
#pragma once
#include "rsim_grad.h"

struct DIkAvoid {
  DGrad g;                       // g.c.q IS q (the call's q_out: the problems' joint vectors, the clearance cores' Cand::q); g.cpart is used for EVERY chunk count;
                                 // g.cost / g.nnear / g.nover: the call's outputs, written at every evaluation of a problem that still runs; g.grad is not used
  float* q;                      // [B][K][n]
  const int* head;               // [n][4]: float-table offset of jnt_range, jnt_limited, qpos address, joint type (the head of rsim_ik.h's chain table)
  int rows;                      // 6 (pose) or 3 (position only)
  int site_slot, o_site_pos, o_site_quat;   // the site body's slot in the pose scratch; float-table offsets of site_pos / site_quat
  unsigned site_sig;             // the site body's dof signature
  const float *tpos, *tquat, *q_init;   // [B][K][3], [B][K][4] wxyz or null, [B][K][n] or null
  float damping, max_dq, pos_tol, rot_tol, posture_gain, avoid_gain, cost_tol;
  int max_iters, clamp_range;
  float* q_rest;                 // [B][K][n]: the clamped start vectors
  int* done;                     // [B][K]: the problem has stopped (finished, or max_iters updates made): every kernel passes it over
  int* any;                      // one word: a lane that updated its q stores 1 (a plain vector store; the host clears it before each block of iterations)
  float* err;                    // [B][K][2]
  int* iters;                    // [B][K]: updates made | converged << 30 | finished << 29
};

extern "C" int rsim_launch_ika_init(const DIkAvoid* a, hipStream_t stream);
extern "C" int rsim_launch_ika_iter(const DIkAvoid* a, hipStream_t stream);   // one evaluation: k_ika_cost, k_ika_step
// k_ika_step alone, behind a cost kernel that another code object ran (rsim_pen_query.hip k_ika_cost_signed)
extern "C" int rsim_launch_ika_step(const DIkAvoid* a, hipStream_t stream);
