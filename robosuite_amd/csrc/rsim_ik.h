// rsim_ik.h -- kernel argument of k_ik (rsim_ik.hip) and the chain table it reads, built by the C-ABI host code (rsim_api.cpp ik_chain).  Not part of the
// public boundary.
#pragma once
#include "rsim_internal.h"

// The chain table of one (site, dofs) key, ints:
//   [0, 64)   per controlled column c < n, four ints: float-table offset of the joint's jnt_range, jnt_limited, qpos address, joint type
//   [64, ..)  the chain from the world to the site in order, RSIM_IK_REC ints per element:
//               IK_BODY   o1 = offset of body_pos, o2 = offset of body_quat
//               IK_SLIDE / IK_HINGE (the model's joint type codes)   o1 = jnt_pos, o2 = jnt_axis, qadr = qpos address, col = controlled column or -1 (held at
//                         the env's qpos), o3 = offset of qpos0
//               IK_SITE   o1 = site_pos, o2 = site_quat
// Offsets are into an env's float table (ft + env * fstride), so per-env overrides and domain-randomisation draws are what FK sees.
#define RSIM_IK_HEAD 64
#define RSIM_IK_REC 8
enum { IK_BODY = 0, IK_SLIDE = 2, IK_HINGE = 3, IK_SITE = 4 };
enum { IKE_KIND, IKE_O1, IKE_O2, IKE_QADR, IKE_COL, IKE_O3 };

struct DIk {
  int B, K, n, nel, rows;    // envs, problems per env, controlled dofs (1 .. RSIM_JNT_MAX), chain elements, 6 (pose) or 3 (position only)
  int nq, fstride;
  const int* chain;
  const float* ft;           // float tables: env e reads ft + e * fstride
  const float* qpos;         // [B][nq]: joints on the path that are not controlled, and the start vector when q_init is null
  const float *tpos, *tquat, *q_init;   // [B][K][3], [B][K][4] wxyz or null, [B][K][n] or null
  float damping, max_dq, pos_tol, rot_tol, posture_gain;
  int max_iters, clamp_range;
  float* q_out;              // [B][K][n]
  float* err;                // [B][K][2]
  int* iters;                // [B][K]: updates made | converged << 30
};

extern "C" int rsim_launch_ik(const DIk* a, hipStream_t stream);
