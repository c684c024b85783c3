// rsim_dyn.hip -- "can the arm hold or execute this?": joint torques, the joint-space inertia and a site Jacobian at K candidate joint vectors per env, for the
// whole batch, on the device: rsim_config_inverse_dynamics, rsim_config_mass_matrix and rsim_config_jacobian (include/rsim.h).  The per-candidate code is
// rsim_dyn_core.h on rsim_grad_core.h, shared with the host rehearsal (tests/san/dyn_core_driver.cpp); robosuite_amd/dynamics.py is the fp64 statement by the
// definition.
//
// A code object of its own, like rsim_grad.hip, whose first two kernels it runs BEHIND: k_clear_fk has left the poses of the moved bodies in the pose scratch and
// k_clear_joints world axis and anchor of every controlled column in the joint store -- those kernels are untouched by this file.  Mapping as there: lane =
// candidate c = env * K + k, 64 consecutive candidates are one wavefront (it may span envs); tables are read at wave-uniform addresses.
//   k_dyn_rne   grid ceil(B K / 64).  One forward walk of the body table carrying velocity, acceleration and wrench, one backward walk that folds every body's
//               wrench into its parent's and projects it on the controlled joints.  Per-body words in the dynamics scratch [slot][18][B K].
//   k_dyn_crb   grid ceil(B K / 64).  Every body's inertia about the reference point into the scratch [slot][10][B K], then the backward walk that sums the
//               subtrees and writes each pair of related columns once, to both triangles.
//   k_dyn_jac   grid ceil(B K / 64).  The site's point from the stored pose of its body, then the columns from the joint store and the body's signature.
// A lane reads and writes only its own words: no atomics, a repeat call is bit-identical.  Every loop is bounded by the table length or RSIM_JNT_MAX.  No LDS, no
// barrier, no private segment.
#include <hip/hip_runtime.h>
#include "../../include/rsim.h"
#include "rsim_dyn.h"
#include "rsim_dyn_core.h"

using namespace rsim_dyn;
static_assert(RSIM_GRAD_COLS == RSIM_JNT_MAX, "rsim_grad_core.h RSIM_GRAD_COLS is include/rsim.h RSIM_JNT_MAX");

namespace {
__device__ __forceinline__ Cand candidate(const DClear& a, int c) {
  const int env = c / a.K;
  Cand r;
  r.ft = a.ft + (size_t)env * a.fstride;
  r.qpos = a.qpos + (size_t)env * a.nq;
  r.q = a.q + (size_t)c * a.n;
  r.xpos = a.xpos + (size_t)env * a.nbody * 3;
  r.xquat = a.xquat + (size_t)env * a.nbody * 4;
  return r;
}
__device__ __forceinline__ PoseStore scratch(const DClear& a, int c) {
  const size_t nc = (size_t)a.NC;
  PoseStore s;
  s.pos = a.scr + c; s.quat = a.scr + 3 * nc + c;
  s.pe = s.qe = 7 * nc; s.ps = s.qs = nc; s.by_body = 0;
  return s;
}
__device__ __forceinline__ JointStore joints(const DGrad& a, int c) {
  JointStore s;
  s.a = a.jscr + c; s.ce = 6 * (size_t)a.c.NC; s.cs = (size_t)a.c.NC;
  return s;
}
__device__ __forceinline__ DynStore dyn_scratch(const DDyn& a, int c, int words) {
  DynStore s;
  s.a = a.dscr + c; s.se = (size_t)words * a.g.c.NC; s.ss = (size_t)a.g.c.NC;
  return s;
}
__device__ __forceinline__ DynModel model(const DDyn& a) {
  DynModel m;
  m.fo_mass = a.fo_mass; m.fo_inertia = a.fo_inertia; m.fo_ipos = a.fo_ipos; m.fo_iquat = a.fo_iquat;
  m.fo_armature = a.fo_armature; m.fo_damping = a.fo_damping; m.fo_opt = a.fo_opt; m.cols = a.cols;
  return m;
}
}  // namespace

__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_dyn_rne(DDyn a) {
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  const DClear& cl = a.g.c;
  if (c >= cl.NC) return;
  const size_t at = (size_t)c * cl.n;
  rne_walk(cl.tab, cl.nel, candidate(cl, c), scratch(cl, c), joints(a.g, c), model(a), a.g.slide_mask, a.qd ? a.qd + at : nullptr, a.qdd ? a.qdd + at : nullptr,
           dyn_scratch(a, c, RSIM_DYN_RNE_WORDS), a.tau + at, 1);
}

__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_dyn_crb(DDyn a) {
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  const DClear& cl = a.g.c;
  if (c >= cl.NC) return;
  crb_walk(cl.tab, cl.nel, candidate(cl, c), scratch(cl, c), joints(a.g, c), model(a), cl.n, a.g.slide_mask, a.g.sig, dyn_scratch(a, c, RSIM_DYN_CRB_WORDS),
           a.M + (size_t)c * cl.n * cl.n);
}

__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_dyn_jac(DDyn a) {
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  const DClear& cl = a.g.c;
  if (c >= cl.NC) return;
  const size_t at = (size_t)c * 3 * cl.n;
  const V3 p = site_point(candidate(cl, c), scratch(cl, c), a.site_slot, a.site_body, a.o_site_pos);
  site_jac(joints(a.g, c), cl.n, a.g.slide_mask, a.site_sig, p, a.jacp ? a.jacp + at : nullptr, a.jacr ? a.jacr + at : nullptr);
}

extern "C" int rsim_launch_dyn_rne(const DDyn* a, hipStream_t stream) {
  if (a->g.c.NC <= 0 || a->g.c.nel <= 0) return 0;
  hipLaunchKernelGGL(k_dyn_rne, dim3((a->g.c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}
extern "C" int rsim_launch_dyn_crb(const DDyn* a, hipStream_t stream) {
  if (a->g.c.NC <= 0 || a->g.c.nel <= 0) return 0;
  hipLaunchKernelGGL(k_dyn_crb, dim3((a->g.c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}
extern "C" int rsim_launch_dyn_jac(const DDyn* a, hipStream_t stream) {
  if (a->g.c.NC <= 0) return 0;
  hipLaunchKernelGGL(k_dyn_jac, dim3((a->g.c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}
