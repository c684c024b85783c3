// rsim_dyn_grad.hip -- "how do the torques, and the accelerations, change with the configuration and its rate?": the analytic first derivatives of the
// dynamics queries at K candidate joint vectors per env, for the whole batch, on the device: rsim_config_inverse_dynamics_grad,
// rsim_config_inverse_dynamics_jvp and rsim_config_forward_dynamics_grad (include/rsim.h).  The per-candidate code is rsim_dyn_grad_core.h on the untouched
// rsim_dyn_core.h, shared with the host rehearsal (tests/san/dyn_grad_core_driver.cpp); robosuite_amd/dynamics.py is the fp64 statement by the definition of a
// derivative.
//
// A code object of its own: rsim_dyn.o, rsim_dyn_att.o, rsim_dyn_solve.o, rsim_clear.o and rsim_grad.o compile to what they compiled to.  Its kernels run BEHIND
// the unchanged k_clear_fk, k_clear_joints and k_dyn_rne: the poses, the joint frames and V, A and the subtree wrench of every moved body at the point of
// linearisation sit in their scratches, and these kernels only read them.  Mapping as in rsim_dyn.hip: lane = candidate c = env * K + k, 64 consecutive
// candidates are one wavefront (it may span envs); tables are read at wave-uniform addresses.
//   k_dyn_rne_jvp    grid ceil(B K / 64).  One tangent walk (rne_tangent) along the caller's direction (dq, dqd, dqdd), each null for zeros.
//   k_dyn_rne_grad   grid ceil(B K / 64).  The 2 n unit directions of dq and dqd, one tangent walk each, in a loop inside the lane: column j of the two
//                    n x n blocks per walk.  negate: minus both, the right-hand sides k_dyn_solve takes in the forward-dynamics chain.
// Tangent words in the tangent scratch [slot][24][B K], reused from direction to direction.  A lane reads and writes only its own words: no atomics, a repeat
// call is bit-identical.  Every loop is bounded by the table length or n <= RSIM_JNT_MAX.  No LDS, no barrier, no private segment.
#include <hip/hip_runtime.h>
#include "../../include/rsim.h"
#include "rsim_dyn_grad.h"
#include "rsim_dyn_grad_core.h"

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
__device__ __forceinline__ DynStore words(float* base, const DDyn& a, int c, int words) {
  DynStore s;
  s.a = base + c; s.se = (size_t)words * a.g.c.NC; s.ss = (size_t)a.g.c.NC;
  return s;
}
__device__ __forceinline__ DynModel model(const DDyn& a) {
  DynModel m;
  m.fo_mass = a.fo_mass; m.fo_inertia = a.fo_inertia; m.fo_ipos = a.fo_ipos; m.fo_iquat = a.fo_iquat;
  m.fo_armature = a.fo_armature; m.fo_damping = a.fo_damping; m.fo_opt = a.fo_opt; m.cols = a.cols;
  return m;
}
}  // namespace

__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_dyn_rne_jvp(DDynGrad a) {
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  const DDyn& d = a.d;
  const DClear& cl = d.g.c;
  if (c >= cl.NC) return;
  const size_t at = (size_t)c * cl.n;
  rne_tangent(cl.tab, cl.nel, candidate(cl, c), scratch(cl, c), joints(d.g, c), model(d), d.g.slide_mask, d.qd ? d.qd + at : nullptr, d.qdd ? d.qdd + at : nullptr,
              a.dq ? a.dq + at : nullptr, a.dqd ? a.dqd + at : nullptr, a.dqdd ? a.dqdd + at : nullptr, -1, -1, words(d.dscr, d, c, RSIM_DYN_RNE_WORDS),
              words(a.tscr, d, c, RSIM_DYN_TAN_WORDS), a.dtau + at, 1, false);
}

__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_dyn_rne_grad(DDynGrad a) {
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  const DDyn& d = a.d;
  const DClear& cl = d.g.c;
  if (c >= cl.NC) return;
  const size_t at = (size_t)c * cl.n;
  rne_grad(cl.tab, cl.nel, candidate(cl, c), scratch(cl, c), joints(d.g, c), model(d), cl.n, d.g.slide_mask, d.qd ? d.qd + at : nullptr, d.qdd ? d.qdd + at : nullptr,
           words(d.dscr, d, c, RSIM_DYN_RNE_WORDS), words(a.tscr, d, c, RSIM_DYN_TAN_WORDS), a.dtau_dq + at * cl.n, a.dtau_dqd + at * cl.n, a.negate != 0);
}

extern "C" int rsim_launch_dyn_rne_jvp(const DDynGrad* a, hipStream_t stream) {
  if (a->d.g.c.NC <= 0 || a->d.g.c.nel <= 0) return 0;
  hipLaunchKernelGGL(k_dyn_rne_jvp, dim3((a->d.g.c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}
extern "C" int rsim_launch_dyn_rne_grad(const DDynGrad* a, hipStream_t stream) {
  if (a->d.g.c.NC <= 0 || a->d.g.c.nel <= 0) return 0;
  if (a->d.g.c.n < 1 || a->d.g.c.n > RSIM_JNT_MAX) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dyn_rne_grad, dim3((a->d.g.c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}
