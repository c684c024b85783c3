// rsim_dyn_att.hip -- "can the arm hold or execute this WITH THE OBJECT IN HAND?": the dynamics queries of rsim_dyn.hip with the payload of carried objects,
// rsim_config_inverse_dynamics_attached, rsim_config_mass_matrix_attached, rsim_config_jacobian_attached and, through them, the three M^-1 entries
// (include/rsim.h).  The per-candidate code is rsim_dyn_att_core.h on the untouched rsim_dyn_core.h, shared with the host rehearsal
// (tests/san/dyn_att_driver.cpp); robosuite_amd/dynamics.py with attach / held / rel is the fp64 statement by the definition.
//
// A code object of its own: rsim_dyn.o, rsim_clear.o and rsim_grad.o compile to what they compiled to.  Its kernels run BEHIND k_clear_fk_att, which leaves the
// attached bodies' poses in the pose scratch (the env's own pose where the env does not hold them), and the unchanged k_clear_joints; k_dyn_solve runs unchanged
// behind them.  Mapping as in rsim_dyn.hip: lane = candidate c = env * K + k, 64 consecutive candidates are one wavefront (it may span envs, so its lanes may
// disagree about `held`); tables are read at wave-uniform addresses, the held row is the lane's own.
//   k_dyn_rne_att   the two walks of k_dyn_rne over the whole table: a held attached body takes V and A from its carrier's slot and adds its wrench there.
//   k_dyn_crb_att   the same with the inertia words.
//   k_dyn_jac_att   the site's point from the stored pose of its body -- attached or not --, the columns from the half of the body's signature word that the
//                   lane's env selects.
// A lane reads and writes only its own words: no atomics, a repeat call is bit-identical.  No LDS, no barrier, no private segment.
#include <hip/hip_runtime.h>
#include "../../include/rsim.h"
#include "rsim_dyn_att.h"
#include "rsim_dyn_att_core.h"

using namespace rsim_dyn;
static_assert(RSIM_CLEAR_ATTACH_MAX == RSIM_ATTACH_MAX, "rsim_clear_core.h RSIM_CLEAR_ATTACH_MAX is include/rsim.h RSIM_ATTACH_MAX");

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
// the held row of the lane's env as a bit mask (rsim_clear_core.h att_of_env)
__device__ __forceinline__ unsigned held_row(const DClear& a, int c) { return att_of_env(a.natt, a.held, nullptr, nullptr, nullptr, c / a.K).held; }
}  // namespace

__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_dyn_rne_att(DDyn a) {
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  const DClear& cl = a.g.c;
  if (c >= cl.NC) return;
  const size_t at = (size_t)c * cl.n;
  rne_walk_att(cl.tab, cl.nel, candidate(cl, c), scratch(cl, c), joints(a.g, c), model(a), a.g.slide_mask, a.qd ? a.qd + at : nullptr, a.qdd ? a.qdd + at : nullptr,
               dyn_scratch(a, c, RSIM_DYN_RNE_WORDS), a.tau + at, 1, held_row(cl, c));
}

__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_dyn_crb_att(DDyn a) {
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  const DClear& cl = a.g.c;
  if (c >= cl.NC) return;
  crb_walk_att(cl.tab, cl.nel, candidate(cl, c), scratch(cl, c), joints(a.g, c), model(a), cl.n, a.g.slide_mask, a.g.sig, dyn_scratch(a, c, RSIM_DYN_CRB_WORDS),
               a.M + (size_t)c * cl.n * cl.n, held_row(cl, c));
}

__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_dyn_jac_att(DDyn a, int site_att) {
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  const DClear& cl = a.g.c;
  if (c >= cl.NC) return;
  const size_t at = (size_t)c * 3 * cl.n;
  const V3 p = site_point(candidate(cl, c), scratch(cl, c), a.site_slot, a.site_body, a.o_site_pos);
  site_jac(joints(a.g, c), cl.n, a.g.slide_mask, site_sig_att(a.site_sig, site_att, held_row(cl, c)), p, a.jacp ? a.jacp + at : nullptr, a.jacr ? a.jacr + at : nullptr);
}

extern "C" int rsim_launch_dyn_rne_att(const DDyn* a, hipStream_t stream) {
  if (a->g.c.NC <= 0 || a->g.c.nel <= 0) return 0;
  hipLaunchKernelGGL(k_dyn_rne_att, dim3((a->g.c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}
extern "C" int rsim_launch_dyn_crb_att(const DDyn* a, hipStream_t stream) {
  if (a->g.c.NC <= 0 || a->g.c.nel <= 0) return 0;
  hipLaunchKernelGGL(k_dyn_crb_att, dim3((a->g.c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}
extern "C" int rsim_launch_dyn_jac_att(const DDyn* a, int site_att, hipStream_t stream) {
  if (a->g.c.NC <= 0) return 0;
  hipLaunchKernelGGL(k_dyn_jac_att, dim3((a->g.c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), 0, stream, *a, site_att);
  return (int)hipGetLastError();
}
