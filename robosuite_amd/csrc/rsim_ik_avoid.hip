// rsim_ik_avoid.hip -- collision-aware inverse kinematics for the whole batch, on the device (rsim_ik_site_avoid, include/rsim.h): damped least squares on the
// site pose with the gradient of the collision cost as a secondary task in the null space of the pose task, K problems per env.  The per-problem code is
// rsim_ik_avoid_core.h on rsim_grad_core.h / rsim_clear_core.h, shared with the host rehearsal (tests/san/ik_avoid_core_driver.cpp);
// robosuite_amd/ik_avoid.py is the fp64 host mirror and the definition of the iteration.
//
// A code object of its own.  Mapping as in rsim_clear.hip and rsim_grad.hip: lane = problem c = env * K + k, 64 consecutive problems are one wavefront; tables
// are read at wave-uniform addresses.  NOT one kernel with the loop inside: a wavefront that walks the whole pair list for its 64 problems leaves the part empty
// at the K that IK users ask for (profiles/grad_bench.txt: Lift @4096, 20 ms per evaluation that way at K = 16 against 0.87 ms cut into pair chunks at K = 1).
// The iteration is a chain of TWO launches per evaluation that keeps the pair-chunk parallelism:
//   k_ika_init (_att)   grid ceil(B K / 64).  Clamps the start vector into q (the call's q_out, which the clearance cores read as Cand::q) and q_rest, clears the
//                       problem's state, then fk_walk and joint_walk at q.
//   k_ika_cost (_att)   grid (pair chunks, ceil(B K / 64)).  rsim_grad_core.h cost_pairs -- a new instantiation in this code object -- behind a test of the
//                       problem's done flag: a lane that has stopped leaves before the pair loop, a wavefront whose lanes have all stopped costs nothing.  Every
//                       chunk count writes partial results.
//   k_ika_step (_att)   grid ceil(B K / 64).  Adds the chunk partials in chunk order, evaluates the site error, writes err / cost / counts / iters, decides
//                       (finished, or max_iters updates made: the done flag), else forms the step (rsim_ik_avoid_core.h ika_step), writes the new q and, in the
//                       same kernel, runs fk_walk and joint_walk at it.  A lane that updated stores 1 to the `any` word: a plain vector store, no atomics.
// A problem that has stopped is frozen: none of its words is touched again.  No LDS, no barrier, no private segment; every loop is bounded by a table length, n,
// the chunk count, max_iters of the distance iteration or a vertex count.
#include <hip/hip_runtime.h>
#include "../../include/rsim.h"
#include "rsim_ik_avoid.h"
#include "rsim_ik_avoid_core.h"

using namespace rsim_ika;
static_assert(RSIM_GRAD_COLS == RSIM_JNT_MAX, "rsim_grad_core.h RSIM_GRAD_COLS is include/rsim.h RSIM_JNT_MAX");
static_assert(RSIM_IKA_PART == RSIM_GRAD_PART, "rsim_ik_avoid_core.h RSIM_IKA_PART is rsim_grad.h RSIM_GRAD_PART");

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
__device__ __forceinline__ Att attachments(const DClear& a, int c) { return att_of_env(a.natt, a.held, a.rel, a.body_sig, a.body_att, c / a.K); }
__device__ __forceinline__ Opts options(const DIkAvoid& a) {
  Opts o;
  o.n = a.g.c.n; o.rows = a.rows; o.max_iters = a.max_iters; o.clamp_range = a.clamp_range;
  o.damping = a.damping; o.max_dq = a.max_dq; o.pos_tol = a.pos_tol; o.rot_tol = a.rot_tol; o.posture_gain = a.posture_gain; o.avoid_gain = a.avoid_gain;
  o.cost_tol = a.cost_tol;
  o.head = a.head; o.slide_mask = a.g.slide_mask; o.site_sig = a.site_sig;
  o.site_slot = a.site_slot; o.o_site_pos = a.o_site_pos; o.o_site_quat = a.o_site_quat;
  return o;
}

// the poses of the moved bodies and the joint frames at the problem's q
template <bool ATT>
__device__ __forceinline__ void walks(const DIkAvoid& a, int c, const Cand& cd) {
  const PoseStore st = scratch(a.g.c, c);
  const CandQ qv = {cd.q};
  Att at = {0u, nullptr, nullptr, nullptr};
  if (ATT) at = attachments(a.g.c, c);
  fk_walk<ATT>(a.g.c.tab, a.g.c.nel, cd, st, qv, at);
  joint_walk(a.g.c.tab, a.g.c.nel, cd, st, joints(a.g, c));
}

template <bool ATT>
__device__ __forceinline__ void ika_init_lane(const DIkAvoid& a) {
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  if (c >= a.g.c.NC) return;
  const int n = a.g.c.n;
  const Cand cd = candidate(a.g.c, c);
  ika_start(options(a), cd.ft, cd.qpos, a.q_init ? a.q_init + (size_t)c * n : nullptr, a.q + (size_t)c * n, a.q_rest + (size_t)c * n);
  a.done[c] = 0; a.iters[c] = 0;
  walks<ATT>(a, c, cd);
}

template <bool ATT>
__device__ __forceinline__ void ika_cost_lane(const DIkAvoid& a) {
  const int chunk = (int)blockIdx.x;
  const int c = (int)blockIdx.y * RSIM_CLEAR_LANES + (int)threadIdx.x;
  if (c >= a.g.c.NC) return;
  if (a.done[c]) return;   // frozen: before the pair loop
  const DClear& k = a.g.c;
  const int n = k.n;
  const int per = (k.npair + k.chunks - 1) / k.chunks;
  const int p0 = chunk * per, p1 = min(k.npair, p0 + per);
  Scene<DRayGeom> sc;
  sc.geom = k.geom; sc.pairs = k.pairs; sc.rec = RSIM_DIST_REC; sc.slot_of_body = k.slot_of_body; sc.mesh_vert = k.mesh_vert;
  sc.fo_size = k.fo_size; sc.fo_pos = k.fo_pos; sc.fo_quat = k.fo_quat;
  Att at = {0u, nullptr, nullptr, nullptr};
  if (ATT) at = attachments(k, c);
  const size_t nc = (size_t)k.NC;
  float* w = a.g.cpart + (size_t)chunk * (RSIM_GRAD_PART + n) * nc + c;
  GradAcc ga;   // the lane's own words of the chunk's partial result
  ga.g = w + RSIM_GRAD_PART * nc; ga.gs = nc;
  const Cost r = cost_pairs<ATT>(sc, p0, p1, candidate(k, c), scratch(k, c), joints(a.g, c), n, a.g.slide_mask, a.g.d_safe, k.tol, k.max_iters, at, a.g.sig,
                                 k.body_att, ga);
  w[0] = r.cost; w[nc] = __int_as_float(r.nnear); w[2 * nc] = __int_as_float(r.nover);
}

template <bool ATT>
__device__ __forceinline__ void ika_step_lane(const DIkAvoid& a) {
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  if (c >= a.g.c.NC) return;
  if (a.done[c]) return;   // frozen
  const int n = a.g.c.n;
  const size_t nc = (size_t)a.g.c.NC;
  const Cand cd = candidate(a.g.c, c);
  Prob pr;
  pr.q = a.q + (size_t)c * n; pr.q_rest = a.q_rest + (size_t)c * n;
  pr.part = a.g.cpart + c; pr.part_ks = (size_t)(RSIM_GRAD_PART + n) * nc; pr.part_ws = nc; pr.chunks = a.g.c.chunks;
  pr.tpos = a.tpos + (size_t)c * 3; pr.tquat = a.tquat ? a.tquat + (size_t)c * 4 : nullptr;
  const int it = a.iters[c];
  bool updated;
  const Eval ev = ika_step(options(a), pr, cd.ft, scratch(a.g.c, c), joints(a.g, c), it, updated);
  a.err[(size_t)c * 2] = ev.en; a.err[(size_t)c * 2 + 1] = ev.wn;
  a.g.cost[c] = ev.cost;
  if (a.g.nnear) a.g.nnear[c] = ev.nnear;
  if (a.g.nover) a.g.nover[c] = ev.nover;
  if (!updated) {
    a.iters[c] = it | (ev.conv ? RSIM_IKA_CONV : 0) | (ev.fin ? RSIM_IKA_FIN : 0);
    a.done[c] = 1;
    return;
  }
  a.iters[c] = it + 1;
  *a.any = 1;
  walks<ATT>(a, c, cd);
}
}  // namespace

__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_ika_init(DIkAvoid a) { ika_init_lane<false>(a); }
__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_ika_init_att(DIkAvoid a) { ika_init_lane<true>(a); }
__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_ika_cost(DIkAvoid a) { ika_cost_lane<false>(a); }
__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_ika_cost_att(DIkAvoid a) { ika_cost_lane<true>(a); }
__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_ika_step(DIkAvoid a) { ika_step_lane<false>(a); }
__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_ika_step_att(DIkAvoid a) { ika_step_lane<true>(a); }

extern "C" int rsim_launch_ika_init(const DIkAvoid* a, hipStream_t stream) {
  if (a->g.c.NC <= 0 || a->g.c.nel <= 0) return 0;
  hipLaunchKernelGGL(a->g.c.natt > 0 ? k_ika_init_att : k_ika_init, dim3((a->g.c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}

extern "C" int rsim_launch_ika_iter(const DIkAvoid* a, hipStream_t stream) {
  if (a->g.c.NC <= 0 || a->g.c.npair <= 0 || a->g.c.chunks <= 0) return 0;
  const int waves = (a->g.c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES;
  hipLaunchKernelGGL(a->g.c.natt > 0 ? k_ika_cost_att : k_ika_cost, dim3(a->g.c.chunks, waves), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  const int e = (int)hipGetLastError();
  if (e) return e;
  hipLaunchKernelGGL(a->g.c.natt > 0 ? k_ika_step_att : k_ika_step, dim3(waves), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}

// k_ika_step (_att) alone, behind a cost kernel that another code object ran (rsim_pen_query.hip k_ika_cost_signed)
extern "C" int rsim_launch_ika_step(const DIkAvoid* a, hipStream_t stream) {
  if (a->g.c.NC <= 0 || a->g.c.npair <= 0 || a->g.c.chunks <= 0) return 0;
  hipLaunchKernelGGL(a->g.c.natt > 0 ? k_ika_step_att : k_ika_step, dim3((a->g.c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}
