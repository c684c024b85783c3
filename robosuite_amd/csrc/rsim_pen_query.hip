// rsim_pen_query.hip -- signed distances in the configuration queries people chain: rsim_config_clearance_signed, rsim_config_clearance_grad_signed and
// rsim_ik_site_avoid_signed (include/rsim.h).  The pair loops are rsim_pen_clear_core.h -- clear_pairs_signed and cost_pairs_signed on rsim_pen_core.h
// pair_signed --, shared with the host rehearsal (tests/san/signed_clear_core_driver.cpp); robosuite_amd/clearance.py and ik_avoid.py with signed=True are the
// fp64 mirrors and the definitions.
//
// A code object of its own: rsim_clear.o, rsim_grad.o, rsim_pen.o and rsim_ik_avoid.o keep the device code they had, and a batch that never passes signed
// launches nothing from here.
//   k_clear_dist_signed (_att)  k_clear_dist's grid (pair chunks, ceil(B K / 64)), lane = candidate, the same partial-result layout; runs behind the unchanged
//                               k_clear_fk (_att) and, with several chunks, in front of the unchanged k_clear_min, whose `dist < best` test takes negative
//                               values as it stands.  The unchanged k_clear_joints / k_clear_grad (_att) read its result for the signed gradient: status 0 and a
//                               direction (p2 - p1) / dist, which grad_dir takes.
//   k_ika_cost_signed (_att)    k_ika_cost with cost_pairs_signed: behind the same done-flag test, the same partial layout, in front of the unchanged
//                               k_ika_step (_att).
// A lane whose pairs do not overlap leaves pair_signed with pair_distance's results, bit for bit, and waits for the lanes of its wavefront that descend.
// Every loop is bounded by pen_iters x max_iters, a table length, n or a vertex count.  No LDS, no barrier, no private segment, no atomics.
#include <hip/hip_runtime.h>
#include "../../include/rsim.h"
#include "rsim_pen_query.h"
#include "rsim_pen_clear_core.h"

using namespace rsim_grad;

namespace {
// the helpers of rsim_clear.hip's and rsim_ik_avoid.hip's kernels, on the same arguments
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
__device__ __forceinline__ Scene<DRayGeom> scene(const DClear& a) {
  Scene<DRayGeom> sc;
  sc.geom = a.geom; sc.pairs = a.pairs; sc.rec = RSIM_DIST_REC; sc.slot_of_body = a.slot_of_body; sc.mesh_vert = a.mesh_vert;
  sc.fo_size = a.fo_size; sc.fo_pos = a.fo_pos; sc.fo_quat = a.fo_quat;
  return sc;
}

template <bool ATT>
__device__ __forceinline__ void clear_dist_signed(const DPenClear& ap) {
  const DClear& a = ap.c;
  const int chunk = (int)blockIdx.x;
  const int c = (int)blockIdx.y * RSIM_CLEAR_LANES + (int)threadIdx.x;
  if (c >= a.NC) return;
  const int per = (a.npair + a.chunks - 1) / a.chunks;
  const int p0 = chunk * per, p1 = min(a.npair, p0 + per);
  Att at = {0u, nullptr, nullptr, nullptr};
  if (ATT) at = attachments(a, c);
  PenOpts po;
  po.pen_tol = ap.pen_tol; po.pen_iters = ap.pen_iters; po.offset = ap.offset;
  const Best r = clear_pairs_signed<ATT>(scene(a), p0, p1, candidate(a, c), scratch(a, c), a.distmax, a.tol, a.max_iters, po, at);
  if (a.chunks > 1) {   // k_clear_dist's partial result, word for word
    const size_t nc = (size_t)a.NC;
    float* w = a.part + (size_t)chunk * RSIM_CLEAR_PART * nc + c;
    w[0] = r.dist; w[nc] = __int_as_float(r.pair); w[2 * nc] = __int_as_float(r.status);
    w[3 * nc] = r.p1.x; w[4 * nc] = r.p1.y; w[5 * nc] = r.p1.z; w[6 * nc] = r.p2.x; w[7 * nc] = r.p2.y; w[8 * nc] = r.p2.z;
    return;
  }
  a.dist[c] = r.dist; a.pair[c] = r.pair;
  if (a.status) a.status[c] = r.status;
  if (a.fromto) {
    float* f = a.fromto + 6 * (size_t)c;
    f[0] = r.p1.x; f[1] = r.p1.y; f[2] = r.p1.z; f[3] = r.p2.x; f[4] = r.p2.y; f[5] = r.p2.z;
  }
}

template <bool ATT>
__device__ __forceinline__ void ika_cost_signed_lane(const DPenIka& ap) {
  const DIkAvoid& a = ap.a;
  const int chunk = (int)blockIdx.x;
  const int c = (int)blockIdx.y * RSIM_CLEAR_LANES + (int)threadIdx.x;
  if (c >= a.g.c.NC) return;
  if (a.done[c]) return;   // frozen: before the pair loop
  const DClear& k = a.g.c;
  const int n = k.n;
  const int per = (k.npair + k.chunks - 1) / k.chunks;
  const int p0 = chunk * per, p1 = min(k.npair, p0 + per);
  Att at = {0u, nullptr, nullptr, nullptr};
  if (ATT) at = attachments(k, c);
  const size_t nc = (size_t)k.NC;
  float* w = a.g.cpart + (size_t)chunk * (RSIM_GRAD_PART + n) * nc + c;
  GradAcc ga;   // the lane's own words of the chunk's partial result
  ga.g = w + RSIM_GRAD_PART * nc; ga.gs = nc;
  PenOpts po;
  po.pen_tol = ap.pen_tol; po.pen_iters = ap.pen_iters; po.offset = ap.offset;
  const Cost r = cost_pairs_signed<ATT>(scene(k), p0, p1, candidate(k, c), scratch(k, c), joints(a.g, c), n, a.g.slide_mask, a.g.d_safe, k.tol, k.max_iters, po, at,
                                        a.g.sig, k.body_att, ga);
  w[0] = r.cost; w[nc] = __int_as_float(r.nnear); w[2 * nc] = __int_as_float(r.nover);
}
}  // namespace

__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_clear_dist_signed(DPenClear a) { clear_dist_signed<false>(a); }
__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_clear_dist_signed_att(DPenClear a) { clear_dist_signed<true>(a); }
__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_ika_cost_signed(DPenIka a) { ika_cost_signed_lane<false>(a); }
__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_ika_cost_signed_att(DPenIka a) { ika_cost_signed_lane<true>(a); }

extern "C" int rsim_launch_clear_dist_signed(const DPenClear* a, hipStream_t stream) {
  if (a->c.NC <= 0 || a->c.npair <= 0 || a->c.chunks <= 0) return 0;
  const int waves = (a->c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES;
  hipLaunchKernelGGL(a->c.natt > 0 ? k_clear_dist_signed_att : k_clear_dist_signed, dim3(a->c.chunks, waves), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  const int e = (int)hipGetLastError();
  return e ? e : rsim_launch_clear_min(&a->c, stream);
}

extern "C" int rsim_launch_ika_iter_signed(const DPenIka* a, hipStream_t stream) {
  if (a->a.g.c.NC <= 0 || a->a.g.c.npair <= 0 || a->a.g.c.chunks <= 0) return 0;
  const int waves = (a->a.g.c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES;
  hipLaunchKernelGGL(a->a.g.c.natt > 0 ? k_ika_cost_signed_att : k_ika_cost_signed, dim3(a->a.g.c.chunks, waves), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  const int e = (int)hipGetLastError();
  return e ? e : rsim_launch_ika_step(&a->a, stream);
}
