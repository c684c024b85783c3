// rsim_grad.hip -- "which way does this joint configuration move away from the scene?": the derivative of the configuration clearance with respect to the
// controlled joints, and a smooth collision cost with its gradient, for K candidate joint vectors per env, for the whole batch, on the device:
// rsim_config_clearance_grad and rsim_config_collision_cost (include/rsim.h).  The per-candidate code is rsim_grad_core.h on rsim_clear_core.h, shared with the
// host rehearsal (tests/san/grad_core_driver.cpp); robosuite_amd/clearance.py clearance_grad / collision_cost is the fp64 host mirror.
//
// A code object of its own, like rsim_clear.hip, whose kernels it runs BEHIND: k_clear_fk (_att) has left the poses of the moved bodies in the scratch, and for
// the gradient k_clear_dist (_att) and k_clear_min have written dist / pair / fromto / status -- those kernels and their outputs are untouched by this file.
// Mapping as there: lane = candidate c = env * K + k, 64 consecutive candidates are one wavefront; tables are read at wave-uniform addresses.
//   k_clear_joints     grid ceil(B K / 64).  Walks the body table, reads the stored poses and leaves world axis and anchor of every controlled column in the joint
//                      store [col][6][B K].  It has no attachment branch: controlled joints sit on ordinary moved bodies only.
//   k_clear_grad       grid ceil(B K / 64).  Each lane reads ITS OWN result, the bodies of its winning pair (a per-lane gather: the pair differs by lane) and the
//   (_att)             joint store, and writes grad[c][0..n).  _att: which half of a signature word counts is the lane's env's held row.
//   k_clear_cost       grid (pair chunks, ceil(B K / 64)).  The pair loop with distmax = d_safe; cost and the two counts in registers, the gradient in the lane's
//   (_att)             own words of the result, touched only by the pairs inside d_safe (rsim_grad_core.h cost_pairs).  One chunk writes the results; several
//   k_clear_cost_sum   write partial results, which a last small pass adds in chunk order.  No atomics: a repeat call is bit-identical.
// Every loop is bounded by a table length, max_iters, a vertex count or RSIM_JNT_MAX.  No LDS, no barrier, no private segment.
#include <hip/hip_runtime.h>
#include "../../include/rsim.h"
#include "rsim_grad.h"
#include "rsim_grad_core.h"

using namespace rsim_grad;
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
__device__ __forceinline__ Att attachments(const DClear& a, int c) { return att_of_env(a.natt, a.held, a.rel, a.body_sig, a.body_att, c / a.K); }

template <bool ATT>
__device__ __forceinline__ void clear_grad_lane(const DGrad& a) {
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  if (c >= a.c.NC) return;
  const int pair = a.c.pair[c];
  const float* f = a.c.fromto + 6 * (size_t)c;
  int b1 = 0, b2 = 0;
  if (pair >= 0) {   // the winning pair differs by lane: a gather
    const int* rec = a.c.pairs + (size_t)pair * RSIM_DIST_REC;
    b1 = a.c.geom[rec[0]].body; b2 = a.c.geom[rec[1]].body;
  }
  unsigned held = 0u;
  if (ATT) held = attachments(a.c, c).held;
  clear_grad(joints(a, c), a.c.n, a.slide_mask, a.c.dist[c], pair, a.c.status[c], ld3(f), ld3(f + 3), b1, b2, a.sig, ATT ? a.c.body_att : nullptr, held,
             a.grad + (size_t)c * a.c.n);
}

template <bool ATT>
__device__ __forceinline__ void clear_cost_lane(const DGrad& a) {
  const int chunk = (int)blockIdx.x;
  const int c = (int)blockIdx.y * RSIM_CLEAR_LANES + (int)threadIdx.x;
  if (c >= a.c.NC) return;
  const int n = a.c.n;
  const int per = (a.c.npair + a.c.chunks - 1) / a.c.chunks;
  const int p0 = chunk * per, p1 = min(a.c.npair, p0 + per);
  Scene<DRayGeom> sc;
  sc.geom = a.c.geom; sc.pairs = a.c.pairs; sc.rec = RSIM_DIST_REC; sc.slot_of_body = a.c.slot_of_body; sc.mesh_vert = a.c.mesh_vert;
  sc.fo_size = a.c.fo_size; sc.fo_pos = a.c.fo_pos; sc.fo_quat = a.c.fo_quat;
  Att at = {0u, nullptr, nullptr, nullptr};
  if (ATT) at = attachments(a.c, c);
  const size_t nc = (size_t)a.c.NC;
  float* w = a.c.chunks > 1 ? a.cpart + (size_t)chunk * (RSIM_GRAD_PART + n) * nc + c : nullptr;
  GradAcc ga;   // the lane's own words: of the chunk's partial result, or of the output
  ga.g = w ? w + RSIM_GRAD_PART * nc : a.grad + (size_t)c * n; ga.gs = w ? nc : 1;
  const Cost r = cost_pairs<ATT>(sc, p0, p1, candidate(a.c, c), scratch(a.c, c), joints(a, c), n, a.slide_mask, a.d_safe, a.c.tol, a.c.max_iters, at, a.sig,
                                 a.c.body_att, ga);
  if (w) {
    w[0] = r.cost; w[nc] = __int_as_float(r.nnear); w[2 * nc] = __int_as_float(r.nover);
    return;
  }
  a.cost[c] = r.cost;
  if (a.nnear) a.nnear[c] = r.nnear;
  if (a.nover) a.nover[c] = r.nover;
}
}  // namespace

__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_clear_joints(DGrad a) {
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  if (c >= a.c.NC) return;
  joint_walk(a.c.tab, a.c.nel, candidate(a.c, c), scratch(a.c, c), joints(a, c));
}
__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_clear_grad(DGrad a) { clear_grad_lane<false>(a); }
__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_clear_grad_att(DGrad a) { clear_grad_lane<true>(a); }
__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_clear_cost(DGrad a) { clear_cost_lane<false>(a); }
__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_clear_cost_att(DGrad a) { clear_cost_lane<true>(a); }

__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_clear_cost_sum(DGrad a) {
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  if (c >= a.c.NC) return;
  const int n = a.c.n;
  const size_t nc = (size_t)a.c.NC, stride = (size_t)(RSIM_GRAD_PART + n) * nc;
  float cost = 0.f;
  int nnear = 0, nover = 0;
  for (int k = 0; k < a.c.chunks; k++) {   // chunk order: the same sum in every call
    const float* w = a.cpart + (size_t)k * stride + c;
    cost += w[0]; nnear += __float_as_int(w[nc]); nover += __float_as_int(w[2 * nc]);
  }
  a.cost[c] = cost;
  if (a.nnear) a.nnear[c] = nnear;
  if (a.nover) a.nover[c] = nover;
  for (int col = 0; col < n; col++) {
    float g = 0.f;
    for (int k = 0; k < a.c.chunks; k++) g += a.cpart[(size_t)k * stride + (RSIM_GRAD_PART + col) * nc + c];
    a.grad[(size_t)c * n + col] = g;
  }
}

extern "C" int rsim_launch_clear_joints(const DGrad* a, hipStream_t stream) {
  if (a->c.NC <= 0 || a->c.nel <= 0) return 0;
  hipLaunchKernelGGL(k_clear_joints, dim3((a->c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}

extern "C" int rsim_launch_clear_grad(const DGrad* a, hipStream_t stream) {
  if (a->c.NC <= 0) return 0;
  hipLaunchKernelGGL(a->c.natt > 0 ? k_clear_grad_att : k_clear_grad, dim3((a->c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), 0, stream,
                     *a);
  return (int)hipGetLastError();
}

extern "C" int rsim_launch_clear_cost(const DGrad* a, hipStream_t stream) {
  if (a->c.NC <= 0 || a->c.npair <= 0 || a->c.chunks <= 0) return 0;
  const int waves = (a->c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES;
  hipLaunchKernelGGL(a->c.natt > 0 ? k_clear_cost_att : k_clear_cost, dim3(a->c.chunks, waves), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  int e = (int)hipGetLastError();
  if (e || a->c.chunks == 1) return e;
  hipLaunchKernelGGL(k_clear_cost_sum, dim3(waves), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}

extern "C" int rsim_launch_clear_cost_sum(const DGrad* a, hipStream_t stream) {
  if (a->c.NC <= 0 || a->c.npair <= 0 || a->c.chunks <= 1) return 0;
  hipLaunchKernelGGL(k_clear_cost_sum, dim3((a->c.NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}
