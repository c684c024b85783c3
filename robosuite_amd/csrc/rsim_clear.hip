// rsim_clear.hip -- "is this joint configuration free, and by how much?" for K candidate joint vectors per env, for the whole batch, on the device:
// rsim_config_fk and rsim_config_clearance (include/rsim.h).  The per-candidate code -- FK of the bodies a candidate moves, the pair loop on the GJK core of
// rsim_dist_core.h -- is rsim_clear_core.h, shared with the host rehearsal (tests/san/clear_core_driver.cpp); robosuite_amd/clearance.py is the fp64 host
// mirror the kernels are tested against.
//
// Like k_ray, k_ik and k_dist these are kernels in a code object of their own that take everything as their own kernel argument: the step kernels, DModel
// and DBatch do not know of them.  A pure query: qpos, the float tables and RSIM_XPOS / RSIM_XQUAT are read, the batch's scratch and the outputs are written.
//
// Mapping: lane = candidate c = env * K + k; 64 consecutive candidates are one wavefront, which may span several envs (env = c / K: the float table, qpos and the
// env's poses are per lane).  Tables -- the body table, the pair table, the geom records, hull vertices -- are read at wave-uniform addresses.
//   k_clear_fk    grid ceil(B K / 64).  Walks the body table serially and leaves the poses of the moved bodies in the scratch, [slot][7][B K]: the 64 lanes of a
//                 wavefront touch 64 consecutive floats.  For rsim_config_fk it writes the caller's arrays instead, unmoved bodies copied from the env's poses.
//   k_clear_dist  grid (pair chunks, ceil(B K / 64)).  Each wavefront loops over its chunk of the pair list; each lane hands ITS RUNNING MINIMUM to pair_distance
//                 as distmax, so a pair that cannot beat it leaves at the far exit.  One chunk writes the results; several write partial results,
//   k_clear_min   which a last small pass reduces in chunk order, a strictly smaller distance replacing the minimum: the lowest pair index wins ties.  No atomics.
// Every loop is bounded by a table length, max_iters or a vertex count.  No LDS, no barrier.
// A call with attachments (rsim_attach) runs k_clear_fk_att / k_clear_dist_att: the same bodies with rsim_clear_core.h's ATT branches compiled in -- the walk of
// the attached subtrees and the per-lane skip of the pairs the lane's env does not evaluate.  Same grids, same scratch layout; k_clear_min serves both.  The
// kernels without the suffix are the instantiation with those branches compiled away: what a call without attachments ran before there were any.
#include <hip/hip_runtime.h>
#include "../../include/rsim.h"
#include "rsim_clear.h"
#include "rsim_clear_core.h"

using namespace rsim_clear;

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
// the lane's env's view of the attachments (rsim_clear_core.h att_of_env)
__device__ __forceinline__ Att attachments(const DClear& a, int c) { return att_of_env(a.natt, a.held, a.rel, a.body_sig, a.body_att, c / a.K); }

template <bool ATT>
__device__ __forceinline__ void clear_fk(const DClear& a) {
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  if (c >= a.NC) return;   // (the loops below have the same trip count in every lane that stays)
  const Cand cd = candidate(a, c);
  const CandQ qv = {cd.q};
  Att at = {0u, nullptr, nullptr, nullptr};
  if (ATT) at = attachments(a, c);
  if (a.xpos_out) {
    PoseStore s;
    s.pos = a.xpos_out + (size_t)c * a.nbody * 3; s.quat = a.xquat_out + (size_t)c * a.nbody * 4;
    s.pe = 3; s.ps = 1; s.qe = 4; s.qs = 1; s.by_body = 1;
    for (int b = 0; b < a.nbody; b++)
      if (__builtin_amdgcn_readfirstlane(a.slot_of_body[b]) < 0) store_pose(s, b, env_pose(cd, b));   // bit for bit the env's pose
    fk_walk<ATT>(a.tab, a.nel, cd, s, qv, at);
  } else {
    fk_walk<ATT>(a.tab, a.nel, cd, scratch(a, c), qv, at);
  }
}

template <bool ATT>
__device__ __forceinline__ void clear_dist(const DClear& a) {
  const int chunk = (int)blockIdx.x;
  const int c = (int)blockIdx.y * RSIM_CLEAR_LANES + (int)threadIdx.x;
  if (c >= a.NC) return;
  const int per = (a.npair + a.chunks - 1) / a.chunks;
  const int p0 = chunk * per, p1 = min(a.npair, p0 + per);
  Scene<DRayGeom> sc;
  sc.geom = a.geom; sc.pairs = a.pairs; sc.rec = RSIM_DIST_REC; sc.slot_of_body = a.slot_of_body; sc.mesh_vert = a.mesh_vert;
  sc.fo_size = a.fo_size; sc.fo_pos = a.fo_pos; sc.fo_quat = a.fo_quat;
  Att at = {0u, nullptr, nullptr, nullptr};
  if (ATT) at = attachments(a, c);
  const Best r = clear_pairs<ATT>(sc, p0, p1, candidate(a, c), scratch(a, c), a.distmax, a.tol, a.max_iters, at);
  if (a.chunks > 1) {
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

}  // namespace

__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_clear_fk(DClear a) { clear_fk<false>(a); }
__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_clear_fk_att(DClear a) { clear_fk<true>(a); }
__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_clear_dist(DClear a) { clear_dist<false>(a); }
__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_clear_dist_att(DClear a) { clear_dist<true>(a); }

__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_clear_min(DClear a) {
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  if (c >= a.NC) return;
  const size_t nc = (size_t)a.NC;
  float best = a.distmax;
  int from = -1;
  for (int k = 0; k < a.chunks; k++) {      // chunk order = pair order: a tie keeps the earlier pair
    const float* w = a.part + (size_t)k * RSIM_CLEAR_PART * nc + c;
    const bool take = __float_as_int(w[nc]) >= 0 && w[0] < best;
    best = take ? w[0] : best; from = take ? k : from;
  }
  const float* w = a.part + (size_t)(from < 0 ? 0 : from) * RSIM_CLEAR_PART * nc + c;
  a.dist[c] = best;
  a.pair[c] = from < 0 ? -1 : __float_as_int(w[nc]);
  if (a.status) a.status[c] = from < 0 ? (int)rsim_dist::DIST_FAR : __float_as_int(w[2 * nc]);
  if (a.fromto) {
    float* f = a.fromto + 6 * (size_t)c;
    for (int k = 0; k < 6; k++) f[k] = from < 0 ? 0.f : w[(3 + k) * nc];
  }
}

extern "C" int rsim_launch_clear_fk(const DClear* a, hipStream_t stream) {
  if (a->NC <= 0 || a->nel <= 0) return 0;
  hipLaunchKernelGGL(a->natt > 0 ? k_clear_fk_att : k_clear_fk, dim3((a->NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}

extern "C" int rsim_launch_clear_dist(const DClear* a, hipStream_t stream) {
  if (a->NC <= 0 || a->npair <= 0 || a->chunks <= 0) return 0;
  const int waves = (a->NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES;
  hipLaunchKernelGGL(a->natt > 0 ? k_clear_dist_att : k_clear_dist, dim3(a->chunks, waves), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  int e = (int)hipGetLastError();
  if (e || a->chunks == 1) return e;
  hipLaunchKernelGGL(k_clear_min, dim3(waves), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}

// k_clear_min alone, behind a pair loop that another code object ran (rsim_pen_query.hip k_clear_dist_signed); nothing with chunks <= 1
extern "C" int rsim_launch_clear_min(const DClear* a, hipStream_t stream) {
  if (a->NC <= 0 || a->npair <= 0 || a->chunks <= 1) return 0;
  hipLaunchKernelGGL(k_clear_min, dim3((a->NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}
