// rsim_dist.hip -- signed distance and nearest points of geom pairs, for the whole batch, on the device: rsim_geom_distance (include/rsim.h), MuJoCo's
// mj_geomDistance with this project's status codes.  The per-pair algorithm -- GJK on the Minkowski difference of the two cores -- is rsim_dist_core.h,
// shared with the host rehearsal (tests/san/dist_core_driver.cpp); robosuite_amd/distance.py is the fp64 host mirror the kernel is tested against.
//
// Like k_ray and k_ik this is a kernel in a code object of its own that takes everything as its own kernel argument: the step kernels, DModel and DBatch do
// not know of it, and a batch that never asks launches and allocates nothing.
//
// Mapping: lane = env.  One 64-lane workgroup is one pair for 64 consecutive envs; the grid is (pairs, ceil(B / 64)).  The two geom types are the same in
// every lane, so the type dispatch inside the support functions is wave-uniform; only poses and float-table entries differ per lane.  Hull vertices are
// shared by the envs and are read at wave-uniform addresses (the pair record is made uniform with readfirstlane, the scan index is a loop counter): every
// lane scans the hull serially against its own direction, no LDS, no barrier.  Lanes whose iteration has ended wait for the slowest lane of their wavefront;
// every loop is bounded by max_iters or a vertex count.
#include <hip/hip_runtime.h>
#include "../../include/rsim.h"
#include "rsim_dist.h"
#include "rsim_dist_core.h"

using namespace rsim_dist;

namespace {
// world pose of geom g in this lane's env; the position is left absolute (the caller subtracts the pair's origin)
__device__ __forceinline__ Geom load_geom(const DDist& a, int g, const float* ft, const float* xpos, const float* xquat, int vadr, int vnum) {
  const DRayGeom& s = a.geom[g];
  V3 size = ld3(s.size), lp = ld3(s.pos);
  Q4 lq = ldq(s.quat);
  if (s.cg >= 0) { size = ld3(ft + a.fo_size + 3 * s.cg); lp = ld3(ft + a.fo_pos + 3 * s.cg); lq = ldq(ft + a.fo_quat + 4 * s.cg); }
  const Q4 bq = ldq(xquat + 4 * s.body);
  return make_geom(s.type, size, ld3(xpos + 3 * s.body) + qrot(bq, lp), qunit(qmul(bq, lq)), a.mesh_vert + 3 * (size_t)vadr, vnum);
}
}  // namespace

__global__ __launch_bounds__(RSIM_DIST_LANES) void k_dist(DDist a) {
  const int pair = (int)blockIdx.x;
  const int env = (int)blockIdx.y * RSIM_DIST_LANES + (int)threadIdx.x;
  const bool active = env < a.B;
  const int e = active ? env : a.B - 1;   // an idle lane of the last block redoes the last env and writes nothing
  const int* rec = a.pairs + (size_t)pair * RSIM_DIST_REC;
  const int g1 = __builtin_amdgcn_readfirstlane(rec[0]), g2 = __builtin_amdgcn_readfirstlane(rec[1]);
  const int adr1 = __builtin_amdgcn_readfirstlane(rec[2]), num1 = __builtin_amdgcn_readfirstlane(rec[3]);
  const int adr2 = __builtin_amdgcn_readfirstlane(rec[4]), num2 = __builtin_amdgcn_readfirstlane(rec[5]);
  const float* ft = a.ft + (size_t)e * a.fstride;
  const float* xpos = a.xpos + (size_t)e * a.nbody * 3;
  const float* xquat = a.xquat + (size_t)e * a.nbody * 4;
  Geom A = load_geom(a, g1, ft, xpos, xquat, adr1, num1), Bg = load_geom(a, g2, ft, xpos, xquat, adr2, num2);
  const V3 org = A.p;
  A.p = v3(0, 0, 0); Bg.p = Bg.p - org;
  const Result r = pair_distance(A, Bg, a.distmax, a.tol, a.max_iters);
  if (!active) return;
  const size_t o = (size_t)env * a.npair + pair;
  const bool far = (r.status & DIST_FAR) != 0;
  a.dist[o] = r.dist;
  if (a.status) a.status[o] = r.status;
  if (a.fromto) {
    const V3 p1 = far ? v3(0, 0, 0) : r.p1 + org, p2 = far ? v3(0, 0, 0) : r.p2 + org;
    float* f = a.fromto + 6 * o;
    f[0] = p1.x; f[1] = p1.y; f[2] = p1.z; f[3] = p2.x; f[4] = p2.y; f[5] = p2.z;
  }
}

extern "C" int rsim_launch_dist(const DDist* a, hipStream_t stream) {
  if (a->B <= 0 || a->npair <= 0) return 0;
  hipLaunchKernelGGL(k_dist, dim3(a->npair, (a->B + RSIM_DIST_LANES - 1) / RSIM_DIST_LANES), dim3(RSIM_DIST_LANES), 0, stream, *a);
  return (int)hipGetLastError();
}
