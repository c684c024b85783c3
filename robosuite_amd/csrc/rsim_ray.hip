// rsim_ray.hip -- ray casting against the scene, for the whole batch, on the device: ray queries (rsim_ray), depth / geom-id images (rsim_render_depth)
// and the rangefinder sensor (RSIM_SENSORDATA) are this one routine.
//
// Semantics: MuJoCo's mj_ray / mju_rayGeom [3P, docs "API reference: ray collisions", "XML reference: sensor/rangefinder"; written from the documentation
// and from memory, no MuJoCo source was at hand].  The result is the nearest surface point at t >= 0 along origin + t dir (dir need not be unit length, t is
// in units of |dir|); a ray that starts inside a solid reports where it leaves it; a plane is hit only from its +Z side by a ray travelling towards -Z, and a
// non-zero size[0] / size[1] bounds the hit; a geom is skipped when its alpha is 0, its group is not in geomgroup (0 = all groups), it sits on the world
// body and flg_static == 0, or its body is bodyexclude; ties between geoms go to the lower geom id; a miss reports `miss` and geom id -1.
// A MESH GEOM IS ITS CONVEX HULL -- the geometry this simulator collides with -- given as face planes n . x <= d (rsim_api.cpp ray_scene).
//
// Every solid here is convex, so the line meets it in one interval [tn, tf]: the hit is tn if tn >= 0, else tf if tf >= 0 (the start is inside), else none.
//
// Like k_sensors this is a kernel in a code object of its own that takes everything as its own kernel argument: the step kernels, DModel and DBatch do not
// know of it, and a batch that never casts a ray launches and allocates nothing.  robosuite_amd/raycast.py is the fp64 host mirror it is tested against.
//
// One workgroup = one env x a tile of that env's rays, one ray per lane.  The prologue of every chunk of RSIM_RAY_CHUNK geoms turns the env's geoms into
// world position + 3 x 3 rotation + bounding sphere + filter verdict once, in LDS; the main loop walks the chunk in geom order, every lane reading the same
// record (equal LDS addresses broadcast: no bank conflicts).  A lane whose ray misses the geom's bounding sphere sits the geom out, and a geom no lane of
// the wavefront wants (__ballot) is skipped by the whole wavefront.  The hull planes are read at a wave-uniform address.
#include <hip/hip_runtime.h>
#include "../../include/rsim.h"
#include "rsim_ray.h"
#include "rsim_vec.h"

namespace {
using namespace rsim_vec;
struct Iv { float n, f; };   // parameter interval of a line inside a convex solid; n > f: empty

constexpr float BIG = 3.0e38f;
constexpr float PAR = 1e-14f;   // a direction component below sqrt(PAR) |dir| counts as parallel (far below what fp32 resolves of a direction)
__device__ __forceinline__ Iv none() { Iv r = {1.f, -1.f}; return r; }

// roots of a t^2 + 2 b t + c = 0 in the form that does not cancel: q = -(b + sign(b) sqrt(b^2 - a c)), roots q / a and c / q
__device__ __forceinline__ Iv quad(float a, float b, float c) {
  const float disc = b * b - a * c;
  if (!(disc >= 0.f) || !(a > 0.f)) return none();
  const float s = sqrtf(disc);
  Iv r;
  if (b < 0.f) { const float q = s - b; r.f = q / a; r.n = c / q; }
  else { const float q = -(b + s); r.n = q / a; r.f = q != 0.f ? c / q : r.n; }
  return r;
}
__device__ __forceinline__ Iv sphere(V3 p, V3 d, float r) { return quad(dot(d, d), dot(p, d), dot(p, p) - r * r); }
__device__ __forceinline__ void slab(float p, float d, float h, float dd, Iv& r) {   // |p + t d| <= h
  if (d * d <= PAR * dd) { if (fabsf(p) > h) r = none(); return; }
  const float a = (-h - p) / d, b = (h - p) / d;
  r.n = fmaxf(r.n, fminf(a, b)); r.f = fminf(r.f, fmaxf(a, b));
}
__device__ __forceinline__ Iv box(V3 p, V3 d, V3 s) {
  const float dd = dot(d, d);
  Iv r = {-BIG, BIG};
  slab(p.x, d.x, s.x, dd, r); slab(p.y, d.y, s.y, dd, r); slab(p.z, d.z, s.z, dd, r);
  return r;
}
// cylinder of radius r about Z, |z| <= h
__device__ __forceinline__ Iv cylinder(V3 p, V3 d, float r, float h) {
  const float dd = dot(d, d), a = d.x * d.x + d.y * d.y, c = p.x * p.x + p.y * p.y - r * r;
  Iv s = {-BIG, BIG};
  if (a <= PAR * dd) { if (c > 0.f) return none(); }
  else { s = quad(a, p.x * d.x + p.y * d.y, c); if (s.n > s.f) return s; }
  slab(p.z, d.z, h, dd, s);
  return s;
}
__device__ __forceinline__ void join(Iv& r, Iv s) { if (s.n <= s.f) { r.n = fminf(r.n, s.n); r.f = fmaxf(r.f, s.f); } }
// capsule: the cylinder and the two end spheres overlap pairwise inside the solid, so the union of their intervals is the capsule's
__device__ __forceinline__ Iv capsule(V3 p, V3 d, float r, float h) {
  Iv u = {BIG, -BIG};
  join(u, cylinder(p, d, r, h));
  join(u, sphere(v3(p.x, p.y, p.z - h), d, r));
  join(u, sphere(v3(p.x, p.y, p.z + h), d, r));
  return u;
}
// plane z = 0, solid below: hit only from above by a ray going down; size bounds the hit where non-zero
__device__ __forceinline__ Iv plane(V3 p, V3 d, V3 s) {
  if (!(d.z < 0.f) || p.z < 0.f) return none();
  const float t = -p.z / d.z;
  const float x = p.x + t * d.x, y = p.y + t * d.y;
  if ((s.x > 0.f && fabsf(x) > s.x) || (s.y > 0.f && fabsf(y) > s.y)) return none();
  Iv r = {t, t};
  return r;
}
// convex hull as planes n . x <= d: the largest entering and the smallest leaving parameter
__device__ __forceinline__ Iv hull(V3 p, V3 d, const float* __restrict__ pl, int n) {
  Iv r = {-BIG, BIG};
  const float dd = dot(d, d);
  for (int k = 0; k < n; k++) {
    const float4 q = *(const float4*)(pl + 4 * k);
    const float den = q.x * d.x + q.y * d.y + q.z * d.z, num = q.w - (q.x * p.x + q.y * p.y + q.z * p.z);
    if (den * den <= PAR * dd) { if (num < 0.f) return none(); continue; }
    const float t = num / den;
    if (den < 0.f) r.n = fmaxf(r.n, t); else r.f = fminf(r.f, t);
  }
  return r;
}
}  // namespace

__global__ __launch_bounds__(RSIM_RAY_TILE) void k_ray(DRay a) {
  __shared__ __attribute__((aligned(16))) float G[RSIM_RAY_CHUNK * RSIM_RAY_REC];
  const int env = (int)blockIdx.y, tid = (int)threadIdx.x, nt = (int)blockDim.x;
  const int r = (int)blockIdx.x * nt + tid;
  const float* ft = a.ft + (size_t)env * a.fstride;
  const float* xpos = a.xpos + (size_t)env * a.nbody * 3;
  const float* xquat = a.xquat + (size_t)env * a.nbody * 4;

  // ---- this lane's ray
  bool active = r < a.n;
  V3 o = v3(0, 0, 0), d = v3(0, 0, -1);
  int excl = a.bodyexclude;
  size_t out = (size_t)env * a.n + (active ? r : 0);
  if (a.mode == RAY_ARRAYS) {
    if (active) { o = ld3(a.origin + out * 3); d = ld3(a.dir + out * 3); }
  } else if (a.mode == RAY_CAMERA) {
    // pixel centres, row 0 at the top: (aspect tan(fovy / 2) (2 (c + 1/2) / W - 1), tan(fovy / 2) (1 - 2 (r + 1/2) / H), -1) in the camera frame, so t is the
    // metric depth along the optical axis
    const Q4 bq = ldq(xquat + 4 * a.cam_body);
    const Q4 cq = qunit(qmul(bq, ldq(a.cam_quat)));
    o = ld3(xpos + 3 * a.cam_body) + qrot(bq, ld3(a.cam_pos));
    const int row = (active ? r : 0) / a.W, col = (active ? r : 0) - row * a.W;
    const float aspect = (float)a.W / (float)a.H;
    d = qrot(cq, v3(aspect * a.tanhalf * ((2.f * col + 1.f) / a.W - 1.f), a.tanhalf * (1.f - (2.f * row + 1.f) / a.H), -1.f));
  } else {
    // rangefinder: lane = sensor; from the site along its +Z, the site's own body excluded
    const int site = active ? a.rf[r] : -1;
    active = site >= 0;
    if (active) {
      excl = a.rf[a.n + r];
      out = (size_t)env * a.nsensordata + a.rf[2 * a.n + r];
      const Q4 bq = ldq(xquat + 4 * excl);
      o = ld3(xpos + 3 * excl) + qrot(bq, ld3(ft + a.fo_site_pos + 3 * site));
      d = qrot(qunit(qmul(bq, ldq(ft + a.fo_site_quat + 4 * site))), v3(0, 0, 1));
    }
  }
  const float dd = dot(d, d);
  float best = BIG;
  int bestg = -1;

  for (int g0 = 0; g0 < a.ngeom; g0 += RSIM_RAY_CHUNK) {
    const int ng = min(RSIM_RAY_CHUNK, a.ngeom - g0);
    __syncthreads();   // the chunk before has been walked by every wavefront
    // ---- prologue: world pose, bounding sphere and filter verdict of the chunk's geoms, once per workgroup
    for (int k = tid; k < ng; k += nt) {
      const DRayGeom& s = a.geom[g0 + k];
      V3 size = ld3(s.size), lp = ld3(s.pos), rc = ld3(s.rcenter);
      Q4 lq = ldq(s.quat);
      float rb = s.rbound;
      if (s.cg >= 0) {
        size = ld3(ft + a.fo_size + 3 * s.cg); lp = ld3(ft + a.fo_pos + 3 * s.cg); lq = ldq(ft + a.fo_quat + 4 * s.cg);
        rc = ld3(ft + a.fo_rcenter + 3 * s.cg); rb = ft[a.fo_rbound + s.cg];
      }
      // bounding radius of a primitive from the size in force (an env may have its own); a mesh keeps its table entry; a plane has none
      if (s.type == 2) rb = size.x;
      else if (s.type == 3) rb = size.x + size.y;
      else if (s.type == 4) rb = fmaxf(size.x, fmaxf(size.y, size.z));
      else if (s.type == 5) rb = sqrtf(size.x * size.x + size.y * size.y);
      else if (s.type == 6) rb = sqrtf(dot(size, size));
      else if (s.type != 7) rb = 0.f;
      const Q4 bq = ldq(xquat + 4 * s.body);
      const Q4 q = qunit(qmul(bq, lq));
      const V3 pos = ld3(xpos + 3 * s.body) + qrot(bq, lp);
      const V3 ex = qrot(q, v3(1, 0, 0)), ey = qrot(q, v3(0, 1, 0)), ez = qrot(q, v3(0, 0, 1));   // columns of R (world = R local + pos)
      const V3 bc = pos + ex * rc.x + ey * rc.y + ez * rc.z;
      const int grp = s.flags >> 8;
      const bool skip = !(s.flags & RAY_VISIBLE) || (a.geomgroup && !((a.geomgroup >> grp) & 1u)) || (s.body == 0 && !a.flg_static) ||
                        s.type < 0 || s.type == 1 || s.type > 7 || (s.type == 7 && s.plane_num <= 0);
      float* w = G + k * RSIM_RAY_REC;
      w[0] = pos.x; w[1] = pos.y; w[2] = pos.z;
      w[3] = ex.x; w[4] = ex.y; w[5] = ex.z; w[6] = ey.x; w[7] = ey.y; w[8] = ey.z; w[9] = ez.x; w[10] = ez.y; w[11] = ez.z;
      w[12] = size.x; w[13] = size.y; w[14] = size.z;
      w[15] = bc.x; w[16] = bc.y; w[17] = bc.z;
      w[18] = rb * 1.0001f + 1e-6f;   // the cull must never drop a hit the exact test would report
      w[19] = __int_as_float(skip ? -1 : s.type);
      w[20] = __int_as_float(s.body); w[21] = __int_as_float(s.plane_adr); w[22] = __int_as_float(s.plane_num); w[23] = 0.f;
    }
    __syncthreads();
    // ---- the chunk's geoms in order, one ray per lane
    for (int k = 0; k < ng; k++) {
      const float* w = G + k * RSIM_RAY_REC;
      const int type = __float_as_int(w[19]);
      if (type < 0) continue;   // (wave-uniform: every lane reads the same record)
      bool want = active && __float_as_int(w[20]) != excl;
      if (want && type != 0) {
        // bounding sphere: the ray's closest approach to the centre lies outside, or the sphere is behind the start
        const V3 m = ld3(w + 15) - o;
        const float rb = w[18], pr = dot(m, d), mm = dot(m, m);
        want = !(mm > rb * rb && (pr < 0.f || mm * dd - pr * pr > rb * rb * dd));
      }
      if (!__ballot(want)) continue;
      if (!want) continue;
      const V3 rel = o - ld3(w);
      const V3 ex = ld3(w + 3), ey = ld3(w + 6), ez = ld3(w + 9), size = ld3(w + 12);
      const V3 p = v3(dot(ex, rel), dot(ey, rel), dot(ez, rel)), dl = v3(dot(ex, d), dot(ey, d), dot(ez, d));   // the ray in the geom frame
      Iv iv;
      if (type == 0) iv = plane(p, dl, size);
      else if (type == 2) iv = sphere(p, dl, size.x);
      else if (type == 3) iv = capsule(p, dl, size.x, size.y);
      else if (type == 4) iv = sphere(v3(p.x / size.x, p.y / size.y, p.z / size.z), v3(dl.x / size.x, dl.y / size.y, dl.z / size.z), 1.f);
      else if (type == 5) iv = cylinder(p, dl, size.x, size.y);
      else if (type == 6) iv = box(p, dl, size);
      else {
        const int adr = __builtin_amdgcn_readfirstlane(__float_as_int(w[21])), num = __builtin_amdgcn_readfirstlane(__float_as_int(w[22]));
        iv = hull(p, dl, a.planes + 4 * (size_t)adr, num);
      }
      if (iv.n <= iv.f) {
        const float t = iv.n >= 0.f ? iv.n : iv.f;
        if (t >= 0.f && t < best) { best = t; bestg = g0 + k; }   // strict: a tie stays with the lower geom id
      }
    }
  }
  if (active) {
    a.dist[out] = bestg >= 0 ? best : a.miss;
    if (a.geomid && a.mode != RAY_RANGEFINDER) a.geomid[out] = bestg;
  }
}

extern "C" int rsim_launch_ray(const DRay* a, hipStream_t stream) {
  if (a->B <= 0 || a->n <= 0) return 0;
  const int nt = a->mode == RAY_RANGEFINDER ? 64 : RSIM_RAY_TILE;   // the rangefinder: one wavefront per env (a model holds at most 64 sensors)
  hipLaunchKernelGGL(k_ray, dim3((a->n + nt - 1) / nt, a->B), dim3(nt), 0, stream, *a);
  return (int)hipGetLastError();
}
