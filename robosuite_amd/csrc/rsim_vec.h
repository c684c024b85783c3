// rsim_vec.h -- the fp32 vector / quaternion small math of every kernel: V3, Q4, their arithmetic, loads, quaternion product / unit / rotation and sincos_f, as
// __host__ __device__ functions in namespace rsim_vec.  Included by rsim_step.hip, rsim_sensors.hip, rsim_ray.hip, rsim_ik.hip and rsim_dist_core.h (and through
// it by rsim_clear_core.h, rsim_sweep_core.h, their kernels and the host drivers under tests/san/, which compile it with plain g++).
//
// ONE copy: the clearance, sweep and IK queries are specified as agreeing with the step kernel's FK, and that holds because they all take these very functions.
// Editing a body here -- the order of an expression included -- changes the bits of EVERY kernel: run tools/isa_compare.sh against the parent and the GPU suite.
#pragma once
#include <math.h>
#if defined(__HIPCC__)
#define RSIM_HD __host__ __device__ __forceinline__
#else
#define RSIM_HD inline
#endif

namespace rsim_vec {
struct V3 { float x, y, z; };
struct Q4 { float w, x, y, z; };
RSIM_HD V3 v3(float x, float y, float z) { V3 r = {x, y, z}; return r; }
RSIM_HD V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
RSIM_HD V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
RSIM_HD V3 operator-(V3 a) { return v3(-a.x, -a.y, -a.z); }
RSIM_HD V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
RSIM_HD float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
RSIM_HD V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
RSIM_HD V3 ld3(const float* p) { return v3(p[0], p[1], p[2]); }
RSIM_HD Q4 ldq(const float* p) { Q4 q = {p[0], p[1], p[2], p[3]}; return q; }
RSIM_HD Q4 qmul(Q4 a, Q4 b) {
  Q4 r = {a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
          a.w * b.y - a.x * b.z + a.y * b.w + a.z * b.x, a.w * b.z + a.x * b.y - a.y * b.x + a.z * b.w};
  return r;
}
RSIM_HD Q4 qunit(Q4 q) {
  const float n = 1.f / sqrtf(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  Q4 r = {q.w * n, q.x * n, q.y * n, q.z * n};
  return r;
}
RSIM_HD V3 qrot(Q4 q, V3 v) {   // v rotated by the unit quaternion q: v + 2 w (u x v) + 2 u x (u x v)
  const V3 u = v3(q.x, q.y, q.z);
  const V3 t = cross(u, v) * 2.f;
  return v + t * q.w + cross(u, t);
}
// sin and cos of a bounded angle (|x| < ~1e3): Cody-Waite reduction to [-pi/4, pi/4] + Taylor kernels (abs error < 2e-7)
RSIM_HD void sincos_f(float x, float& sn, float& cs) {
  const float k = rintf(x * 0.636619772367581343f);
  float r = fmaf(-k, 1.57079625129699707031f, x);
  r = fmaf(-k, 7.54978941586159635335e-08f, r);
  const float r2 = r * r;
  const float sp = r * fmaf(r2, fmaf(r2, fmaf(r2, fmaf(r2, 2.7557319e-6f, -1.9841270e-4f), 8.3333333e-3f), -1.6666667e-1f), 1.0f);
  const float cp = fmaf(r2, fmaf(r2, fmaf(r2, fmaf(r2, fmaf(r2, -2.7557319e-7f, 2.4801587e-5f), -1.3888889e-3f), 4.1666667e-2f), -0.5f), 1.0f);
  const int q = (int)k & 3;
  const float s1 = (q & 1) ? cp : sp, c1 = (q & 1) ? sp : cp;
  sn = (q & 2) ? -s1 : s1;
  cs = ((q + 1) & 2) ? -c1 : c1;
}
}  // namespace rsim_vec
