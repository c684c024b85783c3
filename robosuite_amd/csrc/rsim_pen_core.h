// rsim_pen_core.h -- the signed distance of OVERLAPPING convex pairs (rsim_geom_distance_signed, k_dist_signed in rsim_pen.hip), as fp32 __host__ __device__
// functions on top of rsim_dist_core.h, which this file does not touch.  The kernel includes this file; so does tests/san/pen_core_driver.cpp, which runs the very
// same fp32 code on the host under AddressSanitizer + UndefinedBehaviorSanitizer.  robosuite_amd/penetration.py is the fp64 mirror and the definition.
//
// delta(n) = h_A(n) + h_B(-n) is the support width of the pair along unit n: how far geom2 must move along n to come free.  The penetration depth is a minimum of
// delta over the directions, the minimiser the contact normal (geom1 -> geom2); the result is dist = -depth, p1 in geom1's support set along +n, p2 = p1 + dist n.
// A descent on delta, each step ONE pair_distance call on geom2 moved by x = (delta(n_k) + offset) n_k: x lies outside the Minkowski difference C = A - B by at
// least `offset`, the call projects it onto C, and the witnesses' direction is the outward normal n_{k+1} of C at the foot.  delta(n_{k+1}) is evaluated with
// the support functions and accepted only if it is smaller.  A LOCAL minimum of the separating translation, never less than the true depth.
//
//  * spheres and capsules enter as their cores, as in pair_distance.  Cores that are apart while a radius reaches the other shape: exact, no descent
//    (dist = d_core - rsum, n from the core witnesses).  Cores that overlap: the descent on the cores, dist = -(delta_core + rsum);
//  * seed: least delta among 13 candidates -- geom1's position to geom2's, the +- axes of geom1, of geom2; the first smallest wins -- tilted by PEN_TILT, since an
//    exact axis of an ellipsoid or cylinder is a saddle of delta;
//  * stop: the moved pair overlaps or is within pen_tol of touching; delta does not decrease; it decreased by no more than pen_tol; pen_iters projections
//    (DIST_PEN_CAP: still a valid directional depth, dist = -delta(n) of the returned n);
//  * the projection's gap tolerance is pen_tol * offset (penetration.py says why); one that ends at max_iters is used as it is, guarded by the decrease test;
//  * house rules of the core below: no arrays indexed at run time, selects instead of struct copies, coordinates relative to geom1.
#pragma once
#include "rsim_dist_core.h"

namespace rsim_dist {
enum { DIST_PEN_CAP = 512 };                 // include/rsim.h RSIM_DIST_PEN_CAP
constexpr float PEN_TILT = 1e-3f;            // rad, to first order
constexpr float PEN_TILT_A = 0.8f, PEN_TILT_B = 0.6f;   // its direction in the plane across the seed: oblique to every axis
constexpr float PEN_BIG = 1e30f;             // a distmax no pair reaches

struct PenOpts { float pen_tol; int pen_iters; float offset; };

// the geom as its core: a sphere or capsule with radius zero
RSIM_HD Geom core_of(const Geom& g) {
  Geom c = g;
  c.size.x = round_core(g) ? 0.f : g.size.x;
  return c;
}
// delta(n) of two geoms' CORES along unit n, and the core1 support point it used
RSIM_HD float core_width(const Geom& c1, const Geom& c2, V3 n, V3& a) {
  a = support(c1, n);
  return dot(n, a - support(c2, -n));
}
// delta(n) of the two solids
RSIM_HD float support_width(const Geom& g1, const Geom& g2, V3 n) {
  V3 a;
  return core_width(g1, g2, n, a) + radius(g1) + radius(g2);
}
RSIM_HD V3 unit(V3 v) { return v * (1.f / sqrtf(dot(v, v))); }
RSIM_HD void seed_try(const Geom& c1, const Geom& c2, V3 n, V3& best, float& bw) {
  V3 a;
  const float w = core_width(c1, c2, n, a);
  const bool take = w < bw;
  bw = take ? w : bw; best = sel(take, n, best);
}
// unit n turned by PEN_TILT towards A t1 + B t2: t1 = n x e / |n x e| for the world axis e along which |n| is smallest (x before y before z), t2 = n x t1
RSIM_HD V3 tilted(V3 n) {
  const float ax = fabsf(n.x), ay = fabsf(n.y), az = fabsf(n.z);
  const bool kx = ax <= ay && ax <= az, ky = !kx && ay <= az;
  const V3 e = v3(kx ? 1.f : 0.f, ky ? 1.f : 0.f, (!kx && !ky) ? 1.f : 0.f);
  const V3 t1 = unit(cross(n, e)), t2 = cross(n, t1);
  return unit(n + (t1 * PEN_TILT_A + t2 * PEN_TILT_B) * PEN_TILT);
}
RSIM_HD V3 seed(const Geom& g1, const Geom& g2) {
  const Geom c1 = core_of(g1), c2 = core_of(g2);
  V3 d0 = g2.p - g1.p;
  const float dd = dot(d0, d0);
  d0 = dd > 0.f ? d0 * (1.f / sqrtf(dd)) : v3(1, 0, 0);
  V3 best = d0;
  float bw = 3.0e38f;
  seed_try(c1, c2, d0, best, bw);
  seed_try(c1, c2, g1.ex, best, bw); seed_try(c1, c2, -g1.ex, best, bw);
  seed_try(c1, c2, g1.ey, best, bw); seed_try(c1, c2, -g1.ey, best, bw);
  seed_try(c1, c2, g1.ez, best, bw); seed_try(c1, c2, -g1.ez, best, bw);
  seed_try(c1, c2, g2.ex, best, bw); seed_try(c1, c2, -g2.ex, best, bw);
  seed_try(c1, c2, g2.ey, best, bw); seed_try(c1, c2, -g2.ey, best, bw);
  seed_try(c1, c2, g2.ez, best, bw); seed_try(c1, c2, -g2.ez, best, bw);
  return tilted(best);
}

// pair_distance with every overlap signed.  steps (may be null): the projections made, 0 for a pair that did not descend.  normal (may be null): the unit n of
// an overlap this routine signed, zero otherwise -- the host rehearsal reads it; a caller of the kernels forms (p2 - p1) / dist.
RSIM_HD Result pair_signed(const Geom& g1, const Geom& g2, float distmax, float tol, int max_iters, PenOpts po, int* steps = nullptr, V3* normal = nullptr) {
  Result out = pair_distance(g1, g2, distmax, tol, max_iters);
  if (steps) *steps = 0;
  if (normal) *normal = v3(0, 0, 0);
  if (!(out.status & DIST_OVERLAP)) return out;
  const float r1 = radius(g1), r2 = radius(g2), rsum = r1 + r2;
  const Geom c1 = core_of(g1);
  Geom c2 = core_of(g2);
  if (rsum > 0.f) {
    const Result rc = pair_distance(c1, c2, PEN_BIG, tol, max_iters);
    if (!(rc.status & DIST_OVERLAP)) {           // the cores are apart: exact, as a sphere against a capsule is
      const V3 n = unit(rc.p2 - rc.p1);
      out.dist = rc.dist - rsum; out.status = rc.status & DIST_CAP;
      out.p1 = rc.p1 + n * r1; out.p2 = rc.p2 - n * r2;
      if (normal) *normal = n;
      return out;
    }
  }
  V3 n = seed(g1, g2), a;
  float w = core_width(c1, c2, n, a);
  const V3 p2 = c2.p;
  const float gap = po.pen_tol * po.offset;
  bool capped = true;
  int k = 0;
  while (k < po.pen_iters) {
    const V3 x = n * (w + po.offset);
    c2.p = p2 + x;
    const Result r = pair_distance(c1, c2, PEN_BIG, gap, max_iters);
    k++;
    if ((r.status & DIST_OVERLAP) || !(r.dist > po.pen_tol)) { capped = false; break; }
    const V3 n2 = unit(r.p2 - r.p1);
    c2.p = p2;
    V3 a2;
    const float w2 = core_width(c1, c2, n2, a2);
    if (!(w2 < w)) { capped = false; break; }
    const bool small = w - w2 <= po.pen_tol;
    n = n2; w = w2; a = r.p1;
    if (small) { capped = false; break; }
  }
  if (steps) *steps = k;
  if (normal) *normal = n;
  out.dist = -(w + rsum);
  out.status = capped ? (int)DIST_PEN_CAP : (int)DIST_OK;
  out.p1 = a + n * r1;
  out.p2 = out.p1 + n * out.dist;
  return out;
}
}  // namespace rsim_dist
