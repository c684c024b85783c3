// rsim_dist_core.h -- the per-pair core of the geom distance query (rsim_geom_distance, k_dist in rsim_dist.hip): support functions, the closest point of
// a simplex to the origin, and the GJK iteration on the Minkowski difference, as fp32 __host__ __device__ functions.  The kernel includes this file; so does
// tests/san/dist_core_driver.cpp, which runs the very same fp32 code on the host under AddressSanitizer + UndefinedBehaviorSanitizer.
//
// Semantics: MuJoCo's mj_geomDistance [3P, docs "API reference: mj_geomDistance"; written from the documentation, no MuJoCo source was at hand] with this
// project's status codes (include/rsim.h).  Algorithm: Gilbert-Johnson-Keerthi [3P, IEEE J. Robotics and Automation 4(2), 1988] with the sub-simplex search
// by Voronoi-free enumeration: the closest point of a segment / triangle / tetrahedron is the best of its faces' closest points, so a degenerate simplex
// (repeated or collinear support points) falls back to its best lower-dimensional face and nothing divides by a vanishing determinant.
//
//  * all coordinates are relative to geom1's position (Geom.p): centimetre-sized numbers, as geom_support's `org` in rsim_step.hip;
//  * spheres and capsules enter as their cores (a point, a segment); the radii come off at the end: such pairs are exact and signed;
//  * a plane pair takes no iteration: one support call along the plane normal;
//  * every iteration has an upper bound |v| and a lower bound v . w / |v| on the distance of the cores; it stops when their gap is <= tol, when the lower
//    bound proves the pair beyond distmax, when the simplex encloses the origin, when the support point is one the simplex already holds or |v| no longer
//    shrinks (fp32 has nothing left to resolve: the best iterate so far is the answer) or at max_iters (DIST_CAP);
//  * no runtime-indexed arrays: the simplex is four points in named members, compacted by conditional swaps.
#pragma once
#include <math.h>
#include <stdint.h>
#include "rsim_vec.h"

namespace rsim_dist {
using namespace rsim_vec;
RSIM_HD float triple(V3 a, V3 b, V3 c) { return dot(a, cross(b, c)); }

enum { G_PLANE = 0, G_SPHERE = 2, G_CAPSULE = 3, G_ELLIPSOID = 4, G_CYLINDER = 5, G_BOX = 6, G_MESH = 7 };   // mjtGeom
enum { DIST_OK = 0, DIST_FAR = 1, DIST_OVERLAP = 2, DIST_CAP = 256 };                                        // include/rsim.h RSIM_DIST_*

constexpr float DIST_FMIN = 1e-30f;   // a direction shorter than this has no direction
constexpr float DIST_EPS2 = 1e-14f;   // cores closer than 1e-7 m touch: fp32 resolves no less of coordinates this size
constexpr float DIST_DEG = 1e-10f;    // a triangle whose sin^2 of the corner angle is below this is a segment (1e-5 rad)

// one geom of a pair: position relative to the pair's origin, the columns of its rotation (world = R local + p), its size as in geom_size, and -- a mesh --
// its hull vertices in the geom frame.  type, verts and nvert are the same in every lane of a wavefront.
struct Geom { int type; V3 p, ex, ey, ez, size; const float* verts; int nvert; };
struct Result { float dist; V3 p1, p2; int status; };

RSIM_HD Geom make_geom(int type, V3 size, V3 p, Q4 q, const float* verts, int nvert) {
  Geom g;
  g.type = type; g.size = size; g.p = p; g.verts = verts; g.nvert = nvert;
  g.ex = qrot(q, v3(1, 0, 0)); g.ey = qrot(q, v3(0, 1, 0)); g.ez = qrot(q, v3(0, 0, 1));
  return g;
}
RSIM_HD float radius(const Geom& g) { return (g.type == G_SPHERE || g.type == G_CAPSULE) ? g.size.x : 0.f; }
RSIM_HD bool round_core(const Geom& g) { return g.type == G_SPHERE || g.type == G_CAPSULE; }

// support point of the geom's CORE along direction d (need not be unit length): the per-type rules of geom_support (rsim_step.hip); a hull is scanned
// serially, the lowest index wins ties
RSIM_HD V3 support(const Geom& g, V3 d) {
  const V3 ld = v3(dot(g.ex, d), dot(g.ey, d), dot(g.ez, d));
  const V3 h = g.size;
  V3 lp = v3(0, 0, 0);
  if (g.type == G_BOX) lp = v3(ld.x >= 0 ? h.x : -h.x, ld.y >= 0 ? h.y : -h.y, ld.z >= 0 ? h.z : -h.z);
  else if (g.type == G_CAPSULE) lp.z = ld.z >= 0 ? h.y : -h.y;
  else if (g.type == G_CYLINDER) {
    const float n = sqrtf(ld.x * ld.x + ld.y * ld.y);
    if (n > DIST_FMIN) { lp.x = ld.x / n * h.x; lp.y = ld.y / n * h.x; }
    lp.z = ld.z >= 0 ? h.y : -h.y;
  } else if (g.type == G_ELLIPSOID) {
    const V3 t = v3(ld.x * h.x, ld.y * h.y, ld.z * h.z);
    const float n = sqrtf(dot(t, t));
    if (n > DIST_FMIN) lp = v3(t.x / n * h.x, t.y / n * h.y, t.z / n * h.z);
  } else if (g.type == G_MESH) {
    float bv = -3.0e38f;
    for (int i = 0; i < g.nvert; i++) {
      const float x = g.verts[3 * i], y = g.verts[3 * i + 1], z = g.verts[3 * i + 2];
      const float val = x * ld.x + y * ld.y + z * ld.z;
      const bool take = val > bv;
      bv = take ? val : bv; lp.x = take ? x : lp.x; lp.y = take ? y : lp.y; lp.z = take ? z : lp.z;
    }
  }
  return g.p + g.ex * lp.x + g.ey * lp.y + g.ez * lp.z;
}

// ---- closest point of a simplex to the origin, as weights of its vertices ---------------------------------------------------------------------------------
RSIM_HD void seg_closest(V3 a, V3 b, float& la, float& lb, float& d2) {
  const V3 ab = b - a;
  const float den = dot(ab, ab);
  float t = den > 0.f ? -dot(a, ab) / den : 0.f;
  t = fminf(fmaxf(t, 0.f), 1.f);
  la = 1.f - t; lb = t;
  const V3 p = a + ab * t;
  d2 = dot(p, p);
}
RSIM_HD void tri_closest(V3 a, V3 b, V3 c, float& la, float& lb, float& lc, float& d2) {
  float x, y, e;
  seg_closest(a, b, la, lb, d2); lc = 0.f;
  seg_closest(a, c, x, y, e);
  if (e < d2) { la = x; lb = 0.f; lc = y; d2 = e; }
  seg_closest(b, c, x, y, e);
  if (e < d2) { la = 0.f; lb = x; lc = y; d2 = e; }
  // the foot of the origin's perpendicular, where it falls inside a triangle that is one
  const V3 ab = b - a, ac = c - a, n = cross(ab, ac);
  const float nn = dot(n, n);
  if (nn > DIST_DEG * dot(ab, ab) * dot(ac, ac)) {
    const V3 ap = -a;
    const float u = dot(cross(ap, ac), n) / nn, v = dot(cross(ab, ap), n) / nn, w = 1.f - u - v;
    if (u >= 0.f && v >= 0.f && w >= 0.f) {
      const V3 p = a + ab * u + ac * v;
      e = dot(p, p);
      if (e <= d2) { la = w; lb = u; lc = v; d2 = e; }
    }
  }
}

RSIM_HD V3 blend(float l0, V3 p0, float l1, V3 p1, float l2, V3 p2, float l3, V3 p3) { return p0 * l0 + p1 * l1 + p2 * l2 + p3 * l3; }
struct Simplex {
  V3 w0, w1, w2, w3;      // points of the Minkowski difference core1 - core2
  V3 a0, a1, a2, a3;      // the core1 points they came from
  float l0, l1, l2, l3;   // weights of the closest point
  int n;
};
RSIM_HD V3 sel(bool c, V3 a, V3 b) { return v3(c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z); }   // (per component: a select of whole structs goes through memory)
RSIM_HD void cswap(bool c, V3& wa, V3& aa, float& la, V3& wb, V3& ab, float& lb) {
  const V3 tw = wa, ta = aa; const float tl = la;
  wa = sel(c, wb, wa); aa = sel(c, ab, aa); la = c ? lb : la;
  wb = sel(c, tw, wb); ab = sel(c, ta, ab); lb = c ? tl : lb;
}
// closest point of the simplex (its newest point is slot n - 1) to the origin: sets the weights, moves the vertices that carry none behind the others and
// shrinks n to the rest.  Returns true when a tetrahedron encloses the origin (the weights are then the origin's barycentric coordinates).
RSIM_HD bool simplex_closest(Simplex& s) {
  bool inside = false;
  if (s.n == 1) { s.l0 = 1.f; }
  else if (s.n == 2) { float e; seg_closest(s.w0, s.w1, s.l0, s.l1, e); }
  else if (s.n == 3) { float e; tri_closest(s.w0, s.w1, s.w2, s.l0, s.l1, s.l2, e); }
  else {
    const V3 a = s.w0, b = s.w1, c = s.w2, d = s.w3;
    const V3 ab = b - a, ac = c - a, ad = d - a, bc = c - b, bd = d - b;
    const float v6 = triple(ab, ac, ad);
    const float va = triple(-b, bd, bc), vb = triple(-a, ac, ad), vc = triple(-a, ad, ab), vd = triple(-a, ab, ac);
    if (v6 != 0.f && va * v6 >= 0.f && vb * v6 >= 0.f && vc * v6 >= 0.f && vd * v6 >= 0.f) {
      inside = true;
      s.l0 = va / v6; s.l1 = vb / v6; s.l2 = vc / v6; s.l3 = vd / v6;
    } else {
      // the three faces that hold the newest point (the fourth is the simplex the step before already searched)
      float x, y, z, e, d2;
      tri_closest(a, b, d, s.l0, s.l1, s.l3, d2); s.l2 = 0.f;
      tri_closest(a, c, d, x, y, z, e);
      if (e < d2) { s.l0 = x; s.l1 = 0.f; s.l2 = y; s.l3 = z; d2 = e; }
      tri_closest(b, c, d, x, y, z, e);
      if (e < d2) { s.l0 = 0.f; s.l1 = x; s.l2 = y; s.l3 = z; d2 = e; }
    }
  }
  if (s.n < 4) s.l3 = 0.f;
  if (s.n < 3) s.l2 = 0.f;
  if (s.n < 2) s.l1 = 0.f;
  // a bubble network that moves zero weights to the back
  cswap(s.l0 <= 0.f && s.l1 > 0.f, s.w0, s.a0, s.l0, s.w1, s.a1, s.l1);
  cswap(s.l1 <= 0.f && s.l2 > 0.f, s.w1, s.a1, s.l1, s.w2, s.a2, s.l2);
  cswap(s.l2 <= 0.f && s.l3 > 0.f, s.w2, s.a2, s.l2, s.w3, s.a3, s.l3);
  cswap(s.l0 <= 0.f && s.l1 > 0.f, s.w0, s.a0, s.l0, s.w1, s.a1, s.l1);
  cswap(s.l1 <= 0.f && s.l2 > 0.f, s.w1, s.a1, s.l1, s.w2, s.a2, s.l2);
  cswap(s.l0 <= 0.f && s.l1 > 0.f, s.w0, s.a0, s.l0, s.w1, s.a1, s.l1);
  s.n = (s.l0 > 0.f) + (s.l1 > 0.f) + (s.l2 > 0.f) + (s.l3 > 0.f);
  return inside;
}
RSIM_HD bool same(V3 a, V3 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

// The weights of a tetrahedron that encloses the origin, made good.  The triple products behind them cancel, the more the flatter the tetrahedron: they are the
// barycentric coordinates not of the origin but of a point r nearby (7e-7 m seen).  The coordinates are affine in the point, so two rounds of taking off their
// change over r leave a residual of rounding size.  Only an overlap's common point needs this; the iteration does not pass here.
RSIM_HD void refine_enclosing(Simplex& s) {
  const V3 a = s.w0, b = s.w1, c = s.w2, d = s.w3;
  const V3 ab = b - a, ac = c - a, ad = d - a, bc = c - b, bd = d - b;
  const float v6 = triple(ab, ac, ad);
  float l0 = s.l0, l1 = s.l1, l2 = s.l2, l3 = s.l3;
  if (v6 != 0.f) {
    for (int k = 0; k < 2; k++) {
      const float sum = l0 + l1 + l2 + l3;
      l0 /= sum; l1 /= sum; l2 /= sum; l3 /= sum;
      const V3 r = blend(l0, a, l1, b, l2, c, l3, d);
      l0 -= triple(r, bd, bc) / v6; l1 -= triple(r, ac, ad) / v6; l2 -= triple(r, ad, ab) / v6; l3 -= triple(r, ab, ac) / v6;
    }
  }
  l0 = fmaxf(l0, 0.f); l1 = fmaxf(l1, 0.f); l2 = fmaxf(l2, 0.f); l3 = fmaxf(l3, 0.f);
  const float sum = l0 + l1 + l2 + l3;
  if (sum > 0.f) { s.l0 = l0 / sum; s.l1 = l1 / sum; s.l2 = l2 / sum; s.l3 = l3 / sum; }
}

// ---- a plane against any convex shape: exact and signed, no iteration --------------------------------------------------------------------------------------
RSIM_HD Result plane_pair(const Geom& pl, const Geom& o, bool plane_first, float distmax) {
  const V3 n = pl.ez;                                  // the solid is the half-space below the plane's +Z face
  const float r = radius(o);
  const V3 s = support(o, -n) - n * r;                 // the shape's lowest point over the plane
  const float d = dot(n, s - pl.p);
  const V3 q = s - n * d;                              // ... and the plane's point under it
  Result out;
  out.dist = d; out.status = DIST_OK;
  out.p1 = sel(plane_first, q, s); out.p2 = sel(plane_first, s, q);
  if (d > distmax) { out.dist = distmax; out.status = DIST_FAR; }
  return out;
}

// ---- one pair --------------------------------------------------------------------------------------------------------------------------------------------
// Points of the result are relative to the same origin as the geoms; a DIST_FAR result's points mean nothing (the caller writes zeros).
RSIM_HD Result pair_distance(const Geom& g1, const Geom& g2, float distmax, float tol, int max_iters) {
  if (g1.type == G_PLANE) return plane_pair(g1, g2, true, distmax);
  if (g2.type == G_PLANE) return plane_pair(g2, g1, false, distmax);
  const float r1 = radius(g1), r2 = radius(g2), rsum = r1 + r2;
  const bool exact = round_core(g1) && round_core(g2);   // both cores are a point or a segment: signed distance, overlap included

  Simplex s;
  V3 d0 = g2.p - g1.p;
  if (!(dot(d0, d0) > DIST_FMIN)) d0 = v3(1, 0, 0);
  s.a0 = support(g1, d0);
  s.w0 = s.a0 - support(g2, -d0);
  s.w1 = s.w2 = s.w3 = s.w0; s.a1 = s.a2 = s.a3 = s.a0;
  s.l0 = 1.f; s.l1 = s.l2 = s.l3 = 0.f; s.n = 1;
  V3 v = s.w0, pa = s.a0;       // the best iterate: closest point of core1 - core2 to the origin, and its core1 point
  float vv = dot(v, v);
  bool overlap = false, far = false, stop = false;
  int it = 0;
  for (; it < max_iters; it++) {
    if (vv <= DIST_EPS2) { overlap = true; break; }
    const float vn = sqrtf(vv);
    const V3 sa = support(g1, -v);
    const V3 w = sa - support(g2, v);
    const float lower = dot(v, w) / vn;
    if (lower - rsum > distmax) { far = true; break; }
    if (vn - lower <= tol) { stop = true; break; }
    if (!exact && vn <= rsum) { stop = true; break; }          // a rounded shape reaches the other: an overlap, whatever the cores' distance is
    if (same(w, s.w0) || (s.n > 1 && same(w, s.w1)) || (s.n > 2 && same(w, s.w2))) { stop = true; break; }   // nothing new in this direction
    if (s.n == 1) { s.w1 = w; s.a1 = sa; }
    else if (s.n == 2) { s.w2 = w; s.a2 = sa; }
    else { s.w3 = w; s.a3 = sa; }
    s.n++;
    if (simplex_closest(s)) {
      overlap = true;
      refine_enclosing(s);
      pa = blend(s.l0, s.a0, s.l1, s.a1, s.l2, s.a2, s.l3, s.a3);
      v = blend(s.l0, s.w0, s.l1, s.w1, s.l2, s.w2, s.l3, s.w3);   // what is left between the two blends
      break;
    }
    const V3 nv = blend(s.l0, s.w0, s.l1, s.w1, s.l2, s.w2, s.l3, s.w3);
    const float nvv = dot(nv, nv);
    if (!(nvv < vv)) { stop = true; break; }                   // |v| no longer shrinks: the iterate before is the answer
    v = nv; vv = nvv;
    pa = blend(s.l0, s.a0, s.l1, s.a1, s.l2, s.a2, s.l3, s.a3);
  }
  Result out;
  out.status = (!overlap && !far && !stop) ? DIST_CAP : DIST_OK;
  if (!far && vv <= DIST_EPS2) overlap = true;   // (the last update may have brought the cores together)
  out.p1 = pa; out.p2 = pa;
  if (far) { out.dist = distmax; out.status |= DIST_FAR; return out; }
  if (overlap) {               // the cores themselves meet
    if (exact) {               // (a set of measure zero: segments that cross; the direction is then a convention)
      out.dist = -rsum;
      out.p1 = pa + v3(0, 0, 1) * r1; out.p2 = pa - v3(0, 0, 1) * r2;
    } else {                   // one common point: midway between the blend of geom1's points and that of geom2's, which rounding keeps apart
      out.dist = 0.f; out.status |= DIST_OVERLAP;
      out.p1 = out.p2 = pa - v * 0.5f;
    }
    return out;
  }
  const float dc = sqrtf(vv);
  const V3 n = v * (-1.f / dc);                                // from geom1 towards geom2
  const V3 pb = pa - v;
  const float d = dc - rsum;
  if (exact || d > 0.f) {
    out.dist = d;
    out.p1 = pa + n * r1; out.p2 = pb - n * r2;
    if (d > distmax) { out.dist = distmax; out.status |= DIST_FAR; }
  } else {                                                     // the sphere or capsule holds the other shape's nearest point
    out.dist = 0.f; out.status |= DIST_OVERLAP;
    out.p1 = out.p2 = sel(r1 > 0.f, pb, pa);
  }
  return out;
}
}  // namespace rsim_dist
