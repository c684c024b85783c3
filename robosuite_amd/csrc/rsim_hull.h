// rsim_hull.h -- the convex-hull routine of the MJCF compiler (rsim_mjcf.cpp quickhull), reachable from the other translation units of the library.
// Not part of the public boundary.
#pragma once
#ifdef __cplusplus
extern "C" {
#endif
// Face planes n . x <= d (n unit, outwards) of the convex hull of `nvert` points [nvert][3]: one plane per facet, coplanar triangles merged.  Writes up to
// `cap` rows [4] = (nx, ny, nz, d) to `planes` and returns the number of facets (which may exceed cap), or -1 with the message in rsim_last_error().
int rsim_hull_planes(const double* vert, int nvert, double* planes, int cap);
// geom_rcenter of a mesh geom is MPR's interior point: the compiler keeps it inside the hull by at least this share of geom_rbound
#define RSIM_RCENTER_INSIDE 0.02
// How far (metres) `point` [3] lies inside the convex hull of `nvert` points: the least distance to a face plane, negative outside.  0, or -1 with the message
// in rsim_last_error().
int rsim_hull_inside_by(const double* vert, int nvert, const double* point, double* inside_by);
#ifdef __cplusplus
}
#endif
