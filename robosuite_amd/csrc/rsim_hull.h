// rsim_hull.h -- the convex-hull routine of the MJCF compiler (rsim_mjcf.cpp quickhull), reachable from the other translation units of the library.
// Not part of the public boundary.
#pragma once
#ifdef __cplusplus
extern "C" {
#endif
// Face planes n . x <= d (n unit, outwards) of the convex hull of `nvert` points [nvert][3]: one plane per facet, coplanar triangles merged.  Writes up to
// `cap` rows [4] = (nx, ny, nz, d) to `planes` and returns the number of facets (which may exceed cap), or -1 with the message in rsim_last_error().
int rsim_hull_planes(const double* vert, int nvert, double* planes, int cap);
#ifdef __cplusplus
}
#endif
