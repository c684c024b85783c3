// rsim_dist.h -- kernel argument of k_dist (rsim_dist.hip) and the pair table it reads, filled by the C-ABI host code (rsim_api.cpp).  Not part of the
// public boundary.  The geom records are the ray kernel's scene table (rsim_ray.h DRayGeom).
#pragma once
#include "rsim_internal.h"
#include "rsim_ray.h"

#define RSIM_DIST_LANES 64   /* envs per workgroup: one wavefront, lane = env */
#define RSIM_DIST_REC 6      /* ints per pair: geom1, geom2, first hull vertex and vertex count of geom1, of geom2 (0, 0: no mesh) */

struct DDist {
  int B, npair, nbody, fstride;
  int fo_size, fo_pos, fo_quat;   // float-table offsets (rsim_internal.h FO_cg_*)
  const DRayGeom* geom;           // [ngeom]
  const int* pairs;               // [npair][RSIM_DIST_REC]
  const float* mesh_vert;         // DModel.mesh_vert: hull vertices in the geom frame, [nmeshvert][3]
  const float* ft;                // float tables: env e reads ft + e * fstride
  const float *xpos, *xquat;      // RSIM_XPOS / RSIM_XQUAT
  float distmax, tol;
  int max_iters;
  float* dist;                    // [B][npair]
  float* fromto;                  // [B][npair][6] or null
  int* status;                    // [B][npair] or null
};

extern "C" int rsim_launch_dist(const DDist* a, hipStream_t stream);
