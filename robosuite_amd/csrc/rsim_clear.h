// rsim_clear.h -- kernel argument of the configuration clearance kernels (rsim_clear.hip), filled by the C-ABI host code (rsim_api.cpp).  Not part of the
// public boundary.  The body table is described in rsim_clear_core.h; the geom records are the ray kernel's scene table (rsim_ray.h DRayGeom), the pair table
// the distance query's (rsim_dist.h).
#pragma once
#include "rsim_internal.h"
#include "rsim_ray.h"
#include "rsim_dist.h"

#define RSIM_CLEAR_LANES 64      /* candidates per workgroup: one wavefront, lane = candidate env * K + k */
#define RSIM_CLEAR_PART 9        /* words per partial result of a pair chunk: dist, pair, status, fromto[6] */
#define RSIM_CLEAR_MAX_CHUNKS 1024
#define RSIM_CLEAR_FULL 1024     /* candidate blocks that give every SIMD of the part a wavefront (256 CUs x 4): from there on chunks = 0 means one chunk */

struct DClear {
  int B, K, n, NC;                // envs, candidates per env, controlled dofs, B * K
  int nbody, nq, fstride;
  int nel, nslot;                 // elements of the body table, moved bodies
  const int* tab;                 // [nel][RSIM_CLEAR_REC]
  const int* slot_of_body;        // [nbody]: slot of a moved body, -1 otherwise
  const float* ft;                // float tables: env e reads ft + e * fstride
  const float *qpos, *xpos, *xquat;   // [B][nq], RSIM_XPOS, RSIM_XQUAT
  const float* q;                 // [B][K][n]
  float* scr;                     // [nslot][7][NC]: poses of the moved bodies (null for the FK entry)
  float *xpos_out, *xquat_out;    // the FK entry: [B][K][nbody][3], [B][K][nbody][4] (null otherwise)
  // the distance phase
  int npair, chunks;
  int fo_size, fo_pos, fo_quat;   // float-table offsets (rsim_internal.h FO_cg_*)
  const DRayGeom* geom;           // [ngeom]
  const int* pairs;               // [npair][RSIM_DIST_REC]
  const float* mesh_vert;
  float distmax, tol;
  int max_iters;
  float* part;                    // chunks > 1: [chunks][RSIM_CLEAR_PART][NC] partial results (floats and ints share the words)
  float* dist;                    // [B][K]
  int* pair;                      // [B][K]
  float* fromto;                  // [B][K][6] or null
  int* status;                    // [B][K] or null
  // attachments (include/rsim.h rsim_attach; rsim_clear_core.h Att): natt == 0 is a call without them, which runs the kernels' plain instantiation
  int natt;
  const unsigned char* held;      // [B][natt] or null: every attachment is held in every env
  const float* rel;               // [B][natt][7] or null: from the env's current poses
  const int *body_sig, *body_att; // [nbody] each; body_sig null: no pair is skipped (an explicit pair list)
};

extern "C" int rsim_launch_clear_fk(const DClear* a, hipStream_t stream);
extern "C" int rsim_launch_clear_dist(const DClear* a, hipStream_t stream);
// k_clear_min alone, behind a pair loop that another code object ran (rsim_pen_query.hip k_clear_dist_signed); nothing with chunks <= 1
extern "C" int rsim_launch_clear_min(const DClear* a, hipStream_t stream);
