// rsim_ray.h -- kernel argument of k_ray (rsim_ray.hip) and the scene table it reads, filled by the C-ABI host code (rsim_api.cpp).  Not part of the
// public boundary.
#pragma once
#include "rsim_internal.h"

#define RSIM_RAY_CHUNK 64    /* geoms staged in LDS at a time (world pose + filters), 24 dwords each */
#define RSIM_RAY_REC 24
#define RSIM_RAY_TILE 256    /* rays per workgroup (rsim_ray / rsim_render_depth); the rangefinder launch uses one wavefront */
#define RSIM_RANGEFINDER 15  /* sensor_type code of the model blob (rsim_mjcf.cpp / robosuite_amd/mjcf.py) */

enum { RAY_ARRAYS, RAY_CAMERA, RAY_RANGEFINDER };   // where a launch's rays come from
enum { RAY_VISIBLE = 1 };                           // DRayGeom.flags bit 0: rgba[3] != 0; bits 8..: group

// one record per geom of the model (ALL geoms, not only the colliding ones), shared by the envs.  A colliding geom (cg >= 0) takes size / pos / quat /
// rbound / rcenter from the float table instead (ft + env * fstride: the values an env of a per_env_params batch may have overridden).
struct DRayGeom {
  int type, body, cg, flags, plane_adr, plane_num;   // planes: rows of DRay.planes (mesh geoms: face planes n . x <= d of the hull, geom frame)
  float size[3], pos[3], quat[4], rcenter[3], rbound;
  int pad[2];
};

struct DRay {
  int B, mode, n;            // envs, RAY_*, rays per env (camera: H * W; rangefinder: nsensor)
  int ngeom, nbody, fstride;
  int fo_size, fo_pos, fo_quat, fo_rcenter, fo_rbound, fo_site_pos, fo_site_quat;   // float-table offsets (rsim_internal.h FO_*)
  const DRayGeom* geom;      // [ngeom]
  const float* planes;       // [nplane][4]
  const float* ft;           // float tables: env e reads ft + e * fstride
  const float *xpos, *xquat; // RSIM_XPOS / RSIM_XQUAT
  unsigned geomgroup;        // bit k set: group k is included; 0: all groups
  int flg_static, bodyexclude;
  const float *origin, *dir; // RAY_ARRAYS: [B][n][3] each
  int cam_body, H, W;        // RAY_CAMERA
  float cam_pos[3], cam_quat[4], tanhalf;
  const int* rf;             // RAY_RANGEFINDER: [3][n] site (-1: lane is no carried rangefinder), the site's body, first entry in a sensordata row
  int nsensordata;
  float* dist;               // [B][n] (rangefinder: sensordata)
  int* geomid;               // [B][n] or null
  float miss;                // distance reported for a miss (-1; depth images: +inf)
};

extern "C" int rsim_launch_ray(const DRay* a, hipStream_t stream);
