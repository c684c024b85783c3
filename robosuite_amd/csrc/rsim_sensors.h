// rsim_sensors.h -- kernel argument of k_sensors (rsim_sensors.hip), filled by the C-ABI host code (rsim_api.cpp).  Not part of the public boundary.
#pragma once
#include "rsim_internal.h"

// sensor_type codes of the model blob (rsim_mjcf.cpp / robosuite_amd/mjcf.py SENSOR_TYPES).  0 / 1 (force, torque) are computed inside the step kernel
// (rsim_step.hip sensor_acc), which writes zero to every other entry; k_sensors runs behind it and fills the entries of the codes below.  Code 15, the
// rangefinder, is past RS_TYPE_END on purpose: k_sensors leaves it alone, the ray kernel behind it fills it (rsim_ray.h RSIM_RANGEFINDER).
enum {
  RS_JOINTPOS = 2, RS_TENDONPOS, RS_FRAMEPOS, RS_FRAMEQUAT,                                   // position stage (mj_sensorPos)
  RS_JOINTVEL, RS_TENDONVEL, RS_VELOCIMETER, RS_GYRO, RS_FRAMELINVEL, RS_FRAMEANGVEL,         // velocity stage (mj_sensorVel)
  RS_ACCELEROMETER, RS_TOUCH, RS_ACTUATORFRC,                                                 // acceleration stage (mj_sensorAcc)
  RS_TYPE_END
};
enum { RS_OBJ_NONE, RS_OBJ_JOINT, RS_OBJ_TENDON, RS_OBJ_SITE, RS_OBJ_XBODY, RS_OBJ_BODY, RS_OBJ_ACTUATOR };   // sensor_objtype
enum { RS_STAGE_POS = 1, RS_STAGE_VEL = 2, RS_STAGE_ACC = 4 };

struct DSensors {
  int B, stages;             // envs; RS_STAGE_* bits this launch computes (entries of the other stages are left as they are)
  int nq, nv, nu, nbody, nsensor, nsensordata, ncon_max, fstride;
  int io[IO_COUNT], fo[FO_COUNT];   // offsets into the int / float tables (rsim_internal.h)
  const int* it;             // int tables (shared)
  const float* ft;           // float tables: env e reads ft + e * fstride (site / body offsets differ per env under per_env_params)
  const int* objtype;        // [nsensor] RS_OBJ_*
  const int* carried;        // [nsensor] 1: computed here; 0: force / torque, or a sensor that reads zero
  const int* shape;          // [nsensor] touch: shape of the site (2 sphere, 4 ellipsoid, 6 box)
  const float* site_size;    // [nsensor][3] touch: size of the site
  const int* geom_body;      // [ngeom] body of every geom (contact records name geoms by their model ids)
  // state of the substep the values belong to: the one before its integration (the host hands copies where the launch ahead integrated)
  const float *qpos, *qvel, *qacc, *ctrl;
  const float *xpos, *xquat, *cdof, *rootcom, *contact;   // compatibility arrays the debug form of the step kernel left (RSIM_XPOS .. RSIM_CONTACT)
  const int* ncon;
  float* sensordata;         // [B][nsensordata]
};

extern "C" int rsim_launch_sensors(const DSensors* a, hipStream_t stream);
