// rsim_sweep.h -- kernel argument of the swept clearance kernel (rsim_sweep.hip), filled by the C-ABI host code (rsim_api.cpp).  Not part of the public
// boundary.  A segment is a candidate with two ends: the tables, the env's arrays, the scratch and the sample outputs are DClear's (rsim_clear.h), with q = q0.
#pragma once
#include "rsim_clear.h"

struct DSweep {
  DClear c;                       // q = q0 [B][K][n]; scr [nslot][7][NC]; dist / pair / fromto / status: the outputs of the closest sample; chunks, part unused
  const float* q1;                // [B][K][n]
  int fo_rcenter, fo_rbound;      // float-table offsets (rsim_internal.h FO_cg_*)
  float margin, slack;
  int max_steps;
  float *t, *tmin;                // [B][K]
  int* steps;                     // [B][K] or null
  float* bound;                   // not null: the motion-bound entry -- L [B][K] is written and nothing else is done
};

extern "C" int rsim_launch_sweep(const DSweep* a, hipStream_t stream);
