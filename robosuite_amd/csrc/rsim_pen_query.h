// rsim_pen_query.h -- kernel arguments of the signed clearance and signed collision-aware IK kernels (rsim_pen_query.hip), filled by the C-ABI host code
// (rsim_api.cpp).  Not part of the public boundary.  As in rsim_pen.h they are the arguments of the kernels whose place they take (rsim_clear.h DClear,
// rsim_ik_avoid.h DIkAvoid) with the three penetration options behind them.
#pragma once
#include "rsim_ik_avoid.h"
#include "rsim_pen.h"

struct DPenClear {
  DClear c;
  float pen_tol, offset;
  int pen_iters;
};
struct DPenIka {
  DIkAvoid a;
  float pen_tol, offset;
  int pen_iters;
};

// k_clear_dist_signed (_att) and, with c.chunks > 1, the unchanged k_clear_min behind it (rsim_launch_clear_min, rsim_clear.h)
extern "C" int rsim_launch_clear_dist_signed(const DPenClear* a, hipStream_t stream);
// one evaluation: k_ika_cost_signed (_att), then the unchanged k_ika_step (rsim_launch_ika_step, rsim_ik_avoid.h)
extern "C" int rsim_launch_ika_iter_signed(const DPenIka* a, hipStream_t stream);
