// rsim_pen.h -- kernel arguments of the signed-overlap kernels (rsim_pen.hip), filled by the C-ABI host code (rsim_api.cpp).  Not part of the public boundary.
// They are the arguments of the kernels whose place they take (rsim_dist.h DDist, rsim_grad.h DGrad) with the three penetration options behind them.
#pragma once
#include "rsim_dist.h"
#include "rsim_grad.h"

#define RSIM_PEN_ITERS_LIMIT 128  /* include/rsim.h RSIM_PEN_MAX_ITERS */

struct DPenDist {
  DDist d;
  float pen_tol, offset;
  int pen_iters;
  int* steps;                     // [B][npair] projections per pair, or null (the bench's share of pairs that descend)
};
struct DPenCost {
  DGrad g;
  float pen_tol, offset;
  int pen_iters;
};

extern "C" int rsim_launch_dist_signed(const DPenDist* a, hipStream_t stream);
// the pair loop only: with g.c.chunks > 1 the caller runs rsim_launch_clear_cost_sum (rsim_grad.h) behind it
extern "C" int rsim_launch_clear_cost_signed(const DPenCost* a, hipStream_t stream);
