// rsim_pen_clear_core.h -- the two pair loops of the configuration queries with rsim_pen_core.h pair_signed as the pair routine: the running minimum of
// rsim_config_clearance_signed (and of its gradient entry) and the cost loop of rsim_config_collision_cost_signed / rsim_ik_site_avoid_signed.  fp32 __host__
// __device__ functions in the way of rsim_clear_core.h and rsim_grad_core.h, which this file builds on and does not touch.  The kernels of rsim_pen.hip and
// rsim_pen_query.hip include it; so does tests/san/signed_clear_core_driver.cpp, which runs the very same source on the host under AddressSanitizer +
// UndefinedBehaviorSanitizer.  robosuite_amd/clearance.py (signed=True) is the fp64 mirror and the definition.
//
//  * clear_pairs_signed is clear_pairs with every overlap signed: the minimum runs over the signed per-pair values, replaced only by a strictly smaller one, so
//    the lowest pair index wins ties.  best.status is the winning pair's: 0, or with DIST_CAP / DIST_PEN_CAP; never DIST_OVERLAP.
//  * distmax IS NEVER NEGATIVE.  pair_distance leaves at its far exit once its lower bound exceeds distmax, and reports a far pair AT distmax.  The bound v.w / |v|
//    stays a valid lower bound of the signed distance below zero (it is minus a support width, and every support width is at least the depth), so a negative
//    running minimum handed on as distmax would throw out only pairs whose TRUE depth is smaller -- but pair_signed returns a LOCAL minimum of the descent, which
//    may lie above the true depth, and whether such a pair is seen would then depend on what came before it in the list.  So the pair routine is handed
//    max(best.dist, 0): a separated pair still leaves at the first bound that proves it no closer than the minimum (or than zero, once something overlaps), every
//    overlapping pair is signed, and a result is taken only if r.dist < best.dist.  The result is the plain minimum of pair_signed over the list, whatever the
//    order (tests/test_signed_queries_core_host.py).  While best.dist >= 0 this is clear_pairs' call sequence exactly: a candidate without an overlap is bit for
//    bit the unsigned query's.
//  * NOT BUILT: the prune the bound delta(seed) >= depth allows (an overlapping pair whose seed width is <= -best.dist cannot win and could skip its descent).
//    It needs pair_signed's statements between the overlap test and the descent a second time; DESIGN.md 5.3 has the measured cost it would have to beat.
#pragma once
#include "rsim_pen_core.h"
#include "rsim_grad_core.h"

namespace rsim_grad {

// the smallest SIGNED distance over pairs [p0, p1) at the candidate's poses; nothing closer than distmax: (distmax, -1, DIST_FAR, zeros).
// steps (may be null): the projections the candidate made.
template <bool ATT, class GeomRec>
RSIM_HD Best clear_pairs_signed(const Scene<GeomRec>& sc, int p0, int p1, const Cand& c, const PoseStore& st, float distmax, float tol, int max_iters,
                                const PenOpts& po, const Att& at, int* steps = nullptr) {
  Best best;
  best.dist = distmax; best.pair = -1; best.status = DIST_FAR; best.p1 = best.p2 = v3(0, 0, 0);
  if (steps) *steps = 0;
  for (int p = p0; p < p1; p++) {
    const int* rec = sc.pairs + (size_t)p * sc.rec;
    const int g1 = RSIM_CLEAR_U(rec[0]), g2 = RSIM_CLEAR_U(rec[1]);
    if (ATT && !pair_active(at, RSIM_CLEAR_U(sc.geom[g1].body), RSIM_CLEAR_U(sc.geom[g2].body))) continue;
    Geom A = load_geom(sc, g1, c, st, RSIM_CLEAR_U(rec[2]), RSIM_CLEAR_U(rec[3]));
    Geom Bg = load_geom(sc, g2, c, st, RSIM_CLEAR_U(rec[4]), RSIM_CLEAR_U(rec[5]));
    const V3 org = A.p;
    A.p = v3(0, 0, 0); Bg.p = Bg.p - org;
    int k = 0;
    const Result r = pair_signed(A, Bg, fmaxf(best.dist, 0.f), tol, max_iters, po, &k);      // never a negative distmax
    if (steps) *steps += k;
    const bool take = (r.status & DIST_FAR) == 0 && r.dist < best.dist;
    best.dist = take ? r.dist : best.dist;
    best.pair = take ? p : best.pair;
    best.status = take ? r.status : best.status;
    best.p1 = sel(take, r.p1 + org, best.p1); best.p2 = sel(take, r.p2 + org, best.p2);
  }
  return best;
}

// rsim_grad_core.h cost_pairs with pair_signed as the pair routine; noverlap is dist < 0
template <bool ATT, class GeomRec>
RSIM_HD Cost cost_pairs_signed(const Scene<GeomRec>& sc, int p0, int p1, const Cand& c, const PoseStore& st, const JointStore& js, int n, unsigned slide_mask,
                               float d_safe, float tol, int max_iters, const PenOpts& po, const Att& at, const int* sig, const int* body_att, const GradAcc& ga) {
  Cost acc;
  acc.cost = 0.f; acc.nnear = acc.nover = 0;
  for (int col = 0; col < n; col++) ga.g[col * ga.gs] = 0.f;
  for (int p = p0; p < p1; p++) {
    const int* rec = sc.pairs + (size_t)p * sc.rec;
    const int g1 = RSIM_CLEAR_U(rec[0]), g2 = RSIM_CLEAR_U(rec[1]);
    const int b1 = RSIM_CLEAR_U(sc.geom[g1].body), b2 = RSIM_CLEAR_U(sc.geom[g2].body);
    if (ATT && !pair_active(at, b1, b2)) continue;
    Geom A = load_geom(sc, g1, c, st, RSIM_CLEAR_U(rec[2]), RSIM_CLEAR_U(rec[3]));
    Geom Bg = load_geom(sc, g2, c, st, RSIM_CLEAR_U(rec[4]), RSIM_CLEAR_U(rec[5]));
    const V3 org = A.p;
    A.p = v3(0, 0, 0); Bg.p = Bg.p - org;
    const Result r = pair_signed(A, Bg, d_safe, tol, max_iters, po);
    if ((r.status & DIST_FAR) != 0 || !(r.dist < d_safe)) continue;
    const float w = d_safe - r.dist;
    acc.cost += 0.5f * w * w;
    acc.nnear++;
    acc.nover += r.dist < 0.f ? 1 : 0;
    const V3 q1 = r.p1 + org, q2 = r.p2 + org;
    V3 dir;
    if (!grad_dir(r.dist, p, r.status, q1, q2, dir)) continue;
    const unsigned w1 = (unsigned)RSIM_CLEAR_U(sig[b1]), w2 = (unsigned)RSIM_CLEAR_U(sig[b2]);
    const unsigned s1 = sig_pick(w1, ATT && body_att ? RSIM_CLEAR_U(body_att[b1]) : -1, at.held);
    const unsigned s2 = sig_pick(w2, ATT && body_att ? RSIM_CLEAR_U(body_att[b2]) : -1, at.held);
    for (int col = 0; col < n; col++)
      if (((s1 ^ s2) >> col) & 1u) ga.g[col * ga.gs] -= w * col_grad(js, col, (slide_mask >> col) & 1u, dir, q1, q2, s1, s2);
  }
  return acc;
}
}  // namespace rsim_grad
