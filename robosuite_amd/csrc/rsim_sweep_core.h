// rsim_sweep_core.h -- the per-segment core of the swept clearance query (rsim_config_sweep / rsim_config_motion_bound, rsim_sweep.hip): a certified check of
// the joint-space motion q(t) = q0 + t (q1 - q0), t in [0, 1], by conservative advancement, as fp32 __host__ __device__ functions on rsim_clear_core.h (the FK
// walk, the pruned pair loop) and rsim_dist_core.h (GJK).  The kernel includes it; so does tests/san/sweep_core_driver.cpp, which runs the very same source on
// the host under AddressSanitizer + UndefinedBehaviorSanitizer.  robosuite_amd/sweep.py is the fp64 mirror.
//
//  * the motion bound L (bound_walk, motion_bound): the distance of any listed pair changes by at most L |dt|.  One more walk of the body table, no
//    trigonometry.  A moved body carries Omega, the sum of |q1 - q0| over the controlled hinges on its path (a bound on its angular speed per unit t), and V, a
//    bound on the speed of its origin.  The FK step of a body, p = p_parent + R_parent body_pos, gives V = V_parent + Omega_parent |body_pos|.  A slide,
//    p += R axis x(t), adds |axis| (|dx| + Omega max(|x(0)|, |x(1)|)); a held slide has dx = 0 but its displacement still lengthens the arm.  A hinge or a held
//    ball joint, p = anchor - R_new jnt_pos with anchor = p + R jnt_pos, adds Omega |jnt_pos| before the joint's own |dq| goes into Omega and Omega |jnt_pos|
//    after.  A point fixed to the body at distance r from its origin moves at most V + Omega r per unit t; r of a geom is |geom_pos| plus a radius about the
//    geom's origin that contains it: the larger of the one its type and geom_size give and |geom_rcenter| + geom_rbound (a mesh geom has only the second; an
//    env that overrides geom_size alone is still covered by the first).  A geom of a body that is not moved has speed 0.  The distance of two convex solids is
//    1-Lipschitz in the displacement of either, so a pair's bound is the sum of its two geoms' and L the maximum over the list, times 1 + 2^-16 for the
//    roundings of this very sum (some thirty fp32 operations, 2^-24 each).
//  * ATTACHMENTS (rsim_clear_core.h): a held body has Omega = Omega(carrier) and V = V(carrier) + Omega(carrier) |p_rel| -- the FK step p = p_c + R_c p_rel
//    with p_rel constant -- and its subtree follows by the rules above; one that is not held stands still, Omega = V = 0, and so does its subtree (its joints
//    are held).  L is the maximum over the pairs the lane's env evaluates.  ATT = false compiles all of it away.
//  * Omega and V of a slot live in the first two words of that slot's pose in the scratch until the first FK walk overwrites them: no array in registers.
//  * the loop (sweep): sample c(t) = clear_pairs at the poses of q(t); c <= margin + slack: HIT; t == 1: FREE; else t <- min(1, t + (c - margin) / L), where a
//    far sample reads c = distmax.  Between two samples t_i < t_j the clearance is at least c(t_i) - L (t - t_i) > margin up to the step's end, and past a step
//    that fp32 rounded up by an ulp at least c(t_j) - L ulp > margin + slack - L ulp: the motion is certified on [0, t).  max_steps samples without a decision:
//    UNDECIDED.  L == 0: the first sample decides.
//  * the joint value the FK walk sees is fmaf(t, q1 - q0, q0): one rounding, the same on the host and on the device, so that rsim_config_clearance at that
//    very fp32 vector returns the sample bit for bit.
#pragma once
#include "rsim_clear_core.h"

namespace rsim_sweep {
using namespace rsim_clear;

enum { SWEEP_FREE = 0, SWEEP_HIT = 1, SWEEP_UNDECIDED = 2 };   // include/rsim.h RSIM_SWEEP_*; DIST_CAP is or-ed in at bit 8

// what one segment reads: Cand's env pointers (its q is unused) and the two ends
struct Seg { Cand env; const float *q0, *q1; };

// the point at parameter t of the segment, per controlled column
struct SegQ {
  const float *q0, *q1;
  float t;
  RSIM_HD float operator()(int col) const { return fmaf(t, q1[col] - q0[col], q0[col]); }
};

struct Opts { float distmax, tol; int max_iters; float margin, slack; int max_steps; };
struct Out { int status, steps; float t, t_min; Best best; };

RSIM_HD float norm3(V3 a) { return sqrtf(dot(a, a)); }

// ---- the motion bound ---------------------------------------------------------------------------------------------------------------------------------
// leaves (Omega, V) of every moved body in words 0 and 1 of its slot
template <bool ATT>
RSIM_HD void bound_walk(const int* tab, int nel, const Seg& s, const PoseStore& st, const Att& at) {
  float om = 0.f, v = 0.f, lom = 0.f, lv = 0.f;
  int cur_slot = -1, last_slot = -1;
  const float* ft = s.env.ft;
  for (int e = 0; e <= nel; e++) {
    const int* el = tab + (size_t)RSIM_CLEAR_REC * (e < nel ? e : 0);
    const int kind = e < nel ? RSIM_CLEAR_U(el[CLE_KIND]) : CL_BODY;
    if (kind == CL_BODY || (ATT && kind == CL_ATTACH)) {
      if (cur_slot >= 0) {
        float* w = st.pos + (size_t)cur_slot * st.pe;
        w[0] = om; w[st.ps] = v;
        lom = om; lv = v; last_slot = cur_slot;
      }
      if (e == nel) break;
      const int pslot = RSIM_CLEAR_U(el[CLE_COL]);
      float pom = 0.f, pv = 0.f;   // a parent that is not moved stands still
      if (pslot >= 0) {
        if (pslot == last_slot) { pom = lom; pv = lv; }
        else { const float* w = st.pos + (size_t)pslot * st.pe; pom = w[0]; pv = w[st.ps]; }
      }
      om = pom;
      if (ATT && kind == CL_ATTACH) {
        const int i = RSIM_CLEAR_U(el[CLE_O3]);
        const bool held = (at.held >> i) & 1u;
        const float arm = norm3(attach_rel(at, i, s.env, RSIM_CLEAR_U(el[CLE_ID]), RSIM_CLEAR_U(el[CLE_PBODY])).p);
        om = held ? pom : 0.f;
        v = held ? pv + pom * arm : 0.f;   // (not held: at rest, and its subtree with it -- every joint below is held)
      } else {
        v = pv + pom * norm3(ld3(ft + RSIM_CLEAR_U(el[CLE_O1])));
      }
      cur_slot = RSIM_CLEAR_U(el[CLE_SLOT]);
    } else {
      const int col = RSIM_CLEAR_U(el[CLE_COL]), qadr = RSIM_CLEAR_U(el[CLE_ID]);
      if (kind == CL_SLIDE) {
        const float ref = ft[RSIM_CLEAR_U(el[CLE_O3])];
        const float x0 = (col >= 0 ? s.q0[col] : s.env.qpos[qadr]) - ref, x1 = (col >= 0 ? s.q1[col] : s.env.qpos[qadr]) - ref;
        v += norm3(ld3(ft + RSIM_CLEAR_U(el[CLE_O2]))) * (fabsf(x1 - x0) + om * fmaxf(fabsf(x0), fabsf(x1)));
      } else {
        const float arm = norm3(ld3(ft + RSIM_CLEAR_U(el[CLE_O1])));
        v += om * arm;
        if (kind == CL_HINGE && col >= 0) om += fabsf(s.q1[col] - s.q0[col]);
        v += om * arm;
      }
    }
  }
}
RSIM_HD void bound_walk(const int* tab, int nel, const Seg& s, const PoseStore& st) {
  const Att none = {0u, nullptr, nullptr, nullptr};
  bound_walk<false>(tab, nel, s, st, none);
}

// a radius about the geom's own origin that contains the solid: by type and size, and by the model's bounding sphere (rbound about rcenter); a plane has none
RSIM_HD float geom_radius(int type, V3 size, V3 rc, float rb) {
  float r = 0.f;
  if (type == G_SPHERE) r = size.x;
  else if (type == G_CAPSULE) r = size.x + size.y;
  else if (type == G_ELLIPSOID) r = fmaxf(size.x, fmaxf(size.y, size.z));
  else if (type == G_CYLINDER) r = sqrtf(size.x * size.x + size.y * size.y);
  else if (type == G_BOX) r = norm3(size);
  return type == G_PLANE ? 0.f : fmaxf(r, norm3(rc) + rb);
}

// GeomRec: the ray kernel's scene record (type, body, cg, size, pos, rcenter, rbound); fo_rcenter / fo_rbound: float-table offsets of a colliding geom's
template <class GeomRec>
RSIM_HD float geom_speed(const Scene<GeomRec>& sc, int fo_rcenter, int fo_rbound, int g, const float* ft, const PoseStore& st) {
  const GeomRec& s = sc.geom[g];
  const int cg = RSIM_CLEAR_U(s.cg), slot = RSIM_CLEAR_U(sc.slot_of_body[RSIM_CLEAR_U(s.body)]);
  if (slot < 0) return 0.f;
  V3 size = ld3(s.size), lp = ld3(s.pos), rc = ld3(s.rcenter);
  float rb = s.rbound;
  if (cg >= 0) { size = ld3(ft + sc.fo_size + 3 * cg); lp = ld3(ft + sc.fo_pos + 3 * cg); rc = ld3(ft + fo_rcenter + 3 * cg); rb = ft[fo_rbound + cg]; }
  const float* w = st.pos + (size_t)slot * st.pe;
  return w[st.ps] + w[0] * (norm3(lp) + geom_radius(RSIM_CLEAR_U(s.type), size, rc, rb));
}

template <bool ATT, class GeomRec>
RSIM_HD float motion_bound(const int* tab, int nel, const Scene<GeomRec>& sc, int fo_rcenter, int fo_rbound, int npair, const Seg& s, const PoseStore& st, const Att& at) {
  bound_walk<ATT>(tab, nel, s, st, at);
  float L = 0.f;
  for (int p = 0; p < npair; p++) {
    const int* rec = sc.pairs + (size_t)p * sc.rec;
    const int g1 = RSIM_CLEAR_U(rec[0]), g2 = RSIM_CLEAR_U(rec[1]);
    if (ATT && !pair_active(at, RSIM_CLEAR_U(sc.geom[g1].body), RSIM_CLEAR_U(sc.geom[g2].body))) continue;
    L = fmaxf(L, geom_speed(sc, fo_rcenter, fo_rbound, g1, s.env.ft, st) + geom_speed(sc, fo_rcenter, fo_rbound, g2, s.env.ft, st));
  }
  return L * (1.f + 1.52587890625e-05f);
}
template <class GeomRec>
RSIM_HD float motion_bound(const int* tab, int nel, const Scene<GeomRec>& sc, int fo_rcenter, int fo_rbound, int npair, const Seg& s, const PoseStore& st) {
  const Att none = {0u, nullptr, nullptr, nullptr};
  return motion_bound<false>(tab, nel, sc, fo_rcenter, fo_rbound, npair, s, st, none);
}

// ---- the advancement loop --------------------------------------------------------------------------------------------------------------------------------
// One sample: FK at q(t) and the pair loop; folds it into o and decides.  Returns true when the segment is decided.
template <bool ATT, class GeomRec>
RSIM_HD bool sweep_sample(const int* tab, int nel, const Scene<GeomRec>& sc, int npair, const Seg& s, const PoseStore& st, const Opts& op, float L, float& t, Out& o,
                          const Att& at) {
  const SegQ qv = {s.q0, s.q1, t};
  fk_walk<ATT>(tab, nel, s.env, st, qv, at);
  const Best r = clear_pairs<ATT>(sc, 0, npair, s.env, st, op.distmax, op.tol, op.max_iters, at);
  o.steps++;
  o.t = t;
  o.status |= r.status & DIST_CAP;
  const bool take = r.pair >= 0 && r.dist < o.best.dist;      // a strictly smaller distance: the earliest sample wins ties
  o.best.dist = take ? r.dist : o.best.dist; o.best.pair = take ? r.pair : o.best.pair;
  o.best.p1 = sel(take, r.p1, o.best.p1); o.best.p2 = sel(take, r.p2, o.best.p2);
  o.t_min = take ? t : o.t_min;
  if (r.dist <= op.margin + op.slack) { o.status = (o.status & DIST_CAP) | SWEEP_HIT; return true; }
  if (t == 1.f || !(L > 0.f)) { o.status = (o.status & DIST_CAP) | SWEEP_FREE; o.t = 1.f; return true; }
  t = fminf(1.f, t + (r.dist - op.margin) / L);      // (a far sample reads distmax)
  return false;
}

RSIM_HD Out sweep_begin(float distmax) {
  Out o;
  o.status = SWEEP_UNDECIDED; o.steps = 0; o.t = 0.f; o.t_min = 0.f;
  o.best.dist = distmax; o.best.pair = -1; o.best.status = DIST_FAR; o.best.p1 = o.best.p2 = v3(0, 0, 0);
  return o;
}

// the whole segment, serially (the host's form; the kernel runs the same samples under a wave-uniform loop, rsim_sweep.hip)
template <bool ATT, class GeomRec>
RSIM_HD Out sweep(const int* tab, int nel, const Scene<GeomRec>& sc, int npair, const Seg& s, const PoseStore& st, const Opts& op, float L, const Att& at) {
  Out o = sweep_begin(op.distmax);
  float t = 0.f;
  for (int i = 0; i < op.max_steps; i++)
    if (sweep_sample<ATT>(tab, nel, sc, npair, s, st, op, L, t, o, at)) break;
  return o;
}
template <class GeomRec>
RSIM_HD Out sweep(const int* tab, int nel, const Scene<GeomRec>& sc, int npair, const Seg& s, const PoseStore& st, const Opts& op, float L) {
  const Att none = {0u, nullptr, nullptr, nullptr};
  return sweep<false>(tab, nel, sc, npair, s, st, op, L, none);
}
}  // namespace rsim_sweep
