// rsim_grad_core.h -- the per-candidate core of the clearance gradient and of the collision cost (rsim_config_clearance_grad / rsim_config_collision_cost,
// rsim_grad.hip): fp32 __host__ __device__ functions on top of rsim_clear_core.h, in its way.  The kernels include it; so does tests/san/grad_core_driver.cpp,
// which runs the very same source on the host under AddressSanitizer + UndefinedBehaviorSanitizer.
//
//  * Two convex solids with unique nearest points p1, p2 at distance d (signed or not), n = (p2 - p1) / d:   dd/dq_c = n . (s2_c v_c(p2) - s1_c v_c(p1)),
//    v_c(p) = a_c x (p - anchor_c) for a hinge, a_c for a slide; a_c / anchor_c the world axis / anchor of controlled column c at the candidate, s_i_c bit c of
//    the dof signature of the pair's body i.  No derivative of the witness points enters.
//  * THE JOINT STORE.  joint_walk goes over the body table once more, READING the poses the FK walk left in the pose store, and leaves axis and anchor of every
//    controlled column in a store of its own: axis = R_cur a, anchor = p_cur + R_cur jnt_pos at the moment the joint is applied -- the `anchor` fk_joint forms, so
//    several joints on one body are right.  It writes no pose: what the distance phase reads is what k_clear_fk wrote.  Controlled joints sit on ordinary moved
//    bodies only (clear_plan refuses one below an attached body), so the walk has no attachment branch: a CL_ATTACH element is passed over.
//  * SIGNATURES.  One word per body, the unheld signature in the low 16 bits and the held one in the high 16 (rsim_clear_core.h Att), uploaded for every gradient
//    or cost call -- also for an explicit pair list, where the pair loop's skip rule has none.  Which half counts is the lane's env's `held` row.
//  * grad is all zeros for a far result, for DIST_OVERLAP (distance 0, one common point, no direction) and for |dist| < GRAD_MIN_DIST.
//  * THE COST.  cost_pairs runs the pair loop with distmax = d_safe for every pair (no running minimum): a pair with d < d_safe adds 1/2 (d_safe - d)^2 and
//    -(d_safe - d) grad d.  cost and the counts are registers; the gradient accumulates in the lane's OWN words of the output (or of the chunk's partial
//    result), zeroed first and read-modified-written only by the pairs inside d_safe, which are few.  (Sixteen accumulators in registers, the column loop unrolled
//    with a `col < n` predicate, were built first: k_clear_cost then took 256 registers against k_clear_dist's 136, two wavefronts per SIMD instead of three.)
#pragma once
#include "rsim_clear_core.h"

#define RSIM_GRAD_COLS 16          // include/rsim.h RSIM_JNT_MAX
#define RSIM_GRAD_MIN_DIST_F 1e-7f // include/rsim.h RSIM_GRAD_MIN_DIST

namespace rsim_grad {
using namespace rsim_clear;

// where axis and anchor of the controlled columns live: component k (axis xyz, anchor xyz) of column c at a[c * ce + k * cs].  The kernels' store is laid out
// [col][6][candidates] (cs = candidates), beside the pose scratch.
struct JointStore { float* a; size_t ce, cs; };

RSIM_HD void store_joint(const JointStore& js, int col, const V3& axis, const V3& anchor) {
  float* w = js.a + (size_t)col * js.ce;
  w[0] = axis.x; w[js.cs] = axis.y; w[2 * js.cs] = axis.z; w[3 * js.cs] = anchor.x; w[4 * js.cs] = anchor.y; w[5 * js.cs] = anchor.z;
}

// Walks the table and stores world axis and anchor of every controlled column.  A body starts from its parent's STORED pose (what fk_walk left, after the
// normalisation; the env's pose for a parent that is not moved), then applies its joints in order as fk_walk does.
RSIM_HD void joint_walk(const int* tab, int nel, const Cand& c, const PoseStore& st, const JointStore& js) {
  Pose cur;
  cur.p = v3(0, 0, 0);
  cur.q.w = 1.f; cur.q.x = cur.q.y = cur.q.z = 0.f;
  for (int e = 0; e < nel; e++) {
    const int* el = tab + (size_t)RSIM_CLEAR_REC * e;
    const int kind = RSIM_CLEAR_U(el[CLE_KIND]);
    if (kind == CL_ATTACH) continue;   // no joint follows it
    if (kind == CL_BODY) {
      const int pslot = RSIM_CLEAR_U(el[CLE_COL]), pbody = RSIM_CLEAR_U(el[CLE_PBODY]);
      const Pose par = pslot < 0 ? env_pose(c, pbody) : load_pose(st, st.by_body ? pbody : pslot);
      cur = fk_body(par, c.ft, RSIM_CLEAR_U(el[CLE_O1]), RSIM_CLEAR_U(el[CLE_O2]));
    } else {
      const int col = RSIM_CLEAR_U(el[CLE_COL]), qadr = RSIM_CLEAR_U(el[CLE_ID]), o1 = RSIM_CLEAR_U(el[CLE_O1]), o2 = RSIM_CLEAR_U(el[CLE_O2]);
      if (col >= 0) store_joint(js, col, qrot(cur.q, ld3(c.ft + o2)), cur.p + qrot(cur.q, ld3(c.ft + o1)));
      float x = 0.f;
      if (kind != CL_BALL) x = (col >= 0 ? c.q[col] : c.qpos[qadr]) - c.ft[RSIM_CLEAR_U(el[CLE_O3])];
      cur = fk_joint(cur, kind, c.ft, o1, o2, x, c.qpos + qadr);
    }
  }
}

// which half of a body's signature word counts in an env: the held one if the body belongs to attachment i >= 0 and the env's row holds it
RSIM_HD unsigned sig_pick(unsigned word, int att_i, unsigned held) { return att_i >= 0 && ((held >> att_i) & 1u) ? word >> 16 : word & 0xffffu; }

// n . (s2 v_c(p2) - s1 v_c(p1)) for column col; slide: bit col of the call's slide mask
RSIM_HD float col_grad(const JointStore& js, int col, bool slide, const V3& n, const V3& p1, const V3& p2, unsigned s1, unsigned s2) {
  const float* w = js.a + (size_t)col * js.ce;
  const V3 a = v3(w[0], w[js.cs], w[2 * js.cs]), o = v3(w[3 * js.cs], w[4 * js.cs], w[5 * js.cs]);
  const float f1 = (s1 >> col) & 1u ? 1.f : 0.f, f2 = (s2 >> col) & 1u ? 1.f : 0.f;
  const V3 v = slide ? a * (f2 - f1) : cross(a, (p2 - o) * f2 - (p1 - o) * f1);
  return dot(n, v);
}

// does a result have a gradient, and along which direction?  (far / overlap / shorter than GRAD_MIN_DIST: none)
RSIM_HD bool grad_dir(float dist, int pair, int status, const V3& p1, const V3& p2, V3& n) {
  const bool ok = pair >= 0 && (status & (DIST_OVERLAP | DIST_FAR)) == 0 && fabsf(dist) >= RSIM_GRAD_MIN_DIST_F;
  n = ok ? (p2 - p1) * (1.f / dist) : v3(0, 0, 0);
  return ok;
}

// the gradient of one candidate's clearance result: grad[0..n) written, zeros under the three rules.  b1, b2: the bodies of the winning pair's geoms (anything
// for a far result), sig / body_att [nbody] (body_att null: no attachments)
RSIM_HD void clear_grad(const JointStore& js, int n, unsigned slide_mask, float dist, int pair, int status, const V3& p1, const V3& p2, int b1, int b2,
                        const int* sig, const int* body_att, unsigned held, float* grad) {
  V3 dir;
  const bool ok = grad_dir(dist, pair, status, p1, p2, dir);
  unsigned s1 = 0u, s2 = 0u;
  if (ok) {
    s1 = sig_pick((unsigned)sig[b1], body_att ? body_att[b1] : -1, held);
    s2 = sig_pick((unsigned)sig[b2], body_att ? body_att[b2] : -1, held);
  }
  for (int col = 0; col < n; col++) grad[col] = ok ? col_grad(js, col, (slide_mask >> col) & 1u, dir, p1, p2, s1, s2) : 0.f;
}

struct Cost { float cost; int nnear, nover; };
// where a candidate's gradient accumulates: entry col at g[col * gs]
struct GradAcc { float* g; size_t gs; };

// cost, counts and gradient over pairs [p0, p1) at the candidate's poses, every pair queried with distmax = d_safe.  ATT: the pairs this lane's env does not
// evaluate are passed over, as in clear_pairs.  sig / body_att as above; the table reads are wave-uniform.
template <bool ATT, class GeomRec>
RSIM_HD Cost cost_pairs(const Scene<GeomRec>& sc, int p0, int p1, const Cand& c, const PoseStore& st, const JointStore& js, int n, unsigned slide_mask,
                        float d_safe, float tol, int max_iters, const Att& at, const int* sig, const int* body_att, const GradAcc& ga) {
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
    const Result r = pair_distance(A, Bg, d_safe, tol, max_iters);
    if ((r.status & DIST_FAR) != 0 || !(r.dist < d_safe)) continue;
    const float w = d_safe - r.dist;
    acc.cost += 0.5f * w * w;
    acc.nnear++;
    acc.nover += (r.status & DIST_OVERLAP) ? 1 : 0;
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
