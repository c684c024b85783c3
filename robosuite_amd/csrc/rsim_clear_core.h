// rsim_clear_core.h -- the per-candidate core of the configuration clearance query (rsim_config_fk / rsim_config_clearance, rsim_clear.hip): forward
// kinematics of the bodies a candidate joint vector moves, and the loop over a pair list that keeps the smallest distance, as fp32 __host__ __device__
// functions in the way of rsim_dist_core.h, which this file builds on.  The kernels include it; so does tests/san/clear_core_driver.cpp, which runs the very
// same source on the host under AddressSanitizer + UndefinedBehaviorSanitizer.
//
//  * FK is the position stage's (mjcf.kinematics_np is its fp64 statement): body_pos / body_quat offsets on the parent's pose, a hinge about its anchor
//    jnt_pos, a slide along its axis, qpos - qpos0, a held ball joint's quaternion as it stands; the body's quaternion is normalised once, after its joints.
//    Only MOVED bodies are walked (a body with a controlled joint on its path to the world); the parent of the first one of a branch is read from the env's
//    RSIM_XPOS / RSIM_XQUAT.  A joint that is not controlled reads the env's qpos.
//  * the body table (built on the host, rsim_api.cpp clear_table) is read at addresses that are the same in every lane: RSIM_CLEAR_U makes them provably so
//    on the device.  One lane = one candidate; the walk is a serial loop.
//  * the pair loop hands its running minimum to pair_distance as distmax: a pair that cannot beat it leaves at the far exit after an iteration or two.
//    The minimum is replaced only by a strictly smaller distance, so the lowest pair index wins ties.
//  * NOT HANDLED: a grasped object does not move with the candidate -- it is a free body at its current pose.
#pragma once
#include "rsim_dist_core.h"
#if defined(__HIP_DEVICE_COMPILE__)
#define RSIM_CLEAR_U(x) __builtin_amdgcn_readfirstlane(x)
#else
#define RSIM_CLEAR_U(x) (x)
#endif

namespace rsim_clear {
using namespace rsim_dist;

// The body table, RSIM_CLEAR_REC ints per element, moved bodies in topological order (parents first), each followed by its joints:
//   CL_BODY                      o1 = float-table offset of body_pos, o2 = of body_quat, id = body id, slot = its slot in the pose store,
//                                pslot = the parent's slot or -1 (the parent is not moved: its pose is the env's), pbody = the parent's body id
//   CL_BALL / CL_SLIDE / CL_HINGE (the model's joint type codes)   o1 = jnt_pos, o2 = jnt_axis, id = qpos address, col = controlled column or -1 (held at
//                                the env's qpos), o3 = offset of qpos0 (a ball joint has none)
#define RSIM_CLEAR_REC 8
enum { CL_BODY = 0, CL_BALL = 1, CL_SLIDE = 2, CL_HINGE = 3 };
enum { CLE_KIND, CLE_O1, CLE_O2, CLE_ID, CLE_COL, CLE_O3, CLE_SLOT, CLE_PBODY };   // (a CL_BODY keeps pslot in CLE_COL)

struct Pose { V3 p; Q4 q; };

// what one candidate reads: its env's float table, qpos and body poses, and its own joint vector
struct Cand { const float *ft, *qpos, *q, *xpos, *xquat; };

// where poses of moved bodies live: component k of entry i at pos[i * pe + k * ps] / quat[i * qe + k * qs].  The kernels' scratch is laid out
// [slot][7][candidates] (ps = qs = candidates: the 64 lanes of a wavefront touch 64 consecutive floats); the FK entry writes the caller's [nbody][3] / [nbody][4]
// rows of the candidate, indexed by body id (by_body).
struct PoseStore { float *pos, *quat; size_t pe, ps, qe, qs; int by_body; };

RSIM_HD Pose load_pose(const PoseStore& s, int i) {
  const float *p = s.pos + (size_t)i * s.pe, *q = s.quat + (size_t)i * s.qe;
  Pose r;
  r.p = v3(p[0], p[s.ps], p[2 * s.ps]);
  r.q.w = q[0]; r.q.x = q[s.qs]; r.q.y = q[2 * s.qs]; r.q.z = q[3 * s.qs];
  return r;
}
RSIM_HD void store_pose(const PoseStore& s, int i, const Pose& r) {
  float *p = s.pos + (size_t)i * s.pe, *q = s.quat + (size_t)i * s.qe;
  p[0] = r.p.x; p[s.ps] = r.p.y; p[2 * s.ps] = r.p.z;
  q[0] = r.q.w; q[s.qs] = r.q.x; q[2 * s.qs] = r.q.y; q[3 * s.qs] = r.q.z;
}
RSIM_HD Pose env_pose(const Cand& c, int body) {
  Pose r;
  r.p = ld3(c.xpos + 3 * (size_t)body); r.q = ldq(c.xquat + 4 * (size_t)body);
  return r;
}

// ---- the per-body FK step ---------------------------------------------------------------------------------------------------------------------------------
RSIM_HD Pose fk_body(const Pose& parent, const float* ft, int o_pos, int o_quat) {
  Pose r;
  r.p = parent.p + qrot(parent.q, ld3(ft + o_pos));
  r.q = qmul(parent.q, ldq(ft + o_quat));
  return r;
}
RSIM_HD Pose fk_joint(const Pose& cur, int kind, const float* ft, int o_jpos, int o_axis, float x, const float* ball) {
  Pose r = cur;
  const V3 jp = ld3(ft + o_jpos);
  if (kind == CL_SLIDE) {
    r.p = cur.p + qrot(cur.q, ld3(ft + o_axis)) * x;
  } else {
    const V3 anchor = cur.p + qrot(cur.q, jp);
    Q4 ql;
    if (kind == CL_HINGE) {
      const V3 ja = ld3(ft + o_axis);
      float sn, cs;
      sincos_f(0.5f * x, sn, cs);
      ql.w = cs; ql.x = ja.x * sn; ql.y = ja.y * sn; ql.z = ja.z * sn;
    } else {
      ql = qunit(ldq(ball));
    }
    r.q = qmul(cur.q, ql);
    r.p = anchor - qrot(r.q, jp);
  }
  return r;
}

// the value of controlled column `col`: the candidate's own entry.  (The swept query hands fk_walk another one: a point on a segment, rsim_sweep_core.h.)
struct CandQ {
  const float* q;
  RSIM_HD float operator()(int col) const { return q[col]; }
};

// Walks the table and stores the pose of every moved body.  `last` is the body before in registers: a chain reads its parent from there, a branch from the store
// (what this very candidate wrote earlier in the walk).  qv(col) is the position of controlled column col.
template <class JointValue>
RSIM_HD void fk_walk(const int* tab, int nel, const Cand& c, const PoseStore& st, const JointValue& qv) {
  Pose cur, last;
  cur.p = last.p = v3(0, 0, 0);
  cur.q.w = last.q.w = 1.f; cur.q.x = cur.q.y = cur.q.z = last.q.x = last.q.y = last.q.z = 0.f;
  int cur_slot = -1, cur_body = 0, last_slot = -1;
  for (int e = 0; e <= nel; e++) {
    const int* el = tab + (size_t)RSIM_CLEAR_REC * (e < nel ? e : 0);
    const int kind = e < nel ? RSIM_CLEAR_U(el[CLE_KIND]) : CL_BODY;
    if (kind == CL_BODY) {
      if (cur_slot >= 0) {   // the body before is complete
        cur.q = qunit(cur.q);
        store_pose(st, st.by_body ? cur_body : cur_slot, cur);
        last = cur; last_slot = cur_slot;
      }
      if (e == nel) break;
      const int pslot = RSIM_CLEAR_U(el[CLE_COL]), pbody = RSIM_CLEAR_U(el[CLE_PBODY]);
      Pose par;
      if (pslot < 0) par = env_pose(c, pbody);
      else if (pslot == last_slot) par = last;
      else par = load_pose(st, st.by_body ? pbody : pslot);
      cur = fk_body(par, c.ft, RSIM_CLEAR_U(el[CLE_O1]), RSIM_CLEAR_U(el[CLE_O2]));
      cur_slot = RSIM_CLEAR_U(el[CLE_SLOT]); cur_body = RSIM_CLEAR_U(el[CLE_ID]);
    } else {
      const int col = RSIM_CLEAR_U(el[CLE_COL]), qadr = RSIM_CLEAR_U(el[CLE_ID]);
      float x = 0.f;
      if (kind != CL_BALL) x = (col >= 0 ? qv(col) : c.qpos[qadr]) - c.ft[RSIM_CLEAR_U(el[CLE_O3])];
      cur = fk_joint(cur, kind, c.ft, RSIM_CLEAR_U(el[CLE_O1]), RSIM_CLEAR_U(el[CLE_O2]), x, c.qpos + qadr);
    }
  }
}
RSIM_HD void fk_walk(const int* tab, int nel, const Cand& c, const PoseStore& st) {
  const CandQ qv = {c.q};
  fk_walk(tab, nel, c, st, qv);
}

// ---- the pair loop ----------------------------------------------------------------------------------------------------------------------------------------
// the scene the pairs refer to: GeomRec is the ray kernel's scene record (rsim_ray.h DRayGeom: type, body, cg, size, pos, quat), pairs the distance query's
// pair table (rsim_dist.h: geom1, geom2, first hull vertex and vertex count of each), slot_of_body the pose-store slot of a moved body or -1
template <class GeomRec>
struct Scene {
  const GeomRec* geom;
  const int* pairs;
  int rec;                 // ints per pair record
  const int* slot_of_body;
  const float* mesh_vert;
  int fo_size, fo_pos, fo_quat;
};
struct Best { float dist; int pair, status; V3 p1, p2; };

template <class GeomRec>
RSIM_HD Geom load_geom(const Scene<GeomRec>& sc, int g, const Cand& c, const PoseStore& st, int vadr, int vnum) {
  const GeomRec& s = sc.geom[g];
  const int cg = RSIM_CLEAR_U(s.cg), body = RSIM_CLEAR_U(s.body);
  V3 size = ld3(s.size), lp = ld3(s.pos);
  Q4 lq = ldq(s.quat);
  if (cg >= 0) { size = ld3(c.ft + sc.fo_size + 3 * cg); lp = ld3(c.ft + sc.fo_pos + 3 * cg); lq = ldq(c.ft + sc.fo_quat + 4 * cg); }
  const int slot = RSIM_CLEAR_U(sc.slot_of_body[body]);
  const Pose b = slot >= 0 ? load_pose(st, slot) : env_pose(c, body);
  return make_geom(RSIM_CLEAR_U(s.type), size, b.p + qrot(b.q, lp), qunit(qmul(b.q, lq)), sc.mesh_vert + 3 * (size_t)vadr, vnum);
}

// the smallest distance over pairs [p0, p1) at the candidate's poses; nothing closer than distmax: (distmax, -1, DIST_FAR, zeros)
template <class GeomRec>
RSIM_HD Best clear_pairs(const Scene<GeomRec>& sc, int p0, int p1, const Cand& c, const PoseStore& st, float distmax, float tol, int max_iters) {
  Best best;
  best.dist = distmax; best.pair = -1; best.status = DIST_FAR; best.p1 = best.p2 = v3(0, 0, 0);
  for (int p = p0; p < p1; p++) {
    const int* rec = sc.pairs + (size_t)p * sc.rec;
    const int g1 = RSIM_CLEAR_U(rec[0]), g2 = RSIM_CLEAR_U(rec[1]);
    Geom A = load_geom(sc, g1, c, st, RSIM_CLEAR_U(rec[2]), RSIM_CLEAR_U(rec[3]));
    Geom Bg = load_geom(sc, g2, c, st, RSIM_CLEAR_U(rec[4]), RSIM_CLEAR_U(rec[5]));
    const V3 org = A.p;
    A.p = v3(0, 0, 0); Bg.p = Bg.p - org;
    const Result r = pair_distance(A, Bg, best.dist, tol, max_iters);
    const bool take = (r.status & DIST_FAR) == 0 && r.dist < best.dist;
    best.dist = take ? r.dist : best.dist;
    best.pair = take ? p : best.pair;
    best.status = take ? r.status : best.status;
    best.p1 = sel(take, r.p1 + org, best.p1); best.p2 = sel(take, r.p2 + org, best.p2);
  }
  return best;
}
}  // namespace rsim_clear
