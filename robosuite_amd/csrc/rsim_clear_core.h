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
//  * ATTACHMENTS (include/rsim.h rsim_attach): a free body named in the call rides rigidly on a carrier body, X_body(q) = X_carrier(q) o rel, in the envs whose
//    `held` row says so; elsewhere it is the free body at its current pose that it always was, bit for bit.  The attached body and its subtree sit BEHIND the
//    ordinary moved bodies in the table (a carrier may have the larger body id) and always own a slot.  Every routine below is a template on ATT: ATT = false
//    compiles the attachment branches away, and that instantiation is what a call without attachments runs.  The per-lane data travels in an Att of its own,
//    so that Cand, Seg and Scene stay as the host rehearsals fill them.
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
//   CL_ATTACH                    an attached body, in place of its CL_BODY and of its free joint: id = body id, slot = its slot, col = the CARRIER's slot,
//                                pbody = the carrier's body id, o3 = the attachment's index in the call's list
// A CL_BODY below an attached body keeps that attachment's index + 1 in o3 (0 otherwise): where the attachment is not held it reads the env's pose.
#define RSIM_CLEAR_REC 8
#define RSIM_CLEAR_ATTACH_MAX 4   // include/rsim.h RSIM_ATTACH_MAX
enum { CL_BODY = 0, CL_BALL = 1, CL_SLIDE = 2, CL_HINGE = 3, CL_ATTACH = 4 };
enum { CLE_KIND, CLE_O1, CLE_O2, CLE_ID, CLE_COL, CLE_O3, CLE_SLOT, CLE_PBODY };   // (a CL_BODY keeps pslot in CLE_COL)

struct Pose { V3 p; Q4 q; };

// what one candidate reads: its env's float table, qpos and body poses, and its own joint vector
struct Cand { const float *ft, *qpos, *q, *xpos, *xquat; };

// what one candidate's env says about the call's attachments: bit i of held = attachment i is held in this env; rel = the env's [n][7] rows (position, wxyz
// quaternion of the body in the carrier's frame) or null: taken from the env's current poses.  body_sig / body_att, [nbody] each and the same for every lane,
// serve the pair loop's skip rule: the body's dof signature with its attachment unheld in the low 16 bits and held in the high ones; the index of the
// attachment the body belongs to (itself or above it), -1 for none.  body_sig == null: no pair is skipped (an explicit pair list).
struct Att { unsigned held; const float* rel; const int *body_sig, *body_att; };
// ... of env `env`, from the call's arrays: held [B][natt] bytes read once into the mask (null: every attachment is held), rel [B][natt][7] or null
RSIM_HD Att att_of_env(int natt, const unsigned char* held, const float* rel, const int* body_sig, const int* body_att, int env) {
  Att r;
  r.held = (1u << natt) - 1u;
  if (held) {
    r.held = 0u;
    for (int i = 0; i < natt; i++) r.held |= held[(size_t)env * natt + i] ? 1u << i : 0u;
  }
  r.rel = rel ? rel + (size_t)env * natt * 7 : nullptr;
  r.body_sig = body_sig; r.body_att = body_att;
  return r;
}

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

// the pose of an attached body in its carrier's frame: row `i` of the env's rel (the quaternion normalised), or from the env's current poses of the two,
// p_rel = R_c^T (p_b - p_c), q_rel = conj(q_c) q_b
RSIM_HD Pose attach_rel(const Att& at, int i, const Cand& c, int body, int carrier) {
  Pose r;
  if (at.rel) {
    r.p = ld3(at.rel + 7 * i); r.q = qunit(ldq(at.rel + 7 * i + 3));
  } else {
    const Pose pb = env_pose(c, body), pc = env_pose(c, carrier);
    Q4 cj = pc.q;
    cj.x = -cj.x; cj.y = -cj.y; cj.z = -cj.z;
    r.p = qrot(cj, pb.p - pc.p); r.q = qmul(cj, pb.q);
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
template <bool ATT, class JointValue>
RSIM_HD void fk_walk(const int* tab, int nel, const Cand& c, const PoseStore& st, const JointValue& qv, const Att& at) {
  Pose cur, last;
  cur.p = last.p = v3(0, 0, 0);
  cur.q.w = last.q.w = 1.f; cur.q.x = cur.q.y = cur.q.z = last.q.x = last.q.y = last.q.z = 0.f;
  int cur_slot = -1, cur_body = 0, last_slot = -1;
  bool cur_env = false;   // ATT: the body belongs to an attachment this env does not hold -- it keeps the env's pose
  for (int e = 0; e <= nel; e++) {
    const int* el = tab + (size_t)RSIM_CLEAR_REC * (e < nel ? e : 0);
    const int kind = e < nel ? RSIM_CLEAR_U(el[CLE_KIND]) : CL_BODY;
    if (kind == CL_BODY || (ATT && kind == CL_ATTACH)) {
      if (cur_slot >= 0) {   // the body before is complete
        cur.q = qunit(cur.q);
        if (ATT && cur_env) cur = env_pose(c, cur_body);   // bit for bit
        store_pose(st, st.by_body ? cur_body : cur_slot, cur);
        last = cur; last_slot = cur_slot;
      }
      if (e == nel) break;
      const int pslot = RSIM_CLEAR_U(el[CLE_COL]), pbody = RSIM_CLEAR_U(el[CLE_PBODY]);
      Pose par;
      if (pslot < 0) par = env_pose(c, pbody);
      else if (pslot == last_slot) par = last;
      else par = load_pose(st, st.by_body ? pbody : pslot);
      cur_slot = RSIM_CLEAR_U(el[CLE_SLOT]); cur_body = RSIM_CLEAR_U(el[CLE_ID]);
      if (ATT && kind == CL_ATTACH) {
        const int i = RSIM_CLEAR_U(el[CLE_O3]);
        const Pose rel = attach_rel(at, i, c, cur_body, pbody);
        cur.p = par.p + qrot(par.q, rel.p); cur.q = qmul(par.q, rel.q);
        cur_env = !((at.held >> i) & 1u);
      } else {
        cur = fk_body(par, c.ft, RSIM_CLEAR_U(el[CLE_O1]), RSIM_CLEAR_U(el[CLE_O2]));
        if (ATT) { const int i = RSIM_CLEAR_U(el[CLE_O3]); cur_env = i > 0 && !((at.held >> (i - 1)) & 1u); }
      }
    } else {
      const int col = RSIM_CLEAR_U(el[CLE_COL]), qadr = RSIM_CLEAR_U(el[CLE_ID]);
      float x = 0.f;
      if (kind != CL_BALL) x = (col >= 0 ? qv(col) : c.qpos[qadr]) - c.ft[RSIM_CLEAR_U(el[CLE_O3])];
      cur = fk_joint(cur, kind, c.ft, RSIM_CLEAR_U(el[CLE_O1]), RSIM_CLEAR_U(el[CLE_O2]), x, c.qpos + qadr);
    }
  }
}
template <class JointValue>
RSIM_HD void fk_walk(const int* tab, int nel, const Cand& c, const PoseStore& st, const JointValue& qv) {
  const Att none = {0u, nullptr, nullptr, nullptr};
  fk_walk<false>(tab, nel, c, st, qv, none);
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

// ATT: does this env evaluate the pair of bodies b1, b2?  Only if their dof signatures differ under its held row: a held body has its carrier's.
RSIM_HD unsigned body_sig_of(const Att& at, int body) {
  const unsigned s = (unsigned)RSIM_CLEAR_U(at.body_sig[body]);
  const int i = RSIM_CLEAR_U(at.body_att[body]);
  return i >= 0 && ((at.held >> i) & 1u) ? s >> 16 : s & 0xffffu;
}
RSIM_HD bool pair_active(const Att& at, int b1, int b2) { return !at.body_sig || body_sig_of(at, b1) != body_sig_of(at, b2); }

// the smallest distance over pairs [p0, p1) at the candidate's poses; nothing closer than distmax: (distmax, -1, DIST_FAR, zeros).  ATT: the pairs this lane's
// env does not evaluate are passed over -- a lane predicate, the table reads stay wave-uniform
template <bool ATT, class GeomRec>
RSIM_HD Best clear_pairs(const Scene<GeomRec>& sc, int p0, int p1, const Cand& c, const PoseStore& st, float distmax, float tol, int max_iters, const Att& at) {
  Best best;
  best.dist = distmax; best.pair = -1; best.status = DIST_FAR; best.p1 = best.p2 = v3(0, 0, 0);
  for (int p = p0; p < p1; p++) {
    const int* rec = sc.pairs + (size_t)p * sc.rec;
    const int g1 = RSIM_CLEAR_U(rec[0]), g2 = RSIM_CLEAR_U(rec[1]);
    if (ATT && !pair_active(at, RSIM_CLEAR_U(sc.geom[g1].body), RSIM_CLEAR_U(sc.geom[g2].body))) continue;
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
template <class GeomRec>
RSIM_HD Best clear_pairs(const Scene<GeomRec>& sc, int p0, int p1, const Cand& c, const PoseStore& st, float distmax, float tol, int max_iters) {
  const Att none = {0u, nullptr, nullptr, nullptr};
  return clear_pairs<false>(sc, p0, p1, c, st, distmax, tol, max_iters, none);
}
}  // namespace rsim_clear
