// rsim_dyn_core.h -- the per-candidate core of the dynamics queries (rsim_config_inverse_dynamics / rsim_config_mass_matrix / rsim_config_jacobian, rsim_dyn.hip):
// fp32 __host__ __device__ functions on top of rsim_grad_core.h, in its way.  The kernels include it; so does tests/san/dyn_core_driver.cpp, which runs the very
// same source on the host under AddressSanitizer + UndefinedBehaviorSanitizer.  robosuite_amd/dynamics.py is the fp64 statement by the definition.
//
//  * WHAT IS THERE ALREADY.  fk_walk has left the poses of the moved bodies in the pose store, joint_walk world axis and anchor of every controlled column in the
//    joint store.  Only controlled joints move (every other joint has zero velocity and acceleration), so the joint store holds every motion axis there is.
//  * THE REFERENCE POINT.  All spatial quantities are world-frame vectors taken about ONE point `org`, fixed in the world: the candidate's position of the first
//    moved body (slot 0 of the pose store), which sits on the mechanism.  Levers are then the mechanism's own reach, not its distance from the world origin, and
//    because every body uses the same point wrenches and composite inertias of a subtree ADD, with no transport between bodies.
//    A motion vector is (w, v): angular velocity and the velocity of the body-fixed point that passes through org.  Hinge column: (a, (anchor - org) x a);
//    slide column: (0, a).  A force vector is (n, f): moment about org and force.
//  * INVERSE DYNAMICS (rne_walk), recursive Newton-Euler in that frame.  Forward over the body table:  V_b = V_parent + sum S_j qd_j,
//    A_b = A_parent + sum (S_j qdd_j + (V x S_j) qd_j),  A of an unmoved parent = (0, -g): gravity as an acceleration of the base.  The body's wrench is
//    f = m a_c,  a_c = A.v + A.w x r + V.w x (V.v + V.w x r),  r = com - org;   n = R (I R^T A.w + (R^T V.w) x I R^T V.w) + r x f,  R = body quaternion o iquat.
//    V, A and the wrench go to the lane's own words of the dynamics scratch, [slot][18][candidates].  Backward over the same table: a body's wrench, by then its
//    subtree's, is projected on the body's controlled joints (tau_c = S_c . W + armature qdd_c + damping qd_c) and added into its parent's.
//  * MASS MATRIX (crb_walk), composite rigid bodies.  Forward: every body's own inertia about org (mass, first moment h = m r, the six entries of
//    I_org = R I R^T + m (r.r E - r r^T)) into the scratch, [slot][10][candidates].  Backward: a body's words, by then its subtree's, give F = I_c S_i for each of
//    its controlled joints i, and M_ij = M_ji = S_j . F for every controlled column j on the body's path that sits AT OR BEFORE i in the table -- one product per
//    unordered pair, written to both triangles, so M is symmetric bit for bit; columns on different branches are never paired and stay exactly 0.  The diagonal
//    gains dof_armature.  The lane zeroes its n x n words first.
//  * JACOBIAN (site_jac): column c of mj_jacSite is a_c x (p - anchor_c) | a_c for a hinge, a_c | 0 for a slide, if bit c of the site body's signature is set.
//  * No accumulator array lives in registers: tau, M and J are written straight to the lane's own words of the result (rsim_grad_core.h records why).
//    Every loop is bounded by the table length or by n <= RSIM_JNT_MAX.  Attachments are not carried: a CL_ATTACH element is passed over (the host refuses them).
#pragma once
#include "rsim_grad_core.h"

#define RSIM_DYN_RNE_WORDS 18      // V (6), A (6), wrench (6) per slot
#define RSIM_DYN_CRB_WORDS 10      // mass, first moment (3), inertia about org xx yy zz xy xz yz per slot
#define RSIM_DYN_COL 2             // ints per controlled column in the column table: dof id, element of the body table that holds the joint

namespace rsim_dyn {
using namespace rsim_grad;

struct Sv { V3 w, v; };   // a motion vector (angular, linear at org) or a force vector (moment about org, force)

// where the per-body words live: word k of slot i at a[i * se + k * ss].  The kernels' scratch is [slot][words][candidates] (ss = candidates).
struct DynStore { float* a; size_t se, ss; };
RSIM_HD Sv load_sv(const DynStore& s, int slot, int k0) {
  const float* p = s.a + (size_t)slot * s.se + (size_t)k0 * s.ss;
  Sv r;
  r.w = v3(p[0], p[s.ss], p[2 * s.ss]); r.v = v3(p[3 * s.ss], p[4 * s.ss], p[5 * s.ss]);
  return r;
}
RSIM_HD void store_sv(const DynStore& s, int slot, int k0, const Sv& x) {
  float* p = s.a + (size_t)slot * s.se + (size_t)k0 * s.ss;
  p[0] = x.w.x; p[s.ss] = x.w.y; p[2 * s.ss] = x.w.z; p[3 * s.ss] = x.v.x; p[4 * s.ss] = x.v.y; p[5 * s.ss] = x.v.z;
}

// float-table offsets of the model terms (rsim_internal.h FO_*; entry i of a field at its offset + width * i), and the column table [n][RSIM_DYN_COL]
struct DynModel { int fo_mass, fo_inertia, fo_ipos, fo_iquat, fo_armature, fo_damping, fo_opt; const int* cols; };

RSIM_HD V3 dyn_origin(const PoseStore& st) { return load_pose(st, 0).p; }   // (by slot: the scratch)

// the motion vector of controlled column col about org
RSIM_HD Sv joint_motion(const JointStore& js, int col, bool slide, const V3& org) {
  const float* w = js.a + (size_t)col * js.ce;
  const V3 a = v3(w[0], w[js.cs], w[2 * js.cs]), o = v3(w[3 * js.cs], w[4 * js.cs], w[5 * js.cs]);
  Sv s;
  s.w = slide ? v3(0, 0, 0) : a;
  s.v = slide ? a : cross(o - org, a);
  return s;
}
RSIM_HD float sv_dot(const Sv& m, const Sv& f) { return dot(m.w, f.w) + dot(m.v, f.v); }
RSIM_HD Q4 qconj(Q4 q) { q.x = -q.x; q.y = -q.y; q.z = -q.z; return q; }

// centre of mass relative to org and inertial orientation of body `body` at the stored pose of its slot
RSIM_HD void body_inertial(const Cand& c, const PoseStore& st, const DynModel& dm, int slot, int body, const V3& org, V3& r, Q4& qi) {
  const Pose p = load_pose(st, slot);
  r = p.p + qrot(p.q, ld3(c.ft + dm.fo_ipos + 3 * body)) - org;
  qi = qunit(qmul(p.q, ldq(c.ft + dm.fo_iquat + 4 * body)));
}

// the wrench about org that moves body `body` with velocity V and acceleration A (gravity is inside A)
RSIM_HD Sv body_wrench(const Cand& c, const PoseStore& st, const DynModel& dm, int slot, int body, const V3& org, const Sv& V, const Sv& A) {
  V3 r;
  Q4 qi;
  body_inertial(c, st, dm, slot, body, org, r, qi);
  const float m = c.ft[dm.fo_mass + body];
  const V3 I = ld3(c.ft + dm.fo_inertia + 3 * body);
  const V3 ac = A.v + cross(A.w, r) + cross(V.w, V.v + cross(V.w, r));
  const Q4 qc = qconj(qi);
  const V3 wl = qrot(qc, V.w), al = qrot(qc, A.w);
  const V3 Iw = v3(I.x * wl.x, I.y * wl.y, I.z * wl.z);
  const V3 nl = v3(I.x * al.x, I.y * al.y, I.z * al.z) + cross(wl, Iw);
  Sv W;
  W.v = ac * m;
  W.w = qrot(qi, nl) + cross(r, W.v);
  return W;
}

// tau[col * ts] for every controlled column: inverse dynamics of the candidate at velocity qd and acceleration qdd of the controlled columns (null: zeros)
RSIM_HD void rne_walk(const int* tab, int nel, const Cand& c, const PoseStore& st, const JointStore& js, const DynModel& dm, unsigned slide_mask, const float* qd,
                      const float* qdd, const DynStore& ds, float* tau, size_t ts) {
  const V3 org = dyn_origin(st), zero = v3(0, 0, 0);
  const V3 grav = ld3(c.ft + dm.fo_opt + 1);
  Sv V, A, lastV, lastA;
  V.w = V.v = A.w = A.v = lastV.w = lastV.v = lastA.w = lastA.v = zero;
  int cur_slot = -1, cur_body = 0, last_slot = -1;
  for (int e = 0; e <= nel; e++) {
    const int* el = tab + (size_t)RSIM_CLEAR_REC * (e < nel ? e : 0);
    const int kind = e < nel ? RSIM_CLEAR_U(el[CLE_KIND]) : CL_BODY;
    if (kind == CL_ATTACH) continue;
    if (kind == CL_BODY) {
      if (cur_slot >= 0) {   // the body before is complete
        store_sv(ds, cur_slot, 0, V); store_sv(ds, cur_slot, 6, A);
        store_sv(ds, cur_slot, 12, body_wrench(c, st, dm, cur_slot, cur_body, org, V, A));
        lastV = V; lastA = A; last_slot = cur_slot;
      }
      if (e == nel) break;
      const int pslot = RSIM_CLEAR_U(el[CLE_COL]);
      cur_slot = RSIM_CLEAR_U(el[CLE_SLOT]); cur_body = RSIM_CLEAR_U(el[CLE_ID]);
      if (pslot < 0) { V.w = V.v = A.w = zero; A.v = -grav; }
      else if (pslot == last_slot) { V = lastV; A = lastA; }
      else { V = load_sv(ds, pslot, 0); A = load_sv(ds, pslot, 6); }
    } else {
      const int col = RSIM_CLEAR_U(el[CLE_COL]);
      if (col < 0 || kind == CL_BALL) continue;   // held: no velocity, no acceleration
      const Sv S = joint_motion(js, col, (slide_mask >> col) & 1u, org);
      const float x = qd ? qd[col] : 0.f, xx = qdd ? qdd[col] : 0.f;
      const V3 dw = cross(V.w, S.w), dv = cross(V.w, S.v) + cross(V.v, S.w);   // V x S: the axis rides on the body
      A.w = A.w + S.w * xx + dw * x; A.v = A.v + S.v * xx + dv * x;
      V.w = V.w + S.w * x; V.v = V.v + S.v * x;
    }
  }
  for (int e = nel - 1; e >= 0; e--) {
    const int* el = tab + (size_t)RSIM_CLEAR_REC * e;
    if (RSIM_CLEAR_U(el[CLE_KIND]) != CL_BODY) continue;
    const int slot = RSIM_CLEAR_U(el[CLE_SLOT]), pslot = RSIM_CLEAR_U(el[CLE_COL]);
    const Sv W = load_sv(ds, slot, 12);   // every child has been added: the subtree's
    for (int j = e + 1; j < nel; j++) {
      const int* ej = tab + (size_t)RSIM_CLEAR_REC * j;
      const int kj = RSIM_CLEAR_U(ej[CLE_KIND]);
      if (kj == CL_BODY || kj == CL_ATTACH) break;
      const int col = RSIM_CLEAR_U(ej[CLE_COL]);
      if (col < 0 || kj == CL_BALL) continue;
      const int dof = RSIM_CLEAR_U(dm.cols[RSIM_DYN_COL * col]);
      const float x = qd ? qd[col] : 0.f, xx = qdd ? qdd[col] : 0.f;
      tau[(size_t)col * ts] = sv_dot(joint_motion(js, col, (slide_mask >> col) & 1u, org), W) + c.ft[dm.fo_armature + dof] * xx + c.ft[dm.fo_damping + dof] * x;
    }
    if (pslot >= 0) {
      Sv P = load_sv(ds, pslot, 12);
      P.w = P.w + W.w; P.v = P.v + W.v;
      store_sv(ds, pslot, 12, P);
    }
  }
}

// a body's own inertia about org: mass, first moment, I_org
struct Inertia { float m; V3 h; float xx, yy, zz, xy, xz, yz; };
RSIM_HD Inertia load_inertia(const DynStore& s, int slot) {
  const float* p = s.a + (size_t)slot * s.se;
  Inertia r;
  r.m = p[0]; r.h = v3(p[s.ss], p[2 * s.ss], p[3 * s.ss]);
  r.xx = p[4 * s.ss]; r.yy = p[5 * s.ss]; r.zz = p[6 * s.ss]; r.xy = p[7 * s.ss]; r.xz = p[8 * s.ss]; r.yz = p[9 * s.ss];
  return r;
}
RSIM_HD void store_inertia(const DynStore& s, int slot, const Inertia& r) {
  float* p = s.a + (size_t)slot * s.se;
  p[0] = r.m; p[s.ss] = r.h.x; p[2 * s.ss] = r.h.y; p[3 * s.ss] = r.h.z;
  p[4 * s.ss] = r.xx; p[5 * s.ss] = r.yy; p[6 * s.ss] = r.zz; p[7 * s.ss] = r.xy; p[8 * s.ss] = r.xz; p[9 * s.ss] = r.yz;
}
RSIM_HD Inertia body_inertia(const Cand& c, const PoseStore& st, const DynModel& dm, int slot, int body, const V3& org) {
  V3 r;
  Q4 qi;
  body_inertial(c, st, dm, slot, body, org, r, qi);
  const float m = c.ft[dm.fo_mass + body];
  const V3 I = ld3(c.ft + dm.fo_inertia + 3 * body);
  const V3 ux = qrot(qi, v3(1, 0, 0)), uy = qrot(qi, v3(0, 1, 0)), uz = qrot(qi, v3(0, 0, 1));   // the principal axes in the world
  const float rr = dot(r, r);
  Inertia o;
  o.m = m; o.h = r * m;
  o.xx = I.x * ux.x * ux.x + I.y * uy.x * uy.x + I.z * uz.x * uz.x + m * (rr - r.x * r.x);
  o.yy = I.x * ux.y * ux.y + I.y * uy.y * uy.y + I.z * uz.y * uz.y + m * (rr - r.y * r.y);
  o.zz = I.x * ux.z * ux.z + I.y * uy.z * uy.z + I.z * uz.z * uz.z + m * (rr - r.z * r.z);
  o.xy = I.x * ux.x * ux.y + I.y * uy.x * uy.y + I.z * uz.x * uz.y - m * r.x * r.y;
  o.xz = I.x * ux.x * ux.z + I.y * uy.x * uy.z + I.z * uz.x * uz.z - m * r.x * r.z;
  o.yz = I.x * ux.y * ux.z + I.y * uy.y * uy.z + I.z * uz.y * uz.z - m * r.y * r.z;
  return o;
}
// the momentum (as a force vector about org) of inertia C moving with S:  f = m v - h x w,  n = I_org w + h x v
RSIM_HD Sv inertia_mul(const Inertia& C, const Sv& S) {
  Sv F;
  F.v = S.v * C.m - cross(C.h, S.w);
  F.w = v3(C.xx * S.w.x + C.xy * S.w.y + C.xz * S.w.z, C.xy * S.w.x + C.yy * S.w.y + C.yz * S.w.z, C.xz * S.w.x + C.yz * S.w.y + C.zz * S.w.z) + cross(C.h, S.v);
  return F;
}

// M[i * n + j] for the controlled columns: the block of the joint-space inertia at the candidate, dof_armature on the diagonal, both triangles.  sig [nbody]: the
// dof signatures (low 16 bits)
RSIM_HD void crb_walk(const int* tab, int nel, const Cand& c, const PoseStore& st, const JointStore& js, const DynModel& dm, int n, unsigned slide_mask,
                      const int* sig, const DynStore& ds, float* M) {
  const V3 org = dyn_origin(st);
  for (int i = 0; i < n * n; i++) M[i] = 0.f;
  for (int e = 0; e < nel; e++) {
    const int* el = tab + (size_t)RSIM_CLEAR_REC * e;
    if (RSIM_CLEAR_U(el[CLE_KIND]) != CL_BODY) continue;
    const int slot = RSIM_CLEAR_U(el[CLE_SLOT]);
    store_inertia(ds, slot, body_inertia(c, st, dm, slot, RSIM_CLEAR_U(el[CLE_ID]), org));
  }
  for (int e = nel - 1; e >= 0; e--) {
    const int* el = tab + (size_t)RSIM_CLEAR_REC * e;
    if (RSIM_CLEAR_U(el[CLE_KIND]) != CL_BODY) continue;
    const int slot = RSIM_CLEAR_U(el[CLE_SLOT]), pslot = RSIM_CLEAR_U(el[CLE_COL]);
    const unsigned path = (unsigned)RSIM_CLEAR_U(sig[RSIM_CLEAR_U(el[CLE_ID])]) & 0xffffu;
    const Inertia C = load_inertia(ds, slot);   // every child has been added: the subtree's
    for (int ei = e + 1; ei < nel; ei++) {
      const int* eli = tab + (size_t)RSIM_CLEAR_REC * ei;
      const int ki = RSIM_CLEAR_U(eli[CLE_KIND]);
      if (ki == CL_BODY || ki == CL_ATTACH) break;
      const int i = RSIM_CLEAR_U(eli[CLE_COL]);
      if (i < 0 || ki == CL_BALL) continue;
      const Sv F = inertia_mul(C, joint_motion(js, i, (slide_mask >> i) & 1u, org));
      for (int j = 0; j < n; j++) {
        if (!((path >> j) & 1u) || RSIM_CLEAR_U(dm.cols[RSIM_DYN_COL * j + 1]) > ei) continue;   // not above this joint (a later joint of the body pairs from its side)
        float v = sv_dot(joint_motion(js, j, (slide_mask >> j) & 1u, org), F);
        if (j == i) v += c.ft[dm.fo_armature + RSIM_CLEAR_U(dm.cols[RSIM_DYN_COL * i])];
        M[(size_t)i * n + j] = v; M[(size_t)j * n + i] = v;
      }
    }
    if (pslot >= 0) {
      Inertia P = load_inertia(ds, pslot);
      P.m += C.m; P.h = P.h + C.h;
      P.xx += C.xx; P.yy += C.yy; P.zz += C.zz; P.xy += C.xy; P.xz += C.xz; P.yz += C.yz;
      store_inertia(ds, pslot, P);
    }
  }
}

// jacp / jacr [3][n] (either may be null) of a point p riding on a body with dof signature `path`
RSIM_HD void site_jac(const JointStore& js, int n, unsigned slide_mask, unsigned path, const V3& p, float* jacp, float* jacr) {
  for (int col = 0; col < n; col++) {
    const float* w = js.a + (size_t)col * js.ce;
    const V3 a = v3(w[0], w[js.cs], w[2 * js.cs]), o = v3(w[3 * js.cs], w[4 * js.cs], w[5 * js.cs]);
    const bool on = (path >> col) & 1u, slide = (slide_mask >> col) & 1u;
    const V3 lin = !on ? v3(0, 0, 0) : slide ? a : cross(a, p - o), rot = on && !slide ? a : v3(0, 0, 0);
    if (jacp) { jacp[col] = lin.x; jacp[n + col] = lin.y; jacp[2 * n + col] = lin.z; }
    if (jacr) { jacr[col] = rot.x; jacr[n + col] = rot.y; jacr[2 * n + col] = rot.z; }
  }
}
// the world position of a site at local position o_site (float-table offset) on body `body` (slot: its pose-store slot or -1: the env's pose)
RSIM_HD V3 site_point(const Cand& c, const PoseStore& st, int slot, int body, int o_site) {
  const Pose b = slot >= 0 ? load_pose(st, slot) : env_pose(c, body);
  return b.p + qrot(b.q, ld3(c.ft + o_site));
}
}  // namespace rsim_dyn
