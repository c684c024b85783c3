// rsim_ik_avoid_core.h -- the per-problem core of collision-aware inverse kinematics (rsim_ik_site_avoid, rsim_ik_avoid.hip): fp32 __host__ __device__ functions
// on top of rsim_grad_core.h, in its way.  The kernels include it; so does tests/san/ik_avoid_core_driver.cpp, which runs the very same source on the host under
// AddressSanitizer + UndefinedBehaviorSanitizer.  robosuite_amd/ik_avoid.py is the fp64 statement of the iteration.
//
//  * One problem = one candidate of the clearance cores: its joint vector q lives in ITS OWN global words (the call's q_out), which fk_walk, joint_walk and
//    cost_pairs read as Cand::q.  So do q_rest, the summed gradient and the step: nothing is an array in registers, nothing is indexed at run time.
//  * ika_start clamps the start vector into q and q_rest.  ika_step is one evaluation and, unless the problem stops, one update:
//      - cost, counts and gradient: the pair chunks' partial results added in chunk order (k_clear_cost_sum's rule); the summed gradient goes back into
//        chunk 0's words;
//      - the site pose from the site body's STORED pose (what fk_walk left) and site_pos / site_quat of the env's float table; the error as rsim_ik.hip forms it;
//      - conv = rsim_ik_site's test, finished = conv and cost <= cost_tol; stop if finished or it >= max_iters;
//      - J column by column from the joint store -- zero unless the column's bit is set in the site body's dof signature; hinge: a x (p - anchor) linear, a
//        angular; slide: a linear; a position-only target zeroes the angular rows -- accumulating the 21 entries of J J^T and the 6 of J v,
//        v = posture_gain (q_rest - q) - avoid_gain g;
//      - a fully unrolled 6 x 6 Cholesky with rsim_ik.hip's pivot floor; dq = J^T A^-1 e + v - J^T A^-1 (J v), kept in the gradient's words; scaled to max_dq;
//        q <- clamp(q + dq).
//    J is never held: a column is formed where it is used, twice per update.
//  * Every loop is bounded by n (<= RSIM_GRAD_COLS) or the chunk count.
#pragma once
#include <string.h>
#include "rsim_grad_core.h"

#define RSIM_IKA_PART 3            // rsim_grad.h RSIM_GRAD_PART: words of a chunk's partial result in front of its n gradient entries
#define RSIM_IKA_HEAD 4            // ints per controlled column in the head table: float-table offset of jnt_range, jnt_limited, qpos address, joint type
#define RSIM_IKA_CONV (1 << 30)    // include/rsim.h: bits of iters
#define RSIM_IKA_FIN (1 << 29)
#if defined(__clang__)
#define RSIM_IKA_UNROLL _Pragma("unroll")
#else
#define RSIM_IKA_UNROLL
#endif

namespace rsim_ika {
using namespace rsim_grad;

// A = L L^T in place (lower triangle) for the symmetric positive definite 6 x 6 A, then x <- A^-1 x: rsim_ik.hip's, with its pivot floor, every index a
// compile-time constant
struct Chol6 {
  float L[6][6];
  RSIM_HD void factor() {
RSIM_IKA_UNROLL
    for (int j = 0; j < 6; j++) {
      float d = L[j][j];
RSIM_IKA_UNROLL
      for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k];
      d = sqrtf(fmaxf(d, 1e-30f));
      L[j][j] = d;
      const float inv = 1.f / d;
RSIM_IKA_UNROLL
      for (int i = j + 1; i < 6; i++) {
        float s = L[i][j];
RSIM_IKA_UNROLL
        for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
        L[i][j] = s * inv;
      }
    }
  }
  RSIM_HD void solve(float (&x)[6]) const {
RSIM_IKA_UNROLL
    for (int i = 0; i < 6; i++) {
      float s = x[i];
RSIM_IKA_UNROLL
      for (int k = 0; k < i; k++) s -= L[i][k] * x[k];
      x[i] = s / L[i][i];
    }
RSIM_IKA_UNROLL
    for (int i = 5; i >= 0; i--) {
      float s = x[i];
RSIM_IKA_UNROLL
      for (int k = i + 1; k < 6; k++) s -= L[k][i] * x[k];
      x[i] = s / L[i][i];
    }
  }
};

// the call's options and the site, the same for every problem
struct Opts {
  int n, rows, max_iters, clamp_range;   // rows: 6 (pose) or 3 (position only)
  float damping, max_dq, pos_tol, rot_tol, posture_gain, avoid_gain, cost_tol;
  const int* head;                       // [n][RSIM_IKA_HEAD]
  unsigned slide_mask, site_sig;         // bit c: column c is a slide joint / is on the site body's path
  int site_slot, o_site_pos, o_site_quat;   // the site body's slot in the pose store; float-table offsets of site_pos / site_quat
};
// what one problem reads and writes: its own words.  q / q_rest [n] contiguous; part: word w of chunk k at part[k * part_ks + w * part_ws] (the kernels'
// [chunks][RSIM_IKA_PART + n][problems] with part_ws = problems); target: pos [3], quat [4] wxyz or null
struct Prob {
  float *q, *q_rest;
  float* part; size_t part_ks, part_ws; int chunks;
  const float *tpos, *tquat;
};
struct Eval { float en, wn, cost; int nnear, nover, conv, fin; };

RSIM_HD void ika_range(const Opts& o, const float* ft, int col, float& lo, float& hi) {
  lo = -3.0e38f; hi = 3.0e38f;
  const int* h = o.head + RSIM_IKA_HEAD * col;
  if (o.clamp_range && RSIM_CLEAR_U(h[1])) { lo = ft[RSIM_CLEAR_U(h[0])]; hi = ft[RSIM_CLEAR_U(h[0]) + 1]; }
}

// q <- clamp(q_init or the env's qpos), q_rest = q
RSIM_HD void ika_start(const Opts& o, const float* ft, const float* qpos, const float* q_init, float* q, float* q_rest) {
  for (int col = 0; col < o.n; col++) {
    float lo, hi;
    ika_range(o, ft, col, lo, hi);
    const float v = fminf(fmaxf(q_init ? q_init[col] : qpos[RSIM_CLEAR_U(o.head[RSIM_IKA_HEAD * col + 2])], lo), hi);
    q[col] = v; q_rest[col] = v;
  }
}

// column col of J = [linear; angular] at site position p, from the joint store
RSIM_HD void ika_column(const Opts& o, const JointStore& js, int col, const V3& p, float (&J)[6]) {
  const float* w = js.a + (size_t)col * js.ce;
  const V3 a = v3(w[0], w[js.cs], w[2 * js.cs]), an = v3(w[3 * js.cs], w[4 * js.cs], w[5 * js.cs]);
  const bool on = (o.site_sig >> col) & 1u, slide = (o.slide_mask >> col) & 1u, pose = o.rows == 6;
  const V3 l = slide ? a : cross(a, p - an);
  J[0] = on ? l.x : 0.f; J[1] = on ? l.y : 0.f; J[2] = on ? l.z : 0.f;
  const bool ang = on && pose && !slide;
  J[3] = ang ? a.x : 0.f; J[4] = ang ? a.y : 0.f; J[5] = ang ? a.z : 0.f;
}

// One evaluation at the problem's q (the pose store and the joint store hold its poses and joint frames, the partial results its cost) and, unless it stops
// (finished, or `it` updates made), one update of q.  -> the evaluation; `updated` says whether q moved.
RSIM_HD Eval ika_step(const Opts& o, const Prob& pr, const float* ft, const PoseStore& st, const JointStore& js, int it, bool& updated) {
  const int n = o.n;
  Eval ev;
  // ---- the chunks' partial results, in chunk order
  ev.cost = 0.f; ev.nnear = ev.nover = 0;
  for (int k = 0; k < pr.chunks; k++) {
    const float* w = pr.part + (size_t)k * pr.part_ks;
#if defined(__HIP_DEVICE_COMPILE__)
    ev.cost += w[0]; ev.nnear += __float_as_int(w[pr.part_ws]); ev.nover += __float_as_int(w[2 * pr.part_ws]);
#else
    int a, b;
    memcpy(&a, w + pr.part_ws, 4); memcpy(&b, w + 2 * pr.part_ws, 4);
    ev.cost += w[0]; ev.nnear += a; ev.nover += b;
#endif
  }
  // ---- the site pose and the error
  const Pose body = load_pose(st, o.site_slot);
  const V3 p = body.p + qrot(body.q, ld3(ft + o.o_site_pos));
  const Q4 r = qunit(qmul(body.q, ldq(ft + o.o_site_quat)));
  const bool pose = o.rows == 6;
  const V3 tp = ld3(pr.tpos);
  float err[6] = {tp.x - p.x, tp.y - p.y, tp.z - p.z, 0.f, 0.f, 0.f};
  if (pose) {
    const Q4 tq = qunit(ldq(pr.tquat));
    Q4 cj = r;
    cj.x = -cj.x; cj.y = -cj.y; cj.z = -cj.z;
    Q4 d = qmul(tq, cj);
    if (d.w < 0.f) { d.w = -d.w; d.x = -d.x; d.y = -d.y; d.z = -d.z; }
    const float s = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
    const float k = s > 1e-12f ? 2.f * atan2f(s, d.w) / s : 2.f;
    err[3] = d.x * k; err[4] = d.y * k; err[5] = d.z * k;
  }
  ev.en = sqrtf(err[0] * err[0] + err[1] * err[1] + err[2] * err[2]);
  ev.wn = sqrtf(err[3] * err[3] + err[4] * err[4] + err[5] * err[5]);
  ev.conv = (ev.en < o.pos_tol && (!pose || ev.wn < o.rot_tol)) ? 1 : 0;
  ev.fin = (ev.conv && ev.cost <= o.cost_tol) ? 1 : 0;
  updated = !(ev.fin || it >= o.max_iters);
  if (!updated) return ev;

  // ---- A = J J^T + damping I and J v, column by column; the summed gradient goes into chunk 0's words
  const bool second = o.posture_gain > 0.f || o.avoid_gain > 0.f;
  float* g0 = pr.part + RSIM_IKA_PART * pr.part_ws;   // entry col at g0[col * part_ws]
  Chol6 C;
  float jv[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
RSIM_IKA_UNROLL
  for (int i = 0; i < 6; i++) {
RSIM_IKA_UNROLL
    for (int j = 0; j < 6; j++) C.L[i][j] = 0.f;
  }
  for (int col = 0; col < n; col++) {
    float J[6];
    ika_column(o, js, col, p, J);
RSIM_IKA_UNROLL
    for (int i = 0; i < 6; i++) {
RSIM_IKA_UNROLL
      for (int j = 0; j <= i; j++) C.L[i][j] += J[i] * J[j];
    }
    if (second) {
      float g = 0.f;
      for (int k = 0; k < pr.chunks; k++) g += pr.part[(size_t)k * pr.part_ks + (RSIM_IKA_PART + col) * pr.part_ws];
      const float v = o.posture_gain * (pr.q_rest[col] - pr.q[col]) - o.avoid_gain * g;
      g0[col * pr.part_ws] = v;   // (the gradient is used up: its words carry v, then dq)
RSIM_IKA_UNROLL
      for (int i = 0; i < 6; i++) jv[i] += J[i] * v;
    }
  }
RSIM_IKA_UNROLL
  for (int i = 0; i < 6; i++) C.L[i][i] += o.damping;
  C.factor();
  C.solve(err);
  if (second) C.solve(jv);
  // ---- dq = J^T A^-1 e + v - J^T A^-1 (J v), its largest entry, then the scaled and clamped update
  float big = 0.f;
  for (int col = 0; col < n; col++) {
    float J[6];
    ika_column(o, js, col, p, J);
    float dq = 0.f;
RSIM_IKA_UNROLL
    for (int i = 0; i < 6; i++) dq += J[i] * err[i];
    if (second) {
      float back = 0.f;
RSIM_IKA_UNROLL
      for (int i = 0; i < 6; i++) back += J[i] * jv[i];
      dq += g0[col * pr.part_ws] - back;
    }
    g0[col * pr.part_ws] = dq;
    big = fmaxf(big, fabsf(dq));
  }
  const float scale = big > o.max_dq ? o.max_dq / big : 1.f;
  for (int col = 0; col < n; col++) {
    float lo, hi;
    ika_range(o, ft, col, lo, hi);
    float dq = g0[col * pr.part_ws];
    if (big > o.max_dq) dq *= scale;
    pr.q[col] = fminf(fmaxf(pr.q[col] + dq, lo), hi);
  }
  return ev;
}
}  // namespace rsim_ika
