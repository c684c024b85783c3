// rsim_ik.hip -- inverse kinematics of a site over up to RSIM_JNT_MAX hinge / slide dofs, for the whole batch, on the device (rsim_ik_site): batched
// damped least-squares solves away from the stored state.
//
// Per (env, problem): q <- q_init; repeat { p, R, J = FK(q); err = [p* - p ; rotation vector of q* (x) conj(q_site)]; stop when converged or after
// max_iters updates; A = J J^T + damping I; dq = J^T A^-1 err (+ the posture term v - J^T A^-1 J v); scale to max_dq; q += dq; clamp to jnt_range }.
// robosuite_amd/ik.py is the fp64 host mirror of exactly this, and what the kernel is tested against.
//
// Like k_ray this is a kernel in a code object of its own that takes everything as its own kernel argument: the step kernels, DModel and DBatch do not
// know of it, and a batch that never solves launches and allocates nothing.  It is a pure query: it reads qpos and the env's float table and writes only
// q_out / err / iters.
//
// One wavefront = one (env, problem).  Lane j < n owns column j of J and q[j] / dq[j].  The chain from the world to the site (rsim_ik.h: at most 64
// bodies) is composed by every lane redundantly -- its table is read at wave-uniform addresses, the joint value of a controlled element comes from
// its owner lane by a shuffle -- and lane j keeps the anchor and axis of its own joint as the walk passes it.  The 21 entries of J J^T, the 6 of J v
// and max |dq| are reductions over the 16 low lanes; the 6 x 6 Cholesky factorisation and its solves are unrolled in registers, the same in every lane.
// A position-only problem zeroes the angular rows: A is then block diagonal and the angular part of the solution zero.  No array is indexed at run time.
#include <hip/hip_runtime.h>
#include "../../include/rsim.h"
#include "rsim_ik.h"
#include "rsim_vec.h"

namespace {
using namespace rsim_vec;
// sum / maximum over lanes 0 .. 15 (the lanes above hold zeros), the same value in every lane afterwards
__device__ __forceinline__ float first(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }
__device__ __forceinline__ float sum16(float x) {
  x += __shfl_xor(x, 8); x += __shfl_xor(x, 4); x += __shfl_xor(x, 2); x += __shfl_xor(x, 1);
  return first(x);
}
__device__ __forceinline__ float max16(float x) {
  x = fmaxf(x, __shfl_xor(x, 8)); x = fmaxf(x, __shfl_xor(x, 4)); x = fmaxf(x, __shfl_xor(x, 2)); x = fmaxf(x, __shfl_xor(x, 1));
  return first(x);
}

// A = L L^T in place (lower triangle) for the symmetric positive definite 6 x 6 A, then x <- A^-1 x for each right-hand side.  Fully unrolled: every
// index is a compile-time constant.  A pivot is kept above a tiny floor, so damping = 0 at a singular pose still yields finite numbers.
struct Chol6 {
  float L[6][6];
  __device__ __forceinline__ void factor() {
#pragma unroll
    for (int j = 0; j < 6; j++) {
      float d = L[j][j];
#pragma unroll
      for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k];
      d = sqrtf(fmaxf(d, 1e-30f));
      L[j][j] = d;
      const float inv = 1.f / d;
#pragma unroll
      for (int i = j + 1; i < 6; i++) {
        float s = L[i][j];
#pragma unroll
        for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
        L[i][j] = s * inv;
      }
    }
  }
  __device__ __forceinline__ void solve(float (&x)[6]) const {
#pragma unroll
    for (int i = 0; i < 6; i++) {
      float s = x[i];
#pragma unroll
      for (int k = 0; k < i; k++) s -= L[i][k] * x[k];
      x[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
      float s = x[i];
#pragma unroll
      for (int k = i + 1; k < 6; k++) s -= L[k][i] * x[k];
      x[i] = s / L[i][i];
    }
  }
};
}  // namespace

__global__ __launch_bounds__(64) void k_ik(DIk a) {
  const int prob = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int env = prob / a.K;
  const float* __restrict__ ft = a.ft + (size_t)env * a.fstride;
  const float* __restrict__ qpos = a.qpos + (size_t)env * a.nq;
  const int* __restrict__ chain = a.chain;
  const bool mine = lane < a.n, pose = a.rows == 6;

  // ---- this lane's column: range, start value
  const int cl = mine ? lane : 0;
  float lo = -3.0e38f, hi = 3.0e38f;
  if (mine && a.clamp_range && chain[4 * cl + 1]) { lo = ft[chain[4 * cl]]; hi = ft[chain[4 * cl] + 1]; }
  float q = 0.f;
  if (mine) q = a.q_init ? a.q_init[(size_t)prob * a.n + lane] : qpos[chain[4 * cl + 2]];
  q = fminf(fmaxf(q, lo), hi);
  const float q_rest = q;

  const V3 tp = ld3(a.tpos + (size_t)prob * 3);
  Q4 tq = {1.f, 0.f, 0.f, 0.f};
  if (pose) tq = qunit(ldq(a.tquat + (size_t)prob * 4));

  int it = 0, conv = 0;
  float en = 0.f, wn = 0.f;
  for (;;) {
    // ---- FK: the chain composed from the world outwards (wave-uniform); this lane keeps the world anchor / axis of its own joint
    V3 p = v3(0.f, 0.f, 0.f), an = p, ax = p;
    Q4 r = {1.f, 0.f, 0.f, 0.f};
    int jt = -1;
    for (int e = 0; e < a.nel; e++) {
      const int* el = chain + RSIM_IK_HEAD + RSIM_IK_REC * e;
      const int kind = el[IKE_KIND];
      if (kind == IK_BODY) {
        p = p + qrot(r, ld3(ft + el[IKE_O1]));
        r = qunit(qmul(r, ldq(ft + el[IKE_O2])));
      } else if (kind == IK_SITE) {
        p = p + qrot(r, ld3(ft + el[IKE_O1]));
        r = qunit(qmul(r, ldq(ft + el[IKE_O2])));
      } else {
        const int col = el[IKE_COL];
        const float x = (col >= 0 ? __shfl(q, col) : qpos[el[IKE_QADR]]) - ft[el[IKE_O3]];
        const V3 jp = ld3(ft + el[IKE_O1]), ja = ld3(ft + el[IKE_O2]);
        const V3 anchor = p + qrot(r, jp), axis = qrot(r, ja);
        if (col == lane) { an = anchor; ax = axis; jt = kind; }
        if (kind == IK_HINGE) {
          float sn, cs;
          sincos_f(0.5f * x, sn, cs);
          const Q4 ql = {cs, ja.x * sn, ja.y * sn, ja.z * sn};
          r = qmul(r, ql);
          p = anchor - qrot(r, jp);
        } else {
          p = p + axis * x;
        }
      }
    }
    // ---- this lane's column of J = [linear; angular]
    float J[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (jt == IK_HINGE) {
      const V3 l = cross(ax, p - an);
      J[0] = l.x; J[1] = l.y; J[2] = l.z;
      if (pose) { J[3] = ax.x; J[4] = ax.y; J[5] = ax.z; }
    } else if (jt == IK_SLIDE) {
      J[0] = ax.x; J[1] = ax.y; J[2] = ax.z;
    }
    // ---- error
    float err[6] = {tp.x - p.x, tp.y - p.y, tp.z - p.z, 0.f, 0.f, 0.f};
    if (pose) {
      const Q4 c = {r.w, -r.x, -r.y, -r.z};
      Q4 d = qmul(tq, c);
      if (d.w < 0.f) { d.w = -d.w; d.x = -d.x; d.y = -d.y; d.z = -d.z; }
      const float s = sqrtf(d.x * d.x + d.y * d.y + d.z * d.z);
      const float k = s > 1e-12f ? 2.f * atan2f(s, d.w) / s : 2.f;
      err[3] = d.x * k; err[4] = d.y * k; err[5] = d.z * k;
    }
    en = sqrtf(err[0] * err[0] + err[1] * err[1] + err[2] * err[2]);
    wn = sqrtf(err[3] * err[3] + err[4] * err[4] + err[5] * err[5]);
    conv = __builtin_amdgcn_readfirstlane((en < a.pos_tol && (!pose || wn < a.rot_tol)) ? 1 : 0);
    if (conv || it >= a.max_iters) break;   // (wave-uniform)

    // ---- A = J J^T + damping I, factored; dq = J^T A^-1 err
    Chol6 C;
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
      for (int j = 0; j <= i; j++) C.L[i][j] = sum16(J[i] * J[j]) + (i == j ? a.damping : 0.f);
    }
    C.factor();
    C.solve(err);
    float dq = 0.f;
#pragma unroll
    for (int i = 0; i < 6; i++) dq += J[i] * err[i];
    if (a.posture_gain > 0.f) {   // (wave-uniform)
      const float v = mine ? a.posture_gain * (q_rest - q) : 0.f;
      float jv[6];
#pragma unroll
      for (int i = 0; i < 6; i++) jv[i] = sum16(J[i] * v);
      C.solve(jv);
      float back = 0.f;
#pragma unroll
      for (int i = 0; i < 6; i++) back += J[i] * jv[i];
      dq += v - back;
    }
    if (!mine) dq = 0.f;
    const float big = max16(fabsf(dq));
    if (big > a.max_dq) dq *= a.max_dq / big;
    q = fminf(fmaxf(q + dq, lo), hi);
    it++;
  }
  if (mine) a.q_out[(size_t)prob * a.n + lane] = q;
  if (lane == 0) {
    a.err[(size_t)prob * 2] = en;
    a.err[(size_t)prob * 2 + 1] = wn;
    a.iters[prob] = it | (conv << 30);
  }
}

extern "C" int rsim_launch_ik(const DIk* a, hipStream_t stream) {
  if (a->B <= 0 || a->K <= 0) return 0;
  hipLaunchKernelGGL(k_ik, dim3((unsigned)a->B * (unsigned)a->K), dim3(64), 0, stream, *a);
  return (int)hipGetLastError();
}
