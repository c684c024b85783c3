// rsim_sensors.hip -- the sensors beyond force / torque (include/rsim.h RSIM_SENSORDATA): thirteen MuJoCo sensor types [3P, docs "XML reference: sensor"]
// for the whole batch, on the device.
//
// force / torque are computed inside the step kernel (rsim_step.hip sensor_acc), where the constraint forces of the substep still sit in LDS; it writes zero
// to every other entry.  The types here need nothing that is not in global memory once the debug form of the step kernel has run -- the state, RSIM_XPOS /
// RSIM_XQUAT / RSIM_CDOF / RSIM_ROOTCOM, the contact records with their normal forces, the model tables -- so they are a kernel of their own, launched on the
// batch's stream directly behind it (rsim_api.cpp launch()).  It is compiled once, not per kernel configuration, and takes everything it needs as its own
// kernel argument: the step-kernel code objects (and DModel / DBatch, their kernel arguments) are untouched by the feature, and a model without such a
// sensor launches nothing.  robosuite_amd/sensors.py is the fp64 host mirror the kernel is tested against.
//
// One wavefront per env, lane = sensor (a model holds at most 64).  The lanes are independent: no LDS, no barrier.
//
// Spatial vectors follow the step kernel (and MuJoCo's cdof / cvel / cacc): [angular; linear], the linear part taken at the COM of the body's kinematic
// tree (RSIM_ROOTCOM).  For a body b with the dofs i that move it, in tree order:
//   cvel_b = sum_i cdof_i qvel_i                                                     (mj_comVel)
//   cacc_b = [0; -g] + sum_i (cdof_dot_i qvel_i + cdof_i qacc_i),  cdof_dot_i = cvel_before(i) x cdof_i   (mj_rnePostConstraint)
// where cvel_before(i) is the velocity accumulated up to dof i; the three rotational dofs of a free joint (and a ball joint) all take the velocity from
// before the first of them, and the translational dofs of a free joint have cdof_dot = 0 -- as velocity() of the step kernel and fwd_velocity of the
// oracle do.  A frame at world point p then has velocity [w; v + w x (p - com)], and the classical acceleration of p is a + alpha x (p - com) + w x v_p
// (mj_objectAcceleration).
#include <hip/hip_runtime.h>
#include "../../include/rsim.h"
#include "rsim_sensors.h"
#include "rsim_vec.h"

namespace {
using namespace rsim_vec;
__device__ __forceinline__ V3 qrot_inv(Q4 q, V3 v) { Q4 c = {q.w, -q.x, -q.y, -q.z}; return qrot(c, v); }

// does the ray p + t d, t >= 0, meet the solid (sphere of radius s.x | ellipsoid of semi-axes s | box of half-sizes s) centred at the origin?  A ray that
// starts inside always does.  [3P, docs "sensor/touch": the contact point, or the normal ray re-projected from it, must intersect the site volume]
__device__ __forceinline__ bool ray_hits(int shape, V3 s, V3 p, V3 d) {
  if (shape == 6) {
    float t0 = 0.f, t1 = 3.0e38f;
    const float pk[3] = {p.x, p.y, p.z}, dk[3] = {d.x, d.y, d.z}, sk[3] = {s.x, s.y, s.z};
#pragma unroll
    for (int k = 0; k < 3; k++) {
      if (fabsf(dk[k]) < 1e-12f) { if (fabsf(pk[k]) > sk[k]) return false; continue; }
      const float a = (-sk[k] - pk[k]) / dk[k], b = (sk[k] - pk[k]) / dk[k];
      t0 = fmaxf(t0, fminf(a, b)); t1 = fminf(t1, fmaxf(a, b));
    }
    return t1 >= t0;
  }
  if (shape == 2) s = v3(s.x, s.x, s.x);
  p = v3(p.x / s.x, p.y / s.y, p.z / s.z); d = v3(d.x / s.x, d.y / s.y, d.z / s.z);
  const float a = dot(d, d), b = dot(p, d), c = dot(p, p) - 1.f, disc = b * b - a * c;   // |p + t d|^2 = 1
  return disc >= 0.f && sqrtf(disc) - b >= 0.f;                                           // the larger root is not negative
}
}  // namespace

__global__ __launch_bounds__(64) void k_sensors(DSensors a) {
  const int env = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (env >= a.B || lane >= a.nsensor) return;
  const int* it = a.it;
  const float* ft = a.ft + (size_t)env * a.fstride;
  const int type = it[a.io[IO_sensor_type] + lane];
  if (type < RS_JOINTPOS || type >= RS_TYPE_END || !a.carried[lane]) return;
  const int stage = type < RS_JOINTVEL ? RS_STAGE_POS : (type < RS_ACCELEROMETER ? RS_STAGE_VEL : RS_STAGE_ACC);
  if (!(a.stages & stage)) return;
  const int obj = it[a.io[IO_sensor_site] + lane], kind = a.objtype[lane];
  const int adr = it[a.io[IO_sensor_adr] + lane];
  float* out = a.sensordata + (size_t)env * a.nsensordata + adr;
  const float* qpos = a.qpos + (size_t)env * a.nq;
  const float* qvel = a.qvel + (size_t)env * a.nv;

  if (type == RS_JOINTPOS) { out[0] = qpos[it[a.io[IO_jnt_qposadr] + obj]]; return; }
  if (type == RS_JOINTVEL) { out[0] = qvel[it[a.io[IO_jnt_dofadr] + obj]]; return; }
  if (type == RS_TENDONPOS || type == RS_TENDONVEL) {   // fixed tendon: sum of coef x joint coordinate / rate
    const int w0 = it[a.io[IO_tendon_adr] + obj], wn = it[a.io[IO_tendon_num] + obj];
    float s = 0.f;
    for (int w = w0; w < w0 + wn; w++)
      s += ft[a.fo[FO_wrap_prm] + w] * (type == RS_TENDONPOS ? qpos[it[a.io[IO_wrap_qadr] + w]] : qvel[it[a.io[IO_wrap_dof] + w]]);
    out[0] = s;
    return;
  }
  if (type == RS_ACTUATORFRC) {   // gain x ctrl + bias, as actuation() of the step kernel (fixed gain, affine bias, joint transmission)
    const int j = it[a.io[IO_act_trnid] + obj];
    float ctrl = a.ctrl[(size_t)env * a.nu + obj];
    if (it[a.io[IO_act_ctrllimited] + obj]) ctrl = fmaxf(ft[a.fo[FO_act_ctrlrange] + 2 * obj], fminf(ft[a.fo[FO_act_ctrlrange] + 2 * obj + 1], ctrl));
    float force = ft[a.fo[FO_act_gainprm] + 3 * obj] * ctrl;
    if (it[a.io[IO_act_biastype] + obj] == 1) {
      const float gear = ft[a.fo[FO_act_gear] + obj];
      force += ft[a.fo[FO_act_biasprm] + 3 * obj] + ft[a.fo[FO_act_biasprm] + 3 * obj + 1] * gear * qpos[it[a.io[IO_jnt_qposadr] + j]] +
               ft[a.fo[FO_act_biasprm] + 3 * obj + 2] * gear * qvel[it[a.io[IO_jnt_dofadr] + j]];
    }
    if (it[a.io[IO_act_forcelimited] + obj]) force = fmaxf(ft[a.fo[FO_act_forcerange] + 2 * obj], fminf(ft[a.fo[FO_act_forcerange] + 2 * obj + 1], force));
    out[0] = force;
    return;
  }

  // ---- the frame: a site, a body frame (xbody) or a body's inertial frame (body)
  int body = obj;
  V3 lp = v3(0, 0, 0);
  Q4 lq = {1.f, 0.f, 0.f, 0.f};
  if (kind == RS_OBJ_SITE) { body = it[a.io[IO_site_bodyid] + obj]; lp = ld3(ft + a.fo[FO_site_pos] + 3 * obj); lq = ldq(ft + a.fo[FO_site_quat] + 4 * obj); }
  else if (kind == RS_OBJ_BODY) { lp = ld3(ft + a.fo[FO_body_ipos] + 3 * obj); lq = ldq(ft + a.fo[FO_body_iquat] + 4 * obj); }
  const Q4 xq = ldq(a.xquat + ((size_t)env * a.nbody + body) * 4);
  const V3 fp = ld3(a.xpos + ((size_t)env * a.nbody + body) * 3) + qrot(xq, lp);
  Q4 fq = qmul(xq, lq);
  { const float n = 1.f / sqrtf(fq.w * fq.w + fq.x * fq.x + fq.y * fq.y + fq.z * fq.z); fq.w *= n; fq.x *= n; fq.y *= n; fq.z *= n; }
  if (type == RS_FRAMEPOS) { out[0] = fp.x; out[1] = fp.y; out[2] = fp.z; return; }
  if (type == RS_FRAMEQUAT) { out[0] = fq.w; out[1] = fq.x; out[2] = fq.y; out[3] = fq.z; return; }

  if (type == RS_TOUCH) {
    // sum of the normal forces of the active contacts of the site's body whose contact point, or whose normal ray from it (through the penetration towards
    // the body's own surface: along the contact normal for geom 1, against it for geom 2), meets the site volume
    const int shape = a.shape[lane], nc = a.ncon[env];
    const V3 size = ld3(a.site_size + 3 * lane);
    float s = 0.f;
    for (int c = 0; c < nc && c < a.ncon_max; c++) {
      const float* r = a.contact + ((size_t)env * a.ncon_max + c) * RSIM_CON_REC;
      const float fn = r[17];
      if (r[16] < 0.f || !(fn > 0.f)) continue;
      const int b1 = a.geom_body[(int)r[13]], b2 = a.geom_body[(int)r[14]];
      if (b1 != body && b2 != body) continue;
      V3 n = ld3(r + 4);
      if (b2 == body) n = n * -1.f;
      if (ray_hits(shape, size, qrot_inv(fq, ld3(r + 1) - fp), qrot_inv(fq, n))) s += fn;
    }
    out[0] = s;
    return;
  }

  // ---- velocity (and acceleration) of the frame's body, accumulated along the dofs that move it
  const float* cdof = a.cdof + (size_t)env * a.nv * 6;
  const float* qacc = a.qacc + (size_t)env * a.nv;
  const bool acc = type == RS_ACCELEROMETER;
  unsigned long long mask = (unsigned long long)(unsigned)it[a.io[IO_body_dofmask] + 2 * body] | ((unsigned long long)(unsigned)it[a.io[IO_body_dofmask] + 2 * body + 1] << 32);
  V3 w = v3(0, 0, 0), v = v3(0, 0, 0);            // cvel
  V3 al = v3(0, 0, 0), ac = ld3(ft + a.fo[FO_opt] + 1) * -1.f;   // cacc: the world accelerates at -g
  for (; mask; mask &= mask - 1) {
    const int i = __builtin_ctzll(mask);
    const V3 ca = ld3(cdof + 6 * i), cl = ld3(cdof + 6 * i + 3);
    const float qv = qvel[i];
    if (acc) {
      if (!it[a.io[IO_dof_zerodot] + i]) {        // cdof_dot = cvel_before x cdof (motion cross product); zero for free translations
        // cvel before dof i, summed afresh over the dofs the step kernel's own table names (IO_dof_cvelmask: the dofs ahead of the joint, and for the
        // rotational dofs of a free joint its translations) -- no snapshot carried from one dof of the loop to the next
        unsigned long long bm = (unsigned long long)(unsigned)it[a.io[IO_dof_cvelmask] + 2 * i] | ((unsigned long long)(unsigned)it[a.io[IO_dof_cvelmask] + 2 * i + 1] << 32);
        V3 wb = v3(0, 0, 0), vb = v3(0, 0, 0);
        for (; bm; bm &= bm - 1) {
          const int p = __builtin_ctzll(bm);
          const float pv = qvel[p];
          wb = wb + ld3(cdof + 6 * p) * pv; vb = vb + ld3(cdof + 6 * p + 3) * pv;
        }
        al = al + cross(wb, ca) * qv;
        ac = ac + (cross(wb, cl) + cross(vb, ca)) * qv;
      }
      const float qa = qacc[i];
      al = al + ca * qa; ac = ac + cl * qa;
    }
    w = w + ca * qv; v = v + cl * qv;
  }
  const V3 off = fp - ld3(a.rootcom + ((size_t)env * a.nbody + body) * 3);
  const V3 vp = v + cross(w, off);                // velocity of the frame origin
  V3 r;
  if (type == RS_GYRO) r = qrot_inv(fq, w);
  else if (type == RS_VELOCIMETER) r = qrot_inv(fq, vp);
  else if (type == RS_FRAMEANGVEL) r = w;
  else if (type == RS_FRAMELINVEL) r = vp;
  else r = qrot_inv(fq, ac + cross(al, off) + cross(w, vp));   // accelerometer: classical acceleration minus gravity, in the site frame
  out[0] = r.x; out[1] = r.y; out[2] = r.z;
}

extern "C" int rsim_launch_sensors(const DSensors* a, hipStream_t stream) {
  if (a->B <= 0 || a->nsensor <= 0 || !a->stages) return 0;
  hipLaunchKernelGGL(k_sensors, dim3(a->B), dim3(64), 0, stream, *a);
  return (int)hipGetLastError();
}
