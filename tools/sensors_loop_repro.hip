// sensors_loop_repro.hip -- the EARLIER form of the accelerometer loop of k_sensors (csrc/rsim_sensors.hip), stand-alone: the velocity before the current
// joint (wb, vb) is a snapshot carried from one dof of the loop to the next.  Inside k_sensors that form read the accelerometer on a free body that spins
// while it translates 0.7 .. 3.5 m/s^2 off on gfx950 while the same source was right on the host and in a build with -fno-slp-vectorize
// (profiles/sensors_parity.txt).  The program runs the loop over the arm2_box dof layout (hinge, hinge, slide, free, free) on the device and on the host,
// one lane per (body, sensor type), and prints the worst difference: it tells whether the loop ALONE, outside k_sensors, shows the effect.  Measured on an
// MI355X: it does not -- 1.9e-06 on values up to 40, with the packer on and off.  The cause of the error inside k_sensors is not isolated.
//
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -fno-hip-fp32-correctly-rounded-divide-sqrt -fgpu-flush-denormals-to-zero tools/sensors_loop_repro.hip -o repro_slp
//   hipcc ... -fno-slp-vectorize tools/sensors_loop_repro.hip -o repro_noslp
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct V3 { float x, y, z; };
struct Q4 { float w, x, y, z; };
#define HD __host__ __device__ __forceinline__
HD V3 v3(float x, float y, float z) { V3 r = {x, y, z}; return r; }
HD V3 operator+(V3 a, V3 b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
HD V3 operator-(V3 a, V3 b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
HD V3 operator*(V3 a, float s) { return v3(a.x * s, a.y * s, a.z * s); }
HD V3 cross(V3 a, V3 b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
HD V3 ld3(const float* p) { return v3(p[0], p[1], p[2]); }
HD V3 qrot(Q4 q, V3 v) { const V3 u = v3(q.x, q.y, q.z); const V3 t = cross(u, v) * 2.f; return v + t * q.w + cross(u, t); }
HD V3 qrot_inv(Q4 q, V3 v) { Q4 c = {q.w, -q.x, -q.y, -q.z}; return qrot(c, v); }
HD int ctz64(unsigned long long m) {
#ifdef __HIP_DEVICE_COMPILE__
  return __builtin_ctzll(m);
#else
  int i = 0; while (!((m >> i) & 1ull)) i++; return i;
#endif
}

enum { T_GYRO, T_VELOCIMETER, T_ANGVEL, T_LINVEL, T_ACCELEROMETER, T_COUNT };
struct Args {
  int n, nv;
  int io_dof_jntid, io_jnt_type, io_jnt_dofadr, io_mask, io_type;   // offsets into it
  const int* it;
  const float *cdof, *qvel, *qacc, *frame;   // frame: per lane 3 (origin - com) + 4 (quaternion) + 3 (gravity)
  float* out;
};

HD void lane_body(const Args& a, int lane) {
  const int* it = a.it;
  const int type = it[a.io_type + lane];
  const float* fr = a.frame + 10 * lane;
  const Q4 fq = {fr[3], fr[4], fr[5], fr[6]};
  const bool acc = type == T_ACCELEROMETER;
  unsigned long long mask = (unsigned long long)(unsigned)it[a.io_mask + 2 * lane] | ((unsigned long long)(unsigned)it[a.io_mask + 2 * lane + 1] << 32);
  V3 w = v3(0, 0, 0), v = v3(0, 0, 0);
  V3 wb = w, vb = v;
  V3 al = v3(0, 0, 0), ac = ld3(fr + 7) * -1.f;
  for (; mask; mask &= mask - 1) {
    const int i = ctz64(mask);
    const V3 ca = ld3(a.cdof + 6 * i), cl = ld3(a.cdof + 6 * i + 3);
    const float qv = a.qvel[i];
    if (acc) {
      const int j = it[a.io_dof_jntid + i], jt = it[a.io_jnt_type + j], k = i - it[a.io_jnt_dofadr + j];
      const bool first_rot = jt >= 2 || (jt == 1 && k == 0) || (jt == 0 && k == 3);
      if (first_rot) { wb = w; vb = v; }
      if (!(jt == 0 && k < 3)) {
        al = al + cross(wb, ca) * qv;
        ac = ac + (cross(wb, cl) + cross(vb, ca)) * qv;
      }
      const float qa = a.qacc[i];
      al = al + ca * qa; ac = ac + cl * qa;
    }
    w = w + ca * qv; v = v + cl * qv;
  }
  const V3 off = ld3(fr);
  const V3 vp = v + cross(w, off);
  V3 r;
  if (type == T_GYRO) r = qrot_inv(fq, w);
  else if (type == T_VELOCIMETER) r = qrot_inv(fq, vp);
  else if (type == T_ANGVEL) r = w;
  else if (type == T_LINVEL) r = vp;
  else r = qrot_inv(fq, ac + cross(al, off) + cross(w, vp));
  a.out[3 * lane] = r.x; a.out[3 * lane + 1] = r.y; a.out[3 * lane + 2] = r.z;
}

__global__ __launch_bounds__(64) void k_loop(Args a) {
  const int lane = (int)threadIdx.x;
  if (lane >= a.n) return;
  lane_body(a, lane);
}

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

int main() {
  const int nv = 15, nj = 5, n = 60;
  // joints: hinge, hinge, slide (a chain), free, free; bodies' dof masks: link 1, 2, 3 of the chain, box, cylinder
  const int jtype[nj] = {3, 3, 2, 0, 0}, jdof[nj] = {0, 1, 2, 3, 9};
  const unsigned long long masks[5] = {0x1ull, 0x3ull, 0x7ull, 0x3full << 3, 0x3full << 9};
  std::vector<int> it;
  Args a = {};
  a.n = n; a.nv = nv;
  a.io_dof_jntid = (int)it.size(); for (int i = 0; i < nv; i++) it.push_back(i < 3 ? i : (i < 9 ? 3 : 4));
  a.io_jnt_type = (int)it.size(); for (int j = 0; j < nj; j++) it.push_back(jtype[j]);
  a.io_jnt_dofadr = (int)it.size(); for (int j = 0; j < nj; j++) it.push_back(jdof[j]);
  a.io_mask = (int)it.size(); for (int l = 0; l < n; l++) { const unsigned long long m = masks[(l / T_COUNT) % 5]; it.push_back((int)(unsigned)(m & 0xffffffffull)); it.push_back((int)(unsigned)(m >> 32)); }
  a.io_type = (int)it.size(); for (int l = 0; l < n; l++) it.push_back(l % T_COUNT);
  srand(7);
  auto rnd = [](float s) { return s * (2.f * (float)rand() / (float)RAND_MAX - 1.f); };
  std::vector<float> cdof(nv * 6, 0.f), qvel(nv), qacc(nv), frame(10 * n), out_d(3 * n, 0.f), out_h(3 * n, 0.f);
  for (int i = 0; i < nv; i++) { qvel[i] = rnd(2.f); qacc[i] = rnd(10.f); }
  for (int i = 0; i < 3; i++) for (int c = 0; c < 6; c++) cdof[6 * i + c] = (i == 2 && c < 3) ? 0.f : rnd(1.f);
  for (int f = 0; f < 2; f++) {   // free joints: translations along the world axes, rotations about an orthonormal body frame through the com
    const int d = jdof[3 + f];
    float q[4] = {rnd(1.f), rnd(1.f), rnd(1.f), rnd(1.f)};
    const float nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const Q4 qq = {q[0] / nq, q[1] / nq, q[2] / nq, q[3] / nq};
    for (int k = 0; k < 3; k++) {
      cdof[6 * (d + k) + 3 + k] = 1.f;
      const V3 ax = qrot(qq, v3(k == 0, k == 1, k == 2));
      cdof[6 * (d + 3 + k)] = ax.x; cdof[6 * (d + 3 + k) + 1] = ax.y; cdof[6 * (d + 3 + k) + 2] = ax.z;
    }
  }
  for (int l = 0; l < n; l++) {
    float* fr = frame.data() + 10 * l;
    for (int c = 0; c < 3; c++) fr[c] = rnd(0.1f);
    float q[4] = {rnd(1.f), rnd(1.f), rnd(1.f), rnd(1.f)};
    const float nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int c = 0; c < 4; c++) fr[3 + c] = q[c] / nq;
    fr[7] = 0.f; fr[8] = 0.f; fr[9] = -9.81f;
  }
  int* d_it; float *d_cdof, *d_qvel, *d_qacc, *d_frame, *d_out;
  CHK(hipMalloc(&d_it, it.size() * 4)); CHK(hipMalloc(&d_cdof, cdof.size() * 4)); CHK(hipMalloc(&d_qvel, nv * 4)); CHK(hipMalloc(&d_qacc, nv * 4));
  CHK(hipMalloc(&d_frame, frame.size() * 4)); CHK(hipMalloc(&d_out, out_d.size() * 4));
  CHK(hipMemcpy(d_it, it.data(), it.size() * 4, hipMemcpyHostToDevice)); CHK(hipMemcpy(d_cdof, cdof.data(), cdof.size() * 4, hipMemcpyHostToDevice));
  CHK(hipMemcpy(d_qvel, qvel.data(), nv * 4, hipMemcpyHostToDevice)); CHK(hipMemcpy(d_qacc, qacc.data(), nv * 4, hipMemcpyHostToDevice));
  CHK(hipMemcpy(d_frame, frame.data(), frame.size() * 4, hipMemcpyHostToDevice)); CHK(hipMemset(d_out, 0, out_d.size() * 4));
  Args h = a; h.it = it.data(); h.cdof = cdof.data(); h.qvel = qvel.data(); h.qacc = qacc.data(); h.frame = frame.data(); h.out = out_h.data();
  for (int l = 0; l < n; l++) lane_body(h, l);
  a.it = d_it; a.cdof = d_cdof; a.qvel = d_qvel; a.qacc = d_qacc; a.frame = d_frame; a.out = d_out;
  hipLaunchKernelGGL(k_loop, dim3(1), dim3(64), 0, 0, a);
  CHK(hipGetLastError()); CHK(hipDeviceSynchronize());
  CHK(hipMemcpy(out_d.data(), d_out, out_d.size() * 4, hipMemcpyDeviceToHost));
  float worst = 0.f, worst_acc_free = 0.f;
  for (int l = 0; l < n; l++)
    for (int c = 0; c < 3; c++) {
      const float e = std::fabs(out_d[3 * l + c] - out_h[3 * l + c]);
      worst = std::fmax(worst, e);
      if (l % T_COUNT == T_ACCELEROMETER && (l / T_COUNT) % 5 >= 3) worst_acc_free = std::fmax(worst_acc_free, e);
    }
  printf("sensors_loop_repro: worst |device - host| %.3e over %d lanes; accelerometer on the free bodies %.3e (values up to ~40)\n", worst, n, worst_acc_free);
  return 0;
}
