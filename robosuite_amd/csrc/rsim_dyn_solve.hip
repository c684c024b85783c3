// rsim_dyn_solve.hip -- "what acceleration does this torque give here, what is the end effector's apparent inertia here?": M^-1 at K candidate joint vectors per
// env, for the whole batch, on the device: rsim_config_forward_dynamics, rsim_config_mass_solve and rsim_config_opspace (include/rsim.h).  The per-candidate
// code is rsim_dyn_solve_core.h, shared with the host rehearsal (tests/san/dyn_solve_driver.cpp); robosuite_amd/dynamics.py is the fp64 statement by the
// definition.
//
// A code object of its own whose one kernel runs BEHIND the unchanged kernels of rsim_dyn.hip: k_dyn_crb has left M [B K][n][n] in a batch scratch, and, per
// call, k_dyn_rne the bias torques or k_dyn_jac the site Jacobian in another.  Mapping as there: lane = candidate c = env * K + k, 64 consecutive candidates are
// one wavefront = one workgroup (it may span envs), grid ceil(B K / 64).
//   k_dyn_solve  the lane's lower triangle from the M scratch into LDS, Cholesky in place, then per column: form the column in LDS (tau - bias / a column of
//                rhs / a row of J), forward and back substitution, store to the lane's own words of the result.  The operational-space form also adds up
//                J M^-1 J^T from each solved column, one product per unordered pair, written to both triangles.
// LDS, dynamic: n(n+1)/2 + n words per lane laid out [word][lane] (address (word * 64 + lane) * 4): consecutive lanes, consecutive banks, no conflicts;
// (n(n+1)/2 + n) * 256 B per workgroup -- 8 960 B for n = 7, 38 912 B for n = 16.  The matrix lives there because its indices are loop counters: in registers it
// would be a dynamically indexed array, which is a private segment.  n and the column count are kernel arguments, so every loop counter and every LDS word index
// is wave-uniform: no divergence but the c >= NC return.  A lane reads and writes only its own LDS words: no barrier.  No atomics: a repeat call is
// bit-identical.  Every loop is bounded by n or the column count.
#include <hip/hip_runtime.h>
#include "../../include/rsim.h"
#include "rsim_clear.h"
#include "rsim_dyn_solve.h"
#include "rsim_dyn_solve_core.h"

using namespace rsim_dyn_solve;

namespace {
// the lane's own words of the workgroup's LDS
struct LaneWords {
  float* a;
  __device__ __forceinline__ float& operator()(int word) const { return a[word * RSIM_CLEAR_LANES]; }
};
}  // namespace

__global__ __launch_bounds__(RSIM_CLEAR_LANES) void k_dyn_solve(DSolve a) {
  extern __shared__ float lds[];
  const int c = (int)blockIdx.x * RSIM_CLEAR_LANES + (int)threadIdx.x;
  if (c >= a.NC) return;
  const int n = a.n;
  LaneWords s;
  s.a = lds + threadIdx.x;
  load_lower(s, n, a.M + (size_t)c * n * n);
  const bool good = chol_factor(s, n);
  if (a.ok) a.ok[c] = good ? 1 : 0;
  if (a.mode == RSIM_SOLVE_FD) {
    const size_t at = (size_t)c * n;
    solve_forward_dynamics(s, n, good, a.tau ? a.tau + at : nullptr, a.bias + at, a.x + at);
  } else if (a.mode == RSIM_SOLVE_RHS) {
    const size_t at = (size_t)c * n * a.nrhs;
    solve_columns(s, n, a.nrhs, good, a.rhs + at, a.x + at);
  } else {
    const size_t at = (size_t)c * 3 * n;
    solve_opspace(s, n, good, a.jacp + at, a.jacr + at, a.x ? a.x + (size_t)c * n * 6 : nullptr, a.lambda_inv ? a.lambda_inv + (size_t)c * 36 : nullptr);
  }
}

extern "C" int rsim_dyn_solve_lds(int n) { return (tri_words(n) + n) * RSIM_CLEAR_LANES * (int)sizeof(float); }

extern "C" int rsim_launch_dyn_solve(const DSolve* a, hipStream_t stream) {
  if (a->NC <= 0) return 0;
  if (a->n < 1 || a->n > RSIM_JNT_MAX) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dyn_solve, dim3((a->NC + RSIM_CLEAR_LANES - 1) / RSIM_CLEAR_LANES), dim3(RSIM_CLEAR_LANES), (size_t)rsim_dyn_solve_lds(a->n), stream, *a);
  return (int)hipGetLastError();
}
