// rsim_dyn_solve.h -- kernel argument of the M^-1 kernel (rsim_dyn_solve.hip), filled by the C-ABI host code (rsim_api.cpp).  Not part of the public boundary.
// Everything it reads was left in batch scratches by the unchanged dynamics kernels (rsim_dyn.hip) in front of it on the stream.
#pragma once
#include <hip/hip_runtime.h>

enum { RSIM_SOLVE_FD = 0, RSIM_SOLVE_RHS = 1, RSIM_SOLVE_OPSPACE = 2 };

struct DSolve {
  int NC, n, mode, nrhs;         // candidates B K, controlled dofs, RSIM_SOLVE_*, columns of rhs (RSIM_SOLVE_RHS)
  const float* M;                // [NC][n][n]: k_dyn_crb's result
  const float* bias;             // RSIM_SOLVE_FD: [NC][n], k_dyn_rne's result with qdd null
  const float* tau;              // RSIM_SOLVE_FD: [NC][n] or null: zeros
  const float* rhs;              // RSIM_SOLVE_RHS: [NC][n][nrhs]
  const float *jacp, *jacr;      // RSIM_SOLVE_OPSPACE: [NC][3][n] each, k_dyn_jac's result
  float* x;                      // qdd [NC][n] / x [NC][n][nrhs] / minv_jt [NC][n][6] or null
  float* lambda_inv;             // RSIM_SOLVE_OPSPACE: [NC][6][6] or null
  int* ok;                       // [NC] or null
};

extern "C" int rsim_launch_dyn_solve(const DSolve* a, hipStream_t stream);
// bytes of dynamic LDS per workgroup for n dofs
extern "C" int rsim_dyn_solve_lds(int n);
