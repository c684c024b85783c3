// rsim_dyn_solve_core.h -- the per-candidate core of the M^-1 queries (rsim_config_forward_dynamics / rsim_config_mass_solve / rsim_config_opspace,
// rsim_dyn_solve.hip): fp32 __host__ __device__ functions.  The kernel includes it; so does tests/san/dyn_solve_driver.cpp, which runs the very same source on
// plain arrays on the host under AddressSanitizer + UndefinedBehaviorSanitizer.  robosuite_amd/dynamics.py (forward_dynamics / mass_solve / opspace) is the fp64
// statement by the definition.
//
//  * THE WORKING SET is reached through a storage accessor S: `float& s(int word)`.  Words 0 .. n(n+1)/2 - 1 hold the packed lower triangle, row by row
//    (entry (i, j), j <= i, at word i(i+1)/2 + j); words n(n+1)/2 .. n(n+1)/2 + n - 1 hold ONE right-hand-side column.  On the device the accessor is the lane's
//    own words of LDS, laid out [word][lane]; on the host a plain array.  No array lives in registers: every index below is a loop counter bounded by n, and on the
//    device n is wave-uniform, so every LDS address is the same word for all lanes.
//  * chol_factor: M = L L^T in place, column by column.  The diagonal word keeps 1 / L_jj, the only quantity the substitutions need of it.  A pivot that is not
//    finite and > 0 clears the result `good`; the arithmetic goes on with 1 in its place (no NaN or infinity is fed into anything that is stored for another
//    candidate -- nothing is -- and the lanes of a wavefront stay converged); the caller writes NaN for a candidate that is not good.
//    A block-diagonal M gives a block-diagonal L exactly: (0 - sum of 0 * x) * y = 0.
//  * chol_solve: the column in place, y = L^-1 b forward, x = L^-T y backward.
//  * Every loop is bounded by n <= RSIM_JNT_MAX.
#pragma once
#include "rsim_vec.h"

namespace rsim_dyn_solve {

RSIM_HD int tri(int i, int j) { return i * (i + 1) / 2 + j; }   // word of entry (i, j), j <= i
RSIM_HD int tri_words(int n) { return n * (n + 1) / 2; }

// the lower triangle of the row-major n x n block at M into the working set
template <class S> RSIM_HD void load_lower(S& s, int n, const float* M) {
  for (int i = 0; i < n; i++)
    for (int j = 0; j <= i; j++) s(tri(i, j)) = M[(size_t)i * n + j];
}

template <class S> RSIM_HD bool chol_factor(S& s, int n) {
  bool good = true;
  for (int j = 0; j < n; j++) {
    float d = s(tri(j, j));
    for (int k = 0; k < j; k++) { const float l = s(tri(j, k)); d -= l * l; }
    const bool pos = d > 0.f && d <= 3.402823466e38f;   // false for NaN
    good = good && pos;
    const float inv = 1.f / sqrtf(pos ? d : 1.f);
    s(tri(j, j)) = inv;
    for (int i = j + 1; i < n; i++) {
      float a = s(tri(i, j));
      for (int k = 0; k < j; k++) a -= s(tri(i, k)) * s(tri(j, k));
      s(tri(i, j)) = a * inv;
    }
  }
  return good;
}

template <class S> RSIM_HD void chol_solve(S& s, int n) {
  const int b = tri_words(n);
  for (int i = 0; i < n; i++) {
    float a = s(b + i);
    for (int k = 0; k < i; k++) a -= s(tri(i, k)) * s(b + k);
    s(b + i) = a * s(tri(i, i));
  }
  for (int i = n - 1; i >= 0; i--) {
    float a = s(b + i);
    for (int k = i + 1; k < n; k++) a -= s(tri(k, i)) * s(b + k);
    s(b + i) = a * s(tri(i, i));
  }
}

RSIM_HD float quiet_nan() { return __builtin_nanf(""); }

// forward dynamics: qdd = M^-1 (tau - bias); tau may be null (zeros).  All of [n], the candidate's own.
template <class S> RSIM_HD void solve_forward_dynamics(S& s, int n, bool good, const float* tau, const float* bias, float* qdd) {
  const int b = tri_words(n);
  for (int i = 0; i < n; i++) s(b + i) = (tau ? tau[i] : 0.f) - bias[i];
  chol_solve(s, n);
  for (int i = 0; i < n; i++) qdd[i] = good ? s(b + i) : quiet_nan();
}

// x = M^-1 rhs, both row-major [n][r], column by column
template <class S> RSIM_HD void solve_columns(S& s, int n, int r, bool good, const float* rhs, float* x) {
  const int b = tri_words(n);
  for (int c = 0; c < r; c++) {
    for (int i = 0; i < n; i++) s(b + i) = rhs[(size_t)i * r + c];
    chol_solve(s, n);
    for (int i = 0; i < n; i++) x[(size_t)i * r + c] = good ? s(b + i) : quiet_nan();
  }
}

// J = [jacp; jacr], [3][n] each: minv_jt = M^-1 J^T [n][6], lambda_inv = J M^-1 J^T [6][6]; either output may be null.  Row a of J against the solved column b for
// a <= b only: one product per unordered pair, written to both triangles.
template <class S> RSIM_HD void solve_opspace(S& s, int n, bool good, const float* jacp, const float* jacr, float* minv_jt, float* lambda_inv) {
  const int b = tri_words(n);
  for (int c = 0; c < 6; c++) {
    const float* row = c < 3 ? jacp + (size_t)c * n : jacr + (size_t)(c - 3) * n;
    for (int i = 0; i < n; i++) s(b + i) = row[i];
    chol_solve(s, n);
    if (minv_jt)
      for (int i = 0; i < n; i++) minv_jt[(size_t)i * 6 + c] = good ? s(b + i) : quiet_nan();
    if (lambda_inv)
      for (int a = 0; a <= c; a++) {
        const float* ra = a < 3 ? jacp + (size_t)a * n : jacr + (size_t)(a - 3) * n;
        float l = 0.f;
        for (int i = 0; i < n; i++) l += ra[i] * s(b + i);
        l = good ? l : quiet_nan();
        lambda_inv[a * 6 + c] = l; lambda_inv[c * 6 + a] = l;
      }
  }
}

}  // namespace rsim_dyn_solve
