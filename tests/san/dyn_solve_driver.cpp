// Host rehearsal of the M^-1 core (robosuite_amd/csrc/rsim_dyn_solve_core.h): the same fp32 functions k_dyn_solve runs per candidate, compiled for the host with
// g++ -fsanitize=address,undefined by tests/test_dynamics_solve_core_host.py.  Reads one problem set from a binary file, writes the results to another:
//
//   in : int32 N, n, r, has_tau; float M[N][n][n], bias[N][n], tau[N][n] if has_tau, rhs[N][n][r], jacp[N][3][n], jacr[N][3][n]
//   out: int32 ok[N]; float qdd[N][n], x[N][n][r], minv_jt[N][n][6], lambda_inv[N][6][6]
//
// As in the kernel the working set of 64 consecutive candidates is one block laid out [word][lane], n(n+1)/2 + n words, allocated per block at exactly the size
// the kernel asks of LDS, and factorised once per mode as the three calls do; a malformed file ends the program with status 2, not with a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../robosuite_amd/csrc/rsim_dyn_solve_core.h"

using namespace rsim_dyn_solve;

namespace {
const int LANES = 64, NMAX = 16;
struct LaneWords {
  float* a;
  float& operator()(int word) const { return a[word * LANES]; }
};
struct Reader {
  std::vector<unsigned char> buf;
  size_t at = 0;
  bool ok = true;
  template <class T> T get() {
    T v{};
    if (at + sizeof(T) > buf.size()) { ok = false; return v; }
    memcpy(&v, buf.data() + at, sizeof(T));
    at += sizeof(T);
    return v;
  }
  template <class T> std::vector<T> vec(size_t n) {
    std::vector<T> v;
    if (n > (buf.size() - at) / sizeof(T)) { ok = false; return v; }
    v.resize(n);
    if (n) memcpy(v.data(), buf.data() + at, n * sizeof(T));
    at += n * sizeof(T);
    return v;
  }
};
int bad(const char* what) { fprintf(stderr, "malformed problem set: %s\n", what); return 2; }
template <class T> bool put(FILE* o, const std::vector<T>& v) { return fwrite(v.data(), sizeof(T), v.size(), o) == v.size(); }
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s in.bin out.bin\n", argv[0]); return 2; }
  Reader r;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  unsigned char chunk[65536];
  for (size_t k; (k = fread(chunk, 1, sizeof(chunk), f)) > 0;) r.buf.insert(r.buf.end(), chunk, chunk + k);
  fclose(f);
  const int N = r.get<int32_t>(), n = r.get<int32_t>(), nr = r.get<int32_t>(), has_tau = r.get<int32_t>();
  if (!r.ok || N < 1 || N > 65536 || n < 1 || n > NMAX || nr < 1 || nr > NMAX) return bad("header");
  const size_t sN = (size_t)N;
  const std::vector<float> M = r.vec<float>(sN * n * n), bias = r.vec<float>(sN * n), tau = r.vec<float>(has_tau ? sN * n : 0), rhs = r.vec<float>(sN * n * nr);
  const std::vector<float> jacp = r.vec<float>(sN * 3 * n), jacr = r.vec<float>(sN * 3 * n);
  if (!r.ok) return bad("truncated");

  std::vector<int32_t> ok(sN, -1);
  std::vector<float> qdd(sN * n, 0.f), x(sN * n * nr, 0.f), mjt(sN * n * 6, 0.f), lam(sN * 36, 0.f);
  int done = 0;
  for (int blk = 0; blk * LANES < N; blk++) {
    std::vector<float> lds((size_t)(tri_words(n) + n) * LANES, 0.f);   // one workgroup's LDS
    for (int lane = 0; lane < LANES; lane++) {
      const int c = blk * LANES + lane;
      if (c >= N) break;
      LaneWords s;
      s.a = lds.data() + lane;
      const float* Mc = M.data() + (size_t)c * n * n;
      load_lower(s, n, Mc);
      bool good = chol_factor(s, n);
      solve_forward_dynamics(s, n, good, has_tau ? tau.data() + (size_t)c * n : nullptr, bias.data() + (size_t)c * n, qdd.data() + (size_t)c * n);
      load_lower(s, n, Mc);
      const bool good2 = chol_factor(s, n);
      solve_columns(s, n, nr, good2, rhs.data() + (size_t)c * n * nr, x.data() + (size_t)c * n * nr);
      load_lower(s, n, Mc);
      const bool good3 = chol_factor(s, n);
      solve_opspace(s, n, good3, jacp.data() + (size_t)c * 3 * n, jacr.data() + (size_t)c * 3 * n, mjt.data() + (size_t)c * n * 6, lam.data() + (size_t)c * 36);
      if (good != good2 || good != good3) { fprintf(stderr, "candidate %d: the factorisation is not repeatable\n", c); return 1; }
      ok[c] = good ? 1 : 0;
      done++;
    }
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
  const bool wrote = put(o, ok) && put(o, qdd) && put(o, x) && put(o, mjt) && put(o, lam);
  fclose(o);
  if (!wrote) { fprintf(stderr, "short write\n"); return 2; }
  printf("candidates: %d of %d\n", done, N);
  return 0;
}
