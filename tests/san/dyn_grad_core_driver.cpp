// Host rehearsal of the core of the dynamics derivatives (robosuite_amd/csrc/rsim_dyn_grad_core.h on the untouched rsim_dyn_core.h): the same fp32 functions the
// kernels k_clear_fk / k_clear_joints / k_dyn_rne / k_dyn_rne_grad / k_dyn_rne_jvp run per candidate, compiled for the host with g++ -fsanitize=address,undefined
// by tests/test_dynamics_grad_core_host.py.  Reads one scene from a binary file, writes the results to another:
//
//   in : int32 B, K, n, nbody, nq, nel, nslot, has_qd, has_qdd, has_dq, has_dqd, has_dqdd, slide_mask, fo_mass, fo_inertia, fo_ipos, fo_iquat, fo_armature,
//        fo_damping, fo_opt, nft; int32 tab[nel][RSIM_CLEAR_REC], slot[nbody], cols[n][RSIM_DYN_COL]; float ft[nft], qpos[B][nq], xpos[B][nbody][3],
//        xquat[B][nbody][4], q[B][K][n], then [B][K][n] each of qd, qdd, dq, dqd, dqdd that the header says is there
//   out: float tau[B][K][n], dtau_dq[B][K][n][n], dtau_dqd[B][K][n][n], -dtau_dq, -dtau_dqd (the negate flag), jvp[B][K][n]
//
// As in the kernels the poses pass through a scratch laid out [slot][7][B K], the joint frames through a store [col][6][B K], the words of the primal walk
// through one laid out [slot][18][B K] and the tangent words through one laid out [slot][24][B K]; every table index is checked before it is used: a malformed
// file ends the program with status 2, not with a sanitizer report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../robosuite_amd/csrc/rsim_dyn_grad_core.h"

using namespace rsim_dyn;

namespace {
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
int bad(const char* what) { fprintf(stderr, "malformed scene: %s\n", what); return 2; }
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s scene.bin out.bin\n", argv[0]); return 2; }
  Reader r;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  unsigned char chunk[65536];
  for (size_t n; (n = fread(chunk, 1, sizeof(chunk), f)) > 0;) r.buf.insert(r.buf.end(), chunk, chunk + n);
  fclose(f);
  const int B = r.get<int32_t>(), K = r.get<int32_t>(), n = r.get<int32_t>(), nbody = r.get<int32_t>(), nq = r.get<int32_t>(), nel = r.get<int32_t>();
  const int nslot = r.get<int32_t>();
  int has[5];   // qd, qdd, dq, dqd, dqdd
  for (int i = 0; i < 5; i++) has[i] = r.get<int32_t>();
  const int slide_mask = r.get<int32_t>();
  DynModel dm;
  dm.fo_mass = r.get<int32_t>(); dm.fo_inertia = r.get<int32_t>(); dm.fo_ipos = r.get<int32_t>(); dm.fo_iquat = r.get<int32_t>();
  dm.fo_armature = r.get<int32_t>(); dm.fo_damping = r.get<int32_t>(); dm.fo_opt = r.get<int32_t>();
  const int nft = r.get<int32_t>();
  if (!r.ok || B < 1 || K < 1 || n < 1 || n > RSIM_GRAD_COLS || nbody < 1 || nq < 0 || nel < 1 || nslot < 1 || nft < 0 || B > 4096 || K > 4096 || nbody > 4096)
    return bad("header");
  const std::vector<int32_t> tab = r.vec<int32_t>((size_t)nel * RSIM_CLEAR_REC), slot = r.vec<int32_t>(nbody);
  const std::vector<int32_t> cols = r.vec<int32_t>((size_t)n * RSIM_DYN_COL);
  const std::vector<float> ft = r.vec<float>(nft);
  const std::vector<float> qpos = r.vec<float>((size_t)B * nq), xpos = r.vec<float>((size_t)B * nbody * 3), xquat = r.vec<float>((size_t)B * nbody * 4);
  const std::vector<float> q = r.vec<float>((size_t)B * K * n);
  std::vector<float> in[5];
  for (int i = 0; i < 5; i++) in[i] = r.vec<float>(has[i] ? (size_t)B * K * n : 0);
  if (!r.ok) return bad("truncated");
  // every index the core will follow
  auto in_ft = [&](int o, int w) { return o >= 0 && o + w <= nft; };
  if (!in_ft(dm.fo_mass, nbody) || !in_ft(dm.fo_inertia, 3 * nbody) || !in_ft(dm.fo_ipos, 3 * nbody) || !in_ft(dm.fo_iquat, 4 * nbody) || !in_ft(dm.fo_opt, 4))
    return bad("model offsets");
  for (int b = 0; b < nbody; b++) if (slot[b] < -1 || slot[b] >= nslot) return bad("slot");
  for (int c = 0; c < n; c++) {
    const int dof = cols[RSIM_DYN_COL * c], e = cols[RSIM_DYN_COL * c + 1];
    if (dof < 0 || !in_ft(dm.fo_armature + dof, 1) || !in_ft(dm.fo_damping + dof, 1) || e < 1 || e >= nel) return bad("column table");
    if (tab[(size_t)e * RSIM_CLEAR_REC + CLE_COL] != c) return bad("column table element");
  }
  std::vector<char> seen((size_t)nslot, 0);
  for (int e = 0; e < nel; e++) {
    const int32_t* el = tab.data() + (size_t)e * RSIM_CLEAR_REC;
    if (el[CLE_KIND] == CL_BODY) {
      if (!in_ft(el[CLE_O1], 3) || !in_ft(el[CLE_O2], 4) || el[CLE_ID] < 0 || el[CLE_ID] >= nbody || el[CLE_SLOT] < 0 || el[CLE_SLOT] >= nslot || el[CLE_COL] < -1 ||
          el[CLE_COL] >= nslot || el[CLE_PBODY] < 0 || el[CLE_PBODY] >= nbody || el[CLE_O3] != 0)
        return bad("body element");
      if (el[CLE_COL] >= 0 && !seen[el[CLE_COL]]) return bad("a parent after its child");
      if (e == 0 && el[CLE_SLOT] != 0) return bad("the first moved body is not slot 0");
      seen[el[CLE_SLOT]] = 1;
    } else if (el[CLE_KIND] == CL_BALL || el[CLE_KIND] == CL_SLIDE || el[CLE_KIND] == CL_HINGE) {
      const int w = el[CLE_KIND] == CL_BALL ? 4 : 1;
      if (e == 0 || !in_ft(el[CLE_O1], 3) || !in_ft(el[CLE_O2], 3) || !in_ft(el[CLE_O3], 1) || el[CLE_ID] < 0 || el[CLE_ID] + w > nq || el[CLE_COL] < -1 || el[CLE_COL] >= n)
        return bad("joint element");
    } else {
      return bad("element kind");   // (attachments are not carried)
    }
  }

  const int NC = B * K;
  const size_t nc = (size_t)NC;
  std::vector<float> scr((size_t)nslot * 7 * nc, 0.f), jscr((size_t)n * 6 * nc, 0.f), dscr((size_t)nslot * RSIM_DYN_RNE_WORDS * nc, 0.f);
  std::vector<float> tscr((size_t)nslot * RSIM_DYN_TAN_WORDS * nc, 0.f);
  std::vector<float> tau(nc * n, 0.f), gq(nc * n * n, 0.f), gv(nc * n * n, 0.f), ngq(nc * n * n, 0.f), ngv(nc * n * n, 0.f), jvp(nc * n, 0.f);
  int done = 0;
  for (int c = 0; c < NC; c++) {
    const int env = c / K;
    Cand cd;
    cd.ft = ft.data(); cd.qpos = qpos.data() + (size_t)env * nq; cd.q = q.data() + (size_t)c * n;
    cd.xpos = xpos.data() + (size_t)env * nbody * 3; cd.xquat = xquat.data() + (size_t)env * nbody * 4;
    PoseStore st;    // the scratch, by slot
    st.pos = scr.data() + c; st.quat = scr.data() + 3 * nc + c;
    st.pe = st.qe = 7 * nc; st.ps = st.qs = nc; st.by_body = 0;
    JointStore js;
    js.a = jscr.data() + c; js.ce = 6 * nc; js.cs = nc;
    dm.cols = cols.data();
    fk_walk(tab.data(), nel, cd, st);
    joint_walk(tab.data(), nel, cd, st, js);
    DynStore ds, dt;
    ds.a = dscr.data() + c; ds.se = RSIM_DYN_RNE_WORDS * nc; ds.ss = nc;
    dt.a = tscr.data() + c; dt.se = RSIM_DYN_TAN_WORDS * nc; dt.ss = nc;
    const size_t at = (size_t)c * n;
    const float* p[5];
    for (int i = 0; i < 5; i++) p[i] = has[i] ? in[i].data() + at : nullptr;
    rne_walk(tab.data(), nel, cd, st, js, dm, (unsigned)slide_mask, p[0], p[1], ds, tau.data() + at, 1);
    rne_grad(tab.data(), nel, cd, st, js, dm, n, (unsigned)slide_mask, p[0], p[1], ds, dt, gq.data() + at * n, gv.data() + at * n, false);
    rne_grad(tab.data(), nel, cd, st, js, dm, n, (unsigned)slide_mask, p[0], p[1], ds, dt, ngq.data() + at * n, ngv.data() + at * n, true);
    rne_tangent(tab.data(), nel, cd, st, js, dm, (unsigned)slide_mask, p[0], p[1], p[2], p[3], p[4], -1, -1, ds, dt, jvp.data() + at, 1, false);
    done++;
  }
  FILE* o = fopen(argv[2], "wb");
  if (!o) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
  bool wrote = true;
  for (const std::vector<float>* v : {&tau, &gq, &gv, &ngq, &ngv, &jvp}) wrote = wrote && fwrite(v->data(), sizeof(float), v->size(), o) == v->size();
  fclose(o);
  if (!wrote) { fprintf(stderr, "short write\n"); return 2; }
  printf("candidates: %d of %d\n", done, NC);
  return 0;
}
