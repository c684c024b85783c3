// Host rehearsal of the collision-aware IK core (robosuite_amd/csrc/rsim_ik_avoid_core.h on rsim_grad_core.h on rsim_clear_core.h on rsim_dist_core.h): the same
// fp32 functions the kernels k_ika_init / k_ika_cost / k_ika_step run per problem, compiled for the host with g++ -fsanitize=address,undefined by
// tests/test_ik_avoid_core_host.py.  Reads one scene from a binary file, runs the chain for a few evaluations and writes every iterate to another:
//
//   in : the input of tests/san/clear_core_driver.cpp (tests/clearance_scenes.py pack_scene; q holds the START vectors), then
//        int32 nextra; float extra[nextra] (appended to the float table: jnt_range rows, site_pos, site_quat);
//        int32 site_slot, o_site_pos, o_site_quat, site_sig, slide_mask, rows, max_iters, clamp_range, evals, chunks; int32 head[n][4]; int32 body_sig[nbody];
//        float damping, max_dq, pos_tol, rot_tol, posture_gain, avoid_gain, cost_tol, d_safe; float tpos[B K][3]; float tquat[B K][4] if rows == 6
//   out: float q[B K][n] after the start, then per evaluation float rec[B K][8] = en, wn, cost, nnear, nover, iters word's count, conv, fin (of the problems that
//        were evaluated; a frozen problem repeats its last record) and float q[B K][n] after it
//
// As in the kernels the poses pass through a scratch laid out [slot][7][B K], the joint frames through a store [col][6][B K], the partial results through
// [chunks][3 + n][B K], and every table index is checked before it is used: a malformed file ends the program with status 2, not with a sanitizer report.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../robosuite_amd/csrc/rsim_ik_avoid_core.h"

using namespace rsim_ika;

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
struct GeomRec { int type, body, cg; float size[3], pos[3], quat[4]; };
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
  const int B = r.get<int32_t>(), K = r.get<int32_t>(), n = r.get<int32_t>(), nbody = r.get<int32_t>(), nq = r.get<int32_t>(), ngeom = r.get<int32_t>();
  const int nel = r.get<int32_t>(), nslot = r.get<int32_t>(), npair = r.get<int32_t>(), nvert = r.get<int32_t>();
  (void)r.get<float>();   // distmax: the cost's is d_safe
  const float tol = r.get<float>();
  const int max_gjk = r.get<int32_t>(), fo_size = r.get<int32_t>(), fo_pos = r.get<int32_t>(), fo_quat = r.get<int32_t>();
  if (!r.ok || B < 1 || K < 1 || n < 1 || n > 16 || nbody < 1 || nq < 0 || ngeom < 1 || nel < 1 || nslot < 1 || npair < 1 || nvert < 0 || max_gjk < 1 ||
      max_gjk > 100000 || B > 4096 || K > 4096 || nbody > 4096 || ngeom > 65536 || npair > 65536)
    return bad("header");
  const std::vector<int32_t> tab = r.vec<int32_t>((size_t)nel * RSIM_CLEAR_REC), slot = r.vec<int32_t>(nbody), gtype = r.vec<int32_t>(ngeom), gbody = r.vec<int32_t>(ngeom);
  const std::vector<int32_t> pairs = r.vec<int32_t>((size_t)npair * 6);
  const int nft0 = r.get<int32_t>();
  if (!r.ok || nft0 < 0) return bad("tables");
  std::vector<float> ft = r.vec<float>(nft0);
  const std::vector<float> verts = r.vec<float>((size_t)nvert * 3);
  const std::vector<float> qpos = r.vec<float>((size_t)B * nq), xpos = r.vec<float>((size_t)B * nbody * 3), xquat = r.vec<float>((size_t)B * nbody * 4);
  const std::vector<float> q_init = r.vec<float>((size_t)B * K * n);
  const int nextra = r.get<int32_t>();
  if (!r.ok || nextra < 0 || nextra > 65536) return bad("extra");
  const std::vector<float> extra = r.vec<float>(nextra);
  ft.insert(ft.end(), extra.begin(), extra.end());
  const int nft = (int)ft.size();
  Opts o;
  o.n = n;
  o.site_slot = r.get<int32_t>(); o.o_site_pos = r.get<int32_t>(); o.o_site_quat = r.get<int32_t>();
  o.site_sig = (unsigned)r.get<int32_t>(); o.slide_mask = (unsigned)r.get<int32_t>();
  o.rows = r.get<int32_t>(); o.max_iters = r.get<int32_t>(); o.clamp_range = r.get<int32_t>();
  const int evals = r.get<int32_t>(), chunks = r.get<int32_t>();
  const std::vector<int32_t> head = r.vec<int32_t>((size_t)n * RSIM_IKA_HEAD), bsig = r.vec<int32_t>(nbody);
  o.damping = r.get<float>(); o.max_dq = r.get<float>(); o.pos_tol = r.get<float>(); o.rot_tol = r.get<float>(); o.posture_gain = r.get<float>();
  o.avoid_gain = r.get<float>(); o.cost_tol = r.get<float>();
  const float d_safe = r.get<float>();
  const int NC = B * K;
  const std::vector<float> tpos = r.vec<float>((size_t)NC * 3), tquat = r.vec<float>(o.rows == 6 ? (size_t)NC * 4 : 0);
  if (!r.ok || !(d_safe > 0.f) || (o.rows != 3 && o.rows != 6) || evals < 1 || evals > 1000 || chunks < 1 || chunks > npair || o.max_iters < 0) return bad("truncated");
  o.head = head.data();
  // every index the core will follow
  auto in_ft = [&](int off, int w) { return off >= 0 && off + w <= nft; };
  if (o.site_slot < 0 || o.site_slot >= nslot || !in_ft(o.o_site_pos, 3) || !in_ft(o.o_site_quat, 4)) return bad("site");
  for (int c = 0; c < n; c++) {
    const int32_t* h = head.data() + (size_t)c * RSIM_IKA_HEAD;
    if (!in_ft(h[0], 2) || h[2] < 0 || h[2] >= nq) return bad("head");
  }
  for (int b = 0; b < nbody; b++) if (slot[b] < -1 || slot[b] >= nslot) return bad("slot");
  for (int e = 0; e < nel; e++) {
    const int32_t* el = tab.data() + (size_t)e * RSIM_CLEAR_REC;
    if (el[CLE_KIND] == CL_BODY) {
      if (!in_ft(el[CLE_O1], 3) || !in_ft(el[CLE_O2], 4) || el[CLE_ID] < 0 || el[CLE_ID] >= nbody || el[CLE_SLOT] < 0 || el[CLE_SLOT] >= nslot || el[CLE_COL] < -1 ||
          el[CLE_COL] >= nslot || el[CLE_PBODY] < 0 || el[CLE_PBODY] >= nbody)
        return bad("body element");
    } else if (el[CLE_KIND] == CL_BALL || el[CLE_KIND] == CL_SLIDE || el[CLE_KIND] == CL_HINGE) {
      const int w = el[CLE_KIND] == CL_BALL ? 4 : 1;
      if (e == 0 || !in_ft(el[CLE_O1], 3) || !in_ft(el[CLE_O2], 3) || !in_ft(el[CLE_O3], 1) || el[CLE_ID] < 0 || el[CLE_ID] + w > nq || el[CLE_COL] < -1 || el[CLE_COL] >= n)
        return bad("joint element");
    } else {
      return bad("element kind");   // (the rehearsal runs the plain instantiation: no CL_ATTACH)
    }
  }
  std::vector<GeomRec> geom((size_t)ngeom);
  for (int g = 0; g < ngeom; g++) {
    if (gbody[g] < 0 || gbody[g] >= nbody || !in_ft(fo_size + 3 * g, 3) || !in_ft(fo_pos + 3 * g, 3) || !in_ft(fo_quat + 4 * g, 4)) return bad("geom");
    GeomRec& s = geom[g];
    memset(&s, 0, sizeof(s));
    s.type = gtype[g]; s.body = gbody[g]; s.cg = g;
    s.quat[0] = 1.f;
  }
  for (int p = 0; p < npair; p++) {
    const int32_t* rec = pairs.data() + (size_t)p * 6;
    for (int k = 0; k < 2; k++) {
      const int g = rec[k], adr = rec[2 + 2 * k], num = rec[3 + 2 * k];
      if (g < 0 || g >= ngeom || adr < 0 || num < 0 || adr + num > nvert) return bad("pair");
      const int t = gtype[g];
      if (!(t == G_PLANE || (t >= G_SPHERE && t <= G_MESH)) || (t == G_MESH && num < 1)) return bad("pair geom type");
    }
    if (gtype[rec[0]] == G_PLANE && gtype[rec[1]] == G_PLANE) return bad("plane against plane");
  }

  Scene<GeomRec> sc;
  sc.geom = geom.data(); sc.pairs = pairs.data(); sc.rec = 6; sc.slot_of_body = slot.data(); sc.mesh_vert = verts.data();
  sc.fo_size = fo_size; sc.fo_pos = fo_pos; sc.fo_quat = fo_quat;
  const size_t nc = (size_t)NC;
  std::vector<float> scr((size_t)nslot * 7 * nc, 0.f), jscr((size_t)n * 6 * nc, 0.f), part((size_t)chunks * (RSIM_IKA_PART + n) * nc, 0.f);
  std::vector<float> q(nc * n, 0.f), q_rest(nc * n, 0.f), rec(nc * 8, 0.f);
  std::vector<int> done(nc, 0), iters(nc, 0);
  const Att none = {0u, nullptr, nullptr, nullptr};
  auto cand = [&](int c) {
    const int env = c / K;
    Cand cd;
    cd.ft = ft.data(); cd.qpos = qpos.data() + (size_t)env * nq; cd.q = q.data() + (size_t)c * n;
    cd.xpos = xpos.data() + (size_t)env * nbody * 3; cd.xquat = xquat.data() + (size_t)env * nbody * 4;
    return cd;
  };
  auto store = [&](int c) {
    PoseStore st;
    st.pos = scr.data() + c; st.quat = scr.data() + 3 * nc + c;
    st.pe = st.qe = 7 * nc; st.ps = st.qs = nc; st.by_body = 0;
    return st;
  };
  auto jstore = [&](int c) {
    JointStore js;
    js.a = jscr.data() + c; js.ce = 6 * nc; js.cs = nc;
    return js;
  };
  auto walks = [&](int c) {
    const Cand cd = cand(c);
    const CandQ qv = {cd.q};
    fk_walk<false>(tab.data(), nel, cd, store(c), qv, none);
    joint_walk(tab.data(), nel, cd, store(c), jstore(c));
  };
  FILE* out = fopen(argv[2], "wb");
  if (!out) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
  for (int c = 0; c < NC; c++) {   // k_ika_init
    const Cand cd = cand(c);
    ika_start(o, cd.ft, cd.qpos, q_init.data() + (size_t)c * n, q.data() + (size_t)c * n, q_rest.data() + (size_t)c * n);
    walks(c);
  }
  bool wrote = fwrite(q.data(), sizeof(float), q.size(), out) == q.size();
  const int per = (npair + chunks - 1) / chunks;
  int nfin = 0;
  for (int ev = 0; ev < evals && wrote; ev++) {
    for (int k = 0; k < chunks; k++)   // k_ika_cost
      for (int c = 0; c < NC; c++) {
        if (done[c]) continue;
        float* w = part.data() + (size_t)k * (RSIM_IKA_PART + n) * nc + c;
        GradAcc ga;
        ga.g = w + RSIM_IKA_PART * nc; ga.gs = nc;
        const int p0 = k * per, p1 = p0 + per < npair ? p0 + per : npair;
        const Cost r2 = cost_pairs<false>(sc, p0, p1, cand(c), store(c), jstore(c), n, o.slide_mask, d_safe, tol, max_gjk, none, bsig.data(), nullptr, ga);
        w[0] = r2.cost;
        memcpy(w + nc, &r2.nnear, 4); memcpy(w + 2 * nc, &r2.nover, 4);
      }
    for (int c = 0; c < NC; c++) {   // k_ika_step
      if (done[c]) continue;
      Prob pr;
      pr.q = q.data() + (size_t)c * n; pr.q_rest = q_rest.data() + (size_t)c * n;
      pr.part = part.data() + c; pr.part_ks = (size_t)(RSIM_IKA_PART + n) * nc; pr.part_ws = nc; pr.chunks = chunks;
      pr.tpos = tpos.data() + (size_t)c * 3; pr.tquat = o.rows == 6 ? tquat.data() + (size_t)c * 4 : nullptr;
      bool updated;
      const Eval e2 = ika_step(o, pr, ft.data(), store(c), jstore(c), iters[c], updated);
      float* w = rec.data() + (size_t)c * 8;
      w[0] = e2.en; w[1] = e2.wn; w[2] = e2.cost; w[3] = (float)e2.nnear; w[4] = (float)e2.nover; w[5] = (float)iters[c]; w[6] = (float)e2.conv; w[7] = (float)e2.fin;
      if (!updated) { done[c] = 1; nfin += e2.fin; continue; }
      iters[c]++;
      walks(c);
    }
    wrote = fwrite(rec.data(), sizeof(float), rec.size(), out) == rec.size() && fwrite(q.data(), sizeof(float), q.size(), out) == q.size();
  }
  fclose(out);
  if (!wrote) { fprintf(stderr, "short write\n"); return 2; }
  printf("problems: %d, pairs: %d, evaluations: %d, finished: %d\n", NC, npair, evals, nfin);
  return 0;
}
