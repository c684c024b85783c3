// Host rehearsal of the carried-object paths of the clearance and sweep cores (robosuite_amd/csrc/rsim_clear_core.h, rsim_sweep_core.h with ATT = true): the
// same fp32 functions k_clear_fk_att, k_clear_dist_att and k_sweep_att run per lane -- the walk of the attached subtrees, the per-lane skip of the pairs an env
// does not evaluate, the motion bound of a held body and the advancement loop -- compiled for the host with g++ -fsanitize=address,undefined by
// tests/test_attach_core_host.py.  Reads one scene from a binary file, writes the results to another (tests/attach_scenes.py pack_attach / unpack_attach):
//
//   in : the scene of tests/san/sweep_core_driver.cpp, its body table and slots being those WITH the attached subtrees (CL_ATTACH elements behind the ordinary
//        bodies); then int32 natt, has_rel, skip; int32 body_sig[nbody], body_att[nbody]; uint8 held[B][natt]; float rel[B][natt][7] if has_rel
//   out: float xpos[B][K][nbody][3], xquat[B][K][nbody][4]: the FK entry at q0 (bodies without a slot: the env's pose); per candidate q0 float dist, fromto[6],
//        int32 pair, status: the clearance entry; per segment float L, t, dist, t_min, fromto[6], int32 status, pair, steps: the sweep entry
//
// Every table index is checked before it is used: a malformed file ends the program with status 2, not with a sanitizer report.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../robosuite_amd/csrc/rsim_sweep_core.h"

using namespace rsim_sweep;

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
struct GeomRec { int type, body, cg; float size[3], pos[3], quat[4], rcenter[3], rbound; };
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
  const float distmax = r.get<float>(), tol = r.get<float>();
  const int max_iters = r.get<int32_t>(), fo_size = r.get<int32_t>(), fo_pos = r.get<int32_t>(), fo_quat = r.get<int32_t>();
  if (!r.ok || B < 1 || K < 1 || n < 1 || n > 16 || nbody < 1 || nq < 0 || ngeom < 1 || nel < 1 || nslot < 1 || npair < 1 || nvert < 0 || max_iters < 1 ||
      max_iters > 100000 || B > 4096 || K > 4096 || nbody > 4096 || ngeom > 65536 || npair > 65536)
    return bad("header");
  const std::vector<int32_t> tab = r.vec<int32_t>((size_t)nel * RSIM_CLEAR_REC), slot = r.vec<int32_t>(nbody), gtype = r.vec<int32_t>(ngeom), gbody = r.vec<int32_t>(ngeom);
  const std::vector<int32_t> pairs = r.vec<int32_t>((size_t)npair * 6);
  const int nft = r.get<int32_t>();
  if (!r.ok || nft < 0) return bad("tables");
  std::vector<float> ft = r.vec<float>(nft);
  const std::vector<float> verts = r.vec<float>((size_t)nvert * 3);
  const std::vector<float> qpos = r.vec<float>((size_t)B * nq), xpos = r.vec<float>((size_t)B * nbody * 3), xquat = r.vec<float>((size_t)B * nbody * 4);
  const std::vector<float> q0 = r.vec<float>((size_t)B * K * n);
  const float margin = r.get<float>(), slack = r.get<float>();
  const int max_steps = r.get<int32_t>();
  const std::vector<float> rcenter = r.vec<float>((size_t)ngeom * 3), rbound = r.vec<float>(ngeom), q1 = r.vec<float>((size_t)B * K * n);
  const int natt = r.get<int32_t>(), has_rel = r.get<int32_t>(), skip = r.get<int32_t>();
  if (!r.ok || natt < 1 || natt > RSIM_CLEAR_ATTACH_MAX) return bad("attachment header");
  const std::vector<int32_t> body_sig = r.vec<int32_t>(nbody), body_att = r.vec<int32_t>(nbody);
  const std::vector<unsigned char> held = r.vec<unsigned char>((size_t)B * natt);
  const std::vector<float> rel = has_rel ? r.vec<float>((size_t)B * natt * 7) : std::vector<float>();
  if (!r.ok) return bad("truncated");
  for (int b = 0; b < nbody; b++) if (body_att[b] < -1 || body_att[b] >= natt) return bad("body_att");
  if (!(margin >= 0.f) || !(slack > 0.f) || max_steps < 1 || max_steps > 4096 || !(distmax > margin + slack)) return bad("options");
  // the bounding spheres ride behind the float table, as a colliding geom's do on the device
  const int fo_rcenter = nft, fo_rbound = nft + 3 * ngeom;
  ft.insert(ft.end(), rcenter.begin(), rcenter.end());
  ft.insert(ft.end(), rbound.begin(), rbound.end());
  // every index the core will follow
  auto in_ft = [&](int o, int w) { return o >= 0 && o + w <= nft; };
  for (int b = 0; b < nbody; b++) if (slot[b] < -1 || slot[b] >= nslot) return bad("slot");
  for (int e = 0; e < nel; e++) {
    const int32_t* el = tab.data() + (size_t)e * RSIM_CLEAR_REC;
    if (el[CLE_KIND] == CL_BODY) {
      if (!in_ft(el[CLE_O1], 3) || !in_ft(el[CLE_O2], 4) || el[CLE_ID] < 0 || el[CLE_ID] >= nbody || el[CLE_SLOT] < 0 || el[CLE_SLOT] >= nslot || el[CLE_COL] < -1 ||
          el[CLE_COL] >= nslot || el[CLE_PBODY] < 0 || el[CLE_PBODY] >= nbody || el[CLE_O3] < 0 || el[CLE_O3] > natt)
        return bad("body element");
    } else if (el[CLE_KIND] == CL_ATTACH) {
      if (el[CLE_ID] < 0 || el[CLE_ID] >= nbody || el[CLE_SLOT] < 0 || el[CLE_SLOT] >= nslot || el[CLE_COL] < 0 || el[CLE_COL] >= nslot || el[CLE_PBODY] < 0 ||
          el[CLE_PBODY] >= nbody || el[CLE_O3] < 0 || el[CLE_O3] >= natt || slot[el[CLE_PBODY]] != el[CLE_COL] || slot[el[CLE_ID]] != el[CLE_SLOT])
        return bad("attach element");
    } else if (el[CLE_KIND] == CL_BALL || el[CLE_KIND] == CL_SLIDE || el[CLE_KIND] == CL_HINGE) {
      const int w = el[CLE_KIND] == CL_BALL ? 4 : 1;
      if (e == 0 || !in_ft(el[CLE_O1], 3) || !in_ft(el[CLE_O2], 3) || !in_ft(el[CLE_O3], 1) || el[CLE_ID] < 0 || el[CLE_ID] + w > nq || el[CLE_COL] < -1 || el[CLE_COL] >= n)
        return bad("joint element");
    } else {
      return bad("element kind");
    }
  }
  std::vector<GeomRec> geom((size_t)ngeom);
  for (int g = 0; g < ngeom; g++) {
    if (gbody[g] < 0 || gbody[g] >= nbody || !in_ft(fo_size + 3 * g, 3) || !in_ft(fo_pos + 3 * g, 3) || !in_ft(fo_quat + 4 * g, 4)) return bad("geom");
    GeomRec& s = geom[g];
    memset(&s, 0, sizeof(s));
    s.type = gtype[g]; s.body = gbody[g]; s.cg = g;   // every geom reads the float table, as a colliding geom does on the device
    s.quat[0] = 1.f;
  }
  for (int p = 0; p < npair; p++) {
    const int32_t* rec = pairs.data() + (size_t)p * 6;
    for (int k = 0; k < 2; k++) {
      const int g = rec[k], adr = rec[2 + 2 * k], num = rec[3 + 2 * k];
      if (g < 0 || g >= ngeom || adr < 0 || num < 0 || adr + num > nvert) return bad("pair");
      const int t = gtype[g];
      if (!(t == G_PLANE || (t >= G_SPHERE && t <= G_MESH)) || (t == G_MESH && num < 1)) return bad("pair geom type");
      if (t == G_PLANE && slot[gbody[g]] >= 0) return bad("plane on a moved body");
    }
    if (gtype[rec[0]] == G_PLANE && gtype[rec[1]] == G_PLANE) return bad("plane against plane");
  }

  const int NC = B * K;
  std::vector<float> scr((size_t)nslot * 7 * NC, 0.f);
  Scene<GeomRec> sc;
  sc.geom = geom.data(); sc.pairs = pairs.data(); sc.rec = 6; sc.slot_of_body = slot.data(); sc.mesh_vert = verts.data();
  sc.fo_size = fo_size; sc.fo_pos = fo_pos; sc.fo_quat = fo_quat;
  Opts op;
  op.distmax = distmax; op.tol = tol; op.max_iters = max_iters; op.margin = margin; op.slack = slack; op.max_steps = max_steps;
  FILE* o = fopen(argv[2], "wb");
  if (!o) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
  bool wrote = true;
  int count[3] = {0, 0, 0}, ncap = 0, worst = 0;
  auto lane_att = [&](int env) {
    Att at;
    at.held = 0u;
    for (int i = 0; i < natt; i++) at.held |= held[(size_t)env * natt + i] ? 1u << i : 0u;
    at.rel = has_rel ? rel.data() + (size_t)env * natt * 7 : nullptr;
    at.body_sig = skip ? body_sig.data() : nullptr; at.body_att = body_att.data();
    return at;
  };
  // the FK entry: the caller's [nbody] rows per candidate, bodies without a slot copied from the env
  {
    std::vector<float> xp((size_t)NC * nbody * 3, 0.f), xq((size_t)NC * nbody * 4, 0.f);
    for (int c = 0; c < NC; c++) {
      const int env = c / K;
      Cand cd;
      cd.ft = ft.data(); cd.qpos = qpos.data() + (size_t)env * nq; cd.q = q0.data() + (size_t)c * n;
      cd.xpos = xpos.data() + (size_t)env * nbody * 3; cd.xquat = xquat.data() + (size_t)env * nbody * 4;
      PoseStore ps;
      ps.pos = xp.data() + (size_t)c * nbody * 3; ps.quat = xq.data() + (size_t)c * nbody * 4;
      ps.pe = 3; ps.ps = 1; ps.qe = 4; ps.qs = 1; ps.by_body = 1;
      for (int b = 0; b < nbody; b++) if (slot[b] < 0) store_pose(ps, b, env_pose(cd, b));
      const CandQ qv = {cd.q};
      fk_walk<true>(tab.data(), nel, cd, ps, qv, lane_att(env));
    }
    wrote = fwrite(xp.data(), sizeof(float), xp.size(), o) == xp.size() && fwrite(xq.data(), sizeof(float), xq.size(), o) == xq.size();
  }
  // the clearance entry at q0: the walk into the scratch, then the pair loop in one chunk
  for (int c = 0; c < NC && wrote; c++) {
    const int env = c / K;
    Cand cd;
    cd.ft = ft.data(); cd.qpos = qpos.data() + (size_t)env * nq; cd.q = q0.data() + (size_t)c * n;
    cd.xpos = xpos.data() + (size_t)env * nbody * 3; cd.xquat = xquat.data() + (size_t)env * nbody * 4;
    PoseStore st;
    st.pos = scr.data() + c; st.quat = scr.data() + 3 * (size_t)NC + c;
    st.pe = st.qe = 7 * (size_t)NC; st.ps = st.qs = (size_t)NC; st.by_body = 0;
    const Att at = lane_att(env);
    const CandQ qv = {cd.q};
    fk_walk<true>(tab.data(), nel, cd, st, qv, at);
    const Best b = clear_pairs<true>(sc, 0, npair, cd, st, distmax, tol, max_iters, at);
    const float fl[7] = {b.dist, b.p1.x, b.p1.y, b.p1.z, b.p2.x, b.p2.y, b.p2.z};
    const int32_t in[2] = {b.pair, b.status};
    wrote = fwrite(fl, sizeof(float), 7, o) == 7 && fwrite(in, sizeof(int32_t), 2, o) == 2;
  }
  for (int c = 0; c < NC && wrote; c++) {
    const int env = c / K;
    const Att at = lane_att(env);
    Seg s;
    s.env.ft = ft.data(); s.env.qpos = qpos.data() + (size_t)env * nq;
    s.env.xpos = xpos.data() + (size_t)env * nbody * 3; s.env.xquat = xquat.data() + (size_t)env * nbody * 4;
    s.q0 = q0.data() + (size_t)c * n; s.q1 = q1.data() + (size_t)c * n;
    s.env.q = s.q0;
    PoseStore st;
    st.pos = scr.data() + c; st.quat = scr.data() + 3 * (size_t)NC + c;
    st.pe = st.qe = 7 * (size_t)NC; st.ps = st.qs = (size_t)NC; st.by_body = 0;
    const float L = motion_bound<true>(tab.data(), nel, sc, fo_rcenter, fo_rbound, npair, s, st, at);
    const Out r = sweep<true>(tab.data(), nel, sc, npair, s, st, op, L, at);
    if ((r.status & 3) > 2 || r.steps < 1 || r.steps > max_steps) { fprintf(stderr, "segment %d: status %d after %d samples\n", c, r.status, r.steps); fclose(o); return 3; }
    count[r.status & 3]++; ncap += (r.status & DIST_CAP) ? 1 : 0; worst = r.steps > worst ? r.steps : worst;
    const float fl[10] = {L, r.t, r.best.dist, r.t_min, r.best.p1.x, r.best.p1.y, r.best.p1.z, r.best.p2.x, r.best.p2.y, r.best.p2.z};
    const int32_t in[3] = {r.status, r.best.pair, r.steps};
    wrote = fwrite(fl, sizeof(float), 10, o) == 10 && fwrite(in, sizeof(int32_t), 3, o) == 3;
  }
  fclose(o);
  if (!wrote) { fprintf(stderr, "short write\n"); return 2; }
  printf("segments: %d (free %d, hit %d, undecided %d), pairs: %d, most samples: %d, iteration cap hit: %d\n", NC, count[0], count[1], count[2], npair, worst, ncap);
  return 0;
}
