// Host rehearsal of the clearance gradient / collision cost core (robosuite_amd/csrc/rsim_grad_core.h on rsim_clear_core.h on rsim_dist_core.h): the same fp32
// functions the kernels k_clear_joints / k_clear_grad / k_clear_cost run per candidate, compiled for the host with g++ -fsanitize=address,undefined by
// tests/test_clearance_grad_core_host.py.  Reads one scene from a binary file, writes the poses and the results to another:
//
//   in : the input of tests/san/clear_core_driver.cpp (tests/clearance_scenes.py pack_scene; the body table may hold CL_ATTACH elements), then
//        int32 natt, has_rel, skip; int32 body_sig[nbody] (unheld | held << 16), body_att[nbody]; uint8 held[B][natt]; float rel[B][natt][7] if has_rel;
//        float d_safe; int32 slide_mask
//   out: float xpos[B][K][nbody][3], xquat[B][K][nbody][4] (the FK entry: every body), then per candidate float dist, fromto[6], int32 pair, status,
//        float grad[n], float cost, cgrad[n], int32 nnear, noverlap
//
// As in the kernels the poses of the moved bodies pass through a scratch laid out [slot][7][B K], the joint frames through a store [col][6][B K], and every table
// index is checked before it is used: a malformed file ends the program with status 2, not with a sanitizer report.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../robosuite_amd/csrc/rsim_grad_core.h"

using namespace rsim_grad;

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
  const float distmax = r.get<float>(), tol = r.get<float>();
  const int max_iters = r.get<int32_t>(), fo_size = r.get<int32_t>(), fo_pos = r.get<int32_t>(), fo_quat = r.get<int32_t>();
  if (!r.ok || B < 1 || K < 1 || n < 1 || n > 16 || nbody < 1 || nq < 0 || ngeom < 1 || nel < 1 || nslot < 1 || npair < 1 || nvert < 0 || max_iters < 1 ||
      max_iters > 100000 || B > 4096 || K > 4096 || nbody > 4096 || ngeom > 65536 || npair > 65536)
    return bad("header");
  const std::vector<int32_t> tab = r.vec<int32_t>((size_t)nel * RSIM_CLEAR_REC), slot = r.vec<int32_t>(nbody), gtype = r.vec<int32_t>(ngeom), gbody = r.vec<int32_t>(ngeom);
  const std::vector<int32_t> pairs = r.vec<int32_t>((size_t)npair * 6);
  const int nft = r.get<int32_t>();
  if (!r.ok || nft < 0) return bad("tables");
  const std::vector<float> ft = r.vec<float>(nft), verts = r.vec<float>((size_t)nvert * 3);
  const std::vector<float> qpos = r.vec<float>((size_t)B * nq), xpos = r.vec<float>((size_t)B * nbody * 3), xquat = r.vec<float>((size_t)B * nbody * 4);
  const std::vector<float> q = r.vec<float>((size_t)B * K * n);
  const int natt = r.get<int32_t>(), has_rel = r.get<int32_t>(), skip = r.get<int32_t>();
  if (!r.ok || natt < 0 || natt > RSIM_CLEAR_ATTACH_MAX) return bad("attachments");
  const std::vector<int32_t> bsig = r.vec<int32_t>(nbody), batt = r.vec<int32_t>(nbody);
  const std::vector<unsigned char> held = r.vec<unsigned char>((size_t)B * natt);
  const std::vector<float> rel = r.vec<float>(has_rel ? (size_t)B * natt * 7 : 0);
  const float d_safe = r.get<float>();
  const int slide_mask = r.get<int32_t>();
  if (!r.ok || !(d_safe > 0.f)) return bad("truncated");
  for (int b = 0; b < nbody; b++) if (batt[b] < -1 || batt[b] >= natt) return bad("body_att");
  // every index the core will follow
  auto in_ft = [&](int o, int w) { return o >= 0 && o + w <= nft; };
  for (int b = 0; b < nbody; b++) if (slot[b] < -1 || slot[b] >= nslot) return bad("slot");
  for (int e = 0; e < nel; e++) {
    const int32_t* el = tab.data() + (size_t)e * RSIM_CLEAR_REC;
    if (el[CLE_KIND] == CL_BODY) {
      if (!in_ft(el[CLE_O1], 3) || !in_ft(el[CLE_O2], 4) || el[CLE_ID] < 0 || el[CLE_ID] >= nbody || el[CLE_SLOT] < 0 || el[CLE_SLOT] >= nslot || el[CLE_COL] < -1 ||
          el[CLE_COL] >= nslot || el[CLE_PBODY] < 0 || el[CLE_PBODY] >= nbody || el[CLE_O3] < 0 || el[CLE_O3] > natt)
        return bad("body element");
    } else if (el[CLE_KIND] == CL_BALL || el[CLE_KIND] == CL_SLIDE || el[CLE_KIND] == CL_HINGE) {
      const int w = el[CLE_KIND] == CL_BALL ? 4 : 1;
      if (e == 0 || !in_ft(el[CLE_O1], 3) || !in_ft(el[CLE_O2], 3) || !in_ft(el[CLE_O3], 1) || el[CLE_ID] < 0 || el[CLE_ID] + w > nq || el[CLE_COL] < -1 || el[CLE_COL] >= n)
        return bad("joint element");
    } else if (el[CLE_KIND] == CL_ATTACH) {
      if (el[CLE_ID] < 0 || el[CLE_ID] >= nbody || el[CLE_SLOT] < 0 || el[CLE_SLOT] >= nslot || el[CLE_COL] < 0 || el[CLE_COL] >= nslot || el[CLE_PBODY] < 0 ||
          el[CLE_PBODY] >= nbody || el[CLE_O3] < 0 || el[CLE_O3] >= natt)
        return bad("attach element");
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
    }
    if (gtype[rec[0]] == G_PLANE && gtype[rec[1]] == G_PLANE) return bad("plane against plane");
  }

  const int NC = B * K;
  std::vector<float> scr((size_t)nslot * 7 * NC, 0.f), oxp((size_t)NC * nbody * 3, 0.f), oxq((size_t)NC * nbody * 4, 0.f);
  Scene<GeomRec> sc;
  sc.geom = geom.data(); sc.pairs = pairs.data(); sc.rec = 6; sc.slot_of_body = slot.data(); sc.mesh_vert = verts.data();
  sc.fo_size = fo_size; sc.fo_pos = fo_pos; sc.fo_quat = fo_quat;
  FILE* o = fopen(argv[2], "wb");
  if (!o) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
  std::vector<Best> best((size_t)NC);
  std::vector<Cost> cost((size_t)NC);
  std::vector<float> jscr((size_t)n * 6 * NC, 0.f), grad((size_t)NC * n, 0.f), cgrad((size_t)NC * n, 0.f);
  int ncap = 0;
  for (int c = 0; c < NC; c++) {
    const int env = c / K;
    Cand cd;
    cd.ft = ft.data(); cd.qpos = qpos.data() + (size_t)env * nq; cd.q = q.data() + (size_t)c * n;
    cd.xpos = xpos.data() + (size_t)env * nbody * 3; cd.xquat = xquat.data() + (size_t)env * nbody * 4;
    const Att at = att_of_env(natt, natt ? held.data() : nullptr, has_rel ? rel.data() : nullptr, skip ? bsig.data() : nullptr, batt.data(), env);
    const CandQ qv = {cd.q};
    PoseStore out;   // the FK entry: the caller's rows, by body id
    out.pos = oxp.data() + (size_t)c * nbody * 3; out.quat = oxq.data() + (size_t)c * nbody * 4;
    out.pe = 3; out.ps = 1; out.qe = 4; out.qs = 1; out.by_body = 1;
    for (int b = 0; b < nbody; b++) if (slot[b] < 0) store_pose(out, b, env_pose(cd, b));
    PoseStore st;    // the scratch, by slot
    st.pos = scr.data() + c; st.quat = scr.data() + 3 * (size_t)NC + c;
    st.pe = st.qe = 7 * (size_t)NC; st.ps = st.qs = (size_t)NC; st.by_body = 0;
    JointStore js;
    js.a = jscr.data() + c; js.ce = 6 * (size_t)NC; js.cs = (size_t)NC;
    GradAcc ga;
    ga.g = cgrad.data() + (size_t)c * n; ga.gs = 1;
    if (natt > 0) {   // what a call with attachments runs: the ATT instantiation
      fk_walk<true>(tab.data(), nel, cd, out, qv, at);
      fk_walk<true>(tab.data(), nel, cd, st, qv, at);
      best[c] = clear_pairs<true>(sc, 0, npair, cd, st, distmax, tol, max_iters, at);
      joint_walk(tab.data(), nel, cd, st, js);
      cost[c] = cost_pairs<true>(sc, 0, npair, cd, st, js, n, (unsigned)slide_mask, d_safe, tol, max_iters, at, bsig.data(), batt.data(), ga);
    } else {
      fk_walk<false>(tab.data(), nel, cd, out, qv, at);
      fk_walk<false>(tab.data(), nel, cd, st, qv, at);
      best[c] = clear_pairs<false>(sc, 0, npair, cd, st, distmax, tol, max_iters, at);
      joint_walk(tab.data(), nel, cd, st, js);
      cost[c] = cost_pairs<false>(sc, 0, npair, cd, st, js, n, (unsigned)slide_mask, d_safe, tol, max_iters, at, bsig.data(), nullptr, ga);
    }
    const Best& bb = best[c];
    int b1 = 0, b2 = 0;
    if (bb.pair >= 0) { b1 = geom[pairs[(size_t)bb.pair * 6]].body; b2 = geom[pairs[(size_t)bb.pair * 6 + 1]].body; }
    clear_grad(js, n, (unsigned)slide_mask, bb.dist, bb.pair, bb.status, bb.p1, bb.p2, b1, b2, bsig.data(), natt > 0 ? batt.data() : nullptr, at.held,
               grad.data() + (size_t)c * n);
    if (best[c].status & DIST_CAP) ncap++;
  }
  bool wrote = fwrite(oxp.data(), sizeof(float), oxp.size(), o) == oxp.size() && fwrite(oxq.data(), sizeof(float), oxq.size(), o) == oxq.size();
  for (int c = 0; c < NC && wrote; c++) {
    const Best& b = best[c];
    const float fl[7] = {b.dist, b.p1.x, b.p1.y, b.p1.z, b.p2.x, b.p2.y, b.p2.z};
    const int32_t in[2] = {b.pair, b.status}, cn[2] = {cost[c].nnear, cost[c].nover};
    wrote = fwrite(fl, sizeof(float), 7, o) == 7 && fwrite(in, sizeof(int32_t), 2, o) == 2 && fwrite(grad.data() + (size_t)c * n, sizeof(float), n, o) == (size_t)n &&
            fwrite(&cost[c].cost, sizeof(float), 1, o) == 1 && fwrite(cgrad.data() + (size_t)c * n, sizeof(float), n, o) == (size_t)n &&
            fwrite(cn, sizeof(int32_t), 2, o) == 2;
  }
  fclose(o);
  if (!wrote) { fprintf(stderr, "short write\n"); return 2; }
  printf("candidates: %d, pairs: %d, iteration cap hit: %d\n", NC, npair, ncap);
  return 0;
}
