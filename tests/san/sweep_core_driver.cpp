// Host rehearsal of the swept clearance core (robosuite_amd/csrc/rsim_sweep_core.h on rsim_clear_core.h and rsim_dist_core.h): the same fp32 functions k_sweep
// runs per segment -- the motion-bound walk and the advancement loop -- compiled for the host with g++ -fsanitize=address,undefined by
// tests/test_sweep_core_host.py.  Reads one scene from a binary file, writes the results to another (tests/sweep_scenes.py pack_sweep / unpack_sweep):
//
//   in : the scene of tests/san/clear_core_driver.cpp (tests/clearance_scenes.py pack_scene), its q [B][K][n] being the segments' START q0; then
//        float margin, slack; int32 max_steps; float rcenter[ngeom][3], rbound[ngeom] (the geoms' bounding spheres); float q1[B][K][n] (the segments' ENDS)
//   out: per segment float L, t, dist, t_min, fromto[6]; int32 status, pair, steps
//
// As in the kernel the poses of the moved bodies (and, before the first sample, Omega and V) pass through a scratch laid out [slot][7][B K], and every table
// index is checked before it is used: a malformed file ends the program with status 2, not with a sanitizer report.
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
  if (!r.ok) return bad("truncated");
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
          el[CLE_COL] >= nslot || el[CLE_PBODY] < 0 || el[CLE_PBODY] >= nbody)
        return bad("body element");
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
  for (int c = 0; c < NC && wrote; c++) {
    const int env = c / K;
    Seg s;
    s.env.ft = ft.data(); s.env.qpos = qpos.data() + (size_t)env * nq;
    s.env.xpos = xpos.data() + (size_t)env * nbody * 3; s.env.xquat = xquat.data() + (size_t)env * nbody * 4;
    s.q0 = q0.data() + (size_t)c * n; s.q1 = q1.data() + (size_t)c * n;
    s.env.q = s.q0;
    PoseStore st;
    st.pos = scr.data() + c; st.quat = scr.data() + 3 * (size_t)NC + c;
    st.pe = st.qe = 7 * (size_t)NC; st.ps = st.qs = (size_t)NC; st.by_body = 0;
    const float L = motion_bound(tab.data(), nel, sc, fo_rcenter, fo_rbound, npair, s, st);
    const Out r = sweep(tab.data(), nel, sc, npair, s, st, op, L);
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
