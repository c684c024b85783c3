// Host rehearsal of the signed running minimum (robosuite_amd/csrc/rsim_pen_clear_core.h clear_pairs_signed on rsim_pen_core.h / rsim_clear_core.h): the same fp32
// functions the kernel k_clear_dist_signed runs per candidate, compiled for the host with g++ -fsanitize=address,undefined by
// tests/test_signed_queries_core_host.py.  Reads candidates, each a list of pair records, from a binary file and writes two answers per candidate to another:
// clear_pairs_signed over the list, and the plain minimum of pair_signed over the same records, every pair queried with the call's distmax.
//
//   in : int32 ncand, float distmax, float tol, int32 max_iters, float pen_tol, int32 pen_iters, float offset; then per candidate int32 npair and per pair two
//        geoms, each int32 type, int32 nvert, float size[3], float pos[3] (world), float quat[4] (world, wxyz), float vert[nvert][3] (geom frame)
//        -- tests/san/pen_core_driver.cpp's record
//   out: per candidate float dist, float fromto[6], float brute_dist, int32 pair, int32 status, int32 projections, int32 brute_pair
//
// Every geom of a candidate is a body of its own that no candidate moves (slot -1): load_geom reads its pose as it reads an unmoved body's on the device.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../robosuite_amd/csrc/rsim_pen_clear_core.h"

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
};
struct GeomRec { int type, body, cg; float size[3], pos[3], quat[4]; };
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: %s candidates.bin out.bin\n", argv[0]); return 2; }
  Reader r;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  unsigned char chunk[65536];
  for (size_t n; (n = fread(chunk, 1, sizeof(chunk), f)) > 0;) r.buf.insert(r.buf.end(), chunk, chunk + n);
  fclose(f);
  const int ncand = r.get<int32_t>();
  const float distmax = r.get<float>(), tol = r.get<float>();
  const int max_iters = r.get<int32_t>();
  PenOpts po;
  po.pen_tol = r.get<float>(); po.pen_iters = r.get<int32_t>(); po.offset = r.get<float>();
  if (!r.ok || ncand < 0 || max_iters < 1 || max_iters > 100000 || po.pen_iters < 1 || po.pen_iters > 100000) { fprintf(stderr, "bad header\n"); return 2; }
  FILE* o = fopen(argv[2], "wb");
  if (!o) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
  int ncap = 0, npcap = 0, nneg = 0, ndiffer = 0;
  long long nsteps = 0;
  for (int c = 0; c < ncand; c++) {
    const int npair = r.get<int32_t>();
    if (!r.ok || npair < 1 || npair > 65536) { fprintf(stderr, "candidate %d: bad pair count\n", c); fclose(o); return 2; }
    const int ng = 2 * npair;
    std::vector<GeomRec> geom((size_t)ng);
    std::vector<float> xpos((size_t)ng * 3), xquat((size_t)ng * 4), verts;
    std::vector<int32_t> pairs((size_t)npair * 6), slot((size_t)ng, -1);
    for (int g = 0; g < ng; g++) {
      GeomRec& s = geom[g];
      memset(&s, 0, sizeof(s));
      s.type = r.get<int32_t>();
      const int nvert = r.get<int32_t>();
      s.body = g; s.cg = -1; s.quat[0] = 1.f;
      for (int k = 0; k < 3; k++) s.size[k] = r.get<float>();
      for (int k = 0; k < 3; k++) xpos[(size_t)g * 3 + k] = r.get<float>();
      for (int k = 0; k < 4; k++) xquat[(size_t)g * 4 + k] = r.get<float>();
      if (!r.ok || nvert < 0 || (size_t)nvert > (r.buf.size() - r.at) / 12 || !(s.type == G_PLANE || (s.type >= G_SPHERE && s.type <= G_MESH)) ||
          (s.type == G_MESH && nvert < 1)) {
        fprintf(stderr, "candidate %d: truncated or malformed record\n", c); fclose(o); return 2;
      }
      int32_t* rec = pairs.data() + (size_t)(g / 2) * 6;
      rec[g % 2] = g; rec[2 + 2 * (g % 2)] = (int32_t)(verts.size() / 3); rec[3 + 2 * (g % 2)] = nvert;
      for (int k = 0; k < 3 * nvert; k++) verts.push_back(r.get<float>());
    }
    if (!r.ok) { fprintf(stderr, "candidate %d: truncated\n", c); fclose(o); return 2; }
    verts.push_back(0.f);   // (never empty: mesh_vert + 0 is a valid pointer)
    Scene<GeomRec> sc;
    sc.geom = geom.data(); sc.pairs = pairs.data(); sc.rec = 6; sc.slot_of_body = slot.data(); sc.mesh_vert = verts.data();
    sc.fo_size = sc.fo_pos = sc.fo_quat = 0;
    Cand cd;
    cd.ft = nullptr; cd.qpos = nullptr; cd.q = nullptr; cd.xpos = xpos.data(); cd.xquat = xquat.data();
    PoseStore st;   // no body is moved: never read
    st.pos = st.quat = nullptr; st.pe = st.ps = st.qe = st.qs = 0; st.by_body = 0;
    const Att none = {0u, nullptr, nullptr, nullptr};
    int steps = 0;
    const Best b = clear_pairs_signed<false>(sc, 0, npair, cd, st, distmax, tol, max_iters, po, none, &steps);
    // the definition: every pair with the call's distmax, the smallest signed value, the lowest index on ties
    float bd = distmax;
    int bp = -1;
    for (int p = 0; p < npair; p++) {
      const int32_t* rec = pairs.data() + (size_t)p * 6;
      Geom A = load_geom(sc, rec[0], cd, st, rec[2], rec[3]), Bg = load_geom(sc, rec[1], cd, st, rec[4], rec[5]);
      const V3 org = A.p;
      A.p = v3(0, 0, 0); Bg.p = Bg.p - org;
      const Result res = pair_signed(A, Bg, distmax, tol, max_iters, po);
      if (!(res.status & DIST_FAR) && res.dist < bd) { bd = res.dist; bp = p; }
    }
    if (b.status & DIST_CAP) ncap++;
    if (b.status & DIST_PEN_CAP) npcap++;
    nneg += b.dist < 0.f; nsteps += steps; ndiffer += (b.dist != bd || b.pair != bp);
    const float fl[8] = {b.dist, b.p1.x, b.p1.y, b.p1.z, b.p2.x, b.p2.y, b.p2.z, bd};
    const int32_t in[4] = {b.pair, b.status, steps, bp};
    if (fwrite(fl, sizeof(float), 8, o) != 8 || fwrite(in, sizeof(int32_t), 4, o) != 4) { fprintf(stderr, "short write\n"); fclose(o); return 2; }
  }
  fclose(o);
  printf("candidates: %d, below zero: %d, iteration cap hit: %d, projection cap hit: %d, projections: %lld, differ from the plain minimum: %d\n", ncand, nneg, ncap,
         npcap, nsteps, ndiffer);
  return 0;
}
