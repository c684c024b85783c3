// Host rehearsal of the signed-overlap core (robosuite_amd/csrc/rsim_pen_core.h on rsim_dist_core.h): the same fp32 functions the kernel k_dist_signed runs,
// compiled for the host with g++ -fsanitize=address,undefined by tests/test_penetration_core_host.py.  Reads pair records from a binary file, writes dist /
// fromto / status / projections to another, and with a third argument prints depth, normal and projection count of every pair that descended:
//
//   in : int32 npair, float distmax, float tol, int32 max_iters, float pen_tol, int32 pen_iters, float offset, then per pair two geoms, each
//        int32 type, int32 nvert, float size[3], float pos[3] (world), float quat[4] (world, wxyz), float vert[nvert][3] (geom frame)
//   out: per pair float dist, float fromto[6] (world), float normal[3] (zero for a pair the routine did not sign), int32 status, int32 projections
//
// As in the kernel all coordinates are taken relative to geom1's position and a pair beyond distmax reports zeros as its points.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../robosuite_amd/csrc/rsim_pen_core.h"

using namespace rsim_dist;

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
struct HostGeom { int type, nvert; V3 size, pos; Q4 quat; std::vector<float> verts; };

bool read_geom(Reader& r, HostGeom& g) {
  g.type = r.get<int32_t>(); g.nvert = r.get<int32_t>();
  g.size = v3(0, 0, 0); g.pos = v3(0, 0, 0);
  g.size.x = r.get<float>(); g.size.y = r.get<float>(); g.size.z = r.get<float>();
  g.pos.x = r.get<float>(); g.pos.y = r.get<float>(); g.pos.z = r.get<float>();
  g.quat.w = r.get<float>(); g.quat.x = r.get<float>(); g.quat.y = r.get<float>(); g.quat.z = r.get<float>();
  if (!r.ok || g.nvert < 0 || (size_t)g.nvert > (r.buf.size() - r.at) / 12) return false;
  g.verts.resize((size_t)3 * g.nvert);
  for (float& v : g.verts) v = r.get<float>();
  return r.ok && (g.type != G_MESH || g.nvert >= 1);
}
}  // namespace

int main(int argc, char** argv) {
  if (argc != 3 && argc != 4) { fprintf(stderr, "usage: %s pairs.bin out.bin [print]\n", argv[0]); return 2; }
  Reader r;
  FILE* f = fopen(argv[1], "rb");
  if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  unsigned char chunk[65536];
  for (size_t n; (n = fread(chunk, 1, sizeof(chunk), f)) > 0;) r.buf.insert(r.buf.end(), chunk, chunk + n);
  fclose(f);
  const int npair = r.get<int32_t>();
  const float distmax = r.get<float>(), tol = r.get<float>();
  const int max_iters = r.get<int32_t>();
  PenOpts po;
  po.pen_tol = r.get<float>(); po.pen_iters = r.get<int32_t>(); po.offset = r.get<float>();
  if (!r.ok || npair < 0 || max_iters < 1 || max_iters > 100000 || po.pen_iters < 1 || po.pen_iters > 100000) { fprintf(stderr, "bad header\n"); return 2; }
  FILE* o = fopen(argv[2], "wb");
  if (!o) { fprintf(stderr, "cannot open %s\n", argv[2]); return 2; }
  int ncap = 0, npcap = 0, ndesc = 0, worst = 0;
  long long nsteps = 0;
  for (int p = 0; p < npair; p++) {
    HostGeom h1, h2;
    if (!read_geom(r, h1) || !read_geom(r, h2)) { fprintf(stderr, "pair %d: truncated or malformed record\n", p); fclose(o); return 2; }
    const V3 org = h1.pos;
    const Geom g1 = make_geom(h1.type, h1.size, v3(0, 0, 0), qunit(h1.quat), h1.verts.data(), h1.nvert);
    const Geom g2 = make_geom(h2.type, h2.size, h2.pos - org, qunit(h2.quat), h2.verts.data(), h2.nvert);
    int steps = 0;
    V3 nrm;
    const Result res = pair_signed(g1, g2, distmax, tol, max_iters, po, &steps, &nrm);
    const bool far = (res.status & DIST_FAR) != 0;
    const V3 p1 = far ? v3(0, 0, 0) : res.p1 + org, p2 = far ? v3(0, 0, 0) : res.p2 + org;
    const float out[10] = {res.dist, p1.x, p1.y, p1.z, p2.x, p2.y, p2.z, nrm.x, nrm.y, nrm.z};
    const int32_t st[2] = {res.status, steps};
    if (res.status & DIST_CAP) ncap++;
    if (res.status & DIST_PEN_CAP) npcap++;
    if (steps > 0) {
      ndesc++; nsteps += steps; worst = steps > worst ? steps : worst;
      if (argc == 4) {
        printf("pair %d: depth %.9g normal %.7f %.7f %.7f projections %d\n", p, (double)-res.dist, (double)nrm.x, (double)nrm.y, (double)nrm.z, steps);
      }
    }
    if (fwrite(out, sizeof(float), 10, o) != 10 || fwrite(st, sizeof(int32_t), 2, o) != 2) { fprintf(stderr, "short write\n"); fclose(o); return 2; }
  }
  fclose(o);
  printf("pairs: %d, iteration cap hit: %d, projection cap hit: %d, descended: %d, projections mean %.2f worst %d\n", npair, ncap, npcap, ndesc,
         ndesc ? (double)nsteps / ndesc : 0.0, worst);
  return 0;
}
