"""Host rehearsal of the signed-overlap core (robosuite_amd/csrc/rsim_pen_core.h on rsim_dist_core.h, the code k_dist_signed runs per pair) under AddressSanitizer
+ UndefinedBehaviorSanitizer: tests/san/pen_core_driver.cpp is built with g++ and run as a subprocess on the pairs of tests/penetration_scenes.py scene P at the
70 envs tests/test_penetration.py uses on the device, rounded to fp32, and on degenerate inputs.  Nothing sanitized is loaded into Python.

This is the rehearsal the defaults were chosen on (DESIGN.md 5.3 has the table): offset 4e-3 m, pen_tol 1e-7 m, pen_iters 64.  Printed per run: how many pairs
descend, mean and worst projection count, |depth - mirror| (worst, 99th and 90th percentile) and the certificate's worst residuals.

Pass = the sanitizers report nothing and every call returns; no result carries the iteration-cap or the projection-cap bit at the defaults; a pair the fp64
mirror does not send to status 2 is within tol + 2e-5 m of it (tests/test_distance_core_host.py's bound, the same core); and every overlapping pair outside the
mirror's band
  * has status 0 and dist < 0;
  * | -dist - delta(n) | <= 1e-6 m with delta evaluated in fp64 along the core's own n: the core forms delta as one fp32 dot product of support points up to
    0.5 m from geom1, a few ulp (2^-24 x 0.5 m = 3e-8 m) each; where a sphere's or capsule's core is apart from the other shape dist is GJK's upper bound,
    the query's tol (1e-6) on top;
  * geom2 moved by (depth + 2e-6) n is disjoint from geom1 on the fp64 mirror: the reported depth along n frees the pair (1e-6 of slack as in the mirror's own
    test, 1e-6 for the residual above; again tol on top where a round core was apart).
|depth - mirror| is printed, not asserted here: the device test holds it to four times what one GPU run measured."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from robosuite_amd import distance as D
from robosuite_amd import mjcf
from robosuite_amd import penetration as P
from tests import distance_scenes as S
from tests import penetration_scenes as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "san", "pen_core_driver.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
TOL, MAX_ITERS = D.DEFAULTS["tol"], D.DEFAULTS["max_iters"]
BOUND = TOL + 2e-5
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
B = 70


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pen_san") / "pen_core_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", DRIVER, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run(exe, tmp, geom_pairs, distmax, tol=TOL, max_iters=MAX_ITERS, **pen):
    o = P.options(pen)
    fin, fout = os.path.join(str(tmp), "pairs.bin"), os.path.join(str(tmp), "out.bin")
    with open(fin, "wb") as f:
        f.write(Q.pack_records(geom_pairs, distmax, tol, max_iters, o["pen_tol"], o["pen_iters"], o["offset"]))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-300:], r.stderr[-4000:])       # no sanitizer finding, no crash, every pair returned
    print("driver:", r.stdout.strip())
    with open(fout, "rb") as f:
        return Q.unpack_results(f.read(), len(geom_pairs))


@pytest.mark.parametrize("cast", ("P", "P2"))
def test_scene_p_under_sanitizers(exe, tmp_path, cast):
    flat = Q.scene_p(tmp_path, cast)
    q = Q.scene_p_qpos(flat, B, Q.SEEDS[cast])
    poses = [S.body_poses(flat, q[e]) for e in range(B)]
    ref = Q.reference(flat, S.f32(np.stack([p[0] for p in poses])), S.f32(np.stack([p[1] for p in poses])), Q.all_pairs(flat), Q.DISTMAX)
    recs = [(S.geom32(a), S.geom32(b)) for a, b in ref["recs"]]
    d, ft, nrm, st, steps = run(exe, tmp_path, recs, Q.DISTMAX)
    over, band, rd = ((ref["plain"] & D.OVERLAP) != 0).ravel(), ref["band"].ravel(), ref["dist"].ravel()
    err = np.abs(d - rd)
    held = over & ~band
    print(f"fp32 core on the host, scene {cast}: {len(recs)} pairs, {over.sum()} overlap, {band.sum()} in the band, {(steps > 0).sum()} descend; |depth - mirror| worst "
          f"{err[held].max():.3e}, 99 % {np.quantile(err[held], 0.99):.3e}, 90 % {np.quantile(err[held], 0.9):.3e}; elsewhere worst {err[~over].max():.3e}")
    assert not (st & (D.CAP | P.PEN_CAP)).any()
    assert band[over].mean() <= Q.BAND_SHARE
    assert err[~over].max() <= BOUND and (steps[~over] == 0).all()
    assert (st[held] == D.OK).all() and (d[held] < 0).all()
    worst = [0.0, 0.0]
    for i in np.flatnonzero(held):
        a, b = recs[i]
        assert abs(np.linalg.norm(nrm[i]) - 1) <= 1e-6, i
        res = Q.certificate(a, b, d[i], ft[i], nrm[i])
        worst[int(steps[i] == 0)] = max(worst[int(steps[i] == 0)], res[0])
        assert res[0] <= (1e-6 if steps[i] else TOL + 1e-6), (i, res)
        assert Q.separates(a, b, d[i], nrm[i] / np.linalg.norm(nrm[i]), slack=2e-6 + (0.0 if steps[i] else TOL)), i
    print(f"   worst | -dist - delta(n) |: {worst[0]:.3e} where the core descended, {worst[1]:.3e} where a round core was apart (GJK's tol {TOL:.0e} on top)")


def test_degenerate_inputs_terminate_and_stay_in_range(exe, tmp_path):
    """Coincident and concentric shapes, exact face and vertex contact, flat and point-sized shapes, hulls of one vertex and of repeated vertices, with the widest
    options the library accepts and with one projection: every pair returns a finite result, and an overlap comes back with a unit normal and dist = -delta(n)."""
    g = lambda t, size, pos, quat=(1, 0, 0, 0), verts=None: D.make_geom(t, np.resize(np.asarray(size, dtype=float), 3), pos, np.asarray(quat, dtype=float), verts)      # noqa: E731
    box, sph, cap, ell, cyl, msh = mjcf.GEOM_BOX, mjcf.GEOM_SPHERE, mjcf.GEOM_CAPSULE, mjcf.GEOM_ELLIPSOID, mjcf.GEOM_CYLINDER, mjcf.GEOM_MESH
    one, rep = np.array([[0.01, 0.02, 0.03]]), np.repeat(np.array(Q.WEDGE), 3, axis=0)
    recs = [(g(box, [0.1, 0.1, 0.1], [0, 0, 0]), g(box, [0.1, 0.1, 0.1], [0, 0, 0])),                         # the same box twice
            (g(box, [0.1, 0.1, 0.1], [0, 0, 0]), g(box, [0.1, 0.1, 0.1], [0.2, 0, 0])),                       # exact face contact
            (g(box, [0.1, 0.1, 0.1], [0, 0, 0]), g(box, [0.1, 0.1, 0.1], [0.2, 0.2, 0.2])),                   # exact vertex contact
            (g(ell, [0.1, 0.06, 0.04], [0, 0, 0]), g(ell, [0.1, 0.06, 0.04], [0, 0, 0])),                     # concentric ellipsoids
            (g(cyl, [0.08, 0.15], [0, 0, 0]), g(cyl, [0.08, 0.15], [0, 0, 0.29])),                            # cylinders end in end
            (g(box, [0.1, 0.1, 0.0], [0, 0, 0]), g(box, [0.0, 0.0, 0.0], [0, 0, 0.0])),                       # a point on a flat box
            (g(sph, [0.05], [0, 0, 0]), g(box, [0.1, 0.1, 0.1], [0, 0, 0])),                                   # a sphere at a box's centre
            (g(cap, [0.02, 0.3], [0, 0, 0]), g(box, [0.1, 0.1, 0.1], [0, 0, 0])),                              # a capsule through a box
            (g(msh, [0, 0, 0], [0, 0, 0], verts=one), g(box, [0.1, 0.1, 0.1], [0, 0, 0])),                     # a hull of one vertex inside a box
            (g(msh, [0, 0, 0], [0, 0, 0], verts=rep), g(msh, [0, 0, 0], [0.01, 0.01, 0.01], verts=rep))]      # repeated vertices
    for tol, iters, pen in ((0.0, D.MAX_ITERS_LIMIT, dict(pen_tol=0.0, pen_iters=P.PEN_ITERS_LIMIT)), (TOL, MAX_ITERS, {}), (TOL, MAX_ITERS, dict(pen_iters=1))):
        d, ft, nrm, st, steps = run(exe, tmp_path, recs, 1e9, tol=tol, max_iters=iters, **pen)
        assert np.isfinite(d).all() and np.isfinite(ft).all() and np.isfinite(nrm).all()
        assert ((st & ~(D.FAR | D.CAP | P.PEN_CAP)) == 0).all() and (steps <= P.options(pen)["pen_iters"]).all()
        for i, (a, b) in enumerate(recs):
            if steps[i] > 0:
                assert abs(np.linalg.norm(nrm[i]) - 1) <= 1e-5 and d[i] <= 0, (i, nrm[i], d[i])
                assert Q.certificate(a, b, d[i], ft[i], nrm[i])[0] <= 1e-6, (i, tol, iters)
