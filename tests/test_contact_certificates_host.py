"""The fp64 oracle's narrow phase (oracle/rsim_oracle.c: plane-box, plane-convex, box-box manifold, MPR) held to fp64 geometry at constructed depths: all 36 pair
classes x {1 mm deep, 0.1 mm deep, 0.1 mm apart} x 8 seeded draws (tests/contact_scenes.py: scene, samples, reference and the certificates C1 - C7).  The GPU twin
is tests/test_contact_certificates.py.  Also here: the tetrahedron whose bounding-box centre lies outside its hull (a sphere against each of its four faces, closed
form), and the interior-point check on every mesh geom of every shipped and golden model.

Allowances: four times the worst residual one run measured per certificate against the fp64 geometry (MEASURED, profiles/contact_certificates.txt), with a floor
of 1e-9 m -- ten times the tolerance the reference's GJK is iterated to.  Every geometric certificate measured rounding (<= 4e-16) or slack; the depth against the
exact one is one-sided: never less than delta* - 0.88 um (C5lo, inside MPR's 1 um portal tolerance) but up to 0.43 mm MORE at 1 mm and 32 um more at 0.1 mm (C5da /
C5db: MPR's depth is the depth along the ray from the interior point, delta* / cos of the normal's error, contact_scenes docstring), which C5hi holds exactly."""
import glob
import os

import numpy as np
import pytest

from robosuite_amd import backend, distance, mjcf
from robosuite_amd.raycast import hull_planes
from tests import contact_scenes as CS
from tests.util import make_oracle

# worst residual per certificate of one run of the oracle on these samples (metres; <= 0: slack)
MEASURED = {"C3": 2.223e-16, "C4": 3.643e-16, "C4hi": 4.250e-17, "C4n": 0.0, "C5da": 4.269e-4, "C5db": 3.090e-5, "C5lo": -1.161e-7, "C5hi": 2.290e-16, "C5n": 1.388e-17,
            "C5p": 2.220e-16, "C6": -8.079e-6}
FLOOR = 1e-9
EPS = CS.tolerances(MEASURED, FLOOR)
MAXCON = 64      # oracle/rsim_oracle.c: beyond it the oracle drops contacts


def run_oracle(od, Q):
    xp, xq, cons, ovf = [], [], [], []
    for q in Q:
        od.qpos[:] = q; od.qvel[:] = 0; od.forward()
        xp.append(od.xpos.reshape(-1, 3).copy()); xq.append(od.xquat.reshape(-1, 4).copy()); cons.append(od.contacts()); ovf.append(int(od.ncon >= MAXCON))
    return xp, xq, cons, ovf


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    flat = CS.scene(tmp_path_factory.mktemp("contact_certificates"))
    assert int(flat.nv) == 48 and int(flat.npair) == 36
    smp = CS.samples()
    Q = CS.batch_qpos(flat, smp)
    om, od, _ = make_oracle(flat)
    first = run_oracle(od, Q)
    return flat, smp, Q, od, first


def test_every_pair_class_at_constructed_depths_on_the_oracle(sweep):
    flat, smp, Q, od, (xp, xq, cons, ovf) = sweep
    assert len(smp) == 36 * 3 * CS.DRAWS
    rec = CS.evaluate(flat, smp, xp, xq, cons, ovf)
    print(CS.table(flat, rec, "oracle (fp64)"))
    CS.check(rec, EPS, "oracle")
    kinds = {r["kind"] for r in rec if r["res"]}
    assert kinds == {"plane", "plane-box", "box-box", "round", "general"}
    assert max(r["ncon"] for r in rec if r["kind"] == "box-box") >= 2 and max(r["ncon"] for r in rec if r["kind"] == "plane-box") >= 1


def test_left_out_share_of_the_samples_by_the_mirror_alone(sweep):
    """the robust-overlap filter is the mirror's own: its share is the same whatever code is under test (re-checked here for the seed in use)"""
    flat, smp, Q, od, (xp, xq, cons, ovf) = sweep
    rec = CS.evaluate(flat, smp, xp, xq, [[] for _ in smp], [0] * len(smp))
    (share, where), overall = CS.left_out_report(rec)
    print("left out: worst class x case", share, where, "overall", overall)
    assert share <= CS.LEFT_OUT_CLASS and overall <= CS.LEFT_OUT_ALL


def test_a_second_forward_returns_the_same_contacts(sweep):
    """C7"""
    flat, smp, Q, od, (xp, xq, cons, ovf) = sweep
    idx = list(range(0, len(smp), 5))
    for e in idx:
        od.qpos[:] = Q[e]; od.forward(); od.forward()
        again = od.contacts()
        assert len(again) == len(cons[e])
        for a, b in zip(again, cons[e]):
            assert (a["geom1"], a["geom2"]) == (b["geom1"], b["geom2"]) and a["dist"] == b["dist"] and np.array_equal(a["pos"], b["pos"]) and np.array_equal(a["frame"], b["frame"])


# ---- the tetrahedron -----------------------------------------------------------------------------------------------------------------------------------------
def test_sphere_against_each_face_of_a_tetrahedron(tmp_path):
    """The bounding-box centre of raycast_scenes.TETRA_VERTS lies outside the hull (beyond its slanted face).  As MPR's interior point it gave, 1 mm apart from
    that face, one contact 0.2165 m deep with the normal reversed; the compiler now takes the mean of the hull vertices for such a hull."""
    flat = CS.tet_scene(tmp_path)
    g = flat.names["geom"].index("tet")
    V = distance.mesh_verts(flat, g)
    rc, rb = np.asarray(flat.arrays["geom_rcenter"]).reshape(-1, 3)[g], float(np.asarray(flat.arrays["geom_rbound"]).ravel()[g])
    assert mjcf.hull_inside_by(V, rc) >= mjcf.RCENTER_INSIDE * rb
    assert np.allclose(rc, V.mean(axis=0), atol=1e-15) and rb == pytest.approx(np.linalg.norm(V - rc, axis=1).max(), rel=1e-14)
    om, od, _ = make_oracle(flat)
    a, b = flat.names["geom"].index("sph"), g
    for q, n, gap in CS.tet_cases(flat):
        od.qpos[:] = q; od.forward()
        G = distance.world_geoms(flat, od.xpos.reshape(-1, 3), od.xquat.reshape(-1, 4), (a, b))
        d, ft, st = distance.pair(G[a], G[b], np.inf, **CS.REF)
        if gap > 0:
            assert st == distance.OK and d == pytest.approx(gap, abs=1e-9)       # the mirror: 1 mm apart
        else:
            assert st & distance.OVERLAP
        CS.check_tet(od.contacts(), n, gap, FLOOR, (tuple(np.round(n, 3)), gap))


def test_a_hull_with_its_box_centre_inside_keeps_it(tmp_path):
    """the polyhedron's box centre is inside by more than the threshold: centre and radius stay what they were (such models compile to the same bytes)"""
    flat = CS.scene(tmp_path)
    g = flat.names["geom"].index("poly")
    V = distance.mesh_verts(flat, g)
    c = 0.5 * (V.min(axis=0) + V.max(axis=0))
    assert np.array_equal(np.asarray(flat.arrays["geom_rcenter"]).reshape(-1, 3)[g], c)
    assert float(np.asarray(flat.arrays["geom_rbound"]).ravel()[g]) == np.linalg.norm(V - c, axis=1).max()


def _models():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return sorted(glob.glob(os.path.join(root, "robosuite_amd", "assets", "*.rsim")) + glob.glob(os.path.join(root, "tests", "golden", "*.rsim")))


def test_every_shipped_and_golden_mesh_centre_is_an_interior_point():
    """geom_rcenter of every mesh geom lies inside its hull (raycast.hull_planes) by >= 2 % of geom_rbound -- and it IS the bounding-box centre: the fix leaves
    these models' bytes alone"""
    paths = _models()
    assert len(paths) >= 4
    least = {}
    for p in paths:
        flat = mjcf.load_model(p)
        gt = np.asarray(flat.arrays["geom_type"]).ravel()
        rc, rb = np.asarray(flat.arrays["geom_rcenter"], dtype=np.float64).reshape(-1, 3), np.asarray(flat.arrays["geom_rbound"], dtype=np.float64).ravel()
        planes = {}
        for g in np.flatnonzero(gt == mjcf.GEOM_MESH):
            V = distance.mesh_verts(flat, int(g))
            if V is None:
                continue
            did = int(np.asarray(flat.arrays["geom_dataid"]).ravel()[g])
            if did not in planes:
                planes[did] = hull_planes(V)
            P = planes[did]
            inside = float((P[:, 3] - P[:, :3] @ rc[g]).min())
            assert inside >= mjcf.RCENTER_INSIDE * rb[g], (p, int(g), inside, rb[g])
            assert np.allclose(rc[g], 0.5 * (V.min(axis=0) + V.max(axis=0)), rtol=0, atol=1e-12 * max(1.0, rb[g]))
            least[os.path.basename(p)] = min(least.get(os.path.basename(p), np.inf), inside / rb[g])
    print("least inside margin / rbound per model:", {k: round(v, 3) for k, v in least.items()})


def test_model_create_refuses_a_mesh_centre_outside_its_hull(tmp_path):
    """rsim_model_create, by name: a blob (from an earlier compiler, or hand-made) whose mesh geom has its centre outside the hull"""
    flat = CS.tet_scene(tmp_path)
    backend.HipModel(flat)                                       # as compiled: accepted
    bad = flat.copy()
    g = bad.names["geom"].index("tet")
    V = distance.mesh_verts(bad, g)
    rc = np.asarray(bad.arrays["geom_rcenter"], dtype=np.float64).reshape(-1, 3).copy()
    rc[g] = 0.5 * (V.min(axis=0) + V.max(axis=0))               # what the compilers wrote before
    bad.set("geom_rcenter", rc, np.float64)
    with pytest.raises(backend.RsimError, match="geom_rcenter of mesh geom .* outside its hull"):
        backend.HipModel(bad)
