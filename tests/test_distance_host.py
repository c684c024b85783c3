"""The fp64 mirror of the geom distance query (robosuite_amd/distance.py) on the CPU: against closed forms it shares nothing with, against its own certificate
(containment of the witnesses, upper bound |p2 - p1|, lower bound: the separation along their direction), the share of pairs the touching band leaves out for
the exact seeds tests/test_distance.py uses, the refusals by name, and body_distance's expansion and reduction."""
import numpy as np
import pytest

from robosuite_amd import distance, mjcf
from robosuite_amd.raycast import _rot
from tests import distance_scenes as S
from tests import raycast_scenes as R

EXACT = dict(tol=1e-12, max_iters=1000)
CLOSED_FORM_BOUND = 1e-9      # fp64 against an exact formula


def _q(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _geom(t, size, pos, quat, verts=None):
    return distance.make_geom(t, np.resize(np.asarray(size, dtype=float), 3), pos, quat, verts)


def _check(g1, g2, d_exact, what):
    for a, b in ((g1, g2), (g2, g1)):
        d, ft, st = distance.pair(a, b, distmax=np.inf, **EXACT)
        assert not st & distance.CAP, what
        assert abs(d - d_exact) <= CLOSED_FORM_BOUND, (what, d, d_exact)
        if d_exact > 0 or st == distance.OK:
            assert st == distance.OK and abs(np.linalg.norm(np.array(ft[3:]) - ft[:3]) - abs(d_exact)) <= CLOSED_FORM_BOUND, (what, st, ft)


# ---- 1. closed forms ----------------------------------------------------------------------------------------------------------------------------------------
def test_sphere_sphere_signed():
    rng = np.random.default_rng(0)
    for _ in range(20):
        c1, c2, r1, r2 = rng.uniform(-1, 1, 3), rng.uniform(-1, 1, 3), rng.uniform(0.05, 0.6), rng.uniform(0.05, 0.6)
        _check(_geom(mjcf.GEOM_SPHERE, [r1], c1, _q(rng)), _geom(mjcf.GEOM_SPHERE, [r2], c2, _q(rng)), np.linalg.norm(c2 - c1) - r1 - r2, "sphere-sphere")


@pytest.mark.parametrize("region", ("face", "edge", "vertex"))
def test_sphere_box_regions(region):
    rng = np.random.default_rng(1)
    nout = {"face": 1, "edge": 2, "vertex": 3}[region]
    for _ in range(12):
        s, r, q, c = rng.uniform(0.05, 0.3, 3), rng.uniform(0.02, 0.1), _q(rng), rng.uniform(-0.5, 0.5, 3)
        l = rng.uniform(-1, 1, 3) * s * 0.9
        for k in rng.permutation(3)[:nout]:
            l[k] = np.sign(l[k] or 1.0) * (s[k] + r + rng.uniform(0.01, 0.4))
        d_exact = np.linalg.norm(np.maximum(np.abs(l) - s, 0)) - r
        assert d_exact > 0
        _check(_geom(mjcf.GEOM_BOX, s, c, q), _geom(mjcf.GEOM_SPHERE, [r], c + _rot(q) @ l, _q(rng)), d_exact, region)


def test_capsules_parallel_and_skew():
    rng = np.random.default_rng(2)
    for _ in range(12):
        q, c, r1, r2, h1, h2 = _q(rng), rng.uniform(-0.3, 0.3, 3), rng.uniform(0.02, 0.1), rng.uniform(0.02, 0.1), rng.uniform(0.1, 0.3), rng.uniform(0.1, 0.3)
        M = _rot(q)
        # parallel: axes side by side, the axial ranges overlap -- the distance is the lateral offset (signed when the capsules overlap)
        lat, ax = rng.uniform(0.01, 0.5), rng.uniform(-0.5, 0.5) * (h1 + h2)
        _check(_geom(mjcf.GEOM_CAPSULE, [r1, h1], c, q), _geom(mjcf.GEOM_CAPSULE, [r2, h2], c + M @ np.array([lat, 0, ax]), q), lat - r1 - r2, "parallel capsules")
        # skew: the second axis along the first one's local X, its midpoint over the first axis' interior, `lat` away along local Y: the common perpendicular
        # meets both segments inside
        q2 = mjcf.mat2quat(M @ np.array([[0, 0, 1.0], [0, 1, 0], [-1, 0, 0]]))        # local Z -> the first capsule's X
        off = np.array([rng.uniform(-0.5, 0.5) * h2, lat, rng.uniform(-0.5, 0.5) * h1])
        _check(_geom(mjcf.GEOM_CAPSULE, [r1, h1], c, q), _geom(mjcf.GEOM_CAPSULE, [r2, h2], c + M @ off, q2), lat - r1 - r2, "skew capsules")


@pytest.mark.parametrize("region", ("face", "edge", "vertex"))
def test_axis_aligned_boxes(region):
    rng = np.random.default_rng(3)
    nout = {"face": 1, "edge": 2, "vertex": 3}[region]
    for _ in range(12):
        s1, s2, c1 = rng.uniform(0.05, 0.3, 3), rng.uniform(0.05, 0.3, 3), rng.uniform(-0.5, 0.5, 3)
        off = rng.uniform(-1, 1, 3) * (s1 + s2) * 0.8
        for k in rng.permutation(3)[:nout]:
            off[k] = np.sign(off[k] or 1.0) * (s1[k] + s2[k] + rng.uniform(0.01, 0.4))
        _check(_geom(mjcf.GEOM_BOX, s1, c1, [1, 0, 0, 0]), _geom(mjcf.GEOM_BOX, s2, c1 + off, [1, 0, 0, 0]), np.linalg.norm(np.maximum(np.abs(off) - s1 - s2, 0)), region)


def _h_closed(t, s, n, verts):
    """support function value of the solid in its own frame, closed form per type"""
    if t == mjcf.GEOM_SPHERE:
        return s[0]
    if t == mjcf.GEOM_CAPSULE:
        return s[0] + s[1] * abs(n[2])
    if t == mjcf.GEOM_ELLIPSOID:
        return np.sqrt(((s * n) ** 2).sum())
    if t == mjcf.GEOM_CYLINDER:
        return s[0] * np.hypot(n[0], n[1]) + s[1] * abs(n[2])
    if t == mjcf.GEOM_BOX:
        return (s * np.abs(n)).sum()
    return (verts @ n).max()


@pytest.mark.parametrize("t", (mjcf.GEOM_SPHERE, mjcf.GEOM_CAPSULE, mjcf.GEOM_ELLIPSOID, mjcf.GEOM_CYLINDER, mjcf.GEOM_BOX, mjcf.GEOM_MESH))
def test_every_shape_against_a_tilted_plane(t):
    rng = np.random.default_rng(4)
    verts = np.array(R.POLY_VERTS) if t == mjcf.GEOM_MESH else None
    for i in range(16):
        qp, p0, q, s = _q(rng), rng.uniform(-0.3, 0.3, 3), _q(rng), rng.uniform(0.04, 0.3, 3)
        n = _rot(qp)[:, 2]
        h = _h_closed(t, s, _rot(q).T @ (-n), verts)
        c = p0 + n * (h + rng.uniform(-0.03, 0.3)) + np.cross(n, rng.normal(size=3))      # some of them dip into the half-space: signed
        d_exact = float(n @ (c - p0) - h)
        g, pl = _geom(t, s, c, q, verts), _geom(mjcf.GEOM_PLANE, [0, 0, 0.1], p0, qp)
        for a, b in ((pl, g), (g, pl)):
            d, ft, st = distance.pair(a, b, distmax=np.inf, **EXACT)
            assert st == distance.OK and abs(d - d_exact) <= CLOSED_FORM_BOUND, (t, d, d_exact)
            on_plane, on_geom = (ft[:3], ft[3:]) if a is pl else (ft[3:], ft[:3])        # always oriented geom1 -> geom2
            assert abs(n @ (np.array(on_plane) - p0)) <= CLOSED_FORM_BOUND and abs(n @ (np.array(on_geom) - p0) - d_exact) <= CLOSED_FORM_BOUND
            assert S.outside_by(g, on_geom) <= CLOSED_FORM_BOUND


def test_cylinder_resting_flat_on_the_plane_and_beyond_distmax():
    pl = _geom(mjcf.GEOM_PLANE, [0, 0, 0.1], [0, 0, 0], [1, 0, 0, 0])
    cyl = _geom(mjcf.GEOM_CYLINDER, [0.08, 0.15], [0.3, 0.2, 0.15 + 0.02], [1, 0, 0, 0])
    d, ft, st = distance.pair(pl, cyl, distmax=1.0)
    assert st == distance.OK and abs(d - 0.02) < 1e-12 and abs(ft[5] - 0.02) < 1e-12 and abs(ft[2]) < 1e-12
    assert distance.pair(pl, cyl, distmax=0.01) == (0.01, (0.0,) * 6, distance.FAR)
    b1, b2 = _geom(mjcf.GEOM_BOX, [0.1, 0.1, 0.1], [0, 0, 0], [1, 0, 0, 0]), _geom(mjcf.GEOM_BOX, [0.1, 0.1, 0.1], [0.5, 0, 0], [1, 0, 0, 0])
    assert distance.pair(b1, b2, distmax=0.2)[::2] == (0.2, distance.FAR) and abs(distance.pair(b1, b2, distmax=0.4)[0] - 0.3) < 1e-12
    assert distance.pair(b1, _geom(mjcf.GEOM_BOX, [0.1, 0.1, 0.1], [0.15, 0, 0], [1, 0, 0, 0]))[::2] == (0.0, distance.OVERLAP)
    e1, e2 = _geom(mjcf.GEOM_ELLIPSOID, [0.1, 0.06, 0.04], [0, 0, 0], [1, 0.2, 0.3, 0.1]), _geom(mjcf.GEOM_ELLIPSOID, [0.1, 0.06, 0.04], [0.3, 0.1, 0.2], [1, -0.4, 0.1, 0.5])
    d_ref = distance.pair(e1, e2, **S.REF)[0]
    d, ft, st = distance.pair(e1, e2, distmax=1.0, tol=0.0, max_iters=1)       # one iteration cannot bring the bounds together: the best iterate, an upper bound
    assert st == distance.CAP and d > d_ref + 1e-6 and S.outside_by(e1, ft[:3]) < 1e-12 and S.outside_by(e2, ft[3:]) < 1e-12


# ---- scenes (shared with the GPU test: same seeds, same sizes) -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_a(tmp_path_factory):
    flat = S.scene_a(tmp_path_factory.mktemp("dist_a"))
    q = S.scene_a_qpos(flat, 130)
    poses = [S.body_poses(flat, q[e]) for e in range(130)]
    return flat, S.all_pairs(flat), S.f32(np.stack([p[0] for p in poses])), S.f32(np.stack([p[1] for p in poses]))


@pytest.fixture(scope="module")
def scene_h(tmp_path_factory):
    flat = S.scene_h(tmp_path_factory.mktemp("dist_h"))
    q = S.scene_h_qpos(flat, 130)
    poses = [S.body_poses(flat, q[e]) for e in range(130)]
    return flat, S.all_pairs(flat), S.f32(np.stack([p[0] for p in poses])), S.f32(np.stack([p[1] for p in poses]))


def test_scene_h_hulls_have_the_vertex_counts_the_scene_is_about(scene_h):
    assert sorted(int(n) for n in np.asarray(scene_h[0].arrays["mesh_vertnum"]).ravel()) == [4, S.N_BIG] and S.N_BIG > 256


# ---- 2. the certificate ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tol", (1e-6, 1e-10))
def test_mirror_certificate_scene_a_and_h(scene_a, scene_h, tol):
    n = 0
    for flat, pairs, xp, xq in (scene_a, scene_h):
        for e in range(12):
            G = distance.world_geoms(flat, xp[e], xq[e], pairs.ravel())
            for a, b in pairs:
                d, ft, st = distance.pair(G[int(a)], G[int(b)], distmax=np.inf, tol=tol, max_iters=1000)
                assert not st & distance.CAP
                if st != distance.OK or d <= 0:
                    continue
                o1, o2, up, low = S.certificate(G[int(a)], G[int(b)], ft)
                assert o1 <= 1e-9 and o2 <= 1e-9, (a, b, o1, o2)                  # containment
                assert abs(up - d) <= 1e-12 and low <= up + 1e-12                   # the upper bound is the reported distance
                assert up - low <= tol + 1e-12, (a, b, up - low)                    # the true distance lies between: the gap is the tol passed in
                n += 1
    assert n > 300


# ---- 3. continuity of the status codes: the share the touching band leaves out, for the GPU test's seeds ------------------------------------------------
def test_band_share_scene_a_and_h(scene_a, scene_h):
    for name, (flat, pairs, xp, xq), need in (("A", scene_a, True), ("H", scene_h, False)):
        ref = S.reference(flat, xp, xq, pairs, S.DISTMAX if need else S.DISTMAX_H, S.params32(flat))
        share = ref["band"].mean()
        print(f"scene {name}: {ref['band'].sum()} of {ref['band'].size} pairs in the band ({share:.3%})")
        assert share <= S.BAND_SHARE
        st = ref["status"]
        assert (st == distance.OK).any() and (st == distance.FAR).any() and (st == distance.OVERLAP).any() and not (st & distance.CAP).any()
        if need:      # every env holds separated, touching-band and overlapping pairs; a signed overlap is among them
            sep = ((st == distance.OK) & (ref["d"] > S.BAND)).any(axis=1)
            assert sep.all() and ref["band"].any(axis=1).all() and ((st == distance.OVERLAP) | (ref["d"] < -S.BAND)).any(axis=1).all()
            assert (ref["d"] < -S.BAND).any()
            names = flat.names["geom"]
            k = [i for i, (a, b) in enumerate(pairs) if {names[a], names[b]} == {"box", "box2"}][0]
            assert np.allclose(ref["d"][0::3, k], S.GAPS[0], atol=1e-6) and np.allclose(ref["d"][1::3, k], S.GAPS[1], atol=1e-6) and (st[2::3, k] == distance.OVERLAP).all()
            k = [i for i, (a, b) in enumerate(pairs) if {names[a], names[b]} == {"floor", "cyl2"}][0]
            assert np.allclose(ref["d"][:, k], np.array(S.GAPS)[[1, 2, 1]][np.arange(130) % 3], atol=1e-6)      # the cylinder's flat end over the floor


def test_band_share_scene_l_reset_pose():
    flat, cfg = R.lift()
    xp, xq = S.body_poses(flat, R.lift_init_qpos(flat, cfg))
    pairs = distance.body_pairs(flat, *S.lift_bodies(flat))
    ref = S.reference(flat, S.f32(xp)[None], S.f32(xq)[None], pairs, S.DISTMAX_L, S.params32(flat))
    assert ref["band"].mean() <= S.BAND_SHARE and not (ref["status"] & distance.CAP).any()


def test_distmax_clamps_what_the_unbounded_query_reports(scene_a):
    flat, pairs, xp, xq = scene_a
    d_inf, ft_inf, st_inf = distance.geom_distance(flat, xp[1], xq[1], pairs, distmax=np.inf, **S.REF)
    d, ft, st = distance.geom_distance(flat, xp[1], xq[1], pairs, distmax=S.DISTMAX, **S.REF)
    far = d_inf > S.DISTMAX
    assert far.any() and (~far).any()
    assert (d[far] == S.DISTMAX).all() and (ft[far] == 0).all() and (st[far] == distance.FAR).all()
    assert np.allclose(d[~far], d_inf[~far], atol=1e-9) and (st[~far] == st_inf[~far]).all()


# ---- 4. refusals by name; body_distance's expansion and reduction ---------------------------------------------------------------------------------------
def test_refusals_by_name(scene_a):
    flat = scene_a[0]
    lift, _ = R.lift()
    for model, pairs, word in ((flat, [[0, 99]], "out of range"), (flat, [[-1, 2]], "out of range"), (flat, [[3, 3]], "against itself"), (flat, np.zeros((0, 2)), "npair < 1"),
                               (lift, [[lift.names["geom"].index("robot0_g0_vis"), 7]], "visual-only mesh")):
        with pytest.raises(distance.DistanceError, match=word):
            distance.check_pairs(model, pairs)
    two = mjcf.compile_mjcf('<mujoco><worldbody><geom type="plane" size="1 1 .1"/><geom type="plane" size="1 1 .1" pos="0 0 1"/></worldbody></mujoco>')
    with pytest.raises(distance.DistanceError, match="plane against plane"):
        distance.check_pairs(two, [[0, 1]])
    with pytest.raises(distance.DistanceError, match="max_iters"):
        distance.options(max_iters=0)
    with pytest.raises(distance.DistanceError, match="max_iters"):
        distance.options(max_iters=distance.MAX_ITERS_LIMIT + 1)


def test_body_pairs_expansion_and_reduction():
    flat, cfg = R.lift()
    A, Bs = S.lift_bodies(flat)
    pairs = distance.body_pairs(flat, A, Bs)
    gb, gt, gd = (np.asarray(flat.arrays[k]).ravel() for k in ("geom_bodyid", "geom_type", "geom_dataid"))
    ga = [g for g in range(len(gb)) if gb[g] in A and not (gt[g] == mjcf.GEOM_MESH and gd[g] < 0)]
    gbs = [g for g in range(len(gb)) if gb[g] in Bs]
    assert len(ga) == 8 and len(gbs) == 8 and [tuple(p) for p in pairs] == [(a, b) for a in ga for b in gbs]       # visual-only meshes are skipped, nothing else
    assert not any(gt[g] == mjcf.GEOM_MESH and gd[g] < 0 for g in pairs.ravel())
    distance.check_pairs(flat, pairs)
    with pytest.raises(distance.DistanceError, match="no geom pair"):
        distance.body_pairs(flat, [flat.names["body"].index("robot0_base")], Bs)             # a body without geoms
    xp, xq = S.body_poses(flat, R.lift_init_qpos(flat, cfg))
    d, ft, st = distance.geom_distance(flat, xp, xq, pairs, distmax=S.DISTMAX_L)
    dm, fm, k = distance.reduce_min(d[None], ft[None])
    assert dm[0] == d.min() and k[0] == int(np.argmin(d)) and (fm[0] == ft[k[0]]).all()
    names = flat.names["geom"]
    assert 0.0 < dm[0] < 0.3 and ("cube" in names[pairs[k[0]][1]] or "table" in names[pairs[k[0]][1]])      # the open gripper hovers over the cube
