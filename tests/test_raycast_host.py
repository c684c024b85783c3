"""Ray casting, the parts that need no GPU: the fp64 host mirror (robosuite_amd/raycast.py) -- the reference of the GPU tests in tests/test_raycast.py -- is
held to closed forms for every geom type, filter and rule; the library's hull planes to scipy's; both MJCF compilers agree on a model with a rangefinder; no
shipped blob changes; and the share of ill-conditioned rays the GPU tests leave out stays under its cap.

MuJoCo semantics [3P, docs "API reference: ray collisions", "XML reference: sensor/rangefinder"]."""
import ctypes as C
import os

import numpy as np
import pytest

from robosuite_amd import backend, mjcf, raycast, sensors
from robosuite_amd.raycast import Camera
from tests import raycast_scenes as S
from tests.test_mjcf_cpp import compare

ASSETS = S.ASSETS


def _one(xml_geoms, extra=""):
    """a model with the given world geoms (+ bodies); -> (flat, xpos, xquat) at the model's own pose"""
    flat = mjcf.compile_mjcf(f'<mujoco><compiler angle="radian"/><worldbody>{xml_geoms}</worldbody>{extra}</mujoco>')
    fr = sensors.body_frames(flat, flat.arrays["qpos0"], np.zeros(int(flat.nv)), np.zeros(int(flat.nv)))
    return flat, np.array([f.p for f in fr]), np.array([f.q for f in fr])


def _cast(flat, xp, xq, o, d, **kw):
    t, g = raycast.cast(flat, xp, xq, np.atleast_2d(np.asarray(o, dtype=float)), np.atleast_2d(np.asarray(d, dtype=float)), **kw)
    return t, g


# ---- closed forms, one geom type at a time -----------------------------------------------------------------------------------------------------------
def test_plane_straight_down_and_one_sided():
    flat, xp, xq = _one('<geom type="plane" size="0 0 0.1" pos="0 0 0.25"/>')
    t, g = _cast(flat, xp, xq, [[0.3, -0.2, 1.0], [0.3, -0.2, 1.0], [0, 0, 0.1], [0, 0, 0.1], [0, 0, 1.0]],
                 [[0, 0, -1], [0, 0, -2], [0, 0, 1], [0, 0, -1], [1, 0, 0]])
    assert np.allclose(t[:2], [0.75, 0.375], atol=1e-14) and list(g[:2]) == [0, 0]        # t is in units of |dir|
    assert list(t[2:]) == [-1, -1, -1] and list(g[2:]) == [-1, -1, -1]                    # from below (either way) and parallel: no hit


def test_finite_plane_edge():
    flat, xp, xq = _one('<geom type="plane" size="0.5 0.2 0.1"/>')
    t, g = _cast(flat, xp, xq, [[0.49, 0.19, 1], [0.51, 0, 1], [0, 0.21, 1], [-0.5, -0.2, 1]], [[0, 0, -1]] * 4)
    assert list(g) == [0, -1, -1, 0] and np.allclose(t[[0, 3]], 1.0)


def test_sphere_through_the_centre_and_inside_start():
    flat, xp, xq = _one('<geom type="sphere" size="0.2" pos="1 2 3"/>')
    t, g = _cast(flat, xp, xq, [[1, 2, 5], [1, 2, 3], [1, 2, 3.1], [1.3, 2, 5]], [[0, 0, -1], [0.6, 0, 0.8], [0, 0, -4], [0, 0, -1]])
    assert np.allclose(t[:3], [1.8, 0.2, 0.3 / 4], atol=1e-14) and list(g) == [0, 0, 0, -1]   # an inside start reports where the ray leaves
    t, _ = _cast(flat, xp, xq, [[1.2 - 1e-9, 2, 5]], [[0, 0, -1]])                            # just inside the silhouette: near the equator
    assert abs(t[0] - 2.0) < 1e-4


def test_box_face_corner_and_parallel():
    flat, xp, xq = _one('<geom type="box" size="0.1 0.2 0.3" pos="0 0 1"/>')
    c = np.array([0.1, 0.2, 1.3])
    d = -np.array([1.0, 1.0, 1.0])
    t, g = _cast(flat, xp, xq, [[0.05, -0.1, 3], c - 0.999 * d - [1e-6, 2e-6, 0], [0.05, 0.1, 1.0], [0.0999, 0, 3], [0.1001, 0, 3]],
                 [[0, 0, -1], d, [0, 1, 0], [0, 0, -1], [0, 0, -1]])
    assert abs(t[0] - 1.7) < 1e-14                      # top face
    assert abs(t[1] - 0.999) < 1e-5                     # into the corner, just inside it
    assert abs(t[2] - 0.1) < 1e-14                      # from inside: the +Y face
    assert list(g) == [0, 0, 0, 0, -1]                  # parallel to four faces: inside the cross-section hits, outside misses


def test_cylinder_along_and_across():
    flat, xp, xq = _one('<geom type="cylinder" size="0.1 0.3" pos="0 0 1" euler="0 1.5707963267948966 0"/>')      # axis along world X
    t, g = _cast(flat, xp, xq, [[2, 0.05, 1], [0, 0, 3], [0, 0.06, 3], [2, 0.11, 1], [0.31, 0, 3], [0, 0, 1]],
                 [[-1, 0, 0], [0, 0, -1], [0, 0, -1], [-1, 0, 0], [0, 0, -1], [1, 0, 0]])
    assert np.allclose(t[:3], [1.7, 1.9, 2 - 0.08], atol=1e-12)     # cap (parallel to the axis) | side through the axis | side off the axis: sqrt(.01 - .0036) = .08
    assert abs(t[5] - 0.3) < 1e-12                                  # from the centre along the axis: out through the cap
    assert list(g) == [0, 0, 0, -1, -1, 0]


def test_capsule_along_and_across():
    flat, xp, xq = _one('<geom type="capsule" size="0.1 0.3" pos="0 0 1"/>')                                      # axis along world Z
    t, g = _cast(flat, xp, xq, [[0, 0, 3], [0.06, 0, 3], [2, 0, 1.2], [2, 0, 1.36], [2, 0, 1.41], [0, 0, 1]],
                 [[0, 0, -1], [0, 0, -1], [-1, 0, 0], [-1, 0, 0], [-1, 0, 0], [0, 0, 1]])
    assert np.allclose(t[:4], [2 - 0.4, 2 - 0.3 - 0.08, 1.9, 2 - 0.08], atol=1e-12)     # end sphere on the axis | off it | side | end sphere from the side
    assert g[4] == -1 and abs(t[5] - 0.4) < 1e-12


def test_rotated_ellipsoid():
    q = mjcf.axisangle2quat(np.array([0.0, 0, 1]), np.pi / 2)       # local X (semi-axis 0.3) -> world Y
    flat, xp, xq = _one(f'<geom type="ellipsoid" size="0.3 0.1 0.05" pos="0 0 1" quat="{q[0]} {q[1]} {q[2]} {q[3]}"/>')
    t, g = _cast(flat, xp, xq, [[0, 2, 1], [2, 0, 1], [0, 0, 3], [0, 0.15, 3]], [[0, -1, 0], [-1, 0, 0], [0, 0, -1], [0, 0, -1]])
    assert np.allclose(t, [1.7, 1.9, 1.95, 2 - 0.05 * np.sqrt(0.75)], atol=1e-12) and list(g) == [0] * 4


def test_tetrahedron_hull(tmp_path):
    S.write_obj(str(tmp_path / "t.obj"), S.TETRA_VERTS)
    flat = mjcf.compile_mjcf('<mujoco><asset><mesh name="t" file="t.obj"/></asset><worldbody><body pos="0 0 1"><geom type="mesh" mesh="t"/></body></worldbody></mujoco>',
                             asset_dir=str(tmp_path))
    xp, xq = np.array([[0, 0, 0], [0, 0, 1.0]]), np.array([[1.0, 0, 0, 0]] * 2)
    gp = np.asarray(flat.arrays["geom_pos"], dtype=float).reshape(-1, 3)[0]      # the compiler re-centres mesh geoms: the hull sits at body + gp
    gq = np.asarray(flat.arrays["geom_quat"], dtype=float).reshape(-1, 4)[0]
    R = raycast._rot(gq)
    base = np.array([0, 0, 1.0]) + gp
    V = np.asarray(flat.arrays["mesh_vert"], dtype=float).reshape(-1, 3) @ R.T + base        # world vertices: the tetrahedron, wherever the compiler put its frame
    lo = V.min(axis=0)
    assert np.allclose(sorted(V.max(axis=0) - lo), [0.2, 0.2, 0.2], atol=1e-12)
    # straight down onto the slanted face x + y + z = 0.2 (in the tetrahedron's own corner frame) above (0.05, 0.05): z = 0.1; from below: the bottom face
    t, g = _cast(flat, xp, xq, [lo + [0.05, 0.05, 1.0], lo + [0.05, 0.05, -1.0], lo + [0.15, 0.15, 1.0], lo + [0.02, 0.02, 0.02]], [[0, 0, -1], [0, 0, 1], [0, 0, -1], [0, 0, 1]])
    assert np.allclose(t[[0, 1, 3]], [0.9, 1.0, 0.14], atol=1e-12) and list(g) == [0, 0, -1, 0]
    assert len(raycast.hull_planes(S.TETRA_VERTS)) == 4


# ---- filters, ties --------------------------------------------------------------------------------------------------------------------------------
FILTER_XML = ('<geom name="floor" type="plane" size="0 0 0.1"/><geom name="lid" type="box" size="1 1 0.01" pos="0 0 0.5" group="1"/>'
              '<geom name="glass" type="box" size="1 1 0.01" pos="0 0 0.8" rgba="1 1 1 0"/>'
              '<body name="b" pos="0 0 1.5"><joint type="hinge" axis="0 1 0"/><geom name="ball" type="sphere" size="0.1" group="2"/></body>')


def test_every_filter():
    flat, xp, xq = _one(FILTER_XML)
    gid = {n: i for i, n in enumerate(flat.names["geom"])}
    o, d = [[0, 0, 3.0]], [[0, 0, -1.0]]
    assert _cast(flat, xp, xq, o, d)[1][0] == gid["ball"]                                  # everything on: the ball is nearest
    assert _cast(flat, xp, xq, o, d, bodyexclude=1)[1][0] == gid["lid"]                    # ... without its body: the lid (alpha 0 glass never counts)
    assert _cast(flat, xp, xq, o, d, bodyexclude=1, geomgroup=0b001)[1][0] == gid["floor"]  # groups: only group 0
    assert _cast(flat, xp, xq, o, d, geomgroup=0b010)[1][0] == gid["lid"]
    assert _cast(flat, xp, xq, o, d, geomgroup=0b100, static=False)[1][0] == gid["ball"]
    t, g = _cast(flat, xp, xq, o, d, bodyexclude=1, static=False)                          # nothing left: the miss value
    assert (t[0], g[0]) == (-1.0, -1)
    t, g = _cast(flat, xp, xq, [[0, 0, 3.0]] * 2, [[0, 0, -1.0]] * 2, bodyexclude=np.array([1, -1]))     # a body to exclude per ray
    assert list(g) == [gid["lid"], gid["ball"]]


def test_ties_go_to_the_lower_geom_id():
    flat, xp, xq = _one('<geom name="a" type="box" size="0.5 0.5 0.25" pos="0 0 0.25"/><geom name="b" type="box" size="0.25 0.25 0.125" pos="0 0 0.375"/>'
                        '<geom name="c" type="plane" size="0 0 1" pos="0 0 0.5"/>')
    t, g = _cast(flat, xp, xq, [[0.1, 0.1, 2]], [[0, 0, -1]])          # three surfaces at z = 0.5 exactly (binary fractions)
    assert t[0] == 1.5 and g[0] == 0


# ---- cameras ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W,fovy", [(4, 4, 90.0), (5, 7, 45.0), (24, 32, 60.0)])
def test_pixel_ray_formula(H, W, fovy):
    cam = Camera(0, (0.1, 0.2, 2.0), (1.0, 0, 0, 0), fovy)             # identity orientation: looks down -Z with +Y up
    o, d = raycast.pixel_rays(cam, np.zeros((1, 3)), np.array([[1.0, 0, 0, 0]]), H, W)
    assert o.shape == d.shape == (H * W, 3) and np.allclose(o, [0.1, 0.2, 2.0]) and np.allclose(d[:, 2], -1)
    d = d.reshape(H, W, 3)
    th = np.tan(np.deg2rad(fovy) / 2)
    assert np.isclose(d[0, 0, 1], th * (1 - 1 / H)) and np.isclose(d[-1, 0, 1], -th * (1 - 1 / H))       # row 0 is the top row
    assert np.isclose(d[0, 0, 0], -(W / H) * th * (1 - 1 / W)) and np.isclose(d[0, -1, 0], (W / H) * th * (1 - 1 / W))
    # depth along the optical axis: a floor 2 m below the camera reads 2 in EVERY pixel, however oblique the ray
    flat, xp, xq = _one('<geom type="plane" size="0 0 0.1"/>')
    depth, seg = raycast.render_depth(flat, xp, xq, cam, H, W)
    assert np.allclose(depth, 2.0, atol=1e-12) and (seg == 0).all()
    up = Camera(0, (0, 0, 2.0), tuple(mjcf.axisangle2quat(np.array([1.0, 0, 0]), np.pi)), fovy)          # looking up: nothing there
    depth, seg = raycast.render_depth(flat, xp, xq, up, H, W)
    assert np.isinf(depth).all() and (seg == -1).all()


def test_cameras_from_xml_and_refused_modes():
    xml = ('<mujoco><compiler angle="degree"/><worldbody><camera name="top" pos="0 0 3" fovy="60"/><body name="a" pos="0 0 1"><joint type="hinge"/><geom size="0.1"/>'
           '<camera name="eye" pos="0.1 0 0" euler="0 90 0"/><body name="b" pos="0 0 1"><joint type="hinge"/><geom size="0.1"/><camera name="wrist" pos="0 0.1 0" xyaxes="0 1 0 0 0 1"/></body></body>'
           '</worldbody></mujoco>')
    flat = mjcf.compile_mjcf(xml)
    cams = raycast.cameras_from_xml(xml, flat)
    assert list(cams) == flat.names["camera"] == ["top", "eye", "wrist"]
    assert (cams["top"].body, cams["eye"].body, cams["wrist"].body) == (0, 1, 2) and cams["top"].fovy == 60.0 and cams["eye"].fovy == 45.0
    assert np.allclose(raycast._rot(cams["eye"].quat) @ [0, 0, -1], [-1, 0, 0], atol=1e-12)             # euler 0 90 0: the view direction -Z turns to -X
    assert np.allclose(raycast._rot(cams["wrist"].quat), [[0, 0, 1], [1, 0, 0], [0, 1, 0]], atol=1e-12)
    with pytest.raises(NotImplementedError, match="trackcom"):
        raycast.cameras_from_xml(xml.replace('name="eye"', 'name="eye" mode="trackcom"'), flat)


# ---- hull planes: the library's quickhull against scipy's qhull ------------------------------------------------------------------------------------
def _lib_planes(V):
    L = backend.lib()
    L.rsim_hull_planes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    V = np.ascontiguousarray(V, dtype=np.float64)
    n = L.rsim_hull_planes(V.ctypes.data, len(V), None, 0)
    assert n >= 4, L.rsim_last_error()
    P = np.zeros((n, 4))
    assert L.rsim_hull_planes(V.ctypes.data, len(V), P.ctypes.data, n) == n
    return P


def _same_plane_set(P, Q, tol):
    """every plane of each set has a partner in the other: same unit normal and offset to tol"""
    if len(P) != len(Q):
        return False
    for A, B in ((P, Q), (Q, P)):
        for p in A:
            if np.abs(B - p).max(axis=1).min() > tol:
                return False
    return True


def test_hull_planes_merge_coplanar_triangles():
    P = _lib_planes(S.POLY_VERTS)
    assert len(P) == 13 and _same_plane_set(P, raycast.hull_planes(S.POLY_VERTS), 1e-12)      # the bottom quad + 8 side + 4 top triangles, not 2 V - 4 = 14 triangles
    cube = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=float) * [0.1, 0.2, 0.3]
    P = _lib_planes(cube)
    assert len(P) == 6 and sorted(np.round(P[:, 3], 12)) == [0.1, 0.1, 0.2, 0.2, 0.3, 0.3]
    assert backend.lib().rsim_hull_planes(cube.ctypes.data, 3, None, 0) == -1 and b"fewer than 4" in backend.lib().rsim_last_error()


def test_hull_planes_of_the_lift_asset_equal_scipys():
    flat, _ = S.lift()
    mv = np.asarray(flat.arrays["mesh_vert"], dtype=np.float64).reshape(-1, 3)
    adr, num = np.asarray(flat.arrays["mesh_vertadr"]).ravel(), np.asarray(flat.arrays["mesh_vertnum"]).ravel()
    assert len(adr) == 10
    for a, n in zip(adr, num):
        V = mv[a:a + n]
        P, Q = _lib_planes(V), raycast.hull_planes(V)
        assert (np.abs(np.linalg.norm(P[:, :3], axis=1) - 1) < 1e-12).all()
        assert (V @ P[:, :3].T - P[:, 3] < 1e-9).all()                  # every vertex inside every plane
        assert _same_plane_set(P, Q, 1e-7 * max(1.0, np.abs(V).max())), (n, len(P), len(Q))


# ---- rangefinder: compilers, status, mirror -----------------------------------------------------------------------------------------------------------
RF_XML = """<mujoco><compiler angle="radian"/><worldbody><geom name="floor" type="plane" size="0 0 0.1"/>
    <body name="a" pos="0 0 1"><joint name="h" type="hinge" axis="0 1 0"/><geom name="ga" type="capsule" size="0.03 0.2" pos="0 0 -0.2"/>
      <site name="down" pos="0 0 -0.1" euler="3.141592653589793 0 0"/><site name="side" pos="0 0 -0.2" euler="0 1.5707963267948966 0"/></body>
    <body name="w" pos="2 0 1"><geom name="wall" type="box" size="0.1 1 1"/></body></worldbody>
  <sensor><rangefinder name="r_down" site="down"/><jointpos name="jp" joint="h"/><rangefinder name="r_side" site="side"/>
    <rangefinder name="r_cut" site="down" cutoff="2"/><rangefinder name="r_lost" site="nowhere"/></sensor></mujoco>"""


def test_rangefinder_compiles_the_same_in_both_compilers_and_reports_clean():
    ref, new, _ = compare(RF_XML)                                       # every array of the two blobs equal, same entry table
    assert list(ref.sensor_type) == [15, 2, 15, 15, 15] and list(ref.sensor_dim) == [1] * 5
    assert list(ref.sensor_objtype) == [mjcf.SENSOR_OBJ_SITE, mjcf.SENSOR_OBJ_JOINT] + [mjcf.SENSOR_OBJ_SITE] * 3 and list(ref.sensor_reason) == [0, 0, 0, 6, 7]
    assert backend.compile_mjcf_blob(RF_XML) == mjcf.to_blob(mjcf.compile_mjcf(RF_XML))
    hm = backend.HipModel.from_xml_string(RF_XML)
    st = hm.sensor_status()
    assert [(n, t, c) for n, t, c, _ in st] == [("r_down", "rangefinder", True), ("jp", "jointpos", True), ("r_side", "rangefinder", True),
                                                ("r_cut", "rangefinder", False), ("r_lost", "rangefinder", False)]
    assert [r for *_, r in st] == ["", "", "", "non-zero cutoff not carried", "object not found"] and hm.int("nsensor_zero") == 2
    clean = backend.HipModel.from_xml_string(RF_XML.replace('<rangefinder name="r_cut" site="down" cutoff="2"/><rangefinder name="r_lost" site="nowhere"/>', ""))
    assert clean.int("nsensor_zero") == 0 and all(c for _, _, c, _ in clean.sensor_status())
    assert "rangefinder" not in mjcf.SENSOR_TYPES and mjcf.SENSOR_TYPE_NAMES[15] == "rangefinder"      # (SENSOR_TYPES stays the table of rsim_sensors.hip)


def test_rangefinder_mirror_closed_forms():
    flat = mjcf.compile_mjcf(RF_XML)
    for ang in (0.0, 0.4, -0.3):
        row = sensors.sensor_values(flat, [ang], [0.0], [0.0], [])
        # `down`: 0.1 below the hinge along the link, looking along the link: the floor is hit at (1 - 0.1 cos) / cos ... its own capsule is excluded
        assert abs(row[0] - (1.0 / np.cos(ang) - 0.1)) < 1e-12
        assert row[1] == ang
        # `side`: looks along the link's +X (turned by the hinge about Y): the wall face x = 1.9, unless the ray tilts into the floor first
        o = np.array([-0.2 * np.sin(ang), 0, 1 - 0.2 * np.cos(ang)])
        dx, dz = np.cos(ang), -np.sin(ang)
        want = min((1.9 - o[0]) / dx, o[2] / -dz if dz < 0 else np.inf)
        assert abs(row[2] - want) < 1e-12
        assert row[3] == 0.0 and row[4] == 0.0                         # not carried: zero
    lonely = mjcf.compile_mjcf('<mujoco><worldbody><body pos="0 0 1"><joint type="hinge"/><geom size="0.1"/><site name="s"/></body></worldbody>'
                               '<sensor><rangefinder site="s"/></sensor></mujoco>')
    assert sensors.sensor_values(lonely, [0.0], [0.0], [0.0], [])[0] == -1.0       # nothing but its own body above: -1


# ---- blobs -------------------------------------------------------------------------------------------------------------------------------------------
SHIPPED_SHA256 = {
    "lift_panda.rsim": "5d908f8e25c80c2c86e44ec9315c553a50bfc50419113412af692ece4b423a8a",
    "peg_baxter_joint_velocity.rsim": "f43f3fb97ade7239441ae31a50bd66732602efd58570037d071d99b9c064abcc",
    "pickplace_iiwa.rsim": "811c2b98d2734875e2f3e0ff7025dd3fcaa528fc027bc0b998ab2969f16922a3",
    "stack_panda.rsim": "34becc4ebd2305e807717be349df1d69f5dc263956f304ef2e6f31c4a1c9473b",
}      # sha256 of robosuite_amd/assets/*.rsim on the commit before ray casting existed


def test_shipped_blobs_do_not_change():
    """the blob format did not move: every shipped model is the file it was, byte for byte, still round-trips through the Python reader / writer, and holds no
    rangefinder table"""
    import hashlib

    shipped = sorted(f for f in os.listdir(ASSETS) if f.endswith(".rsim"))
    assert shipped == sorted(SHIPPED_SHA256)
    for f in shipped:
        blob = open(os.path.join(ASSETS, f), "rb").read()
        assert hashlib.sha256(blob).hexdigest() == SHIPPED_SHA256[f], f
        flat = mjcf.from_blob(blob)
        assert mjcf.to_blob(flat) == blob, f
        assert 15 not in set(np.asarray(flat.arrays.get("sensor_type", [])).ravel().tolist())


# ---- the cap on rays the GPU tests leave out --------------------------------------------------------------------------------------------------------
def _state(flat, qpos):
    fr = sensors.body_frames(flat, qpos, np.zeros(int(flat.nv)), np.zeros(int(flat.nv)))
    return np.array([f.p for f in fr]), np.array([f.q for f in fr])


def test_ill_conditioned_share_stays_under_the_cap_scene_a(tmp_path):
    xml, adir = S.scene_a(tmp_path)
    flat = mjcf.compile_mjcf(xml, asset_dir=adir)
    assert sorted(set(np.asarray(flat.arrays["geom_type"]).ravel().tolist())) == [0, 2, 3, 4, 5, 6, 7]       # all seven types
    Q = S.scene_a_qpos(flat)
    bad = tot = hits = 0
    for e in range(3):
        xp, xq = _state(flat, Q[e])
        o, d = S.seeded_rays(flat, xp, xq, 257, seed=100 + e)
        ok = raycast.well_conditioned(flat, xp, xq, o, d)
        t, g = raycast.cast(flat, xp, xq, o, d)
        bad += (~ok).sum(); tot += len(ok); hits += (g >= 0).sum()
        assert (g < 0).sum() >= 20 and len(set(g[g >= 0].tolist())) >= 7      # misses, and every solid (and the floor) is hit by some ray
    assert bad <= 0.10 * tot, (bad, tot)


def test_ill_conditioned_share_stays_under_the_cap_scene_b():
    flat = mjcf.compile_mjcf(S.scene_b_xml())
    assert int(flat.ngeom) == 70
    xp, xq = _state(flat, np.array([0.3, -0.2, 0.5, 0.1]))
    o, d = S.seeded_rays(flat, xp, xq, 257, seed=5)
    ok = raycast.well_conditioned(flat, xp, xq, o, d)
    _, g = raycast.cast(flat, xp, xq, o, d)
    assert (~ok).sum() <= 0.10 * len(ok) and g.max() >= 64, ((~ok).sum(), g.max())        # and geoms past the first staging chunk are hit


def test_ill_conditioned_share_stays_under_the_cap_scene_c():
    flat, cfg = S.lift()
    xp, xq = _state(flat, S.lift_init_qpos(flat, cfg))
    for name, cam in S.lift_cameras(flat).items():
        for fovy in (45.0, 90.0):
            o, d = raycast.pixel_rays(Camera(cam.body, cam.pos, cam.quat, fovy), xp, xq, 24, 32)
            ok = raycast.well_conditioned(flat, xp, xq, o, d)
            _, gid = raycast.cast(flat, xp, xq, o, d)
            assert (~ok).sum() <= 0.10 * len(ok), (name, fovy, int((~ok).sum()))
            assert (gid >= 0).sum() >= 0.3 * len(gid), (name, fovy)           # the camera looks at the scene, not past it
    o, d = S.seeded_rays(flat, xp, xq, 257, seed=300, reach=1.2)
    ok = raycast.well_conditioned(flat, xp, xq, o, d, geomgroup=0b011)
    assert (~ok).sum() <= 0.10 * len(ok), int((~ok).sum())
