"""Scenes, seeded poses and the certificate shared by tests/test_distance_host.py (CPU, the mirror), tests/test_distance_core_host.py (CPU, the fp32 core under
sanitizers) and tests/test_distance.py (GPU, the kernel against the mirror)."""
import functools
import os

import numpy as np

from robosuite_amd import distance, mjcf
from robosuite_amd.raycast import _rot, hull_planes
from tests import raycast_scenes as R

BAND = 1e-4          # status and fromto are compared only where the mirror's |d| and |d - distmax| both exceed this
BAND_SHARE = 0.10    # ... which may leave out at most this share of a scene's pairs
DISTMAX = 0.6        # scene A: far pairs exist, most do not reach it
DISTMAX_H = 0.2      # scene H, whose bodies are drawn closer together
REF = dict(tol=1e-10, max_iters=1000)     # the mirror as a reference: fp64, iterated until its bounds agree to 1e-10 m
SEED_A, SEED_H = 20, 41

# Scene A is raycast_scenes.SCENE_A_XML -- seven geom types, each off-axis, on hinge and free joints -- with two more bodies for the two configurations that
# scene cannot pose: a second box on a free joint (parallel faces against `box`), and a cylinder on a slide joint along the floor's normal whose flat end is
# parallel to the floor (joint position = its clearance).
FLOOR_EULER = (0.05, -0.03, 0.2)
CYL2_SIZE, CYL2_AT = (0.07, 0.05), (0.9, -0.6)
BOX2_SIZE = (0.07, 0.1, 0.04)


def _euler_xyz(e):
    cx, cy, cz, sx, sy, sz = *np.cos(e), *np.sin(e)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]); Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rx @ Ry @ Rz


def scene_a_xml():
    p = _euler_xyz(FLOOR_EULER) @ np.array([CYL2_AT[0], CYL2_AT[1], CYL2_SIZE[1]])
    extra = (f'<body name="fb2" pos="0.4 0.6 0.5"><freejoint name="fb2j"/><geom name="box2" type="box" size="{BOX2_SIZE[0]} {BOX2_SIZE[1]} {BOX2_SIZE[2]}"/></body>'
             f'<body name="cb" pos="{p[0]:.9f} {p[1]:.9f} {p[2]:.9f}" euler="{FLOOR_EULER[0]} {FLOOR_EULER[1]} {FLOOR_EULER[2]}"><joint name="cbj" type="slide" axis="0 0 1"/>'
             f'<geom name="cyl2" type="cylinder" size="{CYL2_SIZE[0]} {CYL2_SIZE[1]}"/></body>')
    assert "</worldbody>" in R.SCENE_A_XML
    return R.SCENE_A_XML.replace("</worldbody>", extra + "</worldbody>")


def scene_a(tmpdir):
    R.write_obj(os.path.join(str(tmpdir), "poly.obj"), R.POLY_VERTS)
    return mjcf.compile_mjcf(scene_a_xml(), asset_dir=str(tmpdir))


def all_pairs(flat, names=None):
    """every pair of the named geoms (all geoms when None) the query accepts, ascending"""
    ids = list(range(int(flat.ngeom))) if names is None else [flat.names["geom"].index(n) for n in names]
    gt = np.asarray(flat.arrays["geom_type"]).ravel()
    return np.array([(a, b) for i, a in enumerate(ids) for b in ids[i + 1:] if not (gt[a] == 0 and gt[b] == 0)], dtype=np.int32)


GAPS = (0.03, 2e-5, -0.01)      # separated, inside the touching band, overlapping


def scene_a_qpos(flat, B, seed=SEED_A):
    """[B, nq].  Every env: hinges and free bodies drawn around the arm so that pairs separate, touch and overlap; box2 face to face with `box` (same
    orientation, clearance GAPS[env % 3] along box's Z) and cyl2's flat end GAPS[(1, 2, 1)[env % 3]] over the floor.  Env e depends on (seed, e) only."""
    q0 = np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel()
    jt, qa = np.asarray(flat.arrays["jnt_type"]).ravel(), np.asarray(flat.arrays["jnt_qposadr"]).ravel()
    jn, gn = flat.names["joint"], flat.names["geom"]
    gq = np.asarray(flat.arrays["geom_quat"], dtype=np.float64).reshape(-1, 4)
    gs = np.asarray(flat.arrays["geom_size"], dtype=np.float64).reshape(-1, 3)
    out = np.tile(q0, (B, 1))
    for e in range(B):
        rng = np.random.default_rng([seed, e])
        for j in range(len(jt)):
            a = qa[j]
            if jt[j] == mjcf.JNT_FREE:
                # towards the fore-arm's neighbourhood, where the hinged geoms are
                out[e, a:a + 3] = np.array([0.55, 0.0, 0.62]) + rng.uniform(-1, 1, 3) * np.array([0.35, 0.3, 0.25])
                q = rng.normal(size=4)
                out[e, a + 3:a + 7] = q / np.linalg.norm(q)
            elif jn[j] != "cbj":
                out[e, a] += rng.uniform(-0.6, 0.6)
        a1, a2 = qa[jn.index("fbj")], qa[jn.index("fb2j")]
        Rb = _rot(out[e, a1 + 3:a1 + 7]) @ _rot(gq[gn.index("box")])            # world frame of `box` (its geom has no offset on the body)
        gap = GAPS[e % 3]
        out[e, a2:a2 + 3] = out[e, a1:a1 + 3] + Rb @ np.array([rng.uniform(-0.05, 0.05), rng.uniform(-0.05, 0.05), gs[gn.index("box")][2] + BOX2_SIZE[2] + gap])
        out[e, a2 + 3:a2 + 7] = mjcf.mat2quat(Rb)
        out[e, qa[jn.index("cbj")]] = GAPS[(1, 2, 1)[e % 3]]
    return out


# Scene H: a hull of 4 vertices, a generated hull of N_BIG > 256 vertices (points on an ellipsoid: all extreme) and a box, each on a free body
N_BIG = 300


def big_hull_verts(n=N_BIG):
    k = np.arange(n) + 0.5
    phi, th = np.arccos(1 - 2 * k / n), np.pi * (1 + 5 ** 0.5) * k
    return np.stack([0.12 * np.cos(th) * np.sin(phi), 0.08 * np.sin(th) * np.sin(phi), 0.05 * np.cos(phi)], axis=1)


SCENE_H_XML = """<mujoco><compiler angle="radian"/>
  <asset><mesh name="tet" file="tet.obj"/><mesh name="big" file="big.obj"/></asset>
  <worldbody>
    <body name="bt" pos="0 0 0.5"><freejoint/><geom name="tet" type="mesh" mesh="tet"/></body>
    <body name="bb" pos="0.3 0 0.5"><freejoint/><geom name="big" type="mesh" mesh="big"/></body>
    <body name="bx" pos="0 0.3 0.5"><freejoint/><geom name="hbox" type="box" size="0.06 0.09 0.05"/></body>
  </worldbody></mujoco>"""


def scene_h(tmpdir):
    R.write_obj(os.path.join(str(tmpdir), "tet.obj"), R.TETRA_VERTS)
    R.write_obj(os.path.join(str(tmpdir), "big.obj"), big_hull_verts())
    return mjcf.compile_mjcf(SCENE_H_XML, asset_dir=str(tmpdir))


def scene_h_qpos(flat, B, seed=SEED_H):
    out = np.tile(np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel(), (B, 1))
    for e in range(B):
        rng = np.random.default_rng([seed, e])
        for k in range(3):
            out[e, 7 * k:7 * k + 3] = np.array([0.0, 0.0, 0.5]) + rng.uniform(-0.16, 0.16, 3)
            q = rng.normal(size=4)
            out[e, 7 * k + 3:7 * k + 7] = q / np.linalg.norm(q)
    return out


# Scene L: shipped Lift / Panda -- the gripper's and the last links' hulls and pads against the table and the cube
L_ROBOT = ("robot0_link5", "robot0_link6", "robot0_link7", "gripper0_right_right_gripper", "gripper0_right_leftfinger", "gripper0_right_finger_joint1_tip",
           "gripper0_right_rightfinger", "gripper0_right_finger_joint2_tip")
L_SCENE = ("table", "cube_main")
DISTMAX_L = 1.0


def lift_bodies(flat):
    return [flat.names["body"].index(n) for n in L_ROBOT], [flat.names["body"].index(n) for n in L_SCENE]


# ---- forward kinematics of the free / hinge / slide scenes here, so that CPU tests need no device ---------------------------------------------------------
def body_poses(flat, qpos):
    """(xpos [nbody, 3], xquat [nbody, 4]) of one env, fp64 (hinge, slide and free joints)"""
    A = lambda n, w: np.asarray(flat.arrays[n], dtype=np.float64).reshape(-1, w)      # noqa: E731
    I = lambda n: np.asarray(flat.arrays[n]).ravel().astype(int)      # noqa: E731
    parent, jadr, jnum, jt, qa = I("body_parentid"), I("body_jntadr"), I("body_jntnum"), I("jnt_type"), I("jnt_qposadr")
    bpos, bquat, jpos, jax = A("body_pos", 3), A("body_quat", 4), A("jnt_pos", 3), A("jnt_axis", 3)
    q0 = np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel()
    nb = int(flat.nbody)
    xpos, xmat = np.zeros((nb, 3)), np.tile(np.eye(3), (nb, 1, 1))
    for b in range(1, nb):
        p, M = xpos[parent[b]] + xmat[parent[b]] @ bpos[b], xmat[parent[b]] @ _rot(bquat[b])
        for j in range(jadr[b], jadr[b] + jnum[b]):
            if jt[j] == mjcf.JNT_FREE:
                p, M = np.array(qpos[qa[j]:qa[j] + 3]), _rot(qpos[qa[j] + 3:qa[j] + 7])
            elif jt[j] == mjcf.JNT_SLIDE:
                p = p + M @ jax[j] * (qpos[qa[j]] - q0[qa[j]])
            elif jt[j] == mjcf.JNT_HINGE:
                ang, ax = qpos[qa[j]] - q0[qa[j]], jax[j] / np.linalg.norm(jax[j])
                anchor = p + M @ jpos[j]
                Rj = _rot(np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax]))
                M = M @ Rj
                p = anchor - M @ jpos[j]
            else:
                raise NotImplementedError("ball joints are not in these scenes")
        xpos[b], xmat[b] = p, M
    return xpos, np.stack([mjcf.mat2quat(m) for m in xmat])


# ---- the certificate ------------------------------------------------------------------------------------------------------------------------------------
def h_value(g, n):
    """support function value h(n) = max over the SOLID of n . x"""
    n = tuple(float(x) for x in n)
    return float(np.dot(distance.support_full(g, n), n))


@functools.lru_cache(maxsize=None)
def _planes_cached(key, shape):
    return hull_planes(np.frombuffer(key, dtype=np.float64).reshape(shape))


def outside_by(g, x):
    """how far (metres, >= 0) point x lies outside the solid g: 0 inside or on the surface.  Analytic per primitive, face planes for a hull; for an ellipsoid
    the excess of the scaled norm times the smallest radius (a lower bound of the distance, exact to first order at the surface)."""
    x = np.asarray(x, dtype=np.float64)
    l = g["R"].T @ (x - np.array(g["pos"]))
    t, s = g["type"], np.array(g["size"])
    if t == mjcf.GEOM_PLANE:
        return max(l[2], 0.0)
    if t == mjcf.GEOM_SPHERE:
        return max(np.linalg.norm(l) - s[0], 0.0)
    if t == mjcf.GEOM_CAPSULE:
        c = np.array([0, 0, np.clip(l[2], -s[1], s[1])])
        return max(np.linalg.norm(l - c) - s[0], 0.0)
    if t == mjcf.GEOM_ELLIPSOID:
        return max(np.linalg.norm(l / s) - 1.0, 0.0) * s.min()
    if t == mjcf.GEOM_CYLINDER:
        return float(np.hypot(max(np.hypot(l[0], l[1]) - s[0], 0.0), max(abs(l[2]) - s[1], 0.0)))
    if t == mjcf.GEOM_BOX:
        return float(np.linalg.norm(np.maximum(np.abs(l) - s, 0.0)))
    if len(g["verts"]) == 1:
        return float(np.linalg.norm(l - g["verts"][0]))
    P = _planes_cached(g["verts"].tobytes(), g["verts"].shape)
    return max(float((P[:, :3] @ l - P[:, 3]).max()), 0.0)


def certificate(g1, g2, fromto):
    """For a reported disjoint pair: (how far p1 is outside geom1, p2 outside geom2, the upper bound |p2 - p1|, the lower bound: the separation of the two solids
    along n = (p2 - p1) / |p2 - p1|, -h2(-n) - h1(n)).  The true distance lies between the two bounds."""
    p1, p2 = np.asarray(fromto[:3], dtype=np.float64), np.asarray(fromto[3:], dtype=np.float64)
    up = float(np.linalg.norm(p2 - p1))
    n = (p2 - p1) / up
    if g1["type"] == mjcf.GEOM_PLANE or g2["type"] == mjcf.GEOM_PLANE:       # a half-space has a support value along its own normal only
        pl, o, sgn = (g1, g2, 1.0) if g1["type"] == mjcf.GEOM_PLANE else (g2, g1, -1.0)
        npl = np.array(pl["cols"][2])
        low = -h_value(o, -npl) - float(np.dot(npl, pl["pos"])) if np.allclose(n * sgn, npl, atol=1e-6) else -np.inf
    else:
        low = -h_value(g2, -n) - h_value(g1, n)
    return outside_by(g1, p1), outside_by(g2, p2), up, low


def diameter(g):
    """diameter of the solid's bounding sphere about its frame (a plane has none)"""
    t, s = g["type"], np.array(g["size"])
    if t == mjcf.GEOM_MESH:
        return 2 * float(np.linalg.norm(g["verts"], axis=1).max())
    return 2 * float({mjcf.GEOM_SPHERE: s[0], mjcf.GEOM_CAPSULE: s[0] + s[1], mjcf.GEOM_ELLIPSOID: s.max(), mjcf.GEOM_CYLINDER: np.hypot(s[0], s[1]),
                      mjcf.GEOM_BOX: np.linalg.norm(s)}.get(t, np.inf))


def fp32_gap_allowance(g1, g2, d):
    """What fp32 can leave of the certified gap beyond tol, by reasoning.  The iteration also ends when |v|^2 no longer shrinks.  A support point w with
    v.v - v.w = g |v| shrinks |v|^2 by at least (g |v|)^2 / |w - v|^2, so the iteration goes on while that exceeds the resolution eta |v|^2 of |v|^2: it ends
    with g < |w - v| sqrt(eta), |w - v| <= the two diameters together.  eta: 4 ulp of the product (2^-22) plus the rounding of v's coordinates -- differences
    of numbers up to ~1 m, 2^-23 m -- relative to |v| >= the distance of the cores >= d, twice for the square."""
    eta = 2.0 ** -22 + 2 * 2.0 ** -23 / max(d, 1e-30)
    return (diameter(g1) + diameter(g2)) * np.sqrt(eta)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def params32(flat):
    """the model's geom arrays rounded to fp32, as the device holds them"""
    return {k: f32(flat.arrays[k]) for k in ("geom_size", "geom_pos", "geom_quat")}


def _robust_overlap(g1, g2):
    """the pair still overlaps with geom2 moved 2 BAND along +-x, +-y, +-z: the Minkowski difference then holds the octahedron of those six points, which holds
    the ball of radius 2 BAND / sqrt(3) > BAND about the origin -- the penetration is deeper than BAND"""
    for k in range(3):
        for sgn in (-1.0, 1.0):
            p = list(g2["pos"]); p[k] += sgn * 2 * BAND
            if not distance.pair(g1, dict(g2, pos=tuple(p)), np.inf, **REF)[2] & distance.OVERLAP:
                return False
    return True


def reference(flat, xpos, xquat, pairs, distmax, params=None):
    """The fp64 mirror on every env, as the reference: {"d": the unclamped distance [B, P] (0 for a status-2 overlap), "dist", "fromto", "status": what the query
    returns at `distmax`, "band": bool [B, P], True where status and fromto are NOT compared -- the mirror's |d| or |d - distmax| is within BAND, or an overlap
    of general convex shapes is not deeper than BAND}.  params: one dict, or a list of one per env."""
    B, P = len(xpos), len(pairs)
    d, ft, st, band = np.zeros((B, P)), np.zeros((B, P, 6)), np.zeros((B, P), dtype=np.int32), np.zeros((B, P), dtype=bool)
    for e in range(B):
        pe = params[e] if isinstance(params, list) else params
        G = distance.world_geoms(flat, xpos[e], xquat[e], np.asarray(pairs).ravel(), pe)
        for k, (a, b) in enumerate(pairs):
            d[e, k], ft[e, k], st[e, k] = distance.pair(G[int(a)], G[int(b)], np.inf, **REF)
            if st[e, k] & distance.OVERLAP:
                band[e, k] = not _robust_overlap(G[int(a)], G[int(b)])
            else:
                band[e, k] = abs(d[e, k]) <= BAND or abs(d[e, k] - distmax) <= BAND
    far = d > distmax
    return {"d": d, "dist": np.where(far, distmax, d), "fromto": np.where(far[..., None], 0.0, ft), "status": np.where(far, st | distance.FAR, st), "band": band}


# ---- records of the host rehearsal (tests/san/dist_core_driver.cpp) ------------------------------------------------------------------------------------------
def pack_records(geom_pairs, distmax, tol, max_iters):
    """bytes of the driver's input: geom_pairs is a list of (mirror geom, mirror geom)"""
    import struct

    out = [struct.pack("<iffi", len(geom_pairs), distmax, tol, max_iters)]
    for pr in geom_pairs:
        for g in pr:
            V = np.zeros((0, 3)) if g["verts"] is None else g["verts"]
            out.append(struct.pack("<ii", g["type"], len(V)))
            out.append(np.concatenate([np.asarray(g["size"]), np.asarray(g["pos"]), mjcf.mat2quat(g["R"])]).astype("<f4").tobytes())
            out.append(np.ascontiguousarray(V, dtype="<f4").tobytes())
    return b"".join(out)


def unpack_results(blob, n):
    """(dist [n], fromto [n, 6], status [n]) of the driver's output"""
    rec = np.frombuffer(blob, dtype=np.dtype([("f", "<f4", 7), ("i", "<i4", 2)]), count=n)
    return rec["f"][:, 0].astype(np.float64), rec["f"][:, 1:].astype(np.float64), rec["i"][:, 0].astype(np.int32)


def geom32(g):
    """the mirror geom with size, position and rotation as the fp32 record carries them"""
    return distance.make_geom(g["type"], f32(g["size"]), f32(g["pos"]), f32(mjcf.mat2quat(g["R"])), None if g["verts"] is None else f32(g["verts"]))
