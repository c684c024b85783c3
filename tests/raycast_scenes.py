"""Scenes, seeded rays and cameras shared by tests/test_raycast_host.py (CPU, the mirror) and tests/test_raycast.py (GPU, the kernel against the mirror)."""
import json
import os

import numpy as np

from robosuite_amd import mjcf
from robosuite_amd.raycast import Camera

ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robosuite_amd", "assets")

# an irregular convex polyhedron: every vertex is extreme, its bottom face is a quadrilateral (a coplanar triangle pair the hull code must merge)
POLY_VERTS = [(-0.10, -0.07, -0.05), (0.10, -0.07, -0.05), (0.10, 0.07, -0.05), (-0.10, 0.07, -0.05),      # bottom quad
              (-0.06, -0.04, 0.06), (0.07, -0.03, 0.06), (0.05, 0.05, 0.06), (-0.05, 0.04, 0.06), (0.0, 0.0, 0.11)]
TETRA_VERTS = [(0.0, 0.0, 0.0), (0.2, 0.0, 0.0), (0.0, 0.2, 0.0), (0.0, 0.0, 0.2)]


def write_obj(path, verts):
    """vertices only (the compiler takes the convex hull)"""
    with open(path, "w") as f:
        for v in verts:
            f.write("v %.9g %.9g %.9g\n" % tuple(v))
        f.write("f 1 2 3\n")


# Scene A: one geom of each of the seven types, each rotated off-axis, on bodies with hinge and free joints; a rangefinder on a site of the forearm
SCENE_A_XML = """<mujoco><compiler angle="radian"/>
  <asset><mesh name="poly" file="poly.obj"/></asset>
  <worldbody>
    <geom name="floor" type="plane" size="3 2 0.1" euler="0.05 -0.03 0.2"/>
    <body name="arm" pos="0 0 0.7"><joint name="h1" type="hinge" axis="0 1 0"/>
      <geom name="cap" type="capsule" size="0.06 0.2" pos="0.2 0 0" euler="0.3 0.4 0.5"/>
      <body name="fore" pos="0.5 0 0"><joint name="h2" type="hinge" axis="0 0 1"/>
        <geom name="cyl" type="cylinder" size="0.08 0.15" euler="0.7 0.2 0.1"/>
        <geom name="ell" type="ellipsoid" size="0.1 0.06 0.04" pos="0.25 0.05 0" euler="0.2 0.9 0.4"/>
        <site name="tip" pos="0.1 0 -0.2" euler="3.0 0.2 0"/>
      </body></body>
    <body name="fb" pos="-0.5 0.3 0.5"><freejoint name="fbj"/><geom name="box" type="box" size="0.12 0.08 0.05" euler="0.4 0.3 0.2"/></body>
    <body name="fs" pos="0.1 -0.5 0.4"><freejoint name="fsj"/><geom name="sph" type="sphere" size="0.11" pos="0.02 0 0" group="2"/></body>
    <body name="fm" pos="-0.3 -0.4 0.5"><freejoint name="fmj"/><geom name="msh" type="mesh" mesh="poly" euler="0.5 0.1 0.8"/>
      <geom name="ghost" type="sphere" size="0.3" rgba="1 0 0 0" contype="0" conaffinity="0"/></body>
  </worldbody>
  <sensor><rangefinder name="rf_tip" site="tip"/><framepos name="fp_tip" objtype="site" objname="tip"/></sensor></mujoco>"""


def scene_a(tmpdir):
    """(xml, asset_dir): writes the mesh file next to nothing else"""
    write_obj(os.path.join(str(tmpdir), "poly.obj"), POLY_VERTS)
    return SCENE_A_XML, str(tmpdir)


def scene_a_qpos(flat, B=3, seed=7):
    """[B, nq]: different joint angles and free-body poses per env (env 0: the model's own)"""
    rng = np.random.default_rng(seed)
    q0 = np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel()
    out = np.tile(q0, (B, 1))
    jt, qa = np.asarray(flat.arrays["jnt_type"]).ravel(), np.asarray(flat.arrays["jnt_qposadr"]).ravel()
    for e in range(1, B):
        for j in range(len(jt)):
            a = qa[j]
            if jt[j] == mjcf.JNT_FREE:
                out[e, a:a + 3] += rng.uniform(-0.08, 0.08, 3)
                q = out[e, a + 3:a + 7] + rng.uniform(-0.4, 0.4, 4)
                out[e, a + 3:a + 7] = q / np.linalg.norm(q)
            else:
                out[e, a] += rng.uniform(-0.5, 0.5)
    return out


def scene_b_xml(n=70):
    """Scene B: `n` spheres over the world and four hinged bodies -- more geoms than one LDS staging chunk of the kernel holds (64).  Only the first sphere of
    every body collides, so the model fits every kernel configuration's colliding-geom capacity."""
    rng = np.random.default_rng(11)
    per = n // 5
    parts = []
    for b in range(5):
        geoms = []
        for k in range(per if b < 4 else n - 4 * per):
            p, r = rng.uniform(-0.35, 0.35, 3), rng.uniform(0.03, 0.08)
            vis = "" if k == 0 else ' contype="0" conaffinity="0"'
            geoms.append(f'<geom type="sphere" size="{r:.4f}" pos="{p[0]:.4f} {p[1]:.4f} {p[2]:.4f}" group="{k % 3}"{vis}/>')
        parts.append(geoms)
    bodies = "".join(f'<body name="b{b}" pos="{0.8 * (b - 1.5):.2f} 0 1.0"><joint name="j{b}" type="hinge" axis="{b % 2} {(b + 1) % 2} 0"/>{"".join(parts[b])}</body>' for b in range(4))
    return f'<mujoco><worldbody><body name="stat" pos="0 0.9 1.0">{"".join(parts[4])}</body>{bodies}</worldbody></mujoco>'


def lift():
    """Scene C: (flat, cfg) of the shipped Lift / Panda asset -- 65 mesh geoms over ten hulls"""
    return mjcf.load_model(os.path.join(ASSETS, "lift_panda.rsim")), json.load(open(os.path.join(ASSETS, "lift_panda.cfg.json")))


def lift_init_qpos(flat, cfg):
    """the pose a Lift episode starts from: arm and open gripper at their initial joint angles (cfg["reset"]), the cube on the table.  (At the model's qpos0 the
    two finger pads overlap with coplanar faces: rays that end there are exact ties between two different geoms, decided by rounding alone.)"""
    q = np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel().copy()
    r = cfg["reset"]
    q[r["arm_qpos_idx"]] = r["arm_init_qpos"]
    for gr in r["grippers"]:
        q[gr["qpos_idx"]] = gr["init_qpos"]
    q[9:12] = [0.01, -0.02, 0.83]
    return q


def lift_cameras(flat):
    """a fixed world camera looking at the table from the front, and one on the hand body looking along the gripper"""
    hand = flat.names["body"].index("robot0_right_hand")
    # world camera: at (1.3, 0.25, 1.55), looking back down at the table centre (0, 0, 0.85)
    eye, at = np.array([1.3, 0.25, 1.55]), np.array([0.0, 0.0, 0.85])
    z = (eye - at) / np.linalg.norm(eye - at)
    x = np.cross([0, 0, 1.0], z); x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return {"front": Camera(0, tuple(eye), tuple(mjcf.mat2quat(np.stack([x, y, z], axis=1))), 45.0),
            "hand": Camera(hand, (0.07, 0.0, 0.03), tuple(mjcf.quat_normalize(np.array([0.05, 0.7, 0.7, 0.08]))), 75.0)}


def geom_world(flat, xpos, xquat):
    """world centres [ngeom, 3] and rotations [ngeom, 3, 3] of the geoms"""
    from robosuite_amd.raycast import _rot

    gb = np.asarray(flat.arrays["geom_bodyid"]).ravel().astype(int)
    gp, gq = np.asarray(flat.arrays["geom_pos"], dtype=np.float64).reshape(-1, 3), np.asarray(flat.arrays["geom_quat"], dtype=np.float64).reshape(-1, 4)
    xpos, xquat = np.asarray(xpos, dtype=np.float64).reshape(-1, 3), np.asarray(xquat, dtype=np.float64).reshape(-1, 4)
    R = np.stack([_rot(xquat[gb[g]]) @ _rot(gq[g]) for g in range(len(gb))])
    c = np.stack([xpos[gb[g]] + _rot(xquat[gb[g]]) @ gp[g] for g in range(len(gb))])
    return c, R


def seeded_rays(flat, xpos, xquat, n, seed, reach=1.5):
    """n rays of one env, in a fixed mix: aimed at (jittered) geom centres from around the scene, pointing away from it (misses), starting at geom centres
    (inside starts), parallel to a face of every box and to the axis of every cylinder / capsule (offset so that they hit), and of non-unit length."""
    rng = np.random.default_rng(seed)
    c, R = geom_world(flat, xpos, xquat)
    gt = np.asarray(flat.arrays["geom_type"]).ravel().astype(int)
    gs = np.asarray(flat.arrays["geom_size"], dtype=np.float64).reshape(-1, 3)
    solid = np.flatnonzero(gt != mjcf.GEOM_PLANE)
    mid = c[solid].mean(axis=0)
    o, d = np.zeros((n, 3)), np.zeros((n, 3))
    for i in range(n):
        kind = i % 8
        g = solid[rng.integers(len(solid))]
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        if kind == 5:          # away from the scene, upwards: nothing to hit
            o[i] = mid + u * reach
            d[i] = u + np.array([0, 0, 1.5])
        elif kind == 6:        # from inside a solid
            pos_sizes = gs[g][gs[g] > 0]                     # (a mesh geom has none: its frame sits at the hull's centre of mass)
            o[i] = c[g] + R[g] @ (rng.uniform(-0.2, 0.2, 3) * (pos_sizes.min() if len(pos_sizes) else 0.03))
            d[i] = u
        elif kind == 7 and np.any(np.isin(gt, (mjcf.GEOM_BOX, mjcf.GEOM_CYLINDER, mjcf.GEOM_CAPSULE))):
            # exactly along a local axis of a box (parallel to four of its faces) / the axis of a cylinder or capsule, offset inside the cross-section
            g = rng.choice(np.flatnonzero(np.isin(gt, (mjcf.GEOM_BOX, mjcf.GEOM_CYLINDER, mjcf.GEOM_CAPSULE))))
            ax = int(rng.integers(3)) if gt[g] == mjcf.GEOM_BOX else 2
            off = rng.uniform(-0.5, 0.5, 3) * (gs[g] if gt[g] == mjcf.GEOM_BOX else np.array([gs[g][0], gs[g][0], 0.0]) * 0.7)
            off[ax] = -1.0
            o[i] = c[g] + R[g] @ off
            d[i] = R[g][:, ax]
        else:                  # from around the scene at a jittered geom centre; the length of dir varies
            o[i] = mid + u * reach * rng.uniform(0.6, 1.2)
            tgt = c[g] + rng.normal(size=3) * 0.04
            d[i] = (tgt - o[i]) * rng.uniform(0.3, 2.5)
    return o, d


def rel_err(t, t_ref):
    """|t - t_ref| / max(1, t_ref), the distance error of the issue; misses (-1 / inf on both sides) count as 0"""
    t, t_ref = np.asarray(t, dtype=np.float64), np.asarray(t_ref, dtype=np.float64)
    both_miss = (~np.isfinite(t) & ~np.isfinite(t_ref)) | ((t < 0) & (t_ref < 0))
    with np.errstate(invalid="ignore"):
        e = np.abs(t - t_ref) / np.maximum(1.0, np.abs(t_ref))
    return np.where(both_miss, 0.0, e)


def add_rangefinder(flat, name, site):
    """A copy of a compiled model (one loaded from a blob has no MJCF to edit) with a rangefinder at site id `site` appended to its sensors."""
    m = flat.copy()
    n0 = int(m.nsensor)
    old_t = [int(t) for t in np.asarray(m.arrays["sensor_type"]).ravel()]
    cat = lambda key, old, add: m.set(key, np.concatenate([np.asarray(old, dtype=np.int32).ravel(), np.asarray(add, dtype=np.int32)]), np.int32)
    kinds = m.arrays.get("sensor_objtype", [mjcf.SENSOR_OBJ_SITE if t >= 0 else mjcf.SENSOR_OBJ_NONE for t in old_t])
    reasons = m.arrays.get("sensor_reason", [0 if t >= 0 else 1 for t in old_t])
    shapes = m.arrays.get("sensor_shape", [-1] * n0)
    cat("sensor_dim", m.arrays["sensor_dim"], [1]); cat("sensor_objid", m.arrays["sensor_objid"], [site])
    cat("sensor_type", m.arrays["sensor_type"], [mjcf.RAY_SENSOR_TYPES["rangefinder"]]); cat("sensor_objtype", kinds, [mjcf.SENSOR_OBJ_SITE])
    cat("sensor_reason", reasons, [0]); cat("sensor_shape", shapes, [-1])
    m.set("nsensor", n0 + 1, np.int32)
    m.names["sensor"] = list(m.names["sensor"]) + [name]
    return m
