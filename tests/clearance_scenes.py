"""Scenes and seeded draws shared by tests/test_clearance_host.py (CPU, the mirror robosuite_amd/clearance.py), tests/test_clearance_core_host.py (CPU, the
fp32 core under sanitizers) and tests/test_clearance.py (GPU, the kernels against the mirror)."""
import os

import numpy as np

from robosuite_amd import clearance, distance, mjcf
from tests import ik_scenes
from tests import raycast_scenes as R
from tests.util import load_golden

SEED_T, SEED_Q = 77, 501
DISTMAX_T = 0.12      # scene T: small enough that a good share of the candidates has nothing closer (the mirror: about a third)
DISTMAX_ARM = 1.0

# Scene T: a small tree that takes every FK branch.  Chain: base hinge h0 (anchor off the body origin, axis off the frame axes, ref != 0), slide s1 (with ref),
# hinge h2; h2's body carries two slide "fingers" -- a branch that is held, never controlled.  A side link hangs from the first body on its own hinge hs: a
# second dof list controls it too, so that bodies with different signatures exist.  Link geoms: capsule, box, cylinder, ellipsoid, mesh.  A plane, a
# world-fixed box and two free bodies (sphere, box) that scene_t_qpos places near the arm's sweep.  One joint per body.
SCENE_T_XML = """<mujoco><compiler angle="radian"/>
  <asset><mesh name="poly" file="poly.obj"/></asset>
  <worldbody>
    <geom name="floor" type="plane" size="3 3 0.1"/>
    <geom name="wbox" type="box" size="0.08 0.12 0.2" pos="0.5 0.35 0.2" euler="0.1 0.2 0.3"/>
    <body name="l0" pos="0 0 0.45" euler="0.1 -0.1 0.2">
      <joint name="h0" type="hinge" axis="0.1 0.2 1" pos="0.02 -0.01 0.03" limited="true" range="-2.0 2.0" ref="0.2"/>
      <geom name="g_cap" type="capsule" size="0.04 0.1" pos="0.13 0 0" euler="0 1.5 0.1"/>
      <body name="side" pos="0.05 -0.22 0.06" euler="0.3 0 0.2">
        <joint name="hs" type="hinge" axis="1 0.2 0" pos="0 0.02 0" limited="true" range="-1.5 1.5"/>
        <geom name="g_msh" type="mesh" mesh="poly" pos="0 -0.12 0" euler="0.5 0.1 0.8"/>
      </body>
      <body name="l1" pos="0.3 0.02 0.01" euler="-0.3 0.2 0.1">
        <joint name="s1" type="slide" axis="1 0.3 -0.2" limited="true" range="-0.15 0.25" ref="0.05"/>
        <geom name="g_box" type="box" size="0.09 0.03 0.04" pos="0.08 0 0" euler="0.2 0.1 -0.3"/>
        <body name="l2" pos="0.25 0 0.03" euler="0.1 0.4 -0.2">
          <joint name="h2" type="hinge" axis="0.1 0.2 1" pos="-0.01 0.02 0.0" limited="true" range="-2.0 2.0"/>
          <geom name="g_cyl" type="cylinder" size="0.035 0.08" pos="0.09 0 0" euler="0.1 1.5 0"/>
          <geom name="g_ell" type="ellipsoid" size="0.06 0.04 0.03" pos="0.2 0.01 0.02" euler="0.2 0.9 0.4"/>
          <body name="f1" pos="0.28 0.04 0"><joint name="fs1" type="slide" axis="0 1 0" limited="true" range="-0.02 0.04"/>
            <geom name="g_f1" type="box" size="0.04 0.008 0.015" pos="0.03 0 0"/></body>
          <body name="f2" pos="0.28 -0.04 0"><joint name="fs2" type="slide" axis="0 -1 0" limited="true" range="-0.02 0.04"/>
            <geom name="g_f2" type="sphere" size="0.015" pos="0.05 0 0"/></body>
        </body>
      </body>
    </body>
    <body name="fsb" pos="0.5 -0.3 0.5"><freejoint name="fsj"/><geom name="fsph" type="sphere" size="0.07"/></body>
    <body name="fbb" pos="0.3 0.4 0.6"><freejoint name="fbj"/><geom name="fbox" type="box" size="0.06 0.09 0.05"/></body>
  </worldbody></mujoco>"""


def scene_t(tmpdir):
    R.write_obj(os.path.join(str(tmpdir), "poly.obj"), R.POLY_VERTS)
    return mjcf.compile_mjcf(SCENE_T_XML, asset_dir=str(tmpdir))


def dofs_of(flat, joints):
    dadr = np.asarray(flat.arrays["jnt_dofadr"]).ravel().astype(int)
    return [int(dadr[flat.names["joint"].index(j)]) for j in joints]


def dofs_t(flat, which="arm"):
    """"arm": the chain, in chain order; "all": the side link too, columns NOT in tree order"""
    return dofs_of(flat, ("h0", "s1", "h2") if which == "arm" else ("hs", "h2", "h0", "s1"))


def scene_t_qpos(flat, B, seed=SEED_T):
    """[B, nq]: every hinge / slide joint uniform in its range (the held ones stay there), the two free bodies near the arm's sweep.  Env e depends on
    (seed, e) only."""
    q0 = np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel()
    jt, qa = np.asarray(flat.arrays["jnt_type"]).ravel(), np.asarray(flat.arrays["jnt_qposadr"]).ravel()
    rng_ = np.asarray(flat.arrays["jnt_range"], dtype=np.float64).reshape(-1, 2)
    out = np.tile(q0, (B, 1))
    for e in range(B):
        rng = np.random.default_rng([seed, e])
        for j in range(len(jt)):
            a = qa[j]
            if jt[j] == mjcf.JNT_FREE:
                out[e, a:a + 3] = np.array([0.4, 0.0, 0.5]) + rng.uniform(-1, 1, 3) * np.array([0.3, 0.35, 0.25])
                q = rng.normal(size=4)
                out[e, a + 3:a + 7] = q / np.linalg.norm(q)
            else:
                out[e, a] = rng.uniform(rng_[j, 0], rng_[j, 1])
    return out


def candidates(flat, dofs, B, K, seed=SEED_Q, overrides=None):
    """[B, K, n] candidates, rng([seed, env, k])-uniform in ik_scenes.ranges, rounded to float32 (what the device is handed), as float64"""
    lo, hi, _ = ik_scenes.ranges(flat, dofs, overrides)
    out = np.zeros((B, K, len(dofs)))
    for e in range(B):
        for k in range(K):
            out[e, k] = np.random.default_rng([seed, e, k]).uniform(lo, hi)
    return out.astype(np.float32).astype(np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def params32(flat):
    return {k: f32(flat.arrays[k]) for k in ("geom_size", "geom_pos", "geom_quat")}


_CACHE = {}


def arm(name):
    """-> dict(flat, cfg, dofs, qpos): "panda" = the golden seed0_gentle Lift model, dofs 0..6; "baxter_right" / "baxter_left" / "baxter_both" = the golden
    peg_baxter ctl_joint_velocity model (the 64-body configuration), one arm with the other held, or both (14 dofs).  qpos is the model's qpos0."""
    if name not in _CACHE:
        if name == "panda":
            _, cfg, flat = load_golden("seed0_gentle")
            dofs = list(range(7))
        else:
            _, cfg, flat = load_golden("ctl_joint_velocity", "peg_baxter")
            dofs = {"baxter_right": list(range(7)), "baxter_left": list(range(7, 14)), "baxter_both": list(range(14))}[name]
        _CACHE[name] = dict(flat=flat, cfg=cfg, dofs=dofs, qpos=np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel().copy(), name=name)
    return _CACHE[name]


def fk_reference(flat, qpos, dofs, q, overrides=None):
    """the mirror's FK for qpos [B, nq], q [B, K, n] -> (xpos [B, K, nbody, 3], xquat [B, K, nbody, 4]); overrides: None, one dict, or a list of one per env"""
    B, K = q.shape[:2]
    xp, xq = np.zeros((B, K, int(flat.nbody), 3)), np.zeros((B, K, int(flat.nbody), 4))
    shared = None if isinstance(overrides, list) else clearance._model32(flat, overrides)
    for e in range(B):
        m32 = shared if shared is not None else clearance._model32(flat, overrides[e])
        for k in range(K):
            xp[e, k], xq[e, k] = clearance.fk(flat, qpos[e], dofs, q[e, k], model32=m32)
    return xp, xq


def pair_reference(flat, xpos, xquat, pairs, params=None):
    """the mirror's distance of every listed pair at poses [B, K, nbody, .], as a reference (distance_scenes.REF: iterated to 1e-10 m), unclamped:
    (d [B, K, P], fromto [B, K, P, 6], status [B, K, P]); params: one dict or a list of one per env"""
    from tests import distance_scenes as S

    B, K = xpos.shape[:2]
    d, ft, st = np.zeros((B, K, len(pairs))), np.zeros((B, K, len(pairs), 6)), np.zeros((B, K, len(pairs)), dtype=np.int32)
    for e in range(B):
        pe = params[e] if isinstance(params, list) else params
        for k in range(K):
            d[e, k], ft[e, k], st[e, k] = distance.geom_distance(flat, xpos[e, k], xquat[e, k], pairs, np.inf, params=pe, check_options=False, **S.REF)
    return d, ft, st


def rot_angle(qa, qb):
    """angle (rad) between unit quaternions [..., 4]"""
    qa, qb = np.asarray(qa, dtype=np.float64), np.asarray(qb, dtype=np.float64)
    s = np.where(np.sum(qa * qb, axis=-1, keepdims=True) < 0, -1.0, 1.0)      # q and -q are one rotation
    return 4 * np.arcsin(np.minimum(np.linalg.norm(qa - s * qb, axis=-1) / 2, 1.0))      # |qa - qb| = 2 sin(angle / 4)


# ---- records of the host rehearsal (tests/san/clear_core_driver.cpp) -------------------------------------------------------------------------------------
def body_table(flat, dofs):
    """The body table of rsim_clear_core.h with offsets into the driver's float table (float_table below), and the slot of every body: the host-side
    restatement of rsim_api.cpp clear_plan for the rehearsal."""
    I = lambda k: np.asarray(flat.arrays[k]).ravel().astype(int)      # noqa: E731
    sig = clearance.signatures(flat, dofs)
    col = clearance._columns(flat, dofs)
    parent, jadr, jnum, jt, qa = I("body_parentid"), I("body_jntadr"), I("body_jntnum"), I("jnt_type"), I("jnt_qposadr")
    off = float_offsets(flat)
    slot, tab = np.full(int(flat.nbody), -1), []
    for b in range(1, int(flat.nbody)):
        if not sig[b]:
            continue
        slot[b] = (slot >= 0).sum()
        tab.append([0, off["body_pos"] + 3 * b, off["body_quat"] + 4 * b, b, slot[parent[b]], 0, slot[b], parent[b]])
        for j in range(jadr[b], jadr[b] + jnum[b]):
            tab.append([jt[j], off["jnt_pos"] + 3 * j, off["jnt_axis"] + 3 * j, qa[j], col.get(j, -1), off["qpos0"] + qa[j], 0, 0])
    return np.asarray(tab, dtype=np.int32), slot.astype(np.int32)


_FT_FIELDS = ("body_pos", "body_quat", "jnt_pos", "jnt_axis", "qpos0", "geom_size", "geom_pos", "geom_quat")


def float_offsets(flat):
    out, at = {}, 0
    for k in _FT_FIELDS:
        out[k] = at
        at += np.asarray(flat.arrays[k]).size
    out["_len"] = at
    return out


def float_table(flat):
    return np.concatenate([np.asarray(flat.arrays[k], dtype=np.float64).ravel() for k in _FT_FIELDS]).astype("<f4")


def pack_scene(flat, dofs, qpos, xpos, xquat, q, pairs, distmax, tol, max_iters):
    """bytes of the driver's input (the layout is documented at the head of tests/san/clear_core_driver.cpp): qpos [B, nq], xpos / xquat [B, nbody, .] the envs'
    current poses, q [B, K, n]"""
    import struct

    tab, slot = body_table(flat, dofs)
    off = float_offsets(flat)
    B, K, n = q.shape
    gt, gb = np.asarray(flat.arrays["geom_type"]).ravel().astype("<i4"), np.asarray(flat.arrays["geom_bodyid"]).ravel().astype("<i4")
    verts, recs = [], []
    for a, b in np.asarray(pairs):
        rec = [int(a), int(b)]
        for g in (int(a), int(b)):
            V = distance.mesh_verts(flat, g) if gt[g] == mjcf.GEOM_MESH else None
            rec += [0, 0] if V is None else [sum(len(v) for v in verts), len(V)]
            if V is not None:
                verts.append(V)
        recs.append(rec)
    V = np.concatenate(verts) if verts else np.zeros((0, 3))
    head = struct.pack("<10i2fi3i", B, K, n, int(flat.nbody), int(flat.nq), int(flat.ngeom), len(tab), int((slot >= 0).sum()), len(recs), len(V), distmax, tol, max_iters,
                       off["geom_size"], off["geom_pos"], off["geom_quat"])
    parts = [head, tab.astype("<i4").tobytes(), slot.astype("<i4").tobytes(), gt.tobytes(), gb.tobytes(), np.asarray(recs, dtype="<i4").tobytes(),
             struct.pack("<i", off["_len"]), float_table(flat).tobytes(), V.astype("<f4").tobytes(), np.asarray(qpos, dtype="<f4").tobytes(),
             np.asarray(xpos, dtype="<f4").tobytes(), np.asarray(xquat, dtype="<f4").tobytes(), np.asarray(q, dtype="<f4").tobytes()]
    return b"".join(parts)


def unpack_scene(blob, B, K, nbody):
    """(xpos [B, K, nbody, 3], xquat [B, K, nbody, 4], dist [B, K], pair [B, K], fromto [B, K, 6], status [B, K]) of the driver's output"""
    n = B * K
    f = np.frombuffer(blob, dtype="<f4", count=n * nbody * 7)
    xp, xq = f[:n * nbody * 3].reshape(B, K, nbody, 3), f[n * nbody * 3:].reshape(B, K, nbody, 4)
    rec = np.frombuffer(blob, dtype=np.dtype([("f", "<f4", 7), ("i", "<i4", 2)]), count=n, offset=n * nbody * 7 * 4)
    return (xp.astype(np.float64), xq.astype(np.float64), rec["f"][:, 0].reshape(B, K).astype(np.float64), rec["i"][:, 0].reshape(B, K),
            rec["f"][:, 1:].reshape(B, K, 6).astype(np.float64), rec["i"][:, 1].reshape(B, K))
