"""Scenes and seeded draws of the carried-object tests: tests/test_attach_host.py (CPU, the mirror robosuite_amd/clearance.py / sweep.py with attach / held /
rel), tests/test_attach_core_host.py (CPU, the fp32 core under sanitizers) and tests/test_attach.py (GPU, the kernels).  Scene T, its states and the candidate
and segment draws are tests/clearance_scenes.py's and tests/sweep_scenes.py's; what is fixed here is what is attached, which envs hold it, and how.

  * scene T: the free sphere `fsb` rides on the last link `l2`, the free box `fbb` on the side link `side`, dofs "all" (the side link's hinge is controlled,
    so both carriers are moved and have different signatures).
  * held[e] = (e % 2 == 0, e % 3 != 0): envs 0 .. 5 show all four rows, and with K = 3 or 5 the lanes of one wavefront disagree about every skip.
  * rel, two modes.  "state": None, taken from the env's seeded poses -- the sphere then often sits under the floor or inside the arm, fine for FK and the
    distance layer, and for a sweep only with segments chosen for it (SEGMENTS["state"]).  "given": the sphere 11 cm ahead of the finger tips, the box beside the side link's
    mesh, each with a small seeded offset and tilt per env: tests/test_attach_host.py test_condition_for_the_gpu_tests holds the mirror to deciding every
    GPU-shape segment of BOTH modes, FREE and HIT at t > 0 both among the envs that hold something.
  * scene J, a tool with a jaw: the free body `tool` carries a SUBTREE -- `jaw` on a hinge, `tip` below it on a slide, `guard` beside them without a joint --
    and rides on the arm's `wrist`.  The joints below the tool are held at the env's qpos.  It takes the table's CL_BODY elements with o3 = attachment + 1:
    the parent from the element before or from the store, the env's pose where the tool is not held.  A mocap body and a second free body stand by.  The
    models the refusals need and the XML compiler cannot produce (a free joint, a mocap body below an attached body) are edited copies: `edited`."""
import copy
import struct

import numpy as np

from robosuite_amd import clearance
from tests import clearance_scenes as S
from tests import sweep_scenes as W

ATTACH_T = (("fsb", "l2"), ("fbb", "side"))
SEED_REL = 911
REL_MODES = ("state", "given")
SHAPES = ((3, 5), (65, 3), (2, 70))      # tests/test_clearance.py SHAPES (that file imports torch; tests/test_attach.py asserts they are the same)
# the two ends of segment (env, k): candidates() draws of these two seeds, the second pulled towards the first -- q1 = q0 + SEGMENT_SCALE (draw1 - q0) --
# so that the mirror decides every segment of SHAPES within max_steps / 2 (tests/test_attach_host.py test_condition_for_the_gpu_tests holds it to that)
SEED_A0, SEED_A1, SEGMENT_SCALE = 2541, 2542, 0.5
# ... with rel from the seeded state most draws are of no use for a sweep (the carried sphere starts under the floor or inside the arm: a HIT at t = 0, or a
# graze that takes every sample).  These seeds and this scale are the first of a search over the MIRROR alone for which it meets the same condition
SEGMENTS = {"given": (SEED_A0, SEED_A1, SEGMENT_SCALE), "state": (3041, 3042, 0.25)}
# the given grasp: centre of the body in the carrier's frame (m); env e adds rng([SEED_REL, e, i]) offsets of +-1 cm and a random tilt of up to 0.3 rad
REL_CENTRE = ((0.46, 0.0, 0.0), (0.0, -0.33, 0.05))


SCENE_J_XML = """<mujoco><compiler angle="radian"/>
  <worldbody>
    <geom name="floor" type="plane" size="3 3 0.1"/>
    <body name="arm" pos="0 0 0.6" euler="0.1 0 0.2"><joint name="j" type="hinge" axis="0 1 0.1" pos="0.01 0 0.02" limited="true" range="-1.2 1.2"/>
      <geom name="bar" type="capsule" size="0.03 0.15" pos="0.15 0 0" euler="0 1.5708 0"/>
      <body name="wrist" pos="0.32 0 0" euler="0 0.2 0.1"><joint name="w" type="hinge" axis="0.2 0 1" limited="true" range="-1.5 1.5"/>
        <geom name="palm" type="box" size="0.03 0.04 0.02" pos="0.03 0 0"/></body></body>
    <body name="target" mocap="true" pos="0.5 0.5 0.5"><geom name="tsph" type="sphere" size="0.03"/></body>
    <body name="tool" pos="0.5 0 0.5"><freejoint name="tf"/><geom name="handle" type="box" size="0.05 0.02 0.02"/>
      <body name="jaw" pos="0.08 0 0.01" euler="0.1 0.2 0.3"><joint name="jh" type="hinge" axis="0 0.1 1" pos="0.01 0 0" limited="true" range="-1 1"/>
        <geom name="blade" type="box" size="0.04 0.01 0.01" pos="0.04 0 0"/>
        <body name="tip" pos="0.09 0 0"><joint name="ts" type="slide" axis="1 0.2 0" limited="true" range="-0.02 0.05" ref="0.01"/>
          <geom name="point" type="sphere" size="0.012"/></body></body>
      <body name="guard" pos="-0.07 0 0.02" euler="0.3 0 0"><geom name="ring" type="capsule" size="0.012 0.03"/></body></body>
    <body name="puck" pos="0.45 0.2 0.3"><freejoint name="pf"/><geom name="disc" type="cylinder" size="0.05 0.02"/></body>
  </worldbody></mujoco>"""
ATTACH_J = (("tool", "wrist"),)
SEED_J = 1207
REL_J = (0.10, 0.0, 0.0)      # the given grasp of scene J: the handle just ahead of the palm, plus rel_given's seeded offset and tilt


def scene_j():
    from robosuite_amd import mjcf

    return mjcf.compile_mjcf(SCENE_J_XML)


def dofs_j(flat):
    return S.dofs_of(flat, ("w", "j"))      # (columns not in tree order)


def attach_j(flat):
    b = flat.names["body"].index
    return [(b(x), b(c)) for x, c in ATTACH_J]


def held_rows_j(B):
    """bool [B, 1]: every other env holds the tool"""
    return (np.arange(B) % 2 == 0)[:, None]


def scene_j_qpos(flat, B):
    """[B, nq]: clearance_scenes.scene_t_qpos's rule (every hinge / slide joint uniform in its range, the free bodies near the arm), then the tool and the
    puck lifted clear of the floor, so that segments are not all a HIT at once"""
    out = S.scene_t_qpos(flat, B, SEED_J)
    jt, qa = clearance._I(flat, "jnt_type"), clearance._I(flat, "jnt_qposadr")
    for a in qa[jt == 0]:
        out[:, a + 2] = np.abs(out[:, a + 2]) + 0.35
    return out


def rel_given_j(B):
    out = rel_given(B)[:, :1].copy()
    out[:, 0, :3] += np.asarray(REL_J) - np.asarray(REL_CENTRE[0])
    return S.f32(out)


def edited(flat, **arrays):
    """a copy of the compiled model with entries of its arrays overwritten: edited(flat, jnt_type={3: 0}).  FOR THE HOST-SIDE REFUSALS ONLY: such a model
    is inconsistent (a free joint with one qpos entry) and must never reach a batch."""
    out = copy.copy(flat)
    out.arrays = type(flat.arrays)((k, np.array(v, copy=True)) for k, v in flat.arrays.items())
    for name, edits in arrays.items():
        for i, v in edits.items():
            out.arrays[name].reshape(-1)[i] = v
    return out


def attach_t(flat):
    b = flat.names["body"].index
    return [(b(x), b(c)) for x, c in ATTACH_T]


def held_rows(B):
    """bool [B, 2]"""
    e = np.arange(B)
    return np.stack([e % 2 == 0, e % 3 != 0], axis=1)


def rel_given(B):
    """float64 [B, 2, 7], rounded to float32 (what the device is handed); row (e, i) depends on (SEED_REL, e, i) only.  The quaternion is NOT unit: the
    kernel and the mirror normalise it."""
    out = np.zeros((B, len(ATTACH_T), 7))
    for e in range(B):
        for i, c in enumerate(REL_CENTRE):
            rng = np.random.default_rng([SEED_REL, e, i])
            out[e, i, :3] = np.asarray(c) + rng.uniform(-0.01, 0.01, 3)
            axis = rng.normal(size=3)
            ang = rng.uniform(-0.3, 0.3)
            out[e, i, 3:] = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * axis / np.linalg.norm(axis)]) * rng.uniform(0.8, 1.3)
    return S.f32(out)


def segments(flat, dofs, B, K, mode="given"):
    """(q0, q1) [B, K, n] float32-rounded ends for the rel mode; segment (env, k) depends on (seeds, env, k) only"""
    s0, s1, scale = SEGMENTS[mode]
    q0, q1 = S.candidates(flat, dofs, B, K, s0), S.candidates(flat, dofs, B, K, s1)
    return q0, S.f32(q0 + scale * (q1 - q0))


def rel_of(mode, B):
    return None if mode == "state" else rel_given(B)


def mirror_fk(flat, qpos, dofs, q, attach, held, rel, now=None):
    """the mirror's attached FK for qpos [B, nq], q [B, K, n], held [B, n], rel [B, n, 7] or None -> (xpos [B, K, nbody, 3], xquat [B, K, nbody, 4]); now:
    (xpos, xquat) [B, nbody, .] the envs' current poses as the device holds them (rel "state" is taken from those)"""
    B, K = q.shape[:2]
    xp, xq = np.zeros((B, K, int(flat.nbody), 3)), np.zeros((B, K, int(flat.nbody), 4))
    m32 = clearance._model32(flat)
    for e in range(B):
        for k in range(K):
            xp[e, k], xq[e, k] = clearance.fk(flat, qpos[e], dofs, q[e, k], model32=m32, attach=attach, held=held[e], rel=None if rel is None else rel[e],
                                              now=None if now is None else (now[0][e], now[1][e]))
    return xp, xq


# ---- records of the host rehearsal (tests/san/attach_core_driver.cpp) ------------------------------------------------------------------------------------
def attach_table(flat, dofs, attach):
    """clearance_scenes.body_table with the attached subtrees appended: the host-side restatement of rsim_api.cpp clear_plan with attachments.  -> (table,
    slot [nbody], body_sig [nbody] (signature not held | held << 16), body_att [nbody])"""
    I = lambda k: np.asarray(flat.arrays[k]).ravel().astype(int)      # noqa: E731
    tab, slot = S.body_table(flat, dofs)
    tab, slot = [list(r) for r in tab], slot.copy()
    parent, jadr, jnum, jt, qa = I("body_parentid"), I("body_jntadr"), I("body_jntnum"), I("jnt_type"), I("jnt_qposadr")
    off = S.float_offsets(flat)
    sig0, sig1 = clearance.signatures(flat, dofs, attach, [False] * len(attach)), clearance.signatures(flat, dofs, attach)
    att_of = np.full(int(flat.nbody), -1)
    for i, (body, carrier) in enumerate(attach):
        for c in clearance.subtree(flat, body):
            att_of[c] = i
            slot[c] = (slot >= 0).sum()
            if c == body:
                tab.append([4, 0, 0, c, slot[carrier], i, slot[c], carrier])
                continue
            tab.append([0, off["body_pos"] + 3 * c, off["body_quat"] + 4 * c, c, slot[parent[c]], i + 1, slot[c], parent[c]])
            for j in range(jadr[c], jadr[c] + jnum[c]):
                tab.append([jt[j], off["jnt_pos"] + 3 * j, off["jnt_axis"] + 3 * j, qa[j], -1, off["qpos0"] + qa[j], 0, 0])
    return np.asarray(tab, dtype=np.int32), slot.astype(np.int32), (sig0 | (sig1 << 16)).astype(np.int32), att_of.astype(np.int32)


def pack_attach(flat, dofs, attach, held, rel, qpos, xpos, xquat, q0, q1, pairs, distmax, tol, max_iters, margin, slack, max_steps, skip=True):
    """bytes of the driver's input: sweep_scenes.pack_sweep with the attached table and slots in place of the plain ones, then int32 natt, has_rel, skip;
    int32 body_sig[nbody], body_att[nbody]; uint8 held[B][natt]; float rel[B][natt][7] if has_rel"""
    plain_tab, plain_slot = S.body_table(flat, dofs)
    tab, slot, bsig, batt = attach_table(flat, dofs, attach)
    blob = W.pack_sweep(flat, dofs, qpos, xpos, xquat, q0, q1, pairs, distmax, tol, max_iters, margin, slack, max_steps)
    head = struct.calcsize("<10i2fi3i")
    fields = list(struct.unpack("<10i2fi3i", blob[:head]))
    assert fields[6] == len(plain_tab)
    fields[6], fields[7] = len(tab), int((slot >= 0).sum())
    old = plain_tab.astype("<i4").tobytes() + plain_slot.astype("<i4").tobytes()
    assert blob[head:head + len(old)] == old
    B = q0.shape[0]
    tail = [struct.pack("<3i", len(attach), int(rel is not None), int(skip)), bsig.astype("<i4").tobytes(), batt.astype("<i4").tobytes(),
            np.asarray(held, dtype=np.uint8).reshape(B, len(attach)).tobytes()]
    if rel is not None:
        tail.append(np.asarray(rel, dtype="<f4").reshape(B, len(attach), 7).tobytes())
    return struct.pack("<10i2fi3i", *fields) + tab.astype("<i4").tobytes() + slot.astype("<i4").tobytes() + blob[head + len(old):] + b"".join(tail)


def unpack_attach(blob, B, K, nbody):
    """-> (xpos [B, K, nbody, 3], xquat [B, K, nbody, 4] at q0, clearance dict at q0 (dist, pair, status, fromto), sweep dict as sweep_scenes.unpack_sweep)"""
    n = B * K
    f = np.frombuffer(blob, dtype="<f4", count=n * nbody * 7)
    xp, xq = f[:n * nbody * 3].reshape(B, K, nbody, 3).astype(np.float64), f[n * nbody * 3:].reshape(B, K, nbody, 4).astype(np.float64)
    at = n * nbody * 7 * 4
    rec = np.frombuffer(blob, dtype=np.dtype([("f", "<f4", 7), ("i", "<i4", 2)]), count=n, offset=at)
    clear = dict(dist=rec["f"][:, 0].reshape(B, K).astype(np.float64), fromto=rec["f"][:, 1:].reshape(B, K, 6).astype(np.float64),
                 pair=rec["i"][:, 0].reshape(B, K), status=rec["i"][:, 1].reshape(B, K))
    return xp, xq, clear, W.unpack_sweep(blob[at + n * 36:], B, K)
