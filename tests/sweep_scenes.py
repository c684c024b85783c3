"""Scenes and seeded draws shared by tests/test_sweep_host.py (CPU, the mirror robosuite_amd/sweep.py against brute force), tests/test_sweep_core_host.py
(CPU, the fp32 core under sanitizers) and tests/test_sweep.py (GPU, the kernel against the mirror and against config_clearance / config_fk).  Scene T, its
states and the candidate draws are tests/clearance_scenes.py's."""
import struct

import numpy as np

from robosuite_amd import mjcf
from tests import clearance_scenes as S

# the two ends of segment (env, k) are candidates() draws of these two seeds.  Chosen so that the mirror decides every segment of the GPU shapes of
# tests/test_sweep.py within max_steps / 2 samples (tests/test_sweep_host.py test_condition_for_the_gpu_tests holds them to it).
SEED_Q0, SEED_Q1 = 2541, 2542
DENSE = 129      # samples per segment of a dense certificate check

# The thin wall: one hinge link (a box 40 cm long, 2 cm wide) turns about the world z axis from -1 rad to +1 rad across a world box 4 mm thick that stands
# radially at angle 0, 35 .. 45 cm from the axis.  Ten uniform samples of the motion (the two ends and eight between them) sit at -1 + 2 i / 9 rad: the two
# nearest the wall are 0.111 rad to either side, where the link's flank is 0.35 tan(0.111) - 0.01 / cos(0.111) - 0.002 = 2.7 cm from the wall's face.
THIN_WALL_XML = """<mujoco><compiler angle="radian"/>
  <worldbody>
    <geom name="wall" type="box" size="0.05 0.002 0.1" pos="0.4 0 0.3"/>
    <body name="link" pos="0 0 0.3">
      <joint name="turn" type="hinge" axis="0 0 1" limited="true" range="-2 2"/>
      <geom name="bar" type="box" size="0.2 0.01 0.01" pos="0.3 0 0"/>
    </body>
  </worldbody></mujoco>"""
THIN_WALL_Q = (-1.0, 1.0)
THIN_WALL_SAMPLES = 8
THIN_WALL_FREE_BY = 0.01


def thin_wall():
    """-> (flat, dofs, pairs [1, 2], q0 [1], q1 [1])"""
    flat = mjcf.compile_mjcf(THIN_WALL_XML)
    g = flat.names["geom"].index
    return flat, S.dofs_of(flat, ("turn",)), np.array([[g("bar"), g("wall")]], dtype=np.int32), np.array([THIN_WALL_Q[0]]), np.array([THIN_WALL_Q[1]])


def without_adjacent(flat, pairs):
    """pairs [P, 2] without those whose two bodies are parent and child.  Panda's link0 / link1 collision geoms stand 1.0 mm apart whatever joint 1 does: with
    them in the list every motion is a HIT at the default slack of 1 mm, and with a smaller slack every step is a 1 mm step."""
    parent = np.asarray(flat.arrays["body_parentid"]).ravel().astype(int)
    gb = np.asarray(flat.arrays["geom_bodyid"]).ravel().astype(int)
    keep = [not (parent[gb[a]] == gb[b] or parent[gb[b]] == gb[a]) for a, b in np.asarray(pairs)]
    return np.ascontiguousarray(np.asarray(pairs)[keep], dtype=np.int32)


def segments(flat, dofs, B, K, overrides=None):
    """(q0, q1) [B, K, n] float32-rounded ends; segment (env, k) depends on (seed, env, k) only"""
    return S.candidates(flat, dofs, B, K, SEED_Q0, overrides), S.candidates(flat, dofs, B, K, SEED_Q1, overrides)


def at(q0, q1, t):
    """q(t) in fp64"""
    return q0 + t * (q1 - q0)


def at32(q0, q1, t):
    """q(t) as the kernel rounds it: fmaf(t, q1 - q0, q0) on float32 operands -- the difference rounded to float32, the product and the sum exact in float64
    (24 + 24 bits, then one float64 addition), rounded to float32 once"""
    q0, q1, t = (np.asarray(x, dtype=np.float32) for x in (q0, q1, t))
    d = (q1 - q0).astype(np.float64)
    return (t.astype(np.float64) * d + q0.astype(np.float64)).astype(np.float32)


# ---- records of the host rehearsal (tests/san/sweep_core_driver.cpp) -------------------------------------------------------------------------------------
def pack_sweep(flat, dofs, qpos, xpos, xquat, q0, q1, pairs, distmax, tol, max_iters, margin, slack, max_steps):
    """bytes of the driver's input: clearance_scenes.pack_scene with q = q0, then the sweep's own options, the bounding spheres and q1"""
    head = S.pack_scene(flat, dofs, qpos, xpos, xquat, q0, pairs, distmax, tol, max_iters)
    tail = [struct.pack("<2fi", margin, slack, max_steps), np.asarray(flat.arrays["geom_rcenter"], dtype="<f4").tobytes(),
            np.asarray(flat.arrays["geom_rbound"], dtype="<f4").tobytes(), np.asarray(q1, dtype="<f4").tobytes()]
    return head + b"".join(tail)


def unpack_sweep(blob, B, K):
    """dict of the driver's output, each [B, K(, 6)]"""
    rec = np.frombuffer(blob, dtype=np.dtype([("f", "<f4", 10), ("i", "<i4", 3)]), count=B * K)
    f, i = rec["f"].astype(np.float64), rec["i"]
    return dict(L=f[:, 0].reshape(B, K), t=f[:, 1].reshape(B, K), dist=f[:, 2].reshape(B, K), t_min=f[:, 3].reshape(B, K), fromto=f[:, 4:].reshape(B, K, 6),
                status=i[:, 0].reshape(B, K), pair=i[:, 1].reshape(B, K), steps=i[:, 2].reshape(B, K))
