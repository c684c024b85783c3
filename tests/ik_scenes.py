"""Arms, chains and seeded cases shared by tests/test_ik_host.py (CPU, the fp64 mirror robosuite_amd/ik.py) and tests/test_ik.py (GPU, the kernel against it)."""
import numpy as np

from robosuite_amd import ik, mjcf
from tests import capacity_models
from tests.util import load_golden

FREE_RANGE = 1.5      # an unlimited joint is sampled within +- this of qpos0 (rad / m)

# hinge, slide, hinge: position only, n = 3.  One joint per body (a batch is only created for such a model); anchors off the body origins, axes off
# the frame axes, a `ref` on two of the joints (qpos0 offsets).
CHAIN3_XML = """<mujoco><compiler angle="radian"/><worldbody><geom name="floor" type="plane" size="2 2 0.1"/>
  <body name="a" pos="0.1 -0.2 0.9" euler="0.2 -0.1 0.3"><joint name="h0" type="hinge" axis="0.2 1 0.1" pos="0.02 0.01 -0.03" limited="true" range="-1.8 1.6" ref="0.15"/>
    <geom type="capsule" size="0.02" fromto="0 0 0 0.3 0 0" contype="0" conaffinity="0"/>
    <body name="b" pos="0.3 0.02 0.01" euler="-0.3 0.2 0.1"><joint name="s1" type="slide" axis="1 0.3 -0.2" limited="true" range="-0.15 0.25" ref="0.05"/>
      <geom type="capsule" size="0.02" fromto="0 0 0 0.2 0 0" contype="0" conaffinity="0"/>
      <body name="c" pos="0.2 0 0.03" euler="0.1 0.4 -0.2"><joint name="h2" type="hinge" axis="0.1 0.2 1" pos="-0.01 0.02 0.0" limited="true" range="-2.0 2.0"/>
        <geom type="capsule" size="0.02" fromto="0 0 0 0.25 0 0" contype="0" conaffinity="0"/>
        <site name="tip" pos="0.25 0.03 -0.02" euler="0.3 0.1 0.2"/></body></body></body>
</worldbody></mujoco>"""

# one hinge, a site off its axis: the targets lie on the site's circle
HINGE1_XML = """<mujoco><compiler angle="radian"/><worldbody><geom name="floor" type="plane" size="2 2 0.1"/>
  <body name="a" pos="0 0.1 0.8" euler="0.1 0.2 -0.3"><joint name="h0" type="hinge" axis="0.3 -0.2 1" pos="0.01 0 0.02" limited="true" range="-2.5 2.5"/>
    <geom type="capsule" size="0.02" fromto="0 0 0 0.3 0 0" contype="0" conaffinity="0"/>
    <site name="tip" pos="0.3 0.05 0.04"/></body>
</worldbody></mujoco>"""

_CACHE = {}


def scene(name):
    """-> dict(flat, cfg, site, dofs, quat): the arm or chain, the site solved for, the controlled dofs, whether the target carries an orientation"""
    if name in _CACHE:
        return _CACHE[name]
    cfg = None
    if name == "panda":
        _, cfg, flat = load_golden("seed0_gentle")
        s = dict(site=3, dofs=list(range(7)), quat=True)
    elif name == "baxter_left":      # the 64-body configuration; the chain passes bodies whose other children carry the right arm
        _, cfg, flat = load_golden("ctl_joint_velocity", "peg_baxter")
        s = dict(site=11, dofs=list(range(7, 14)), quat=True)
    elif name == "baxter_right":
        _, cfg, flat = load_golden("ctl_joint_velocity", "peg_baxter")
        s = dict(site=3, dofs=list(range(7)), quat=True)
    elif name == "iiwa":
        _, cfg, flat = load_golden("seed0_full", "pickplace_iiwa")
        s = dict(site=2, dofs=list(range(7)), quat=True)
    elif name == "chain3":
        flat = mjcf.compile_mjcf(CHAIN3_XML)
        s = dict(site=flat.names["site"].index("tip"), dofs=[0, 1, 2], quat=False)
    elif name == "hinge1":
        flat = mjcf.compile_mjcf(HINGE1_XML)
        s = dict(site=flat.names["site"].index("tip"), dofs=[0], quat=False)
    elif name == "chain16":          # n = RSIM_JNT_MAX: sixteen hinges in series (tests/capacity_models.py), every fifth limited to +- 0.4 rad
        flat = mjcf.compile_mjcf(capacity_models.model_xml(16, 0))
        s = dict(site=flat.names["site"].index("tip"), dofs=list(range(16)), quat=True)
    else:
        raise KeyError(name)
    _CACHE[name] = dict(s, flat=flat, cfg=cfg, name=name)
    return _CACHE[name]


def ranges(flat, dofs, overrides=None):
    """(lo, hi, qpos addresses) of the controlled joints: jnt_range where limited, qpos0 +- FREE_RANGE otherwise"""
    jid = _joints_of(flat, dofs)
    t = ik._tables(flat, overrides)
    lim = np.asarray(flat.arrays["jnt_limited"]).ravel().astype(bool)[jid]
    qa = np.asarray(flat.arrays["jnt_qposadr"]).ravel().astype(int)[jid]
    lo = np.where(lim, t["jnt_range"][jid, 0], t["qpos0"][qa] - FREE_RANGE)
    hi = np.where(lim, t["jnt_range"][jid, 1], t["qpos0"][qa] + FREE_RANGE)
    return lo, hi, qa


def _joints_of(flat, dofs):
    dadr = np.asarray(flat.arrays["jnt_dofadr"]).ravel().astype(int)
    return np.array([int(np.flatnonzero(dadr == d)[0]) for d in dofs])


def cases(flat, site, dofs, n, seed, spread=0.3, qpos=None, overrides=None, quat=True):
    """n seeded cases: q_true uniform in the middle 90 % of each joint range, the target ik.fk(q_true) (reachable by construction), q_init =
    clip(q_true + spread U(-1, 1)).  -> dict(q_true [n, ndof], pos [n, 3], quat [n, 4] or None, q_init [n, ndof]), everything rounded to float32 (what the
    device is handed), as float64."""
    rng = np.random.default_rng(seed)
    lo, hi, qa = ranges(flat, dofs, overrides)
    base = np.asarray(flat.arrays["qpos0"] if qpos is None else qpos, dtype=np.float64).ravel()
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    out = dict(q_true=[], pos=[], quat=[], q_init=[])
    for _ in range(n):
        qt = mid + 0.9 * half * rng.uniform(-1, 1, len(dofs))
        q = base.copy()
        q[qa] = qt
        p, R = ik.fk(flat, q, site, overrides)
        out["q_true"].append(qt); out["pos"].append(p); out["quat"].append(mjcf.mat2quat(R))
        out["q_init"].append(np.clip(qt + spread * rng.uniform(-1, 1, len(dofs)), lo, hi))
    out = {k: np.asarray(v).astype(np.float32).astype(np.float64) for k, v in out.items()}
    if not quat:
        out["quat"] = None
    return out


def well(flat, qpos, site, dofs, c, overrides=None, **opts):
    """bool [n]: the well-conditioned cases (ik.well_conditioned, the mirror alone)"""
    return np.array([ik.well_conditioned(flat, qpos, site, dofs, c["pos"][i], None if c["quat"] is None else c["quat"][i], c["q_init"][i], overrides, **opts)
                     for i in range(len(c["pos"]))])


def case_seed(name, env):
    """the seed of env `env`'s cases of a scene: the host test of the 10 % cap and the device tests draw the same cases"""
    return 1000 + 10 * sorted(("panda", "baxter_left", "baxter_right", "iiwa", "chain3", "hinge1", "chain16", "panda_per_env")).index(name) + env
