"""Scene A and its seeded cases, shared by tests/test_ik_avoid_host.py (CPU, the fp64 mirror robosuite_amd/ik_avoid.py), tests/test_ik_avoid_core_host.py (CPU, the
fp32 core under sanitizers) and tests/test_ik_avoid.py (GPU, the kernels against the mirror).

Scene A: a five-hinge arm on a base at z = 0.4 -- j0 about z, j1 .. j3 about y, j4 about (0, 1, 0.2); links of 0.15 / 0.25 / 0.25 / 0.2 / 0.12 m, capsules of
radius 0.03 and a box on link 3 -- with a site 0.14 m along the last link: position targets leave two redundant dofs.  A plane, a fixed box post, and a
sphere of radius 0.07 on a FREE body, so that each env places its own obstacle through qpos.  A second free body, a small box parked far away, is what the
carried-object cases attach to the last link.

The cases of env e (the sphere is the env's, so its K problems share it): ONE q_true and target ik.fk(q_true) (position only), drawn until plain ik.solve's
answer stands FREE_MIN clear of the scene without the sphere; K start vectors q_true + 0.3 U(-1, 1); the sphere's centre 0.06 m above the origin of body l3 at
plain IK's answer from start 0; starts 1 .. K - 1 are drawn until their plain answers, too, are free without the sphere and at least HIT_MIN inside it with it.
The draws look at plain IK and the clearance mirror only, never at the solver under test.

The carried-object cases (cargo_cases): the box rides 0.27 m along the last link, beyond the site; targets drawn until plain IK's answer is free without it and
the box, held, stands inside the scene -- the post, the floor or the arm itself."""
import numpy as np

from robosuite_amd import clearance, ik, ik_avoid, mjcf
from tests import clearance_scenes as S
from tests import ik_scenes

SCENE_A_XML = """<mujoco><compiler angle="radian"/><worldbody>
  <geom name="floor" type="plane" size="2 2 0.1"/>
  <geom name="post" type="box" size="0.04 0.04 0.25" pos="0.42 0.3 0.25"/>
  <body name="l0" pos="0 0 0.4"><joint name="j0" type="hinge" axis="0 0 1" limited="true" range="-2.8 2.8"/>
    <geom name="c0" type="capsule" size="0.03" fromto="0 0 0 0 0 0.15"/>
    <body name="l1" pos="0 0 0.15"><joint name="j1" type="hinge" axis="0 1 0" limited="true" range="-2.0 2.0"/>
      <geom name="c1" type="capsule" size="0.03" fromto="0 0 0 0.25 0 0"/>
      <body name="l2" pos="0.25 0 0"><joint name="j2" type="hinge" axis="0 1 0" limited="true" range="-2.4 2.4"/>
        <geom name="c2" type="capsule" size="0.03" fromto="0 0 0 0.25 0 0"/>
        <body name="l3" pos="0.25 0 0"><joint name="j3" type="hinge" axis="0 1 0" limited="true" range="-2.4 2.4"/>
          <geom name="c3" type="capsule" size="0.03" fromto="0 0 0 0.2 0 0"/>
          <geom name="b3" type="box" size="0.03 0.045 0.02" pos="0.1 0 0"/>
          <body name="l4" pos="0.2 0 0"><joint name="j4" type="hinge" axis="0 1 0.2" limited="true" range="-2.0 2.0"/>
            <geom name="c4" type="capsule" size="0.03" fromto="0 0 0 0.12 0 0"/>
            <site name="tip" pos="0.14 0 0"/></body></body></body></body></body>
  <body name="ball" pos="1.5 1.5 1.0"><freejoint name="ballj"/><geom name="ball_g" type="sphere" size="0.07"/></body>
  <body name="cargo" pos="1.5 -1.5 1.0"><freejoint name="cargoj"/><geom name="cargo_g" type="box" size="0.05 0.04 0.04"/></body>
</worldbody></mujoco>"""

SEED = 4100
D_SAFE, MAX_ITERS = 0.04, 60
OPTS = dict(d_safe=D_SAFE, max_iters=MAX_ITERS)      # everything else: ik_avoid.DEFAULTS
SPHERE_UP = 0.06
FREE_MIN, HIT_MIN = 0.06, 0.02      # a drawn case: plain IK's answer at least FREE_MIN clear of the scene without the sphere, at least HIT_MIN inside it with it
CAP = 0.40           # at most this share of the cases may be left out (the mirror alone left out 25 to 33 %)
_CACHE = {}


def scene_a():
    """-> dict(flat, site, dofs, pairs, l3, ball_qadr)"""
    if "a" not in _CACHE:
        flat = mjcf.compile_mjcf(SCENE_A_XML)
        dofs = S.dofs_of(flat, [f"j{i}" for i in range(5)])
        ja = int(np.asarray(flat.arrays["jnt_qposadr"]).ravel()[flat.names["joint"].index("ballj")])
        _CACHE["a"] = dict(flat=flat, site=flat.names["site"].index("tip"), dofs=dofs, pairs=clearance.default_pairs(flat, dofs), l3=flat.names["body"].index("l3"),
                           ball_qadr=ja, ball=flat.names["body"].index("ball"))
    return _CACHE["a"]


def cases(B, K, seed=SEED):
    """-> dict(qpos [B, nq], pos [B, K, 3], q_init [B, K, n], q_plain [B, K, n]): per env one target and K start vectors (the module's docstring), everything
    rounded to float32 (what the device is handed), as float64; q_plain is plain ik.solve's answer of every start, with the sphere where it cannot matter."""
    key = ("cases", B, K, seed)
    if key in _CACHE:
        return _CACHE[key]
    a = scene_a()
    flat, site, dofs = a["flat"], a["site"], a["dofs"]
    n = len(dofs)
    q0 = np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel()
    lo, hi, _ = ik_scenes.ranges(flat, dofs)
    out = dict(qpos=np.tile(q0, (B, 1)), pos=np.zeros((B, K, 3)), q_init=np.zeros((B, K, n)), q_plain=np.zeros((B, K, n)))
    plain = lambda p, qi: ik.solve(flat, q0, site, dofs, p, None, qi, max_iters=MAX_ITERS)      # noqa: E731
    free = lambda qp, q: clearance.clearance(flat, qp, dofs, q, a["pairs"])[0]      # noqa: E731
    for e in range(B):
        rng = np.random.default_rng([seed, e])
        for _ in range(200):      # a target whose plain answer stands free of the scene WITHOUT the sphere (qpos0 keeps it far away)
            c = ik_scenes.cases(flat, site, dofs, 1, int(rng.integers(1 << 30)), quat=False)
            q, _, _, ok = plain(c["pos"][0], c["q_init"][0])
            if ok and free(q0, q) >= FREE_MIN and free(q0, c["q_true"][0]) >= FREE_MIN:
                break
        else:
            raise RuntimeError("scene A: no free target drawn")
        out["pos"][e], out["q_init"][e, 0], out["q_plain"][e, 0] = c["pos"][0], c["q_init"][0], q
        xp, _ = clearance.fk(flat, q0, dofs, q)
        out["qpos"][e, a["ball_qadr"]:a["ball_qadr"] + 3] = xp[a["l3"]] + np.array([0.0, 0.0, SPHERE_UP])
        out["qpos"][e] = S.f32(out["qpos"][e])
        for k in range(1, K):      # further starts whose plain answers are free without the sphere and inside it with it
            for _ in range(200):
                qi = S.f32(np.clip(c["q_true"][0] + 0.3 * rng.uniform(-1, 1, n), lo, hi))
                q, _, _, ok = plain(c["pos"][0], qi)
                if ok and free(q0, q) >= FREE_MIN and free(out["qpos"][e], q) <= -HIT_MIN:
                    break
            else:
                raise RuntimeError("scene A: no start vector drawn")
            out["q_init"][e, k], out["q_plain"][e, k] = qi, q
    _CACHE[key] = out
    return out


def solve_case(c, e, k, **opts):
    a = scene_a()
    return ik_avoid.solve(a["flat"], c["qpos"][e], a["site"], a["dofs"], c["pos"][e, k], None, c["q_init"][e, k], a["pairs"], **dict(OPTS, **opts))


def held(B, K, seed=SEED, **opts):
    """bool [B, K]: the cases the device is held to (ik_avoid.held_to, the mirror alone)"""
    key = ("held", B, K, seed, tuple(sorted(opts.items())))
    if key not in _CACHE:
        a, c = scene_a(), cases(B, K, seed)
        _CACHE[key] = np.array([[ik_avoid.held_to(a["flat"], c["qpos"][e], a["site"], a["dofs"], c["pos"][e, k], None, c["q_init"][e, k], a["pairs"], **dict(OPTS, **opts))
                                 for k in range(K)] for e in range(B)])
    return _CACHE[key]


def plain_clearance(c):
    """[B, K]: the mirror's clearance at plain IK's answers"""
    a = scene_a()
    B, K = c["pos"].shape[:2]
    return np.array([[clearance.clearance(a["flat"], c["qpos"][e], a["dofs"], c["q_plain"][e, k], a["pairs"])[0] for k in range(K)] for e in range(B)])


CARGO_REL = np.array([0.27, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])      # the box in l4's frame: 13 cm beyond the site


def cargo_attach():
    a = scene_a()
    return [(a["flat"].names["body"].index("cargo"), a["flat"].names["body"].index("l4"))]


def cargo_cases(B, K, seed=SEED + 77):
    """-> dict(qpos [B, nq] = qpos0, pos [B, K, 3], q_init [B, K, n], pairs = default_pairs with the attachment, rel [B, 1, 7], held bool [B, 1]): the first half
    of the envs holds the box, the second half does not and is handed the first half's problems again.  A drawn case: plain IK's answer at least FREE_MIN clear
    without the box, at least HIT_MIN inside the scene with the box held, and the mirror, with the box held, finishes it (ik_avoid.held_to)."""
    key = ("cargo", B, K, seed)
    if key in _CACHE:
        return _CACHE[key]
    a = scene_a()
    flat, site, dofs = a["flat"], a["site"], a["dofs"]
    att = cargo_attach()
    pairs = clearance.default_pairs(flat, dofs, att)
    q0 = S.f32(np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel())
    half = B // 2
    out = dict(qpos=np.tile(q0, (B, 1)), pos=np.zeros((B, K, 3)), q_init=np.zeros((B, K, len(dofs))), pairs=pairs, rel=np.tile(CARGO_REL, (B, 1, 1)),
               held=np.arange(B)[:, None] < half)
    rng = np.random.default_rng(seed)
    for e in range(half):
        for k in range(K):
            for _ in range(1000):
                c = ik_scenes.cases(flat, site, dofs, 1, int(rng.integers(1 << 30)), quat=False)
                q, _, _, ok = ik.solve(flat, q0, site, dofs, c["pos"][0], None, c["q_init"][0], max_iters=MAX_ITERS)
                if not ok or clearance.clearance(flat, q0, dofs, q, a["pairs"])[0] < FREE_MIN:
                    continue
                if clearance.clearance(flat, q0, dofs, q, pairs, attach=att, held=[True], rel=CARGO_REL[None])[0] > -HIT_MIN:
                    continue
                if ik_avoid.held_to(flat, q0, site, dofs, c["pos"][0], None, c["q_init"][0], pairs, attach=att, held=[True], rel=CARGO_REL[None], **OPTS):
                    break
            else:
                raise RuntimeError("scene A: no carried-object case drawn")
            out["pos"][e, k] = out["pos"][e + half, k] = c["pos"][0]
            out["q_init"][e, k] = out["q_init"][e + half, k] = c["q_init"][0]
    _CACHE[key] = out
    return out
