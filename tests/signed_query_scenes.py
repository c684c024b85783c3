"""The sunk starts shared by tests/test_signed_queries_host.py (CPU, the fp64 mirrors) and tests/test_signed_ik_avoid.py (GPU, solve_ik_avoid(signed=True) against
them): IK problems whose START vector sits in a general convex overlap with the target already reached -- the robot's current, touching configuration.  CPU
only; the draws look at the mirrors only, never at the solver under test.

Scene A of tests/ik_avoid_scenes.py, B = 20 envs x K = 4 starts = 80 problems: a full wavefront and a partial one.  d_safe = penetration_scenes.ARM_D_SAFE,
max_iters = 60.  Env e: a base configuration at least FREE_MIN clear of the scene; the cargo box placed, through qpos, touching geom b3 (even e: box x box, the
descent runs) or c2 (odd e: capsule x box, the exact branch) along the pair's GJK normal and pushed ARM_SINK further -- the recipe of penetration_scenes.arm_cases
-- accepted if the signed mirror's smallest distance lies in ARM_DEPTH.  Start 0 is the base configuration, starts 1 .. 3 the base shaken by ARM_SHAKE, drawn
until still in ARM_DEPTH.  Each problem's target is the site position AT ITS OWN START, rounded to float32: the pose error is zero, only the null space acts."""
import numpy as np

from robosuite_amd import clearance, distance as D, ik, ik_avoid
from tests import distance_scenes as S
from tests import ik_avoid_scenes as IA
from tests import ik_scenes
from tests import penetration_scenes as Q

SEED = 6100
B, K = 20, 4
D_SAFE, MAX_ITERS = Q.ARM_D_SAFE, 60
OPTS = dict(d_safe=D_SAFE, max_iters=MAX_ITERS)
FREE_MIN = 0.06
SUNK_INTO = ("b3", "c2")      # even envs, odd envs
CAP = IA.CAP                  # at most this share of the cases may be left out
_CACHE = {}


def smallest(flat, qpos, dofs, q, pairs, params, signed=True):
    """the smallest per-pair distance of one candidate on the mirror at its reference settings, and the per-pair (dist, status)"""
    d, _, st = clearance._pair_distances(flat, qpos, dofs, q, pairs, 1.0, Q.REF["tol"], Q.REF["max_iters"], params, None, None, None, None, None, False, signed)[1:4]
    return float(d.min()), d, st


def cases(nb=B, nk=K, seed=SEED):
    """-> dict(flat, site, dofs, pairs, qpos [B, nq], q_init [B, K, n], pos [B, K, 3], depth [B, K] the signed mirror's smallest distance at the start, nneg int
    [B, K] how many pairs are below zero there), everything rounded to float32, as float64"""
    key = ("cases", nb, nk, seed)
    if key in _CACHE:
        return _CACHE[key]
    a = IA.scene_a()
    flat, site, dofs, pairs = a["flat"], a["site"], a["dofs"], a["pairs"]
    n = len(dofs)
    lo, hi, _ = ik_scenes.ranges(flat, dofs, None)
    params = S.params32(flat)
    q0 = S.f32(np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel())
    ca = int(np.asarray(flat.arrays["jnt_qposadr"]).ravel()[flat.names["joint"].index("cargoj")])
    g_cargo, cargo = flat.names["geom"].index("cargo_g"), flat.names["body"].index("cargo")
    out = dict(flat=flat, site=site, dofs=dofs, pairs=pairs, qpos=np.tile(q0, (nb, 1)), q_init=np.zeros((nb, nk, n)), pos=np.zeros((nb, nk, 3)),
               depth=np.zeros((nb, nk)), nneg=np.zeros((nb, nk), dtype=int))
    inside = lambda d: -Q.ARM_DEPTH[1] <= d <= -Q.ARM_DEPTH[0]      # noqa: E731
    for e in range(nb):
        rng = np.random.default_rng([seed, e])
        g_arm = flat.names["geom"].index(SUNK_INTO[e % 2])
        while True:
            qb = S.f32(rng.uniform(lo, hi))
            if not clearance.clearance(flat, q0, dofs, qb, pairs, params=params)[0] >= FREE_MIN:
                continue
            xpos, xquat = clearance.fk(flat, q0, dofs, qb)
            ga = D.world_geoms(flat, xpos, xquat, [g_arm], params)[g_arm]
            v = rng.normal(size=3)
            v /= np.linalg.norm(v)
            cq = Q._rand_quat(rng)
            cpos = np.array(ga["pos"]) + 0.5 * v
            xpos[cargo], xquat[cargo] = cpos, cq
            gb = D.world_geoms(flat, xpos, xquat, [g_cargo], params)[g_cargo]
            d, ft, st = D.pair(ga, gb, np.inf, **Q.REF)
            if st != D.OK or d < 0.1:
                continue
            cpos = cpos - (np.array(ft[3:]) - np.array(ft[:3])) / d * (d + Q.ARM_SINK)
            out["qpos"][e, ca:ca + 7] = S.f32(np.concatenate([cpos, cq]))
            if inside(smallest(flat, out["qpos"][e], dofs, qb, pairs, params)[0]):
                break
        for k in range(nk):
            for _ in range(200):
                q = S.f32(qb + (rng.uniform(-1, 1, n) * Q.ARM_SHAKE if k else 0.0))
                dmin, d, _ = smallest(flat, out["qpos"][e], dofs, q, pairs, params)
                if inside(dmin):
                    break
            else:
                raise RuntimeError(f"sunk starts: no start drawn (env {e}, start {k}, last {dmin})")
            out["q_init"][e, k], out["depth"][e, k], out["nneg"][e, k] = q, dmin, int((d < 0).sum())
            out["pos"][e, k] = S.f32(ik.fk(flat, clearance.candidate_qpos(flat, out["qpos"][e], dofs, q), site)[0])
    _CACHE[key] = out
    return out


def solve_case(c, e, k, signed=True, **opts):
    return ik_avoid.solve(c["flat"], c["qpos"][e], c["site"], c["dofs"], c["pos"][e, k], None, c["q_init"][e, k], c["pairs"], params=S.params32(c["flat"]),
                          **(dict(signed=True) if signed else {}), **dict(OPTS, **opts))


def held(c):
    """bool [B, K]: the cases the device is held to -- ik_avoid.held_to(signed=True), the mirror alone"""
    key = ("held", id(c))
    if key not in _CACHE:
        nb, nk = c["pos"].shape[:2]
        _CACHE[key] = np.array([[ik_avoid.held_to(c["flat"], c["qpos"][e], c["site"], c["dofs"], c["pos"][e, k], None, c["q_init"][e, k], c["pairs"],
                                                  params=S.params32(c["flat"]), signed=True, **OPTS) for k in range(nk)] for e in range(nb)])
    return _CACHE[key]


def stuck(c):
    """bool [B, K]: the starts at which the UNSIGNED cost has nnear == noverlap > 0 on the mirror -- every near pair a general overlap: cost and no push"""
    key = ("stuck", id(c))
    if key not in _CACHE:
        nb, nk = c["pos"].shape[:2]
        r = [[clearance.collision_cost(c["flat"], c["qpos"][e], c["dofs"], c["q_init"][e, k], c["pairs"], D_SAFE, params=S.params32(c["flat"]))[2:] for k in range(nk)]
             for e in range(nb)]
        _CACHE[key] = np.array([[nn == no and no > 0 for nn, no in row] for row in r])
    return _CACHE[key]
