"""Scenes, closed-form cases, the band and the certificate shared by tests/test_penetration_host.py (CPU, the mirror robosuite_amd/penetration.py),
tests/test_penetration_core_host.py (CPU, the fp32 core under sanitizers) and tests/test_penetration.py (GPU, k_dist_signed against the mirror).

Scene P (and P2, a second cast): eight free bodies (the compiled kernel configurations carry eight articulated trees) of the six convex geom types.  Every env deals them into two
clusters of four -- a centre and three satellites -- by a permutation of its own, so that over the envs every type combination meets.  A satellite is built the way the fp64 prototype found necessary: posed
disjoint from its centre, brought to touching along the pair's GJK normal, then pushed T = 0.5, 2 or 5 mm further (setting a width along an arbitrary direction
does not produce an overlap).  The pair list is all 28 pairs: satellites of one cluster may or may not overlap each other, clusters are a metre apart."""
import os

import numpy as np

from robosuite_amd import distance as D
from robosuite_amd import mjcf
from robosuite_amd import penetration as P
from tests import distance_scenes as S
from tests import raycast_scenes as R

T_PUSH = (0.5e-3, 2e-3, 5e-3)
SHALLOW = 1e-4        # a depth below this is in the band
SPLIT = 1e-5          # ... and so is a pair whose descents from four other tilts of the seed end further apart than this
BAND_TILT = 1e-2
BAND_DIRS = ((-0.6, 0.8), (-0.8, -0.6), (0.6, -0.8), (1.0, 0.0))
BAND_SHARE = 0.10
DISTMAX = 0.5
REF = dict(tol=1e-10, max_iters=1000)      # the mirror as a reference, as distance_scenes.REF

ICO = [tuple(0.07 * x for x in v) for v in P.icosphere(0)]      # a 12-vertex hull
WEDGE = [(-0.08, -0.05, -0.03), (0.08, -0.05, -0.03), (0.08, 0.05, -0.03), (-0.08, 0.05, -0.03), (-0.03, -0.02, 0.05), (0.04, 0.0, 0.06), (0.0, 0.03, 0.04)]
# two casts of eight: the first has two boxes and two hulls, the second two cylinders and two ellipsoids, so that every same-type pair meets in one of them
BODIES = {"P": (("box", 'type="box" size="0.08 0.06 0.04"'), ("box2", 'type="box" size="0.05 0.09 0.07"'),
                ("cyl", 'type="cylinder" size="0.05 0.08"'), ("ell", 'type="ellipsoid" size="0.09 0.05 0.07"'),
                ("ico", 'type="mesh" mesh="ico"'), ("wedge", 'type="mesh" mesh="wedge"'),
                ("sph", 'type="sphere" size="0.06"'), ("cap", 'type="capsule" size="0.03 0.08"')),
          "P2": (("cyl", 'type="cylinder" size="0.05 0.08"'), ("disc", 'type="cylinder" size="0.09 0.02"'),
                 ("ell", 'type="ellipsoid" size="0.09 0.05 0.07"'), ("ell2", 'type="ellipsoid" size="0.04 0.06 0.1"'),
                 ("box", 'type="box" size="0.08 0.06 0.04"'), ("wedge", 'type="mesh" mesh="wedge"'),
                 ("sph2", 'type="sphere" size="0.035"'), ("cap2", 'type="capsule" size="0.05 0.04"'))}
SEEDS = {"P": 7, "P2": 8}
TETRA = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / np.sqrt(3.0)


def scene_p_xml(cast="P"):
    bodies = "".join(f'<body name="b_{n}" pos="{0.4 * i} 0 0.5"><freejoint/><geom name="{n}" {spec}/></body>' for i, (n, spec) in enumerate(BODIES[cast]))
    return ('<mujoco><compiler angle="radian"/><asset><mesh name="ico" file="ico.obj"/><mesh name="wedge" file="wedge.obj"/></asset><worldbody>'
            + bodies + "</worldbody></mujoco>")


def scene_p(tmpdir, cast="P"):
    R.write_obj(os.path.join(str(tmpdir), "ico.obj"), ICO)
    R.write_obj(os.path.join(str(tmpdir), "wedge.obj"), WEDGE)
    return mjcf.compile_mjcf(scene_p_xml(cast), asset_dir=str(tmpdir))


def _rand_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _geom_at(flat, g, pos, quat):
    """mirror geom of free body g's geom (no offset on its body) at a body pose"""
    gt = int(np.asarray(flat.arrays["geom_type"]).ravel()[g])
    size = np.asarray(flat.arrays["geom_size"], dtype=np.float64).reshape(-1, 3)[g]
    return D.make_geom(gt, size, pos, np.asarray(quat, dtype=np.float64), D.mesh_verts(flat, g) if gt == mjcf.GEOM_MESH else None)


def scene_p_qpos(flat, B, seed=SEEDS["P"]):
    """[B, nq]; env e depends on (seed, e) only"""
    ng = int(flat.ngeom)
    assert ng == 8 and int(flat.nq) == 7 * ng
    out = np.zeros((B, 7 * ng))
    for e in range(B):
        rng = np.random.default_rng([seed, e])
        perm = rng.permutation(ng)
        for c in range(2):
            centre, sats = int(perm[4 * c]), [int(x) for x in perm[4 * c + 1:4 * c + 4]]
            cpos, cq = np.array([1.0 * c, 0.0, 0.5]) + rng.uniform(-0.05, 0.05, 3), _rand_quat(rng)
            out[e, 7 * centre:7 * centre + 7] = np.concatenate([cpos, cq])
            gc = _geom_at(flat, centre, cpos, cq)
            u0 = _rand_quat(rng)
            for j, s in enumerate(sats):
                # three of the four directions of a tetrahedron, turned at random, each shaken
                u = S._rot(u0) @ TETRA[j] + rng.uniform(-0.25, 0.25, 3)
                u /= np.linalg.norm(u)
                sq = _rand_quat(rng)
                spos = cpos + 0.6 * u
                d, ft, st = D.pair(gc, _geom_at(flat, s, spos, sq), np.inf, **REF)
                assert st == D.OK and d > 0.1
                n = (np.array(ft[3:]) - np.array(ft[:3])) / d
                spos = spos - n * (d + T_PUSH[(e + j) % 3])
                out[e, 7 * s:7 * s + 7] = np.concatenate([spos, sq])
    return out


def all_pairs(flat):
    return S.all_pairs(flat)


def env_geoms(flat, xpos, xquat):
    """{geom id: mirror geom} of one env with the model's geometry rounded to fp32, as the device holds it"""
    return D.world_geoms(flat, xpos, xquat, np.arange(int(flat.ngeom)), S.params32(flat))


# ---- the band and the reference ----------------------------------------------------------------------------------------------------------------------------
def in_band(g1, g2, depth, opts=None):
    """defined from the mirror alone: a depth below SHALLOW, or descents from the seed tilted in four other directions by BAND_TILT that end at depths more than
    SPLIT apart (two minima within reach of rounding)"""
    if depth < SHALLOW:
        return True
    ends = [depth]
    for dr in BAND_DIRS:
        ends.append(-P.pair_signed(g1, g2, np.inf, **REF, n0=P.seed(g1, g2, BAND_TILT, dr), **(opts or {}))[0])
    return max(ends) - min(ends) > SPLIT


def reference_pairs(recs, distmax, opts=None):
    """recs: list of (g1, g2).  -> {"dist", "fromto", "status": the mirror's signed result at `distmax`, "plain": distance.pair's status (the overlap bit says which
    pairs the signed call changes), "band": bool, "steps": projections, "normal": the mirror's n (zeros where it did not descend and the cores met no radius)}"""
    n = len(recs)
    out = {"dist": np.zeros(n), "fromto": np.zeros((n, 6)), "status": np.zeros(n, dtype=np.int32), "plain": np.zeros(n, dtype=np.int32),
           "band": np.zeros(n, dtype=bool), "steps": np.zeros(n, dtype=np.int32), "normal": np.zeros((n, 3))}
    for i, (a, b) in enumerate(recs):
        out["plain"][i] = D.pair(a, b, distmax, **REF)[2]
        info = {}
        out["dist"][i], out["fromto"][i], out["status"][i] = P.pair_signed(a, b, distmax, **REF, info=info, **(opts or {}))
        if out["plain"][i] & D.OVERLAP:
            out["steps"][i], out["normal"][i] = info["steps"], info["normal"]
            out["band"][i] = in_band(a, b, -out["dist"][i], opts)
    return out


def reference(flat, xpos, xquat, pairs, distmax, opts=None):
    """the same over envs: arrays [B, P(, ...)], and "recs": the (g1, g2) list in env-major order"""
    recs = []
    for e in range(len(xpos)):
        G = env_geoms(flat, xpos[e], xquat[e])
        recs += [(G[int(a)], G[int(b)]) for a, b in pairs]
    ref = reference_pairs(recs, distmax, opts)
    B, Pn = len(xpos), len(pairs)
    out = {k: v.reshape((B, Pn) + v.shape[1:]) for k, v in ref.items()}
    out["recs"] = recs
    return out


# ---- the certificate of a signed overlap -------------------------------------------------------------------------------------------------------------------
def certificate(g1, g2, dist, fromto, n=None):
    """residuals of a reported overlap, fp64: (| -dist - delta(n) |, h_A(n) - n . p1, h_B(-n) + n . p2, |p2 - p1 - dist n|); n: the reported normal, or
    (p2 - p1) / dist -- the gradient formula's -- when the caller has none"""
    p1, p2 = np.asarray(fromto[:3], dtype=np.float64), np.asarray(fromto[3:], dtype=np.float64)
    n = (p2 - p1) / dist if n is None else np.asarray(n, dtype=np.float64)
    n = n / np.linalg.norm(n)
    nt = tuple(float(x) for x in n)
    return (abs(-dist - P.support_width(g1, g2, nt)), S.h_value(g1, n) - float(n @ p1), S.h_value(g2, -n) + float(n @ p2),
            float(np.linalg.norm(p2 - p1 - dist * n)))


def separates(g1, g2, dist, n, slack=1e-6):
    """geom2 moved by (depth + slack) n is disjoint from geom1, on distance.pair"""
    moved = dict(g2, pos=tuple(np.asarray(g2["pos"]) + (-dist + slack) * np.asarray(n)))
    d, _, st = D.pair(g1, moved, np.inf, **REF)
    return not (st & D.OVERLAP) and d > 0


# ---- closed forms ------------------------------------------------------------------------------------------------------------------------------------------
def closed_forms():
    """[(name, g1, g2, depth, normal)]: every geom1 is the box of half sizes (0.1, 0.08, 0.06) at the origin, every answer its top face"""
    g = lambda t, size, pos, verts=None: D.make_geom(t, np.resize(np.asarray(size, dtype=float), 3), pos, np.array([1.0, 0, 0, 0]), verts)      # noqa: E731
    box = g(mjcf.GEOM_BOX, [0.1, 0.08, 0.06], [0, 0, 0])
    up = (0.0, 0.0, 1.0)
    ico_low = 0.07 * max(-v[2] for v in P.icosphere(0))
    return [("box on box: the least face overlap", box, g(mjcf.GEOM_BOX, [0.05, 0.07, 0.09], [0.02, 0.01, 0.06 + 0.09 - 0.003]), 0.003, up),
            ("sphere centre inside the box", box, g(mjcf.GEOM_SPHERE, [0.03], [0.02, 0.01, 0.05]), 0.01 + 0.03, up),
            ("ellipsoid sunk axis-first", box, g(mjcf.GEOM_ELLIPSOID, [0.05, 0.03, 0.08], [0.02, 0.01, 0.06 + 0.08 - 0.004]), 0.004, up),
            ("cylinder sunk axis-first", box, g(mjcf.GEOM_CYLINDER, [0.04, 0.05], [0.02, 0.01, 0.06 + 0.05 - 0.004]), 0.004, up),
            ("capsule segment across the face", box, g(mjcf.GEOM_CAPSULE, [0.02, 0.05], [0.02, 0.01, 0.07]), 0.04 + 0.02, up),
            ("12-vertex hull on the face", box, g(mjcf.GEOM_MESH, [0, 0, 0], [0.02, 0.01, 0.06 + ico_low - 0.003], np.array(P.icosphere(0)) * 0.07), 0.003, up)]


# ---- records of the host rehearsal (tests/san/pen_core_driver.cpp) -------------------------------------------------------------------------------------------
def pack_records(geom_pairs, distmax, tol, max_iters, pen_tol, pen_iters, offset):
    """bytes of the driver's input: distance_scenes.pack_records with the three penetration options behind the header"""
    import struct

    blob = S.pack_records(geom_pairs, distmax, tol, max_iters)
    return blob[:16] + struct.pack("<fif", pen_tol, pen_iters, offset) + blob[16:]


def unpack_results(blob, n):
    """(dist [n], fromto [n, 6], normal [n, 3], status [n], projections [n]) of the driver's output"""
    rec = np.frombuffer(blob, dtype=np.dtype([("f", "<f4", 10), ("i", "<i4", 2)]), count=n)
    f = rec["f"].astype(np.float64)
    return f[:, 0], f[:, 1:7], f[:, 7:], rec["i"][:, 0].astype(np.int32), rec["i"][:, 1].astype(np.int32)


# ---- the five-hinge arm of tests/ik_avoid_scenes.py with its cargo box as each env's obstacle -----------------------------------------------------------------
SEED_ARM = 5200
ARM_D_SAFE = 0.01                 # small, so that a sunk last link is the only near pair of many candidates
ARM_SINK = 3.5e-3                 # how far the cargo box is pushed into the last link at the env's base configuration
ARM_DEPTH = (2e-3, 5e-3)          # the depth window of a sunk candidate, on the mirror
ARM_SHAKE = 1.5e-3                # rad: a sunk candidate is the base configuration plus U(-1, 1) of this per joint
_ARM = {}


def arm_cases(B, K, seed=SEED_ARM):
    """-> dict(flat, dofs, pairs, qpos [B, nq], q [B, K, n], sunk bool [B, K]), everything rounded to float32 as float64.  Env e: a base configuration clear of the
    scene by 2 cm, the cargo box brought to touching the last link's capsule along the pair's GJK normal and pushed ARM_SINK further (as scene P's satellites).
    Odd k: the base configuration shaken by ARM_SHAKE, drawn until the mirror's deepest pair is ARM_DEPTH inside; even k: uniform in the joint ranges, drawn
    until the mirror reports no status-2 overlap.  The draws look at the mirror only."""
    from robosuite_amd import clearance
    from tests import ik_avoid_scenes as IA
    from tests import ik_scenes

    key = (B, K, seed)
    if key in _ARM:
        return _ARM[key]
    a = IA.scene_a()
    flat, dofs, pairs = a["flat"], a["dofs"], a["pairs"]
    n = len(dofs)
    lo, hi, _ = ik_scenes.ranges(flat, dofs, None)
    params = S.params32(flat)
    q0 = S.f32(np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel())
    ca = int(np.asarray(flat.arrays["jnt_qposadr"]).ravel()[flat.names["joint"].index("cargoj")])
    g_c4, g_cargo = flat.names["geom"].index("c4"), flat.names["geom"].index("cargo_g")
    l4, cargo = flat.names["body"].index("l4"), flat.names["body"].index("cargo")
    out = dict(flat=flat, dofs=dofs, pairs=pairs, qpos=np.tile(q0, (B, 1)), q=np.zeros((B, K, n)), sunk=np.zeros((B, K), dtype=bool))

    def dists(qpos, q, signed):
        return clearance._pair_distances(flat, qpos, dofs, q, pairs, 1.0, REF["tol"], REF["max_iters"], params, None, None, None, None, None, False, signed)[1:4]

    for e in range(B):
        rng = np.random.default_rng([seed, e])
        while True:      # drawn until the cargo box, placed, meets nothing but the last link
            qb = S.f32(rng.uniform(lo, hi))
            if not clearance.clearance(flat, q0, dofs, qb, pairs, params=params)[0] > 0.02:
                continue
            xpos, xquat = clearance.fk(flat, q0, dofs, qb)
            R4 = S._rot(xquat[l4])
            gc = D.world_geoms(flat, xpos, xquat, [g_c4], params)[g_c4]
            v = rng.normal(size=3)
            v /= np.linalg.norm(v)
            cq = _rand_quat(rng)
            cpos = np.array(gc["pos"]) + R4 @ np.array([0.05, 0.0, 0.0]) + 0.5 * v
            xpos[cargo], xquat[cargo] = cpos, cq
            gb = D.world_geoms(flat, xpos, xquat, [g_cargo], params)[g_cargo]
            d, ft, st = D.pair(gc, gb, np.inf, **REF)
            if st != D.OK or d < 0.1:
                continue
            cpos = cpos - (np.array(ft[3:]) - np.array(ft[:3])) / d * (d + ARM_SINK)
            out["qpos"][e, ca:ca + 7] = S.f32(np.concatenate([cpos, cq]))
            if -ARM_DEPTH[1] <= dists(out["qpos"][e], qb, True)[0].min() <= -ARM_DEPTH[0]:
                break
        for k in range(K):
            for _ in range(200):
                if k % 2:
                    q = S.f32(qb + (rng.uniform(-1, 1, n) * ARM_SHAKE if k > 1 else 0.0))
                    dmin = dists(out["qpos"][e], q, True)[0].min()
                    ok = -ARM_DEPTH[1] <= dmin <= -ARM_DEPTH[0]
                else:
                    q = S.f32(rng.uniform(lo, hi))
                    ok = not (dists(out["qpos"][e], q, False)[2] & D.OVERLAP).any()
                if ok:
                    break
            else:
                raise RuntimeError(f"arm cases: no candidate drawn (env {e}, k {k}, last {dmin if k % 2 else None})")
            out["q"][e, k], out["sunk"][e, k] = q, bool(k % 2)
    _ARM[key] = out
    return out
