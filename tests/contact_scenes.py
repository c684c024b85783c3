"""Scene, samples, fp64 reference and certificates shared by tests/test_contact_certificates_host.py (CPU, the oracle) and tests/test_contact_certificates.py
(GPU, the kernel): convex-pair and plane contacts at CONSTRUCTED depths, held to fp64 geometry that shares neither code nor algorithm with the narrow phase --
robosuite_amd/distance.py (GJK, support functions) and tests/distance_scenes.py (h_value, outside_by).  The reference is always that geometry on the poses read
back from the code under test, never the oracle or the kernel.

A sample is (pair class (i, j), case, draw s) and depends on nothing else (np.random.default_rng([SEED, i, j, s])).  Every body is parked 2.5 m from the others
and over a metre above the plane; body i goes within 0.3 m of the world origin with a random orientation, body j 0.35 m from it in a random direction with another.
The mirror gives the distance d > 0 of the two solids and the unit direction n from i's witness to j's; j is then translated by -(d + c) n, c = CASES[case]:
1 mm deep, 0.1 mm deep, 0.1 mm apart.  Plane rows do the same against the plane's signed distance.

Certificates (depth = -dist of a contact, n_c its normal frame[0], pointing from geom1 to geom2; residuals in metres, positive = violated):
  C1  apart case => the pair has no contact                                       (the mirror's distance on the read-back pose is >= 0.5e-4)
  C2  a counted deep sample => >= 1 contact: exactly 1 for MPR pairs and plane x non-box, <= 8 box-box, <= 4 plane-box; every contact names the pair, no
      other pair of the env has a contact, nothing overflowed
  C3  placement: outside_by(g1, pos), outside_by(g2, pos) <= depth / 2 + eps; the witnesses pos + n_c depth / 2 in geom1, pos - n_c depth / 2 in geom2 within eps
  C4  depth against its own normal: h1(n_c) + h2(-n_c) >= depth - eps; box-box additionally <= c + eps, one normal per manifold
  C5  exact pairs (sphere / capsule x anything, plane x anything), delta* the exact depth and n the exact normal: n_c . n > 0 and
        C5d  |depth - delta*| <= 1e-6 + eps          two-sided, the plain statement.  MPR misses this on the HIGH side by construction (below), so its
                                                     measured allowance is wide; the two one-sided bounds carry the weight:
        C5lo depth >= delta* - 1e-6 - eps            MPR never reports less than the true depth beyond its portal tolerance
        C5hi depth (n_c . n) <= delta* + eps         geometry: the witnesses differ by depth n_c and lie in the two solids, whose overlap along n is delta*
      plane rows: |n_c - n_plane| <= eps and the point at the deepest support point + depth / 2 (plane-box: one contact per corner below the plane, at most four)
  C6  general pairs: depth >= c / 4 - eps.  A sample counts only if the mirror still reports overlap with geom j moved SHIFT c = sqrt(3) c / 4 along +-x, +-y,
      +-z: the Minkowski difference then holds the octahedron of those six points and with it the ball of radius c / 4 about the origin, so the true depth is
      >= c / 4 by geometry.  (Shifts of c / 4 only certify c / (4 sqrt 3): a rehearsal with them met a cylinder rim on a box edge whose reported depth of
      0.20 mm at c = 1 mm was not wrong.)  Otherwise the sample is LEFT OUT: moving along n does not guarantee overlap at sharp vertex / edge features, whose
      tangent cone need not contain n.
  C7  (in the tests) a second forward() on the unchanged state returns the same contacts.

What MPR reports (measured, profiles/contact_certificates.txt): the closest point of the FINAL PORTAL TRIANGLE, which shrinks around the point where the ray from
the interior point through the origin leaves the Minkowski difference -- not around the foot of the perpendicular.  On curved pairs the normal is therefore pulled
towards that ray and the depth is the depth along it, delta* / cos(angle): at 1 mm the fp64 oracle's depth exceeds delta* by up to 0.43 mm (capsule x tetrahedron),
at 0.1 mm by up to 32 um (sphere x polyhedron); it is never below delta* - 0.88 um."""
import os

import numpy as np

from robosuite_amd import distance, mjcf
from tests import distance_scenes as S
from tests import raycast_scenes as R

SEED = 2039
CASES = (1e-3, 1e-4, -1e-4)                  # 1 mm deep, 0.1 mm deep, 0.1 mm apart
CASE_NAMES = ("1mm deep", "0.1mm deep", "0.1mm apart")
DRAWS = 8
REF = dict(tol=1e-10, max_iters=1000)
MPR_TOL = 1e-6                               # the narrow phase's own portal tolerance (oracle/rsim_oracle.c convex_convex, rsim_step.hip)
LEFT_OUT_CLASS, LEFT_OUT_ALL = 0.15, 0.05    # at most this share of a class x case / of all deep samples may be left out
APART_MIN = 0.5e-4
SHIFT = float(np.sqrt(3.0)) / 4                   # general pairs: overlap must survive shifts of SHIFT x c along +-x, +-y, +-z (C6)
NAMES = ("sph", "cap", "ell", "cyl", "box1", "box2", "poly", "tet")
PLANE = len(NAMES)                           # class index of the plane
PLANE_Z, PLANE_EULER = -1.2, (0.05, -0.03, 0.2)
PARK = [(2.5 * (k % 4) + 2.5, 2.5 * (k // 4) - 1.25, 1.5) for k in range(len(NAMES))]
ROUND = (mjcf.GEOM_SPHERE, mjcf.GEOM_CAPSULE)

XML = f"""<mujoco><compiler angle="radian"/>
  <asset><mesh name="poly" file="poly.obj"/><mesh name="tet" file="tet.obj"/></asset>
  <worldbody>
    <geom name="floor" type="plane" size="8 8 0.1" pos="0 0 {PLANE_Z}" euler="{PLANE_EULER[0]} {PLANE_EULER[1]} {PLANE_EULER[2]}"/>
    <body name="b_sph"><freejoint/><geom name="sph" type="sphere" size="0.05"/></body>
    <body name="b_cap"><freejoint/><geom name="cap" type="capsule" size="0.03 0.06"/></body>
    <body name="b_ell"><freejoint/><geom name="ell" type="ellipsoid" size="0.08 0.05 0.03"/></body>
    <body name="b_cyl"><freejoint/><geom name="cyl" type="cylinder" size="0.04 0.06"/></body>
    <body name="b_box1"><freejoint/><geom name="box1" type="box" size="0.06 0.04 0.03"/></body>
    <body name="b_box2"><freejoint/><geom name="box2" type="box" size="0.05 0.07 0.04"/></body>
    <body name="b_poly"><freejoint/><geom name="poly" type="mesh" mesh="poly"/></body>
    <body name="b_tet"><freejoint/><geom name="tet" type="mesh" mesh="tet"/></body>
  </worldbody></mujoco>"""


def write_meshes(tmpdir):
    R.write_obj(os.path.join(str(tmpdir), "poly.obj"), R.POLY_VERTS)
    R.write_obj(os.path.join(str(tmpdir), "tet.obj"), R.TETRA_VERTS)


def scene(tmpdir):
    write_meshes(tmpdir)
    return mjcf.compile_mjcf(XML, asset_dir=str(tmpdir))


def classes():
    """the 36 pair classes: 28 convex pairs (i < j) and the plane against each of the eight"""
    n = len(NAMES)
    return [(i, j) for i in range(n) for j in range(i + 1, n)] + [(PLANE, j) for j in range(n)]


def geom_id(flat, cls_index):
    return flat.names["geom"].index("floor" if cls_index == PLANE else NAMES[cls_index])


def body_id(flat, cls_index):
    return flat.names["body"].index("b_" + NAMES[cls_index])


def _unit(rng, n):
    v = rng.normal(size=n)
    return v / np.linalg.norm(v)


def _poses(flat, qpos):
    """(xpos, xquat) [nbody] of the free bodies of this scene from one env's qpos (body k + 1 = free joint k)"""
    nb = int(flat.nbody)
    xp, xq = np.zeros((nb, 3)), np.tile([1.0, 0, 0, 0], (nb, 1))
    q = np.asarray(qpos, dtype=np.float64).reshape(-1, 7)
    xp[1:], xq[1:] = q[:, :3], q[:, 3:]
    return xp, xq


def sample_qpos(flat, i, j, case, s):
    """qpos [nq] (fp64) of sample (class (i, j), case, draw s)"""
    rng = np.random.default_rng([SEED, i, j, s])
    q = np.zeros((len(NAMES), 7))
    for k in range(len(NAMES)):
        q[k, :3], q[k, 3:] = PARK[k], (1.0, 0, 0, 0)
    c = CASES[case]
    if i == PLANE:
        q[j, :3], q[j, 3:] = np.array([0.0, 0.0, PLANE_Z + 0.35]) + rng.uniform(-0.3, 0.3, 3) * [1, 1, 0], _unit(rng, 4)
    else:
        q[i, :3], q[i, 3:] = rng.uniform(-0.3, 0.3, 3), _unit(rng, 4)
        q[j, :3], q[j, 3:] = q[i, :3] + 0.35 * _unit(rng, 3), _unit(rng, 4)
    assert int(flat.nq) == 7 * len(NAMES)
    g1, g2 = geom_id(flat, i), geom_id(flat, j)
    G = distance.world_geoms(flat, *_poses(flat, q.ravel()), (g1, g2))
    d, ft, st = distance.pair(G[g1], G[g2], np.inf, **REF)
    assert st == distance.OK and d > 0.01, (i, j, s, d, st)
    n = (np.array(ft[3:]) - np.array(ft[:3])) / d
    q[j, :3] -= (d + c) * n
    return q.ravel()


def samples(draws=DRAWS):
    return [(i, j, case, s) for (i, j) in classes() for case in range(len(CASES)) for s in range(draws)]


def batch_qpos(flat, smp):
    return np.stack([sample_qpos(flat, *x) for x in smp])


# ---- reference and certificates of one sample ------------------------------------------------------------------------------------------------------------
def _shifted_overlap(g1, g2, h):
    for k in range(3):
        for sgn in (-1.0, 1.0):
            p = list(g2["pos"]); p[k] += sgn * h
            if not distance.pair(g1, dict(g2, pos=tuple(p)), np.inf, **REF)[2] & distance.OVERLAP:
                return False
    return True


def _box_corners(g):
    s = np.array(g["size"])
    return np.array([np.array(g["pos"]) + g["R"] @ (np.array([sx, sy, sz]) * s) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])


def kind_of(t1, t2):
    if t1 == mjcf.GEOM_PLANE:
        return "plane-box" if t2 == mjcf.GEOM_BOX else "plane"
    if t1 == mjcf.GEOM_BOX and t2 == mjcf.GEOM_BOX:
        return "box-box"
    return "round" if (t1 in ROUND or t2 in ROUND) else "general"


def evaluate(flat, smp, xpos, xquat, contacts, overflow, params=None):
    """One record per sample: {"cls", "case", "draw", "kind", "left_out", "ncon", "errors": [str] (C1, C2: structure), "res": {certificate: worst residual},
    "angle": of n_c to the exact normal (exact pairs, report only), "ratio": (h1(n_c) + h2(-n_c)) / depth (report only)}.
    contacts[e]: list of dicts (dist, pos, frame, geom1, geom2) of env e; overflow[e]: its overflow counter."""
    out = []
    for e, (i, j, case, s) in enumerate(smp):
        c = CASES[case]
        a, b = geom_id(flat, i), geom_id(flat, j)
        G = distance.world_geoms(flat, xpos[e], xquat[e], (a, b), params)
        t1, t2 = G[a]["type"], G[b]["type"]
        g1, g2 = (a, b) if t1 <= t2 else (b, a)               # the pair list orders a pair by geom type (MuJoCo's convention)
        if t1 == t2:
            g1, g2 = min(a, b), max(a, b)
        A, Bg = G[g1], G[g2]
        kind = kind_of(A["type"], Bg["type"])
        rec = {"cls": (i, j), "case": case, "draw": s, "kind": kind, "left_out": False, "errors": [], "res": {}, "angle": None, "ratio": None, "ncon": len(contacts[e])}
        out.append(rec)
        err, res = rec["errors"], rec["res"]
        if overflow[e] != 0:
            err.append(f"overflow counter {overflow[e]}")
        other = [(k["geom1"], k["geom2"]) for k in contacts[e] if (k["geom1"], k["geom2"]) != (g1, g2)]
        if other:
            err.append(f"C2 contacts of other pairs {other[:4]} (the pair is {(g1, g2)})")
        cons = [k for k in contacts[e] if (k["geom1"], k["geom2"]) == (g1, g2)]
        d, ft, st = distance.pair(A, Bg, np.inf, **REF)
        if c < 0:                                             # ---- C1
            if not (st == distance.OK and d >= APART_MIN):
                err.append(f"the mirror's distance of the apart case is {d} (status {st})")
            if cons:
                err.append(f"C1 phantom: {len(cons)} contact(s), first dist {cons[0]['dist']:.6g}, the solids are {d:.6g} m apart")
            continue
        # ---- the exact answer / the robust-overlap filter
        n_ref = delta = None
        if kind in ("plane", "plane-box"):
            n_ref, delta = np.array(A["cols"][2]), -d
        elif kind == "round":
            dc, p1, p2, flag = distance.gjk(A, Bg, REF["tol"], REF["max_iters"])
            assert flag == "ok" and dc > 0, (i, j, case, s, flag, dc)
            n_ref, delta = (np.array(p2) - np.array(p1)) / dc, distance.radius(A) + distance.radius(Bg) - dc
        else:
            if not _shifted_overlap(A, Bg, SHIFT * c):
                rec["left_out"] = True
                continue
        if delta is not None and not delta > 0:
            err.append(f"the exact depth of a deep case is {delta}")
            continue
        # ---- C2
        most = {"plane-box": 4, "box-box": 8}.get(kind, 1)
        if not 1 <= len(cons) <= most:
            err.append(f"C2 {len(cons)} contact(s) of a pair {c} deep (1..{most})")
            if not cons:
                continue
        res.update({"C3": -np.inf, "C4": -np.inf})
        normals = np.array([np.asarray(k["frame"], dtype=np.float64).reshape(3, 3)[0] for k in cons])
        for k, nc in zip(cons, normals):
            depth, pos = -float(k["dist"]), np.asarray(k["pos"], dtype=np.float64)
            if not depth >= 0:
                err.append(f"contact with dist {k['dist']} at margin 0")
            parts = (S.outside_by(A, pos) - depth / 2, S.outside_by(Bg, pos) - depth / 2, S.outside_by(A, pos + nc * depth / 2), S.outside_by(Bg, pos - nc * depth / 2))
            if max(parts) > res["C3"]:
                res["C3"], rec["c3_parts"], rec["c3_depth"] = max(parts), parts, depth
            if A["type"] == mjcf.GEOM_PLANE:                  # a half-space has a support value along its own normal only
                along = float(np.dot(n_ref, A["pos"])) + S.h_value(Bg, -n_ref)
            else:
                along = S.h_value(A, nc) + S.h_value(Bg, -nc)
            res["C4"] = max(res["C4"], depth - along)
            if kind == "box-box":
                res["C4hi"] = max(res.get("C4hi", -np.inf), along - c)
                res["C4n"] = max(res.get("C4n", 0.0), float(np.abs(nc - normals[0]).max()))
        deepest = max(cons, key=lambda k: -k["dist"])
        depth, nc = -float(deepest["dist"]), np.asarray(deepest["frame"], dtype=np.float64).reshape(3, 3)[0]
        if A["type"] != mjcf.GEOM_PLANE:
            rec["ratio"] = (S.h_value(A, nc) + S.h_value(Bg, -nc)) / depth if depth > 0 else None
        if delta is not None:                                 # ---- C5
            res["C5d" + "ab"[case]] = abs(depth - delta) - MPR_TOL      # per case: the high side grows with the depth
            res["C5lo"] = delta - depth - MPR_TOL
            res["C5hi"] = depth * float(np.dot(nc, n_ref)) - delta
            rec["signed_depth_err"] = depth - delta
            if not float(np.dot(nc, n_ref)) > 0:
                err.append(f"C5 normal against the exact one: n_c . n = {float(np.dot(nc, n_ref)):.4f}")
            rec["angle"] = float(np.arccos(np.clip(np.dot(nc, n_ref), -1.0, 1.0)))
            if kind == "plane":
                sp = np.array(distance.support_full(Bg, tuple(-n_ref)))
                res["C5n"] = float(np.abs(normals - n_ref).max())
                res["C5p"] = float(np.abs(np.asarray(deepest["pos"], dtype=np.float64) - (sp + n_ref * depth / 2)).max())
            elif kind == "plane-box":
                res["C5n"] = float(np.abs(normals - n_ref).max())
                corners = _box_corners(Bg)
                sd = (corners - np.array(A["pos"])) @ n_ref   # signed distance of the eight corners
                worst, used = 0.0, set()
                for k in cons:
                    pos, dk = np.asarray(k["pos"], dtype=np.float64), -float(k["dist"])
                    m = int(np.argmin(np.linalg.norm(corners - n_ref * sd[:, None] / 2 - pos, axis=1)))
                    worst = max(worst, float(np.abs(corners[m] - n_ref * sd[m] / 2 - pos).max()), abs(dk + sd[m]))
                    if m in used:
                        err.append("C5 plane-box: two contacts at one corner")
                    used.add(m)
                res["C5p"] = worst
                below = int((sd < -2e-6).sum())               # corners clearly below the plane
                if len(cons) < min(below, 4):
                    err.append(f"C5 plane-box: {len(cons)} contacts, {below} corners below the plane")
        elif kind == "general":                                # ---- C6
            res["C6"] = c / 4 - depth
    return out


def left_out_report(records):
    """((worst share of a class x case left out, which), the share of all deep samples left out)"""
    deep = [r for r in records if CASES[r["case"]] > 0]
    per = {}
    for r in deep:
        per.setdefault((r["cls"], r["case"]), []).append(r["left_out"])
    worst = max((np.mean(v), k) for k, v in per.items())
    return worst, float(np.mean([r["left_out"] for r in deep]))


def worst_residuals(records):
    out = {}
    for r in records:
        for k, v in r["res"].items():
            out[k] = max(out.get(k, -np.inf), v)
    return out


def check(records, eps, label):
    """assert every certificate on every record; eps: {certificate: allowance}"""
    bad = [(r["cls"], CASE_NAMES[r["case"]], r["draw"], r["errors"]) for r in records if r["errors"]]
    assert not bad, (label, len(bad), bad[:6])
    (share, where), overall = left_out_report(records)
    assert share <= LEFT_OUT_CLASS and overall <= LEFT_OUT_ALL, (label, "left out", share, where, overall)
    for r in records:
        for k, v in r["res"].items():
            assert v <= eps[k], (label, k, r["cls"], CASE_NAMES[r["case"]], r["draw"], v, eps[k])


def tolerances(measured, floor):
    """4 x the worst residual one run measured per certificate (the project's convention: one box, one run, pose-dependent rounding), not below `floor`"""
    return {k: max(4 * v, floor) for k, v in measured.items()}


COLS = ("C3", "C4", "C4hi", "C5da", "C5db", "C5lo", "C5hi", "C5n", "C5p", "C6")


# ---- the record (profiles/contact_certificates.txt) ------------------------------------------------------------------------------------------------------
def table(flat, records, title):
    names = list(NAMES) + ["plane"]
    lines = [title, f"{'class':<12}{'case':<12}{'n':>3}{'out':>4}{'ncon':>5}  " + "".join(f"{k:>10}" for k in COLS)
             + "   angle p50 / p90 / max [rad]     (h1 + h2) / depth p50 / p90 / max"]
    for cls in classes():
        for case in range(len(CASES)):
            rs = [r for r in records if r["cls"] == cls and r["case"] == case]
            res = worst_residuals(rs)
            ang = [r["angle"] for r in rs if r["angle"] is not None]
            rat = [r["ratio"] for r in rs if r["ratio"] is not None]
            q = lambda v: " ".join(f"{x:9.2e}" for x in (np.percentile(v, 50), np.percentile(v, 90), np.max(v))) if v else " " * 29      # noqa: E731
            lines.append(f"{names[cls[1]] + ' x ' + names[cls[0]]:<12}{CASE_NAMES[case]:<12}{len(rs):>3}{sum(r['left_out'] for r in rs):>4}{sum(r['ncon'] for r in rs):>5}  "
                         + "".join(f"{res[k]:>10.1e}" if k in res else f"{'-':>10}" for k in COLS) + "   " + q(ang) + "     " + q(rat))
    res = worst_residuals(records)
    (share, where), overall = left_out_report(records)
    w = max((r for r in records if "C3" in r["res"]), key=lambda r: r["res"]["C3"])
    lines.append(f"worst C3: {names[w['cls'][1]]} x {names[w['cls'][0]]}, {CASE_NAMES[w['case']]}, draw {w['draw']}: depth {w['c3_depth']:.4e}, point outside geom1 / geom2 beyond depth / 2 "
                 f"{w['c3_parts'][0]:.3e} / {w['c3_parts'][1]:.3e}, witness pos + n depth / 2 outside geom1 {w['c3_parts'][2]:.3e}, pos - n depth / 2 outside geom2 {w['c3_parts'][3]:.3e}"
                 + (f", (h1 + h2) / depth {w['ratio']:.4f}" if w["ratio"] is not None else ""))
    big = sorted((r for r in records if r["res"].get("C3", 0) > 1e-6), key=lambda r: -r["res"]["C3"])
    lines.append(f"samples with C3 above 1e-6: {len(big)}: " + "; ".join(f"{names[r['cls'][1]]} x {names[r['cls'][0]]} {CASE_NAMES[r['case']]} #{r['draw']} {r['res']['C3']:.2e} (depth {r['c3_depth']:.2e}, "
                                                                       f"parts {' '.join(f'{x:.1e}' for x in r['c3_parts'])})" for r in big[:12]))
    lines.append("worst residuals: " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(res.items())))
    sd = [r["signed_depth_err"] for r in records if "signed_depth_err" in r]
    lines.append(f"depth - delta* of the exact pairs: {min(sd):.3e} .. {max(sd):.3e}; left out: worst class x case {share:.3f} {where}, of all deep samples {overall:.4f}")
    return "\n".join(lines)


# ---- the tetrahedron: a sphere against each of its four faces, closed form ---------------------------------------------------------------------------------
TET_XML = """<mujoco><compiler angle="radian"/><asset><mesh name="tet" file="tet.obj"/></asset><worldbody>
    <body name="b_sph"><freejoint/><geom name="sph" type="sphere" size="0.05"/></body>
    <body name="b_tet"><freejoint/><geom name="tet" type="mesh" mesh="tet"/></body></worldbody></mujoco>"""
TET_R = 0.05


def tet_scene(tmpdir):
    write_meshes(tmpdir)
    return mjcf.compile_mjcf(TET_XML, asset_dir=str(tmpdir))


def tet_cases(flat):
    """[(qpos [14], face normal (world), signed gap)] : the sphere's centre at a face's centroid + its outward normal x (r + gap), gap = +-1 mm; the tetrahedron's
    body sits at the origin, unrotated, so its hull is raycast_scenes.TETRA_VERTS moved by nothing"""
    V = np.array(R.TETRA_VERTS, dtype=np.float64)
    out = []
    for f in range(4):
        tri = V[[k for k in range(4) if k != f]]
        n = np.cross(tri[1] - tri[0], tri[2] - tri[0]); n /= np.linalg.norm(n)
        if np.dot(n, V[f] - tri[0]) > 0:
            n = -n
        for gap in (1e-3, -1e-3):
            q = np.zeros(14); q[3] = q[10] = 1.0
            q[:3] = tri.mean(axis=0) + n * (TET_R + gap)
            out.append((q, n, gap))
    return out


def check_tet(contacts, n, gap, tol, label):
    """the closed form: no contact 1 mm apart; 1 mm deep one contact, depth 1 mm, normal from the sphere (geom1) into the face = -n, the point half-way"""
    if gap > 0:
        assert len(contacts) == 0, (label, "phantom contact", [(k["dist"], k["frame"][0]) for k in contacts])
        return
    assert len(contacts) == 1, (label, len(contacts))
    k = contacts[0]
    assert abs(k["dist"] - gap) <= MPR_TOL + tol, (label, k["dist"], gap)
    assert np.abs(np.asarray(k["frame"]).reshape(3, 3)[0] + n).max() <= 2e-3, (label, k["frame"])
