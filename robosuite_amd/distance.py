"""Geom distance queries: the fp64 host mirror of the device routine (csrc/rsim_dist.hip, rsim_geom_distance) and the pair bookkeeping around it.

The mirror is float64, one env, written from MuJoCo's documentation of mj_geomDistance [3P, docs "API reference: mj_geomDistance"] and from the GJK paper
[3P, Gilbert, Johnson, Keerthi 1988]; it shares no code with csrc/ -- the idiom of raycast.py and ik.py.  Its sub-simplex search is the Voronoi-region walk of
Ericson's "Real-Time Collision Detection" (ch. 5.1), not the face enumeration the kernel uses.  The kernel is tested against this file
(tests/test_distance.py); this file is tested against closed forms and against its own certificate (tests/test_distance_host.py).  One function per layer:

    support(geom, d)                        -> support point of the geom's core along d           (geom: make_geom / world_geoms)
    closest_on_simplex(points)              -> (weights, encloses_origin)
    pair(g1, g2, distmax, tol, max_iters)   -> (dist, fromto [6], status)
    geom_distance(flat, xpos, xquat, pairs, distmax=1.0, tol=1e-6, max_iters=64, params=None) -> (dist [P], fromto [P, 6], status [P])
    check_pairs(flat, pairs)                -> int array [P, 2], or DistanceError naming what the query refuses
    body_pairs(flat, bodies_a, bodies_b)    -> the geom pairs between two body sets the query accepts
    reduce_min(dist, fromto)                -> (min dist, its fromto, its pair index) per env

Semantics (include/rsim.h rsim_geom_distance).  dist: the Euclidean distance of the two solids when they are disjoint and closer than distmax; a mesh geom is its
convex hull, a plane the half-space below its +Z face.  fromto: the nearest point on geom1, then on geom2.  status 0: such a pair -- or an overlapping pair whose
signed distance is exact (one member a plane, or both spheres / capsules): dist is then minus the penetration depth and fromto the deepest points.  status 1: beyond
distmax, dist = distmax, fromto zero.  status 2: any other overlapping pair, dist = 0, fromto one common point twice.  Bit 8 (256): the iteration stopped at
max_iters before its bounds were within tol; dist and fromto are the best iterate.
"""
from __future__ import annotations

import math

import numpy as np

from . import mjcf

OK, FAR, OVERLAP, CAP = 0, 1, 2, 256
DEFAULTS = {"tol": 1e-6, "max_iters": 64}
MAX_ITERS_LIMIT = 1024        # rsim_geom_distance refuses more: no input may keep a wavefront spinning
_ROUND = (mjcf.GEOM_SPHERE, mjcf.GEOM_CAPSULE)
_TOUCH2 = 1e-28               # cores closer than 1e-14 m touch


class DistanceError(ValueError):
    pass


# ---- small vectors as tuples (an order of magnitude faster than numpy at this size) --------------------------------------------------------------------
def _sub(a, b): return (a[0] - b[0], a[1] - b[1], a[2] - b[2])
def _add(a, b): return (a[0] + b[0], a[1] + b[1], a[2] + b[2])
def _mul(a, s): return (a[0] * s, a[1] * s, a[2] * s)
def _dot(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
def _cross(a, b): return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])
def _neg(a): return (-a[0], -a[1], -a[2])


def _rot(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def make_geom(gtype, size, pos, rot, verts=None):
    """A geom of the mirror: world position, world rotation matrix (or wxyz quaternion), geom_size, hull vertices [n, 3] in the geom frame for a mesh."""
    R = np.asarray(rot, dtype=np.float64)
    R = _rot(R) if R.shape == (4,) else R
    return {"type": int(gtype), "size": tuple(float(s) for s in np.asarray(size, dtype=np.float64).ravel()[:3]), "pos": tuple(float(p) for p in pos),
            "R": R, "cols": tuple(tuple(float(v) for v in R[:, k]) for k in range(3)),
            "verts": None if verts is None else np.ascontiguousarray(verts, dtype=np.float64).reshape(-1, 3)}


def radius(g):
    return g["size"][0] if g["type"] in _ROUND else 0.0


# ---- layer 1: support functions ----------------------------------------------------------------------------------------------------------------------
def support(g, d):
    """Support point (world) of the geom's CORE along world direction d: a sphere is its centre, a capsule its axis segment (radius() is the rest); the other
    types are themselves.  Ties: the + side for a zero component, the lowest vertex index for a hull."""
    ex, ey, ez = g["cols"]
    ld = (_dot(ex, d), _dot(ey, d), _dot(ez, d))
    t, h = g["type"], g["size"]
    lx = ly = lz = 0.0
    if t == mjcf.GEOM_BOX:
        lx, ly, lz = (h[0] if ld[0] >= 0 else -h[0]), (h[1] if ld[1] >= 0 else -h[1]), (h[2] if ld[2] >= 0 else -h[2])
    elif t == mjcf.GEOM_CAPSULE:
        lz = h[1] if ld[2] >= 0 else -h[1]
    elif t == mjcf.GEOM_CYLINDER:
        n = math.hypot(ld[0], ld[1])
        if n > 0:
            lx, ly = ld[0] / n * h[0], ld[1] / n * h[0]
        lz = h[1] if ld[2] >= 0 else -h[1]
    elif t == mjcf.GEOM_ELLIPSOID:
        tx, ty, tz = ld[0] * h[0], ld[1] * h[1], ld[2] * h[2]
        n = math.sqrt(tx * tx + ty * ty + tz * tz)
        if n > 0:
            lx, ly, lz = tx / n * h[0], ty / n * h[1], tz / n * h[2]
    elif t == mjcf.GEOM_MESH:
        V = g["verts"]
        lx, ly, lz = V[int(np.argmax(V @ np.array(ld)))]
    elif t != mjcf.GEOM_SPHERE:
        raise DistanceError(f"geom type {t} has no support function here")
    p = g["pos"]
    return (p[0] + ex[0] * lx + ey[0] * ly + ez[0] * lz, p[1] + ex[1] * lx + ey[1] * ly + ez[1] * lz, p[2] + ex[2] * lx + ey[2] * ly + ez[2] * lz)


def support_full(g, d):
    """support point of the whole solid (core plus radius) along d"""
    s, r = support(g, d), radius(g)
    n = math.sqrt(_dot(d, d))
    return _add(s, _mul(d, r / n)) if r > 0 and n > 0 else s


# ---- layer 2: closest point of a simplex to the origin -------------------------------------------------------------------------------------------------
def _closest_segment(a, b):
    ab = _sub(b, a)
    den = _dot(ab, ab)
    t = -_dot(a, ab) / den if den > 0 else 0.0
    t = min(max(t, 0.0), 1.0)
    return (1.0 - t, t)


def _closest_triangle(a, b, c):
    """Voronoi regions of the triangle, the point being the origin"""
    ab, ac = _sub(b, a), _sub(c, a)
    d1, d2 = -_dot(ab, a), -_dot(ac, a)
    if d1 <= 0 and d2 <= 0:
        return (1.0, 0.0, 0.0)
    d3, d4 = -_dot(ab, b), -_dot(ac, b)
    if d3 >= 0 and d4 <= d3:
        return (0.0, 1.0, 0.0)
    vc = d1 * d4 - d3 * d2
    if vc <= 0 and d1 >= 0 and d3 <= 0:
        v = d1 / (d1 - d3) if d1 - d3 > 0 else 0.0
        return (1.0 - v, v, 0.0)
    d5, d6 = -_dot(ab, c), -_dot(ac, c)
    if d6 >= 0 and d5 <= d6:
        return (0.0, 0.0, 1.0)
    vb = d5 * d2 - d1 * d6
    if vb <= 0 and d2 >= 0 and d6 <= 0:
        w = d2 / (d2 - d6) if d2 - d6 > 0 else 0.0
        return (1.0 - w, 0.0, w)
    va = d3 * d6 - d5 * d4
    if va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:
        den = (d4 - d3) + (d5 - d6)
        w = (d4 - d3) / den if den > 0 else 0.0
        return (0.0, 1.0 - w, w)
    den = va + vb + vc
    if not den > 0:           # a degenerate triangle no region claimed: its best edge
        best = None
        for (i, j), (p, q) in (((0, 1), (a, b)), ((0, 2), (a, c)), ((1, 2), (b, c))):
            l = _closest_segment(p, q)
            x = _add(_mul(p, l[0]), _mul(q, l[1]))
            if best is None or _dot(x, x) < best[0]:
                lam = [0.0, 0.0, 0.0]
                lam[i], lam[j] = l
                best = (_dot(x, x), tuple(lam))
        return best[1]
    v, w = vb / den, vc / den
    return (1.0 - v - w, v, w)


def closest_on_simplex(points):
    """points: 1 to 4 points (3-tuples).  -> (weights, encloses): the convex weights of the simplex's closest point to the origin; encloses is True when a
    tetrahedron holds the origin (the weights are then its barycentric coordinates)."""
    n = len(points)
    if n == 1:
        return (1.0,), False
    if n == 2:
        return _closest_segment(*points), False
    if n == 3:
        return _closest_triangle(*points), False
    a, b, c, d = points
    best, outside = None, False
    for idx in ((0, 1, 2), (0, 2, 3), (0, 3, 1), (1, 3, 2)):
        p, q, r = points[idx[0]], points[idx[1]], points[idx[2]]
        o = points[6 - sum(idx)]
        nrm = _cross(_sub(q, p), _sub(r, p))
        so, s0 = _dot(_sub(o, p), nrm), -_dot(p, nrm)          # the fourth vertex and the origin against the face's plane
        if so == 0.0 or so * s0 < 0:                             # the origin is outside this face (or the tetrahedron is flat)
            outside = True
            l = _closest_triangle(p, q, r)
            x = _add(_add(_mul(p, l[0]), _mul(q, l[1])), _mul(r, l[2]))
            if best is None or _dot(x, x) < best[0]:
                lam = [0.0] * 4
                lam[idx[0]], lam[idx[1]], lam[idx[2]] = l
                best = (_dot(x, x), tuple(lam))
    if outside:
        return best[1], False
    A = np.array([[a[0], b[0], c[0], d[0]], [a[1], b[1], c[1], d[1]], [a[2], b[2], c[2], d[2]], [1.0, 1.0, 1.0, 1.0]])
    lam = np.linalg.solve(A, np.array([0.0, 0.0, 0.0, 1.0]))
    return tuple(float(x) for x in lam), True


# ---- layer 3: one pair -----------------------------------------------------------------------------------------------------------------------------------
def gjk(g1, g2, tol, max_iters, far_core=math.inf):
    """Distance of the two CORES.  -> (dc, p1, p2, flag): flag "ok" (bounds within tol, or nothing left to resolve), "far" (the lower bound exceeds far_core),
    "overlap" (the cores meet: p1 = p2 is a common point), "cap" (max_iters reached: the best iterate; "cap overlap" when that iterate is a common point)."""
    d0 = _sub(g2["pos"], g1["pos"])
    if not _dot(d0, d0) > 0:
        d0 = (1.0, 0.0, 0.0)
    a = support(g1, d0)
    W, A = [_sub(a, support(g2, _neg(d0)))], [a]
    v, pa = W[0], a
    vv = _dot(v, v)
    for _ in range(max_iters):
        if vv <= _TOUCH2:
            return 0.0, pa, pa, "overlap"
        vn = math.sqrt(vv)
        sa = support(g1, _neg(v))
        w = _sub(sa, support(g2, v))
        lower = _dot(v, w) / vn
        if lower > far_core:
            return vn, pa, _sub(pa, v), "far"
        if vn - lower <= tol or w in W:
            return vn, pa, _sub(pa, v), "ok"
        W.append(w); A.append(sa)
        lam, inside = closest_on_simplex(W)
        keep = [i for i, l in enumerate(lam) if l > 0] if not inside else list(range(4))
        x = (0.0, 0.0, 0.0); y = (0.0, 0.0, 0.0)
        for i in keep:
            x, y = _add(x, _mul(W[i], lam[i])), _add(y, _mul(A[i], lam[i]))
        if inside:
            return 0.0, y, y, "overlap"
        if not _dot(x, x) < vv:
            return vn, pa, _sub(pa, v), "ok"
        W, A = [W[i] for i in keep], [A[i] for i in keep]
        v, pa, vv = x, y, _dot(x, x)
    if vv <= _TOUCH2:            # (the last update brought the cores together)
        return 0.0, pa, pa, "cap overlap"
    return math.sqrt(vv), pa, _sub(pa, v), "cap"


def pair(g1, g2, distmax=1.0, tol=DEFAULTS["tol"], max_iters=DEFAULTS["max_iters"]):
    """-> (dist, fromto (6 floats: nearest point on g1, on g2), status)"""
    zero = (0.0,) * 6
    if g1["type"] == mjcf.GEOM_PLANE and g2["type"] == mjcf.GEOM_PLANE:
        raise DistanceError("plane against plane has no distance")
    if g1["type"] == mjcf.GEOM_PLANE or g2["type"] == mjcf.GEOM_PLANE:
        first = g1["type"] == mjcf.GEOM_PLANE
        pl, o = (g1, g2) if first else (g2, g1)
        n = pl["cols"][2]
        s = support_full(o, _neg(n))
        d = _dot(n, _sub(s, pl["pos"]))
        q = _sub(s, _mul(n, d))
        if d > distmax:
            return distmax, zero, FAR
        return d, (q + s) if first else (s + q), OK
    r1, r2 = radius(g1), radius(g2)
    exact = g1["type"] in _ROUND and g2["type"] in _ROUND
    dc, pa, pb, flag = gjk(g1, g2, tol, max_iters, far_core=distmax + r1 + r2)
    st = CAP if flag.startswith("cap") else OK
    if flag == "far":
        return distmax, zero, FAR
    if flag.endswith("overlap"):
        if exact:
            return -(r1 + r2), (pa[0], pa[1], pa[2] + r1, pa[0], pa[1], pa[2] - r2), st
        return 0.0, pa + pa, st | OVERLAP
    n = _mul(_sub(pb, pa), 1.0 / dc)
    d = dc - r1 - r2
    if exact or d > 0:
        if d > distmax:
            return distmax, zero, st | FAR
        return d, _add(pa, _mul(n, r1)) + _sub(pb, _mul(n, r2)), st
    x = pb if r1 > 0 else pa
    return 0.0, x + x, st | OVERLAP


# ---- the scene: geoms of one env ---------------------------------------------------------------------------------------------------------------------------
def _I(flat, name):
    return np.asarray(flat.arrays[name]).ravel().astype(int)


def mesh_verts(flat, g):
    """hull vertices [n, 3] (geom frame) of mesh geom g, or None when the model does not hold them (visual-only meshes)"""
    did = _I(flat, "geom_dataid")[g] if "geom_dataid" in flat.arrays else -1
    if did < 0 or "mesh_vert" not in flat.arrays:
        return None
    adr, num = _I(flat, "mesh_vertadr")[did], _I(flat, "mesh_vertnum")[did]
    return np.asarray(flat.arrays["mesh_vert"], dtype=np.float64).reshape(-1, 3)[adr:adr + num]


def world_geoms(flat, xpos, xquat, geoms, params=None):
    """{geom id: mirror geom} of one env from its body poses; params: {"geom_size" | "geom_pos" | "geom_quat": array} the env's own values"""
    A = lambda name, w: np.asarray((params or {}).get(name, flat.arrays[name]), dtype=np.float64).reshape(-1, w)      # noqa: E731
    xpos, xquat = np.asarray(xpos, dtype=np.float64).reshape(-1, 3), np.asarray(xquat, dtype=np.float64).reshape(-1, 4)
    gtype, gbody = _I(flat, "geom_type"), _I(flat, "geom_bodyid")
    gsize, gpos, gquat = A("geom_size", 3), A("geom_pos", 3), A("geom_quat", 4)
    out = {}
    for g in sorted(set(int(x) for x in geoms)):
        b = gbody[g]
        Rb = _rot(xquat[b])
        out[g] = make_geom(gtype[g], gsize[g], xpos[b] + Rb @ gpos[g], Rb @ _rot(gquat[g]), mesh_verts(flat, g) if gtype[g] == mjcf.GEOM_MESH else None)
    return out


def check_pairs(flat, pairs):
    """The refusals of rsim_geom_distance, by name: -> int array [P, 2] or DistanceError"""
    p = np.asarray(pairs, dtype=np.int64)
    if p.size == 0 or p.ndim != 2 or p.shape[1] != 2:
        raise DistanceError(f"geom_distance: npair < 1 or pairs not of shape [P, 2] (got shape {tuple(p.shape)})")
    gtype = _I(flat, "geom_type")
    for k, (g1, g2) in enumerate(p):
        for g in (g1, g2):
            if g < 0 or g >= len(gtype):
                raise DistanceError(f"geom_distance: pair {k}: geom id {g} out of range ({len(gtype)} geoms)")
        if g1 == g2:
            raise DistanceError(f"geom_distance: pair {k}: geom {g1} against itself")
        if gtype[g1] == mjcf.GEOM_PLANE and gtype[g2] == mjcf.GEOM_PLANE:
            raise DistanceError(f"geom_distance: pair {k}: plane against plane ({g1}, {g2})")
        for g in (g1, g2):
            if gtype[g] == mjcf.GEOM_MESH and mesh_verts(flat, g) is None:
                raise DistanceError(f"geom_distance: pair {k}: the model holds no hull vertices of mesh geom {g} (a visual-only mesh)")
            if gtype[g] not in (mjcf.GEOM_PLANE, mjcf.GEOM_SPHERE, mjcf.GEOM_CAPSULE, mjcf.GEOM_ELLIPSOID, mjcf.GEOM_CYLINDER, mjcf.GEOM_BOX, mjcf.GEOM_MESH):
                raise DistanceError(f"geom_distance: pair {k}: geom {g} has type {gtype[g]}, which is not carried (heightfields are out of scope)")
    return p


def options(tol=DEFAULTS["tol"], max_iters=DEFAULTS["max_iters"]):
    tol, max_iters = float(tol), int(max_iters)
    if not tol >= 0 or max_iters < 1 or max_iters > MAX_ITERS_LIMIT:
        raise DistanceError(f"geom_distance: option out of range (tol {tol}, max_iters {max_iters}: 1..{MAX_ITERS_LIMIT})")
    return {"tol": tol, "max_iters": max_iters}


def geom_distance(flat, xpos, xquat, pairs, distmax=1.0, tol=DEFAULTS["tol"], max_iters=DEFAULTS["max_iters"], params=None, check_options=True):
    """One env.  -> (dist float64 [P], fromto [P, 6], status int [P])"""
    p = check_pairs(flat, pairs)
    if check_options:
        options(tol, max_iters)
    G = world_geoms(flat, xpos, xquat, p.ravel(), params)
    dist, fromto, status = np.zeros(len(p)), np.zeros((len(p), 6)), np.zeros(len(p), dtype=np.int32)
    for k, (g1, g2) in enumerate(p):
        dist[k], fromto[k], status[k] = pair(G[int(g1)], G[int(g2)], distmax, tol, max_iters)
    return dist, fromto, status


# ---- body sets -----------------------------------------------------------------------------------------------------------------------------------------------
def body_pairs(flat, bodies_a, bodies_b):
    """All geom pairs (geom of a body of A, geom of a body of B), in (A geom, B geom) order of ascending ids.  Geoms the query refuses are SKIPPED, silently:
    mesh geoms whose hull vertices the model does not hold (visual-only meshes), heightfields, a geom against itself (a body in both sets), plane against
    plane.  DistanceError when nothing is left."""
    gbody, gtype = _I(flat, "geom_bodyid"), _I(flat, "geom_type")
    carried = (mjcf.GEOM_PLANE, mjcf.GEOM_SPHERE, mjcf.GEOM_CAPSULE, mjcf.GEOM_ELLIPSOID, mjcf.GEOM_CYLINDER, mjcf.GEOM_BOX, mjcf.GEOM_MESH)

    def geoms(bodies):
        bs = set(int(b) for b in np.asarray(bodies).ravel())
        for b in bs:
            if b < 0 or b >= int(flat.nbody):
                raise DistanceError(f"body_distance: body id {b} out of range ({int(flat.nbody)} bodies)")
        return [g for g in range(len(gbody)) if gbody[g] in bs and gtype[g] in carried and not (gtype[g] == mjcf.GEOM_MESH and mesh_verts(flat, g) is None)]

    ga, gb = geoms(bodies_a), geoms(bodies_b)
    out = [(a, b) for a in ga for b in gb if a != b and not (gtype[a] == mjcf.GEOM_PLANE and gtype[b] == mjcf.GEOM_PLANE)]
    if not out:
        raise DistanceError("body_distance: no geom pair is left between the two body sets")
    return np.asarray(out, dtype=np.int32)


def reduce_min(dist, fromto):
    """dist [..., P], fromto [..., P, 6] (numpy) -> (min dist [...], its fromto [..., 6], its pair index [...]); the lowest index wins ties"""
    dist, fromto = np.asarray(dist), np.asarray(fromto)
    k = np.argmin(dist, axis=-1)
    return np.take_along_axis(dist, k[..., None], axis=-1)[..., 0], np.take_along_axis(fromto, k[..., None, None], axis=-2)[..., 0, :], k
