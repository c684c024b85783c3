"""Signed distance of overlapping convex pairs: the fp64 host mirror -- and the definition -- of the device routine (csrc/rsim_pen_core.h pair_signed, k_dist_signed in
csrc/rsim_pen.hip, rsim_geom_distance_signed).  One env, float64, built on distance.py's layers (support, gjk, pair); it shares no code with csrc/.

The quantity.  For two convex solids A (geom1) and B (geom2), C = A - B is their Minkowski difference; they overlap exactly when the origin is inside C.
delta(n) = h_A(n) + h_B(-n) is the support width along a unit n: how far B must move along n to come free.  The penetration depth is the minimum of delta over
the sphere of directions = the distance of the origin to the boundary of C; the minimiser is the contact normal, from geom1 towards geom2.

    dist = -depth,  p1 on geom1's surface in its support set along +n,  p2 on geom2's along -n,  p2 - p1 = dist * n

(MuJoCo's convention for a negative mj_geomDistance, the one distance.pair already follows for plane and sphere / capsule pairs.)

The algorithm is a descent on delta that reuses the GJK of distance.py unchanged.  Given n_k and w_k = delta(n_k), the point x = (w_k + offset) n_k lies outside C by
at least `offset` (the supporting plane of C along n_k is at w_k).  One GJK call on geom2 moved by x projects x onto C: its witnesses give the foot c and the
outward normal n_{k+1} = (x - c) / |x - c| of C there, and delta(n_{k+1}) -- evaluated with the support functions, not from c -- is accepted only if it is smaller.
A fixed point is a stationary point of delta: the foot of the origin on the supporting plane lies in C.  WHAT COMES OUT IS A LOCAL MINIMUM OF THE SEPARATING
TRANSLATION, NEVER LESS THAN THE TRUE DEPTH: each face of a polytope C that holds the origin's foot is one.  multistart_depth is the global reference.

  * round cores: spheres and capsules enter as a point / a segment.  Cores that are disjoint while a radius reaches the other shape are exact without descent:
    dist = d_core - rsum, n from the core witnesses.  Cores that overlap descend on the cores: dist = -(delta_core + rsum), the witnesses pushed out by the radii.
  * seed: the direction of least delta among 13 candidates, in this order: geom1's position to geom2's, the +- axes of geom1, the +- axes of geom2; the first
    smallest wins.  It is then tilted by TILT = 1e-3 (rad, to first order): an exact axis of an ellipsoid or a cylinder is a saddle of delta, where the descent
    would sit.  Where the axis is the answer (box on box) one projection takes the tilt back.
  * stop: the moved pair overlaps or is within pen_tol of touching (nothing to project from); delta does not decrease (the iterate before is the answer); delta
    decreased by no more than pen_tol (the new iterate is the answer); pen_iters projections were made: status bit PEN_CAP (512), the result is still a valid
    directional depth, dist = -delta(n) for the returned n, an upper bound of the depth.
  * the projection is asked for a gap of pen_tol * offset / (1 m): a gap g tilts the normal by sqrt(2 g / offset), which costs a surface of curvature radius R
    up to R g / offset of depth -- pen_tol for R up to one metre.  A projection that ends at max_iters instead is used as it is: every unit n is a valid direction
    and the decrease test guards the result, so that cap is not reported.

    support_width(g1, g2, n)                         -> delta(n) of the two solids
    seed(g1, g2)                                     -> the tilted start direction
    descend(c1, c2, n0, ...)                         -> (delta_core, n, core1 witness, projections, capped)
    pair_signed(g1, g2, distmax, tol, max_iters, pen_tol, pen_iters, offset) -> (dist, fromto, status)
    geom_distance_signed(flat, xpos, xquat, pairs, ...) -> (dist [P], fromto [P, 6], status [P])
    multistart_depth(g1, g2, starts)                 -> the least depth over descents from an icosphere of directions
"""
from __future__ import annotations

import math

import numpy as np

from . import distance as D
from .distance import _add, _cross, _dot, _mul, _neg, _sub

PEN_CAP = 512
# offset 4 mm, pen_tol 1e-7 m: chosen on the fp32 host rehearsal (tests/test_penetration_core_host.py prints the figures; DESIGN.md 5.3 records them)
DEFAULTS = {"pen_tol": 1e-7, "pen_iters": 64, "offset": 4e-3}
PEN_ITERS_LIMIT = 128         # rsim_geom_distance_signed refuses more: no input may keep a wavefront spinning
TILT = 1e-3
TILT_DIR = (0.8, 0.6)         # the tilt's direction in the plane across the seed: oblique, so that it lies in no symmetry plane of an axis-aligned pair


class PenetrationError(D.DistanceError):
    pass


def options(pen=None):
    """{"pen_tol", "pen_iters", "offset"} with defaults filled in; PenetrationError for what rsim_geom_distance_signed refuses"""
    o = dict(DEFAULTS)
    for k, v in dict(pen or {}).items():
        if k not in o:
            raise PenetrationError(f"geom_distance: unknown penetration option {k!r} (pen_tol, pen_iters, offset)")
        o[k] = v
    o = {"pen_tol": float(o["pen_tol"]), "pen_iters": int(o["pen_iters"]), "offset": float(o["offset"])}
    if not o["pen_tol"] >= 0 or not (o["offset"] > 0 and math.isfinite(o["offset"])) or o["pen_iters"] < 1 or o["pen_iters"] > PEN_ITERS_LIMIT:
        raise PenetrationError(f"geom_distance: penetration option out of range (pen_tol {o['pen_tol']}, offset {o['offset']}, pen_iters {o['pen_iters']}: "
                               f"1..{PEN_ITERS_LIMIT})")
    return o


def _unit(v):
    return _mul(v, 1.0 / math.sqrt(_dot(v, v)))


def core(g):
    """the geom's core as a geom of its own: a sphere or capsule with radius zero, any other type itself"""
    return dict(g, size=(0.0,) + tuple(g["size"][1:])) if g["type"] in D._ROUND else g


def _core_width(c1, c2, n):
    return _dot(n, _sub(D.support(c1, n), D.support(c2, _neg(n))))


def support_width(g1, g2, n):
    """delta(n) = h_A(n) + h_B(-n) of the two SOLIDS along unit n: how far geom2 must move along n to come free of geom1"""
    return _core_width(g1, g2, n) + D.radius(g1) + D.radius(g2)


def tilted(n, angle=TILT, direction=TILT_DIR):
    """unit n turned by `angle` (to first order) towards direction[0] t1 + direction[1] t2, where t1 = n x e / |n x e| for the world axis e along which |n| is
    smallest (x before y before z) and t2 = n x t1"""
    k = min(range(3), key=lambda i: (abs(n[i]), i))
    t1 = _unit(_cross(n, tuple(1.0 if i == k else 0.0 for i in range(3))))
    t2 = _cross(n, t1)
    return _unit(_add(n, _mul(_add(_mul(t1, direction[0]), _mul(t2, direction[1])), angle)))


def seed_candidates(g1, g2):
    d0 = _sub(g2["pos"], g1["pos"])
    d0 = _unit(d0) if _dot(d0, d0) > 0 else (1.0, 0.0, 0.0)
    out = [d0]
    for g in (g1, g2):
        for ax in g["cols"]:
            out += [ax, _neg(ax)]
    return out


def seed(g1, g2, angle=TILT, direction=TILT_DIR):
    """the start direction: the candidate of least delta, the first smallest, tilted"""
    c1, c2 = core(g1), core(g2)
    best, bw = None, math.inf
    for n in seed_candidates(g1, g2):
        w = _core_width(c1, c2, n)
        if w < bw:
            best, bw = n, w
    return tilted(best, angle, direction)


def descend(c1, c2, n, pen_tol=DEFAULTS["pen_tol"], pen_iters=DEFAULTS["pen_iters"], offset=DEFAULTS["offset"], max_iters=D.DEFAULTS["max_iters"], trace=None):
    """The descent on two CORES that overlap, from unit n.  -> (delta, n, a, steps, capped): the width reached, its direction, a point of core1 on its supporting
    plane along n (the projection's witness; the seed's support point when no projection was accepted), the projections made, and whether pen_iters ended it.
    trace: a list that receives delta of every accepted iterate."""
    w, a = _core_width(c1, c2, n), D.support(c1, n)
    if trace is not None:
        trace.append(w)
    steps = 0
    while True:
        if steps >= pen_iters:
            return w, n, a, steps, True
        x = _mul(n, w + offset)
        try:
            dc, pa, pb, flag = D.gjk(c1, dict(c2, pos=_add(c2["pos"], x)), pen_tol * offset, max_iters)
        except np.linalg.LinAlgError:      # distance.py cannot solve for the weights of a flat enclosing tetrahedron (seen at gaps of 1e-13 only): the iterate stands
            return w, n, a, steps + 1, False
        steps += 1
        if flag.endswith("overlap") or dc <= pen_tol:
            return w, n, a, steps, False
        n2 = _mul(_sub(pb, pa), 1.0 / dc)
        w2 = _core_width(c1, c2, n2)
        if not w2 < w:
            return w, n, a, steps, False
        small = w - w2 <= pen_tol
        n, w, a = n2, w2, pa
        if trace is not None:
            trace.append(w)
        if small:
            return w, n, a, steps, False


def pair_signed(g1, g2, distmax=1.0, tol=D.DEFAULTS["tol"], max_iters=D.DEFAULTS["max_iters"], pen_tol=DEFAULTS["pen_tol"], pen_iters=DEFAULTS["pen_iters"],
                offset=DEFAULTS["offset"], n0=None, info=None):
    """distance.pair with every overlap signed.  -> (dist, fromto, status); a pair distance.pair does not send to status 2 comes back as distance.pair returns
    it.  n0: a start direction instead of the seed; info: a dict that receives "steps", "normal", "trace" of a pair that descended."""
    d, ft, st = D.pair(g1, g2, distmax, tol, max_iters)
    if not st & D.OVERLAP:
        return d, ft, st
    r1, r2 = D.radius(g1), D.radius(g2)
    c1, c2 = core(g1), core(g2)
    if r1 + r2 > 0:
        dc, pa, pb, flag = D.gjk(c1, c2, tol, max_iters)
        if not flag.endswith("overlap"):                 # the cores are apart: exact, as a sphere against a capsule is
            n = _mul(_sub(pb, pa), 1.0 / dc)
            if info is not None:
                info.update(steps=0, normal=n, trace=[])
            return dc - r1 - r2, _add(pa, _mul(n, r1)) + _sub(pb, _mul(n, r2)), D.CAP if flag.startswith("cap") else D.OK
    trace = []
    w, n, a, steps, capped = descend(c1, c2, seed(g1, g2) if n0 is None else n0, pen_tol, pen_iters, offset, max_iters, trace)
    if info is not None:
        info.update(steps=steps, normal=n, trace=trace)
    dist = -(w + r1 + r2)
    p1 = _add(a, _mul(n, r1))
    return dist, p1 + _add(p1, _mul(n, dist)), PEN_CAP if capped else D.OK


def geom_distance_signed(flat, xpos, xquat, pairs, distmax=1.0, tol=D.DEFAULTS["tol"], max_iters=D.DEFAULTS["max_iters"], params=None, pen=None):
    """One env.  -> (dist float64 [P], fromto [P, 6], status int [P]): distance.geom_distance with every overlap signed"""
    p = D.check_pairs(flat, pairs)
    D.options(tol, max_iters)
    o = options(pen)
    G = D.world_geoms(flat, xpos, xquat, p.ravel(), params)
    dist, fromto, status = np.zeros(len(p)), np.zeros((len(p), 6)), np.zeros(len(p), dtype=np.int32)
    for k, (g1, g2) in enumerate(p):
        dist[k], fromto[k], status[k] = pair_signed(G[int(g1)], G[int(g2)], distmax, tol, max_iters, **o)
    return dist, fromto, status


def icosphere(level=2):
    """unit directions [10 * 4^level + 2, 3]: an icosahedron's vertices, its edges halved `level` times (162 at level 2)"""
    t = (1 + 5 ** 0.5) / 2
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6),
         (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.array(v, dtype=np.float64) / np.linalg.norm(v) for v in V]
    for _ in range(level):
        mid, F2 = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                v = V[i] + V[j]
                V.append(v / np.linalg.norm(v))
                mid[key] = len(V) - 1
            return mid[key]

        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            F2 += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = F2
    return np.array(V)


def multistart_depth(g1, g2, starts=None, pen_tol=1e-10, pen_iters=200, offset=DEFAULTS["offset"], max_iters=1000, keep=None):
    """The global reference: the least depth the descent reaches from the directions `starts` ([n, 3] unit vectors; None: icosphere(2), 162 of them), untilted.
    -> (depth, its normal).  For a pair whose cores are apart: the exact value.  keep=None descends from EVERY start.  keep=k is a cheaper screen, not the
    reference: every start's delta is an upper bound of the depth already, and the descent runs only from the k starts of least delta and from every start
    that is a local minimum of delta among the starts within 0.45 rad."""
    r1, r2 = D.radius(g1), D.radius(g2)
    c1, c2 = core(g1), core(g2)
    if r1 + r2 > 0:
        dc, pa, pb, flag = D.gjk(c1, c2, 1e-12, max_iters)
        if not flag.endswith("overlap"):
            return r1 + r2 - dc, _mul(_sub(pb, pa), 1.0 / dc)
    S = icosphere(2) if starts is None else np.asarray(starts, dtype=np.float64)
    pick = range(len(S))
    if keep is not None:
        W = np.array([_core_width(c1, c2, tuple(s)) for s in S])
        near = S @ S.T > math.cos(0.45)
        local = np.array([W[i] <= W[near[i]].min() for i in range(len(S))])
        pick = sorted(set(np.argsort(W, kind="stable")[:keep].tolist()) | set(np.flatnonzero(local).tolist()))
    best, bn = math.inf, None
    for i in pick:
        w, n, _, _, _ = descend(c1, c2, tuple(S[i]), pen_tol, pen_iters, offset, max_iters)
        if w < best:
            best, bn = w, n
    return best + r1 + r2, bn
