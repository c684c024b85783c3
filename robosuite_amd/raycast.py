"""Ray casting: cameras, and the fp64 host mirror of the device routine (csrc/rsim_ray.hip).

The mirror is float64 numpy, one env, written from MuJoCo's documentation of mj_ray / mju_rayGeom and of the rangefinder sensor [3P, docs "API reference:
ray collisions", "XML reference: sensor/rangefinder"] and sharing no code with csrc/ -- the idiom of sensors.py.  The kernel is tested against this file
(tests/test_raycast.py); this file is tested against closed forms (tests/test_raycast_host.py).  The face planes of a mesh geom's convex hull come from
scipy's qhull here and from the MJCF compiler's own quickhull in the library.

    cast(flat, xpos, xquat, origins, dirs, geomgroup=0, static=True, bodyexclude=-1, params=None) -> (dist [N], geomid [N])
    render_depth(flat, xpos, xquat, camera, height, width, **opts)                                 -> (depth [H, W], geomid [H, W])
    well_conditioned(flat, xpos, xquat, origins, dirs, **opts)                                     -> bool [N]

Semantics (include/rsim.h rsim_ray): the nearest surface point at t >= 0 along origin + t dir, t in units of |dir|; a start inside a solid reports where the
ray leaves it; a plane is hit only from +Z, bounded by its non-zero sizes; a mesh geom is its convex hull; ties go to the lower geom id; a miss is (-1, -1).
"""
from __future__ import annotations

import xml.etree.ElementTree as ET
from dataclasses import dataclass, field

import numpy as np

from . import mjcf

RANGEFINDER = mjcf.RAY_SENSOR_TYPES["rangefinder"]


@dataclass
class Camera:
    """A pinhole camera fixed in a body frame (body 0 = world): looks along its -Z, +Y up (MuJoCo's camera frame); fovy in degrees."""
    body: int = 0
    pos: tuple = (0.0, 0.0, 0.0)
    quat: tuple = (1.0, 0.0, 0.0, 0.0)
    fovy: float = 45.0
    name: str | None = field(default=None, compare=False)


def cameras_from_xml(xml: str, flat) -> dict:
    """{name: Camera} of the <camera> elements of an MJCF string: pos, orientation (quat / euler / axisangle / xyaxes / zaxis, under the <compiler> angle and
    eulerseq settings) and fovy; `flat` is the model compiled from the same string (it names the bodies).  Only fixed cameras: any other `mode` is refused."""
    root = ET.fromstring(xml)
    comp = root.find("compiler")
    compiler = {"angle": comp.get("angle", "degree") if comp is not None else "degree", "eulerseq": comp.get("eulerseq", "xyz") if comp is not None else "xyz"}
    defaults = mjcf._Defaults(root)
    found, nbody = [], [0]

    def walk(belem, bid, childclass):      # the compiler's own order: a body's cameras, then its child bodies depth-first
        cc = belem.get("childclass") or childclass
        for ch in belem:
            if ch.tag == "camera":
                found.append((defaults.apply(ch, "camera", cc), bid))
        for ch in belem:
            if ch.tag == "body":
                nbody[0] += 1
                walk(ch, nbody[0], cc)

    wb = root.find("worldbody")
    if wb is not None:
        walk(wb, 0, None)
    if nbody[0] + 1 != int(flat.nbody):
        raise mjcf.MJCFError(f"cameras_from_xml: the XML has {nbody[0] + 1} bodies, the compiled model {int(flat.nbody)}")
    out = {}
    for i, (e, bid) in enumerate(found):
        name = e.get("name") or f"camera{i}"
        mode = e.get("mode", "fixed")
        if mode != "fixed":
            raise NotImplementedError(f"camera {name!r}: mode {mode!r} is not carried (fixed cameras only; tracking and targeting cameras are out of scope)")
        out[name] = Camera(body=bid, pos=tuple(mjcf._floats(e.get("pos"), 3, [0, 0, 0])), quat=tuple(mjcf._orientation(e, compiler)),
                           fovy=float(e.get("fovy", 45.0)), name=name)
    return out


# ---- the mirror ------------------------------------------------------------------------------------------------------------------------------------
def _rot(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def hull_planes(verts) -> np.ndarray:
    """Face planes [n, 4] = (unit outward normal, d), n . x <= d inside, of the convex hull of `verts`, one per facet (qhull merges coplanar triangles; the
    triangles of one merged facet carry the same equation)."""
    from scipy.spatial import ConvexHull

    eq = ConvexHull(np.asarray(verts, dtype=np.float64)).equations      # n . x + c <= 0
    planes = np.concatenate([eq[:, :3], -eq[:, 3:]], axis=1)
    _, first = np.unique(np.round(planes, 12), axis=0, return_index=True)
    return planes[np.sort(first)]


def _interval_quadratic(a, b, c):
    """[t0, t1] with a t^2 + 2 b t + c <= 0 (a > 0); empty -> (inf, -inf)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        disc = b * b - a * c
        s = np.sqrt(np.where(disc >= 0, disc, 0.0))
        ok = (disc >= 0) & (a > 0)
        return np.where(ok, (-b - s) / a, np.inf), np.where(ok, (-b + s) / a, -np.inf)


def _interval_slab(p, d, h, lo, hi):
    """intersect [lo, hi] with |p + t d| <= h"""
    with np.errstate(invalid="ignore", divide="ignore"):
        par = d == 0.0
        t0, t1 = (-h - p) / np.where(par, 1.0, d), (h - p) / np.where(par, 1.0, d)
        a, b = np.minimum(t0, t1), np.maximum(t0, t1)
        out = par & (np.abs(p) > h)
        lo = np.where(par, lo, np.maximum(lo, a))
        hi = np.where(par, hi, np.minimum(hi, b))
        return np.where(out, np.inf, lo), np.where(out, -np.inf, hi)


def _interval_cylinder(p, d, r, h):
    a = d[:, 0] ** 2 + d[:, 1] ** 2
    b = p[:, 0] * d[:, 0] + p[:, 1] * d[:, 1]
    c = p[:, 0] ** 2 + p[:, 1] ** 2 - r * r
    par = a == 0.0
    lo, hi = _interval_quadratic(np.where(par, 1.0, a), b, c)
    lo = np.where(par, np.where(c > 0, np.inf, -np.inf), lo)
    hi = np.where(par, np.where(c > 0, -np.inf, np.inf), hi)
    return _interval_slab(p[:, 2], d[:, 2], h, lo, hi)


def _geom_interval(gtype, size, planes, p, d):
    """parameter interval [lo, hi] of the lines p + t d (geom frame, [N, 3] each) inside the solid; lo > hi: empty.  A plane returns lo = hi = its one-sided hit."""
    n = len(p)
    if gtype == mjcf.GEOM_PLANE:
        with np.errstate(invalid="ignore", divide="ignore"):
            ok = (d[:, 2] < 0) & (p[:, 2] >= 0)
            t = -p[:, 2] / np.where(ok, d[:, 2], -1.0)
            x, y = p[:, 0] + t * d[:, 0], p[:, 1] + t * d[:, 1]
            if size[0] > 0:
                ok &= np.abs(x) <= size[0]
            if size[1] > 0:
                ok &= np.abs(y) <= size[1]
        return np.where(ok, t, np.inf), np.where(ok, t, -np.inf)
    if gtype == mjcf.GEOM_SPHERE:
        return _interval_quadratic((d * d).sum(1), (p * d).sum(1), (p * p).sum(1) - size[0] ** 2)
    if gtype == mjcf.GEOM_ELLIPSOID:
        ps, ds = p / size, d / size
        return _interval_quadratic((ds * ds).sum(1), (ps * ds).sum(1), (ps * ps).sum(1) - 1.0)
    if gtype == mjcf.GEOM_BOX:
        lo, hi = np.full(n, -np.inf), np.full(n, np.inf)
        for k in range(3):
            lo, hi = _interval_slab(p[:, k], d[:, k], size[k], lo, hi)
        return lo, hi
    if gtype == mjcf.GEOM_CYLINDER:
        return _interval_cylinder(p, d, size[0], size[1])
    if gtype == mjcf.GEOM_CAPSULE:             # the union of the cylinder and the two end spheres, which overlap inside the solid
        lo, hi = _interval_cylinder(p, d, size[0], size[1])
        for s in (size[1], -size[1]):
            q = p - np.array([0.0, 0.0, s])
            l2, h2 = _interval_quadratic((d * d).sum(1), (q * d).sum(1), (q * q).sum(1) - size[0] ** 2)
            e1, e2 = lo > hi, l2 > h2
            lo, hi = np.where(e1, l2, np.where(e2, lo, np.minimum(lo, l2))), np.where(e1, h2, np.where(e2, hi, np.maximum(hi, h2)))
        return lo, hi
    if gtype == mjcf.GEOM_MESH:                # the largest entering and the smallest leaving parameter over the hull's planes n . x <= d
        with np.errstate(invalid="ignore", divide="ignore"):
            den, num = d @ planes[:, :3].T, planes[:, 3] - p @ planes[:, :3].T          # [N, nplane]
            par = den == 0.0
            t = num / np.where(par, 1.0, den)
            lo = np.where(~par & (den < 0), t, -np.inf).max(axis=1)
            hi = np.where(~par & (den > 0), t, np.inf).min(axis=1)
            out = (par & (num < 0)).any(axis=1)
        return np.where(out, np.inf, lo), np.where(out, -np.inf, hi)
    return np.full(n, np.inf), np.full(n, -np.inf)      # heightfields and unknown types are not carried


_PLANE_CACHE: dict = {}


def _mesh_planes(flat, g):
    I = lambda name: np.asarray(flat.arrays[name]).ravel().astype(int)
    did = I("geom_dataid")[g]
    adr, num = I("mesh_vertadr")[did], I("mesh_vertnum")[did]
    V = np.asarray(flat.arrays["mesh_vert"], dtype=np.float64).reshape(-1, 3)[adr:adr + num]
    key = (V.tobytes(),)
    if key not in _PLANE_CACHE:
        _PLANE_CACHE[key] = hull_planes(V)
    return _PLANE_CACHE[key]


def cast(flat, xpos, xquat, origins, dirs, geomgroup=0, static=True, bodyexclude=-1, params=None):
    """One env.  xpos [nbody, 3], xquat [nbody, 4]: the body poses; origins / dirs [N, 3]; bodyexclude: one body id or [N]; params: {"geom_size" | "geom_pos" |
    "geom_quat": array} the env's own values where they differ from the model's.  -> (dist float64 [N], geomid int [N])."""
    A = lambda name, w: np.asarray((params or {}).get(name, flat.arrays[name]), dtype=np.float64).reshape(-1, w)
    I = lambda name: np.asarray(flat.arrays[name]).ravel().astype(int)
    o, d = np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    n = len(o)
    xpos, xquat = np.asarray(xpos, dtype=np.float64).reshape(-1, 3), np.asarray(xquat, dtype=np.float64).reshape(-1, 4)
    gtype, gbody, ggroup, gdata = I("geom_type"), I("geom_bodyid"), I("geom_group"), I("geom_dataid")
    gsize, gpos, gquat, rgba = A("geom_size", 3), A("geom_pos", 3), A("geom_quat", 4), A("geom_rgba", 4)
    excl = np.broadcast_to(np.asarray(bodyexclude, dtype=int), (n,))
    best, bestg = np.full(n, np.inf), np.full(n, -1)
    for g in range(len(gtype)):
        b = gbody[g]
        if rgba[g, 3] == 0 or (geomgroup and not (int(geomgroup) >> int(ggroup[g])) & 1) or (b == 0 and not static):
            continue
        if gtype[g] == mjcf.GEOM_MESH and gdata[g] < 0:      # a mesh geom whose mesh the model does not hold (visual-only meshes): nothing to hit
            continue
        Rb = _rot(xquat[b])
        R = Rb @ _rot(gquat[g])
        pos = xpos[b] + Rb @ gpos[g]
        p, dl = (o - pos) @ R, d @ R            # rows: R^T (o - pos), R^T d
        lo, hi = _geom_interval(gtype[g], gsize[g], _mesh_planes(flat, g) if gtype[g] == mjcf.GEOM_MESH else None, p, dl)
        t = np.where(lo >= 0, lo, hi)
        hit = (lo <= hi) & (t >= 0) & (excl != b) & (t < best)
        best, bestg = np.where(hit, t, best), np.where(hit, g, bestg)
    return np.where(bestg >= 0, best, -1.0), bestg


def camera_pose(camera: Camera, xpos, xquat):
    """(position, rotation matrix) of the camera frame in the world"""
    xpos, xquat = np.asarray(xpos, dtype=np.float64).reshape(-1, 3), np.asarray(xquat, dtype=np.float64).reshape(-1, 4)
    Rb = _rot(xquat[camera.body])
    return xpos[camera.body] + Rb @ np.asarray(camera.pos, dtype=np.float64), Rb @ _rot(camera.quat)


def pixel_rays(camera: Camera, xpos, xquat, height: int, width: int):
    """(origins, dirs) [H * W, 3] of the pixel centres, row 0 at the top: in the camera frame the direction of pixel (r, c) is
    (a tan(fovy / 2) (2 (c + 1/2) / W - 1), tan(fovy / 2) (1 - 2 (r + 1/2) / H), -1), a = W / H -- t along such a ray is the depth along the optical axis."""
    pos, R = camera_pose(camera, xpos, xquat)
    th = np.tan(0.5 * np.deg2rad(float(camera.fovy)))
    r, c = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    dc = np.stack([(width / height) * th * (2 * (c + 0.5) / width - 1), th * (1 - 2 * (r + 0.5) / height), -np.ones_like(r, dtype=np.float64)], axis=-1).reshape(-1, 3)
    return np.broadcast_to(pos, dc.shape).copy(), dc @ R.T


def render_depth(flat, xpos, xquat, camera: Camera, height: int, width: int, **opts):
    """-> (depth [H, W], +inf where nothing is hit; geomid [H, W], -1 there)"""
    o, d = pixel_rays(camera, xpos, xquat, height, width)
    t, g = cast(flat, xpos, xquat, o, d, **opts)
    return np.where(g >= 0, t, np.inf).reshape(height, width), g.reshape(height, width)


def well_conditioned(flat, xpos, xquat, origins, dirs, angle=1e-4, rel=0.01, **opts):
    """bool [N]: the ray is no silhouette or grazing hit -- tilted by `angle` rad towards four directions across it, it hits the same geom (or misses as
    before) and its distance moves by no more than `rel` of itself.  Decided by the mirror alone."""
    o, d = np.asarray(origins, dtype=np.float64).reshape(-1, 3), np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    t0, g0 = cast(flat, xpos, xquat, o, d, **opts)
    ln = np.linalg.norm(d, axis=1, keepdims=True)
    u = d / ln
    k = np.where(np.abs(u[:, :1]) < 0.7, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    e1 = np.cross(u, k)
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(u, e1)
    ok = np.ones(len(o), dtype=bool)
    for e in (e1, -e1, e2, -e2):
        t, g = cast(flat, xpos, xquat, o, (u * np.cos(angle) + e * np.sin(angle)) * ln, **opts)
        ok &= (g == g0) & ((g0 < 0) | (np.abs(t - t0) <= rel * np.abs(t0)))
    return ok


def rangefinder_values(flat, xpos, xquat, params=None):
    """{sensor index: distance} of the carried rangefinders: from the site along its +Z, the site's body excluded, all groups, static geoms included; -1 when
    nothing is hit.  params may also carry the env's own "site_pos" / "site_quat"."""
    I = lambda name: np.asarray(flat.arrays[name]).ravel().astype(int)
    A = lambda name, w: np.asarray((params or {}).get(name, flat.arrays[name]), dtype=np.float64).reshape(-1, w)
    out = {}
    if int(flat.nsensor) == 0 or "sensor_reason" not in flat.arrays:
        return out
    xpos, xquat = np.asarray(xpos, dtype=np.float64).reshape(-1, 3), np.asarray(xquat, dtype=np.float64).reshape(-1, 4)
    stype, sobj, sreason = I("sensor_type"), I("sensor_objid"), I("sensor_reason")
    for i in range(int(flat.nsensor)):
        if stype[i] != RANGEFINDER or sreason[i] != 0:
            continue
        body = I("site_bodyid")[sobj[i]]
        Rb = _rot(xquat[body])
        o = xpos[body] + Rb @ A("site_pos", 3)[sobj[i]]
        d = Rb @ _rot(A("site_quat", 4)[sobj[i]]) @ np.array([0.0, 0.0, 1.0])
        out[i] = float(cast(flat, xpos, xquat, o[None], d[None], bodyexclude=body, params=params)[0][0])
    return out
