"""Configuration clearance: the fp64 host mirror of the device routines (csrc/rsim_clear.hip, rsim_config_fk / rsim_config_pairs / rsim_config_clearance) --
"is this joint configuration free, and by how much?" for candidate joint vectors that are never written into the state.

One env, float64, built on the layers that exist: mjcf.kinematics_np is FK, distance.geom_distance the per-pair distance, distance.reduce_min the minimum.  It
shares no code with csrc/ -- the idiom of ik.py and distance.py; the kernels are tested against this file (tests/test_clearance.py), this file against brute
force (tests/test_clearance_host.py).

    moved_bodies(flat, dofs)      -> the bodies with a controlled joint on their path to the world, ascending (parents first)
    signatures(flat, dofs)        -> int [nbody]: bit c set = controlled column c is on the body's path (0: the body is not moved)
    default_pairs(flat, dofs)     -> int32 [P, 2]: the model's collision pairs whose two bodies have different signatures, in the collision list's order
    fk(flat, qpos, dofs, q, overrides=None)  -> (xpos [nbody, 3], xquat [nbody, 4]) at the candidate, on fp32-rounded parameters (ik.rounded)
    clearance(flat, qpos, dofs, q, pairs=None, distmax=1.0, tol=1e-6, max_iters=64, params=None, overrides=None) -> (dist, pair, fromto [6], status)

Semantics (include/rsim.h).  A candidate holds positions of the controlled dofs, each of a hinge or slide joint; every other joint is held at `qpos`, and no
range clamp is applied.  dist is the minimum over the pair list of that pair's geom distance at the candidate's poses, pair the index into the list of the pair
that attains it (the lowest on ties), fromto and status that pair's; with no pair closer than distmax: (distmax, -1, zeros, distance.FAR).  A pair whose two
bodies have the same signature cannot be changed by any candidate: the default list drops it, and skips what the distance query refuses.  NOT HANDLED: a
grasped object does not move with the candidate -- it is a free body at its current pose."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from . import distance, ik, mjcf

MAX_DOFS = 16      # RSIM_JNT_MAX


class ClearanceError(ValueError):
    pass


def _I(flat, name):
    return np.asarray(flat.arrays[name]).ravel().astype(int)


def _columns(flat, dofs):
    """{joint id: controlled column}, or ClearanceError naming what the query refuses"""
    dofs = [int(d) for d in np.asarray(dofs).ravel()]
    if not 1 <= len(dofs) <= MAX_DOFS:
        raise ClearanceError(f"clearance: ndof {len(dofs)} outside 1..{MAX_DOFS}")
    jtype, dadr, nv = _I(flat, "jnt_type"), _I(flat, "jnt_dofadr"), int(flat.nv)
    names = flat.names.get("joint", []) if hasattr(flat, "names") else []
    out = {}
    for c, d in enumerate(dofs):
        if d < 0 or d >= nv:
            raise ClearanceError(f"clearance: controlled dof {d} out of range ({nv} dofs)")
        if d in dofs[:c]:
            raise ClearanceError(f"clearance: dof {d} is listed twice")
        width = np.where(jtype == mjcf.JNT_FREE, 6, np.where(jtype == mjcf.JNT_BALL, 3, 1))
        j = int(np.flatnonzero((dadr <= d) & (d < dadr + width))[0])
        if jtype[j] not in (mjcf.JNT_HINGE, mjcf.JNT_SLIDE):
            nm = f"joint {j}" + (f" ({names[j]})" if j < len(names) and names[j] else "")
            raise ClearanceError(f"clearance: controlled dof {d} belongs to {nm}, a {'free' if jtype[j] == mjcf.JNT_FREE else 'ball'} joint (hinge and slide joints only)")
        out[j] = c
    return out


def signatures(flat, dofs):
    """int [nbody]: the dof signature of every body as a bit mask of controlled columns"""
    col = _columns(flat, dofs)
    parent, jadr, jnum = _I(flat, "body_parentid"), _I(flat, "body_jntadr"), _I(flat, "body_jntnum")
    jtype = _I(flat, "jnt_type")
    mocap = _I(flat, "body_mocapid") if "body_mocapid" in flat.arrays else np.full(len(parent), -1)
    sig = np.zeros(int(flat.nbody), dtype=np.int64)
    for b in range(1, int(flat.nbody)):
        if not 0 <= parent[b] < b:
            raise ClearanceError(f"clearance: body {b} names parent {parent[b]}: the body tree is not in topological order")
        s = int(sig[parent[b]])
        for j in range(jadr[b], jadr[b] + jnum[b]):
            if j in col:
                s |= 1 << col[j]
        sig[b] = s
        if s and mocap[b] >= 0:
            raise ClearanceError(f"clearance: body {b}, which the controlled dofs move, is a mocap body")
        if s and any(jtype[j] == mjcf.JNT_FREE for j in range(jadr[b], jadr[b] + jnum[b])):
            raise ClearanceError(f"clearance: body {b}, which the controlled dofs move, has a free joint")
    return sig


def moved_bodies(flat, dofs):
    return [int(b) for b in np.flatnonzero(signatures(flat, dofs))]


def default_pairs(flat, dofs):
    """The model's collision pair list restricted to candidate-dependent pairs (the two bodies' signatures differ), in the list's order; pairs the distance
    query refuses (visual-only meshes, heightfields, plane against plane) are skipped.  An empty list is an error."""
    sig = signatures(flat, dofs)
    gbody, gtype = _I(flat, "geom_bodyid"), _I(flat, "geom_type")
    carried = (mjcf.GEOM_PLANE, mjcf.GEOM_SPHERE, mjcf.GEOM_CAPSULE, mjcf.GEOM_ELLIPSOID, mjcf.GEOM_CYLINDER, mjcf.GEOM_BOX, mjcf.GEOM_MESH)
    ok = lambda g: gtype[g] in carried and not (gtype[g] == mjcf.GEOM_MESH and distance.mesh_verts(flat, g) is None)      # noqa: E731
    out = []
    if "pair_geom1" in flat.arrays:
        for a, b in zip(_I(flat, "pair_geom1"), _I(flat, "pair_geom2")):
            if a == b or not ok(a) or not ok(b) or (gtype[a] == mjcf.GEOM_PLANE and gtype[b] == mjcf.GEOM_PLANE):
                continue
            if sig[gbody[a]] != sig[gbody[b]]:
                out.append((int(a), int(b)))
    if not out:
        raise ClearanceError("clearance: the default pair list is empty: no collision pair of the model depends on the controlled dofs")
    return np.asarray(out, dtype=np.int32)


def _model32(flat, overrides=None):
    """the model with every table FK reads rounded to float32: what the device holds"""
    m = mjcf.FlatModel()
    m.arrays = OrderedDict(flat.arrays)
    m.names = flat.names
    for k, v in ik.rounded(flat, overrides).items():
        m.arrays[k] = v.reshape(np.asarray(flat.arrays[k]).shape)
    return m


def candidate_qpos(flat, qpos, dofs, q):
    """qpos with the controlled joints set to the candidate"""
    col = _columns(flat, dofs)
    qa = _I(flat, "jnt_qposadr")
    out = np.asarray(qpos, dtype=np.float64).ravel().copy()
    q = np.asarray(q, dtype=np.float64).ravel()
    if len(q) != len(col):
        raise ClearanceError(f"clearance: a candidate holds {len(col)} positions, got {len(q)}")
    for j, c in col.items():
        out[qa[j]] = q[c]
    return out


def fk(flat, qpos, dofs, q, overrides=None, model32=None):
    """(xpos [nbody, 3], xquat [nbody, 4]) of every body with the controlled dofs at q and every other joint at qpos: mjcf.kinematics_np on the parameters
    rounded to fp32.  overrides: {field: array} the env's own tables (ik.FIELDS); model32: the result of an earlier _model32 call, to save the rounding."""
    signatures(flat, dofs)      # (the refusals)
    m = model32 if model32 is not None else _model32(flat, overrides)
    xpos, xquat = mjcf.kinematics_np(m, candidate_qpos(flat, qpos, dofs, q))[:2]
    return xpos, xquat


def clearance(flat, qpos, dofs, q, pairs=None, distmax=1.0, tol=distance.DEFAULTS["tol"], max_iters=distance.DEFAULTS["max_iters"], params=None, overrides=None,
              poses=None):
    """One candidate: -> (dist, pair, fromto [6], status).  pairs=None: default_pairs.  params: the env's geom arrays (distance.world_geoms); overrides: its FK
    tables; poses: (xpos, xquat) to use instead of fk() -- the device tests hand the device's own poses in, to hold the distance layer apart from FK."""
    p = default_pairs(flat, dofs) if pairs is None else distance.check_pairs(flat, pairs)
    xpos, xquat = fk(flat, qpos, dofs, q, overrides) if poses is None else poses
    d, ft, st = distance.geom_distance(flat, xpos, xquat, p, distmax, tol, max_iters, params)
    near = np.where((st & distance.FAR) == 0, d, np.inf)      # (a far pair reads distmax: it never attains the minimum)
    rd, rf, rk = distance.reduce_min(near, ft)
    if not rd < distmax:
        return float(distmax), -1, np.zeros(6), distance.FAR
    return float(rd), int(rk), rf, int(st[rk])
