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
    clearance / clearance_grad (..., signed=True, pen=None): the minimum over the SIGNED per-pair values (penetration.pair_signed), include/rsim.h
                                  rsim_config_clearance_signed / rsim_config_clearance_grad_signed

Semantics (include/rsim.h).  A candidate holds positions of the controlled dofs, each of a hinge or slide joint; every other joint is held at `qpos`, and no
range clamp is applied.  dist is the minimum over the pair list of that pair's geom distance at the candidate's poses, pair the index into the list of the pair
that attains it (the lowest on ties), fromto and status that pair's; with no pair closer than distmax: (distmax, -1, zeros, distance.FAR).  A pair whose two
bodies have the same signature cannot be changed by any candidate: the default list drops it, and skips what the distance query refuses.

Carried objects (include/rsim.h rsim_attach).  attach = [(body, carrier), ...], up to ATTACH_MAX pairs of body ids: `body` a child of the world whose only joint
is a free joint, `carrier` a body the dofs move.  held = ONE env's row, a bool per attachment (None: all held); rel = that env's [n, 7] rows, position and wxyz
quaternion of body in the carrier's frame (None: from the poses at qpos, p_rel = R_c^T (p_b - p_c), q_rel = conj(q_c) q_b).  A held body rides on its carrier,
X_body(q) = X_carrier(q) o rel, its free joint ignored, the bodies below it walked with their joints at qpos; it and its subtree take the carrier's signature.
One that is not held is the free body at its current pose, with its own (empty) signature.  The default list with attachments holds the pairs whose two
signatures differ under at least one held row; an env evaluates a listed pair only if they differ under its own row (active_pairs); an explicit list is taken
as given, every pair in every env.  Without attach every function here is what it was.

    active_pairs(flat, dofs, pairs, attach, held) -> bool [P]: which pairs of the default list an env with that held row evaluates

Gradients and the collision cost (include/rsim.h rsim_config_clearance_grad / rsim_config_collision_cost, csrc/rsim_grad.hip).

    joint_frames(flat, qpos, dofs, q, overrides=None, model32=None) -> (axis [n, 3], anchor [n, 3], slide bool [n]): world axis and anchor of every controlled
                                     column at the candidate, from mjcf.kinematics_np's walk on the fp32-rounded model
    pair_grad(frames, s1, s2, p1, p2, d) -> [n]: n . (s2_c v_c(p2) - s1_c v_c(p1)), n = (p2 - p1) / d, v_c(p) = a_c x (p - anchor_c) for a hinge, a_c for a slide
    reduce_grad / reduce_cost        the two below from per-pair results (distance.geom_distance's), for a caller that has them already
    clearance_grad(...)  -> clearance(...)'s four and grad [n]: pair_grad of the pair that attains the minimum; zeros for a far result, an OVERLAP status
                                     and |dist| < GRAD_MIN_DIST
    collision_cost(flat, qpos, dofs, q, pairs=None, d_safe=0.05, ...) -> (cost, grad [n], nnear, noverlap): every pair the env evaluates with distmax = d_safe; a
                                     pair with d < d_safe adds 1/2 (d_safe - d)^2 and -(d_safe - d) grad d (the zero rules), an overlapping one 1/2 d_safe^2 only

NOT HANDLED: deciding whether an object is grasped (the caller says so); an object attached to an attached object; per-env skipping for explicit lists."""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from . import distance, ik, mjcf

MAX_DOFS = 16      # RSIM_JNT_MAX
ATTACH_MAX = 4     # RSIM_ATTACH_MAX
GRAD_MIN_DIST = 1e-7      # RSIM_GRAD_MIN_DIST


class ClearanceError(ValueError):
    pass


def _I(flat, name):
    return np.asarray(flat.arrays[name]).ravel().astype(int)


def _joint_name(flat, j):
    """'joint 3 (name)', the words of rsim_api.cpp ik_joint_name"""
    names = flat.names.get("joint", []) if hasattr(flat, "names") else []
    return f"joint {j}" + (f" ({names[j]})" if j < len(names) and names[j] else "")


def _columns(flat, dofs):
    """{joint id: controlled column}, or ClearanceError naming what the query refuses"""
    dofs = [int(d) for d in np.asarray(dofs).ravel()]
    if not 1 <= len(dofs) <= MAX_DOFS:
        raise ClearanceError(f"clearance: ndof {len(dofs)} outside 1..{MAX_DOFS}")
    jtype, dadr, nv = _I(flat, "jnt_type"), _I(flat, "jnt_dofadr"), int(flat.nv)
    out = {}
    for c, d in enumerate(dofs):
        if d < 0 or d >= nv:
            raise ClearanceError(f"clearance: controlled dof {d} out of range ({nv} dofs)")
        if d in dofs[:c]:
            raise ClearanceError(f"clearance: dof {d} is listed twice")
        width = np.where(jtype == mjcf.JNT_FREE, 6, np.where(jtype == mjcf.JNT_BALL, 3, 1))
        j = int(np.flatnonzero((dadr <= d) & (d < dadr + width))[0])
        if jtype[j] not in (mjcf.JNT_HINGE, mjcf.JNT_SLIDE):
            raise ClearanceError(f"clearance: controlled dof {d} belongs to {_joint_name(flat, j)}, a {'free' if jtype[j] == mjcf.JNT_FREE else 'ball'} joint (hinge and slide joints only)")
        out[j] = c
    return out


def signatures(flat, dofs, attach=None, held=None):
    """int [nbody]: the dof signature of every body as a bit mask of controlled columns; with attach, under one env's held row (None: all held)"""
    sig = _signatures(flat, dofs)
    att = _attachments(flat, dofs, attach, sig)
    for (body, carrier), h in zip(att, _held_row(att, held)):
        if h:
            sig[subtree(flat, body)] = sig[carrier]
    return sig


def subtree(flat, body):
    """the body and every body below it, ascending"""
    parent = _I(flat, "body_parentid")
    out = [int(body)]
    for b in range(int(body) + 1, int(flat.nbody)):
        if parent[b] in out:
            out.append(b)
    return out


def _held_row(att, held):
    if held is None:
        return [True] * len(att)
    row = [bool(h) for h in np.asarray(held).ravel()]
    if len(row) != len(att):
        raise ClearanceError(f"clearance: held has {len(row)} entries for {len(att)} attachments")
    return row


def _attachments(flat, dofs, attach, sig=None):
    """[(body, carrier), ...] as ints, or ClearanceError naming what the query refuses (the order and the words of rsim_api.cpp clear_plan)"""
    if attach is None or len(attach) == 0:
        return []
    att = [(int(b), int(c)) for b, c in np.asarray(attach).reshape(-1, 2)]
    if len(att) > ATTACH_MAX:
        raise ClearanceError(f"clearance: {len(att)} attachments outside 0..{ATTACH_MAX} (RSIM_ATTACH_MAX)")
    sig = _signatures(flat, dofs) if sig is None else sig
    col = _columns(flat, dofs)
    nbody = int(flat.nbody)
    parent, jadr, jnum, jtype = _I(flat, "body_parentid"), _I(flat, "body_jntadr"), _I(flat, "body_jntnum"), _I(flat, "jnt_type")
    mocap = _I(flat, "body_mocapid") if "body_mocapid" in flat.arrays else np.full(nbody, -1)
    att_of = np.full(nbody, -1)
    for i, (body, carrier) in enumerate(att):
        for x in (body, carrier):
            if not 0 <= x < nbody:
                raise ClearanceError(f"clearance: attachment {i}: body id {x} out of range ({nbody} bodies)")
        if body in [a[0] for a in att[:i]]:
            raise ClearanceError(f"clearance: attachment {i}: body {body} is attached twice")
        if mocap[body] >= 0:
            raise ClearanceError(f"clearance: attachment {i}: body {body} is a mocap body")
        if body == 0 or parent[body] != 0 or jnum[body] != 1 or jtype[jadr[body]] != mjcf.JNT_FREE:
            raise ClearanceError(f"clearance: attachment {i}: body {body} is not a child of the world with exactly one free joint")
        for c in subtree(flat, body):
            att_of[c] = i
            for j in range(jadr[c], jadr[c] + jnum[c]) if c != body else ():
                if jtype[j] == mjcf.JNT_FREE:
                    raise ClearanceError(f"clearance: attachment {i}: {_joint_name(flat, j)} of body {c}, below the attached body {body}, is a free joint")
                if j in col:
                    raise ClearanceError(f"clearance: attachment {i}: {_joint_name(flat, j)} of body {c}, below the attached body {body}, is a controlled joint")
            if c != body and mocap[c] >= 0:
                raise ClearanceError(f"clearance: attachment {i}: body {c}, below the attached body {body}, is a mocap body")
    for i, (body, carrier) in enumerate(att):
        if att_of[carrier] >= 0:
            raise ClearanceError(f"clearance: attachment {i}: carrier {carrier} is an attached body or below one")
        if not sig[carrier]:
            raise ClearanceError(f"clearance: attachment {i}: carrier {carrier} is not moved by the controlled dofs")
    return att


def _signatures(flat, dofs):
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


def _held_rows(n):
    return [[bool((r >> i) & 1) for i in range(n)] for r in range(1 << n)]


def active_pairs(flat, dofs, pairs, attach, held):
    """bool [P]: the pairs of a default list that an env with this held row evaluates -- those whose two bodies' signatures differ under it"""
    sig, gbody = signatures(flat, dofs, attach, held), _I(flat, "geom_bodyid")
    return np.array([sig[gbody[a]] != sig[gbody[b]] for a, b in np.asarray(pairs).reshape(-1, 2)], dtype=bool)


def default_pairs(flat, dofs, attach=None):
    """The model's collision pair list restricted to candidate-dependent pairs (the two bodies' signatures differ; with attach: under at least one held row),
    in the list's order; pairs the distance query refuses (visual-only meshes, heightfields, plane against plane) are skipped.  An empty list is an error."""
    att = _attachments(flat, dofs, attach)
    sigs = [signatures(flat, dofs, att, row) for row in _held_rows(len(att))]
    gbody, gtype = _I(flat, "geom_bodyid"), _I(flat, "geom_type")
    carried = (mjcf.GEOM_PLANE, mjcf.GEOM_SPHERE, mjcf.GEOM_CAPSULE, mjcf.GEOM_ELLIPSOID, mjcf.GEOM_CYLINDER, mjcf.GEOM_BOX, mjcf.GEOM_MESH)
    ok = lambda g: gtype[g] in carried and not (gtype[g] == mjcf.GEOM_MESH and distance.mesh_verts(flat, g) is None)      # noqa: E731
    out = []
    if "pair_geom1" in flat.arrays:
        for a, b in zip(_I(flat, "pair_geom1"), _I(flat, "pair_geom2")):
            if a == b or not ok(a) or not ok(b) or (gtype[a] == mjcf.GEOM_PLANE and gtype[b] == mjcf.GEOM_PLANE):
                continue
            if any(sig[gbody[a]] != sig[gbody[b]] for sig in sigs):
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


def relative_poses(flat, qpos, attach, rel=None, overrides=None, model32=None, xpos=None, xquat=None):
    """[n, 7]: position and unit wxyz quaternion of every attached body in its carrier's frame -- the rows of rel, the quaternion normalised, or (rel None)
    from the env's current poses: xpos / xquat if given, else FK at qpos"""
    att = [(int(b), int(c)) for b, c in np.asarray(attach).reshape(-1, 2)]
    if rel is not None:
        out = np.asarray(rel, dtype=np.float64).reshape(len(att), 7).copy()
        out[:, 3:] /= np.linalg.norm(out[:, 3:], axis=1, keepdims=True)
        return out
    if xpos is None:
        m = model32 if model32 is not None else _model32(flat, overrides)
        xpos, xquat = mjcf.kinematics_np(m, np.asarray(qpos, dtype=np.float64).ravel())[:2]
    out = np.zeros((len(att), 7))
    for i, (body, carrier) in enumerate(att):
        conj = np.asarray(xquat[carrier], dtype=np.float64) * [1, -1, -1, -1]
        out[i, :3] = mjcf.quat2mat(xquat[carrier]).T @ (np.asarray(xpos[body], dtype=np.float64) - xpos[carrier])
        out[i, 3:] = mjcf.quat_mul(conj, xquat[body])
    return out


def fk(flat, qpos, dofs, q, overrides=None, model32=None, attach=None, held=None, rel=None, now=None):
    """(xpos [nbody, 3], xquat [nbody, 4]) of every body with the controlled dofs at q and every other joint at qpos: mjcf.kinematics_np on the parameters
    rounded to fp32.  overrides: {field: array} the env's own tables (ik.FIELDS); model32: the result of an earlier _model32 call, to save the rounding.
    attach / held / rel: the env's carried objects (the module's docstring); now: (xpos, xquat) the env's current poses, which rel=None is taken from and a
    body that is not held keeps (None: FK at qpos)."""
    sig = _signatures(flat, dofs)      # (the refusals)
    att = _attachments(flat, dofs, attach, sig)
    m = model32 if model32 is not None else _model32(flat, overrides)
    qc = candidate_qpos(flat, qpos, dofs, q)
    xpos, xquat = mjcf.kinematics_np(m, qc)[:2]
    if not att:
        return xpos, xquat
    r = relative_poses(flat, qpos, att, rel, model32=m, xpos=None if now is None else now[0], xquat=None if now is None else now[1])
    jadr, qa = _I(flat, "body_jntadr"), _I(flat, "jnt_qposadr")
    for (body, carrier), h, ri in zip(att, _held_row(att, held), r):
        below = subtree(flat, body)
        if h:
            p = xpos[carrier] + mjcf.quat2mat(xquat[carrier]) @ ri[:3]
            qb = mjcf.quat_normalize(mjcf.quat_mul(xquat[carrier], ri[3:]))
            if len(below) > 1:      # the bodies below it: the walk from the composed pose, their joints at qpos
                a = qa[jadr[body]]
                qc[a:a + 3], qc[a + 3:a + 7] = p, qb
                sp, sq = mjcf.kinematics_np(m, qc)[:2]
                xpos[below], xquat[below] = sp[below], sq[below]
            xpos[body], xquat[body] = p, qb
        elif now is not None:
            xpos[below], xquat[below] = np.asarray(now[0])[below], np.asarray(now[1])[below]
    return xpos, xquat


def clearance(flat, qpos, dofs, q, pairs=None, distmax=1.0, tol=distance.DEFAULTS["tol"], max_iters=distance.DEFAULTS["max_iters"], params=None, overrides=None,
              poses=None, attach=None, held=None, rel=None, signed=False, pen=None):
    """One candidate: -> (dist, pair, fromto [6], status).  pairs=None: default_pairs.  params: the env's geom arrays (distance.world_geoms); overrides: its FK
    tables; poses: (xpos, xquat) to use instead of fk() -- the device tests hand the device's own poses in, to hold the distance layer apart from FK.
    attach / held / rel: the env's carried objects; with the default list the pairs the env does not evaluate (active_pairs) are left out of the minimum,
    `pair` still indexing the whole list.  signed=True: the minimum runs over the SIGNED per-pair values (penetration.pair_signed; pen: its options), the
    lowest index on ties: a colliding candidate reports its deepest pair, dist < 0, with that pair's witnesses and status (never OVERLAP)."""
    if signed:
        p, d, ft, st, _ = _pair_distances(flat, qpos, dofs, q, pairs, distmax, tol, max_iters, params, overrides, poses, attach, held, rel, True, True, pen)
        rd, rf, rk = distance.reduce_min(np.where(((st & distance.FAR) == 0) & (d < distmax), d, np.inf), ft)
        if not rd < distmax:
            return float(distmax), -1, np.zeros(6), distance.FAR
        return float(rd), int(rk), rf, int(st[rk])
    p = default_pairs(flat, dofs, attach) if pairs is None else distance.check_pairs(flat, pairs)
    xpos, xquat = fk(flat, qpos, dofs, q, overrides, attach=attach, held=held, rel=rel) if poses is None else poses
    d, ft, st = distance.geom_distance(flat, xpos, xquat, p, distmax, tol, max_iters, params)
    if pairs is None and attach is not None and len(attach):
        st = np.where(active_pairs(flat, dofs, p, attach, held), st, st | distance.FAR)      # (reads far: never attains the minimum)
    near = np.where((st & distance.FAR) == 0, d, np.inf)      # (a far pair reads distmax: it never attains the minimum)
    rd, rf, rk = distance.reduce_min(near, ft)
    if not rd < distmax:
        return float(distmax), -1, np.zeros(6), distance.FAR
    return float(rd), int(rk), rf, int(st[rk])


# ---- gradients and the collision cost ------------------------------------------------------------------------------------------------------------------------
def joint_frames(flat, qpos, dofs, q, overrides=None, model32=None):
    """(axis [n, 3], anchor [n, 3], slide bool [n]) of the controlled columns at the candidate: what mjcf.kinematics_np's walk forms at the moment each joint is
    applied (axis = R_cur a, anchor = p_cur + R_cur jnt_pos), on the parameters rounded to fp32"""
    col = _columns(flat, dofs)
    m = model32 if model32 is not None else _model32(flat, overrides)
    xanchor, xaxis = mjcf.kinematics_np(m, candidate_qpos(flat, qpos, dofs, q))[5:7]
    jtype = _I(flat, "jnt_type")
    axis, anchor, slide = np.zeros((len(col), 3)), np.zeros((len(col), 3)), np.zeros(len(col), dtype=bool)
    for j, c in col.items():
        axis[c], anchor[c], slide[c] = xaxis[j], xanchor[j], jtype[j] == mjcf.JNT_SLIDE
    return axis, anchor, slide


def pair_grad(frames, s1, s2, p1, p2, d):
    """[n]: the derivative of the distance d between nearest points p1 (on a body with signature s1) and p2 (s2) with respect to every controlled column"""
    axis, anchor, slide = frames
    p1, p2 = np.asarray(p1, dtype=np.float64), np.asarray(p2, dtype=np.float64)
    nrm = (p2 - p1) / d
    out = np.zeros(len(axis))
    for c in range(len(axis)):
        f1, f2 = float((int(s1) >> c) & 1), float((int(s2) >> c) & 1)
        v = axis[c] * (f2 - f1) if slide[c] else np.cross(axis[c], (p2 - anchor[c]) * f2 - (p1 - anchor[c]) * f1)
        out[c] = nrm @ v
    return out


def _has_dir(d, status):
    return (int(status) & (distance.FAR | distance.OVERLAP)) == 0 and abs(d) >= GRAD_MIN_DIST


def _pair_distances(flat, qpos, dofs, q, pairs, distmax, tol, max_iters, params, overrides, poses, attach, held, rel, check_options, signed=False, pen=None):
    """the listed pairs' (list, dist, fromto, status) at the candidate, a pair the env does not evaluate reading far; and the bodies' signatures under its row.
    signed: every overlap with its negative distance and witnesses (penetration.pair_signed)"""
    p = default_pairs(flat, dofs, attach) if pairs is None else distance.check_pairs(flat, pairs)
    xpos, xquat = fk(flat, qpos, dofs, q, overrides, attach=attach, held=held, rel=rel) if poses is None else poses
    if signed:
        from . import penetration

        o = penetration.options(pen)
        G = distance.world_geoms(flat, xpos, xquat, p.ravel(), params)
        d, ft, st = np.zeros(len(p)), np.zeros((len(p), 6)), np.zeros(len(p), dtype=np.int32)
        for k, (g1, g2) in enumerate(p):
            d[k], ft[k], st[k] = penetration.pair_signed(G[int(g1)], G[int(g2)], distmax, tol, max_iters, **o)
    else:
        d, ft, st = distance.geom_distance(flat, xpos, xquat, p, distmax, tol, max_iters, params, check_options=check_options)
    if pairs is None and attach is not None and len(attach):
        st = np.where(active_pairs(flat, dofs, p, attach, held), st, st | distance.FAR)
    return p, d, ft, st, signatures(flat, dofs, attach, held)


def reduce_grad(flat, p, d, ft, st, sig, frames, distmax):
    """the minimum and its gradient from per-pair results (d, ft, st of distance.geom_distance over list p, at any distmax >= this one): -> clearance_grad's five"""
    n = len(frames[0])
    rd, rf, rk = distance.reduce_min(np.where(((st & distance.FAR) == 0) & (d < distmax), d, np.inf), ft)
    if not rd < distmax:
        return float(distmax), -1, np.zeros(6), distance.FAR, np.zeros(n)
    grad = np.zeros(n)
    if _has_dir(rd, st[rk]):
        gb = _I(flat, "geom_bodyid")
        grad = pair_grad(frames, sig[gb[p[rk][0]]], sig[gb[p[rk][1]]], rf[:3], rf[3:], rd)
    return float(rd), int(rk), rf, int(st[rk]), grad


def reduce_cost(flat, p, d, ft, st, sig, frames, d_safe, signed=False):
    """the collision cost from per-pair results (as reduce_grad): -> collision_cost's four.  signed: the results are penetration.pair_signed's, noverlap counts
    dist < 0"""
    gb = _I(flat, "geom_bodyid")
    cost, grad, nnear, nover = 0.0, np.zeros(len(frames[0])), 0, 0
    for k in range(len(p)):
        if (st[k] & distance.FAR) or not d[k] < d_safe:
            continue
        w = d_safe - d[k]
        cost += 0.5 * w * w
        nnear += 1
        nover += 1 if (d[k] < 0 if signed else st[k] & distance.OVERLAP) else 0
        if _has_dir(d[k], st[k]):
            grad -= w * pair_grad(frames, sig[gb[p[k][0]]], sig[gb[p[k][1]]], ft[k, :3], ft[k, 3:], d[k])
    return float(cost), grad, nnear, nover


def clearance_grad(flat, qpos, dofs, q, pairs=None, distmax=1.0, tol=distance.DEFAULTS["tol"], max_iters=distance.DEFAULTS["max_iters"], params=None,
                   overrides=None, poses=None, attach=None, held=None, rel=None, frames=None, check_options=True, signed=False, pen=None):
    """One candidate: -> (dist, pair, fromto [6], status, grad [n]): clearance()'s result and the derivative of dist with respect to the controlled columns.
    frames: joint_frames() of the candidate, to save the walk; check_options=False lets the distance be iterated past the query's own limits (a reference).
    signed=True: clearance(signed=True)'s four, and the gradient along n = (p2 - p1) / dist of the deepest pair where dist < 0."""
    p, d, ft, st, sig = _pair_distances(flat, qpos, dofs, q, pairs, distmax, tol, max_iters, params, overrides, poses, attach, held, rel, check_options, signed, pen)
    fr = frames if frames is not None else joint_frames(flat, qpos, dofs, q, overrides)
    return reduce_grad(flat, p, d, ft, st, sig, fr, distmax)


def collision_cost(flat, qpos, dofs, q, pairs=None, d_safe=0.05, tol=distance.DEFAULTS["tol"], max_iters=distance.DEFAULTS["max_iters"], params=None,
                   overrides=None, poses=None, attach=None, held=None, rel=None, frames=None, check_options=True, signed=False, pen=None):
    """One candidate: -> (cost, grad [n], nnear, noverlap): the sum of 1/2 (d_safe - d)^2 over the pairs the env evaluates that are closer than d_safe, its
    derivative with respect to the controlled columns, and how many pairs contribute / overlap.  signed=True: an overlapping pair enters with its negative
    distance (penetration.pair_signed; pen: its options) and its gradient, and noverlap counts dist < 0."""
    if not d_safe > 0:
        raise ClearanceError(f"clearance: d_safe {d_safe} is not > 0")
    p, d, ft, st, sig = _pair_distances(flat, qpos, dofs, q, pairs, d_safe, tol, max_iters, params, overrides, poses, attach, held, rel, check_options, signed, pen)
    fr = frames if frames is not None else joint_frames(flat, qpos, dofs, q, overrides)
    return reduce_cost(flat, p, d, ft, st, sig, fr, d_safe, signed)
