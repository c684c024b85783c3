"""Swept clearance: the fp64 host mirror of the device routines (csrc/rsim_sweep.hip, rsim_config_sweep / rsim_config_motion_bound) -- "is the motion from q0
to q1 free?" for a joint-space segment q(t) = q0 + t (q1 - q0), t in [0, 1], answered by conservative advancement: a certificate, not a set of samples.

One env, float64, built on clearance.py (FK, the pair list, the minimum); it shares no code with csrc/.  The kernel is tested against this file
(tests/test_sweep.py), this file against brute force (tests/test_sweep_host.py).

    motion_bound(flat, qpos, dofs, q0, q1, pairs=None, overrides=None, params=None) -> L >= 0
    sweep(flat, qpos, dofs, q0, q1, pairs=None, distmax=1.0, margin=0.0, slack=1e-3, max_steps=256, tol=1e-6, max_iters=64, params=None, overrides=None)
        -> (status, t, dist, t_min, pair, fromto [6], steps)

Semantics (include/rsim.h).  c(t) is clearance.clearance at q(t).  L bounds how fast the distance of any listed pair can change per unit t: a moved body
carries Omega, the sum of |q1 - q0| over the controlled hinges on its path, and V, a bound on the speed of its origin; V(child) = V(parent) +
Omega(parent) |body_pos|; a slide adds |axis| (|dx| + Omega max(|x(0)|, |x(1)|)) with x = q - qpos0 (a held slide: dx = 0, x its current displacement); a hinge
or a held ball joint adds Omega |jnt_pos| before its own |dq| goes into Omega and Omega |jnt_pos| after.  A geom moves at most V + Omega r with r = |geom_pos| +
a radius about the geom's origin that contains it; a geom of a body that is not moved has speed 0, and a plane on a moved body is refused.  L is the maximum
over the list of the sum of a pair's two bounds, times 1 + 2^-16 (the device's allowance for its fp32 roundings, kept here so that both state one bound).

The loop: t = 0; sample c(t); c <= margin + slack: HIT; t == 1: FREE; else t <- min(1, t + (c - margin) / L), a far sample reading c = distmax; max_steps
samples without a decision: UNDECIDED.  The motion is certified to have clearance > margin on [0, t).

Carried objects (clearance.py: attach, one env's held row, its rel rows).  A held body has Omega = Omega(carrier) and V = V(carrier) + Omega(carrier) |p_rel|,
and its subtree follows by the rules above; one that is not held stands still.  L is the maximum over the pairs the env evaluates (clearance.active_pairs; an
explicit list: all of them).  The certificate is unchanged: the held body's origin is p_c(t) + R_c(t) p_rel with p_rel constant, so it moves at most
V(carrier) + Omega(carrier) |p_rel| per unit t and turns at most Omega(carrier) -- the body step's bound with p_rel in place of body_pos; and which pairs the
env evaluates does not depend on t, so c(t) is L-Lipschitz as before.  A plane on an attached body is refused, as on any moved body.

NOT HANDLED: free and ball joints as controlled dofs; interpolation other than linear in joint space; per-pair bounds."""
from __future__ import annotations

import numpy as np

from . import clearance, distance, ik, mjcf

FREE, HIT, UNDECIDED = 0, 1, 2
DEFAULTS = {"margin": 0.0, "slack": 1e-3, "max_steps": 256}
MAX_STEPS_LIMIT = 4096      # RSIM_SWEEP_MAX_STEPS
INFLATE = 1.0 + 2.0 ** -16


class SweepError(ValueError):
    pass


def options(distmax=1.0, margin=DEFAULTS["margin"], slack=DEFAULTS["slack"], max_steps=DEFAULTS["max_steps"]):
    """the refusals of rsim_config_sweep's own options, by name"""
    distmax, margin, slack, max_steps = float(distmax), float(margin), float(slack), int(max_steps)
    if not margin >= 0:
        raise SweepError(f"config_sweep: margin {margin:g} is not >= 0")
    if not slack > 0:
        raise SweepError(f"config_sweep: slack {slack:g} is not > 0")
    if not 1 <= max_steps <= MAX_STEPS_LIMIT:
        raise SweepError(f"config_sweep: max_steps {max_steps} outside 1..{MAX_STEPS_LIMIT}")
    if not distmax > margin + slack:
        raise SweepError(f"config_sweep: distmax {distmax:g} is not above margin + slack = {margin + slack:g}: no sample could pass")
    return {"distmax": distmax, "margin": margin, "slack": slack, "max_steps": max_steps}


def geom_radius(gtype, size, rcenter, rbound):
    """a radius about the geom's own origin that contains the solid: the larger of what type and size give and |rcenter| + rbound"""
    s = [float(x) for x in size]
    r = {mjcf.GEOM_SPHERE: s[0], mjcf.GEOM_CAPSULE: s[0] + s[1], mjcf.GEOM_ELLIPSOID: max(s), mjcf.GEOM_CYLINDER: float(np.hypot(s[0], s[1])),
         mjcf.GEOM_BOX: float(np.linalg.norm(s))}.get(int(gtype), 0.0)
    return 0.0 if gtype == mjcf.GEOM_PLANE else max(r, float(np.linalg.norm(rcenter)) + float(rbound))


def body_rates(flat, qpos, dofs, q0, q1, overrides=None, attach=None, held=None, rel=None):
    """(Omega [nbody], V [nbody]) of the segment, on the FK tables rounded to fp32 (ik.rounded); zero for a body that is not moved"""
    sig = clearance._signatures(flat, dofs)
    att = clearance._attachments(flat, dofs, attach, sig)
    col = clearance._columns(flat, dofs)
    t = ik.rounded(flat, overrides)
    I = clearance._I
    parent, jadr, jnum, jtype, qa = I(flat, "body_parentid"), I(flat, "body_jntadr"), I(flat, "body_jntnum"), I(flat, "jnt_type"), I(flat, "jnt_qposadr")
    qpos = np.asarray(qpos, dtype=np.float64).ravel()
    q0, q1 = np.asarray(q0, dtype=np.float64).ravel(), np.asarray(q1, dtype=np.float64).ravel()
    if len(q0) != len(col) or len(q1) != len(col):
        raise SweepError(f"config_sweep: a segment end holds {len(col)} positions, got {len(q0)} and {len(q1)}")
    om, v = np.zeros(int(flat.nbody)), np.zeros(int(flat.nbody))
    for b in range(1, int(flat.nbody)):
        if not sig[b]:
            continue
        p = parent[b]
        om[b], v[b] = om[p], v[p] + om[p] * np.linalg.norm(t["body_pos"][b])
        for j in range(jadr[b], jadr[b] + jnum[b]):
            c = col.get(j, -1)
            if jtype[j] == mjcf.JNT_SLIDE:
                ref = t["qpos0"][qa[j]]
                x0, x1 = ((q0[c], q1[c]) if c >= 0 else (qpos[qa[j]], qpos[qa[j]]))
                x0, x1 = x0 - ref, x1 - ref
                v[b] += np.linalg.norm(t["jnt_axis"][j]) * (abs(x1 - x0) + om[b] * max(abs(x0), abs(x1)))
            else:
                arm = np.linalg.norm(t["jnt_pos"][j])
                v[b] += om[b] * arm
                if jtype[j] == mjcf.JNT_HINGE and c >= 0:
                    om[b] += abs(q1[c] - q0[c])
                v[b] += om[b] * arm
    if att:
        r = clearance.relative_poses(flat, qpos, att, rel, overrides)
        for (body, carrier), h, ri in zip(att, clearance._held_row(att, held), r):
            if not h:
                continue
            om[body], v[body] = om[carrier], v[carrier] + om[carrier] * np.linalg.norm(ri[:3])
            for b in clearance.subtree(flat, body)[1:]:      # (their joints are held: dx = 0, no |dq|)
                p = parent[b]
                om[b], v[b] = om[p], v[p] + om[p] * np.linalg.norm(t["body_pos"][b])
                for j in range(jadr[b], jadr[b] + jnum[b]):
                    if jtype[j] == mjcf.JNT_SLIDE:
                        v[b] += np.linalg.norm(t["jnt_axis"][j]) * om[b] * abs(qpos[qa[j]] - t["qpos0"][qa[j]])
                    else:
                        v[b] += 2 * om[b] * np.linalg.norm(t["jnt_pos"][j])
    return om, v


def _pairs(flat, dofs, pairs, attach=None):
    p = clearance.default_pairs(flat, dofs, attach) if pairs is None else distance.check_pairs(flat, pairs)
    sig = clearance.signatures(flat, dofs, attach)      # (all held: an attached body counts as moved whatever the env's row)
    gtype, gbody = clearance._I(flat, "geom_type"), clearance._I(flat, "geom_bodyid")
    for k, pr in enumerate(p):
        for g in pr:
            if gtype[g] == mjcf.GEOM_PLANE and sig[gbody[g]]:
                raise SweepError(f"config_sweep: pair {k}: plane geom {int(g)} sits on body {int(gbody[g])}, which the controlled dofs move: an unbounded solid "
                                 "has no motion bound")
    return p


def geom_speeds(flat, qpos, dofs, q0, q1, geoms, overrides=None, params=None, attach=None, held=None, rel=None):
    """{geom id: bound on the speed of any of its points per unit t}; params: the env's own geom arrays (geom_size, geom_pos, geom_rbound, geom_rcenter)"""
    om, v = body_rates(flat, qpos, dofs, q0, q1, overrides, attach, held, rel)
    A = lambda name, w: np.asarray((params or {}).get(name, flat.arrays[name]), dtype=np.float64).astype(np.float32).astype(np.float64).reshape(-1, w)   # noqa: E731
    gsize, gpos, rc, rb = A("geom_size", 3), A("geom_pos", 3), A("geom_rcenter", 3), A("geom_rbound", 1)
    gtype, gbody = clearance._I(flat, "geom_type"), clearance._I(flat, "geom_bodyid")
    sig = clearance.signatures(flat, dofs, attach, held)
    out = {}
    for g in sorted(set(int(x) for x in geoms)):
        b = gbody[g]
        out[g] = 0.0 if not sig[b] else float(v[b] + om[b] * (np.linalg.norm(gpos[g]) + geom_radius(gtype[g], gsize[g], rc[g], rb[g, 0])))
    return out


def motion_bound(flat, qpos, dofs, q0, q1, pairs=None, overrides=None, params=None, attach=None, held=None, rel=None):
    """L of one segment: the distance of every pair the env evaluates changes by at most L |dt|"""
    p = _pairs(flat, dofs, pairs, attach)
    s = geom_speeds(flat, qpos, dofs, q0, q1, p.ravel(), overrides, params, attach, held, rel)
    on = clearance.active_pairs(flat, dofs, p, attach, held) if pairs is None and attach is not None and len(attach) else np.ones(len(p), dtype=bool)
    return max([s[int(a)] + s[int(b)] for (a, b), k in zip(p, on) if k], default=0.0) * INFLATE


def sweep(flat, qpos, dofs, q0, q1, pairs=None, distmax=1.0, margin=DEFAULTS["margin"], slack=DEFAULTS["slack"], max_steps=DEFAULTS["max_steps"],
          tol=distance.DEFAULTS["tol"], max_iters=distance.DEFAULTS["max_iters"], params=None, overrides=None, attach=None, held=None, rel=None):
    """One segment: -> (status, t, dist, t_min, pair, fromto [6], steps); bit 8 of status (distance.CAP) is set if any sample's iteration was capped"""
    o = options(distmax, margin, slack, max_steps)
    p = _pairs(flat, dofs, pairs, attach)
    q0, q1 = np.asarray(q0, dtype=np.float64).ravel(), np.asarray(q1, dtype=np.float64).ravel()
    L = motion_bound(flat, qpos, dofs, q0, q1, pairs, overrides, params, attach, held, rel)
    m32 = clearance._model32(flat, overrides)
    gparams = None if params is None else {k: v for k, v in params.items() if k in ("geom_size", "geom_pos", "geom_quat")}
    best, t_min, cap, t, steps = (o["distmax"], -1, np.zeros(6)), 0.0, 0, 0.0, 0
    while steps < o["max_steps"]:
        q = q0 + t * (q1 - q0)
        poses = clearance.fk(flat, qpos, dofs, q, model32=m32, attach=attach, held=held, rel=rel)
        d, k, ft, st = clearance.clearance(flat, qpos, dofs, q, pairs if attach is not None and len(attach) else p, o["distmax"], tol, max_iters, gparams, poses=poses,
                                           attach=attach, held=held)
        steps += 1
        cap |= st & distance.CAP
        if k >= 0 and d < best[0]:
            best, t_min = (d, k, ft), t
        if d <= o["margin"] + o["slack"]:
            return HIT | cap, t, best[0], t_min, best[1], best[2], steps
        if t == 1.0 or not L > 0:
            return FREE | cap, 1.0, best[0], t_min, best[1], best[2], steps
        at, t = t, min(1.0, t + (d - o["margin"]) / L)
    return UNDECIDED | cap, at, best[0], t_min, best[1], best[2], steps      # (the parameter of the last sample, not the end of the step behind it)
