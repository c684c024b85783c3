"""Collision-aware inverse kinematics: the fp64 NumPy mirror of the device solver (csrc/rsim_ik_avoid.hip, `rsim_ik_site_avoid`, `HipBatch.solve_ik_avoid`),
and its definition.  Composed from the two layers that exist: ik.Problem (site error, Jacobian, clamp) and clearance.collision_cost (cost, gradient, counts).

Per problem, q <- clamp(q_init), q_rest = q, it = 0; then repeat

    e, J              = the site error and Jacobian over the controlled dofs at q (ik.Problem.error; a position-only target zeroes the angular rows)
    cost, g, nnear, nover = clearance.collision_cost at q with the call's pair list, d_safe and attachments
    conv              = |e_pos| < pos_tol and (with an orientation target) |w| < rot_tol            (ik.solve's test)
    finished          = conv and cost <= cost_tol
    stop              if finished or it >= max_iters
    A  = J J^T + damping I,   v = posture_gain (q_rest - q) - avoid_gain g
    dq = J^T A^-1 e + v - J^T A^-1 (J v), scaled so that max |dq| <= max_dq;   q <- clamp(q + dq), it += 1

Avoidance is a secondary task in the null space of the pose task, in the form of ik.py's posture term (and with its leak: the projection uses the DAMPED
inverse).  Every term of the cost is at most the cost, so cost <= 1/2 (d_safe - d_free)^2 proves every listed pair at least d_free apart; the default
cost_tol = 1/2 (d_safe / 2)^2 proves d_free = d_safe / 2 and excludes an overlapping pair (which adds 1/2 d_safe^2).  cost_tol = inf: never wait for the cost.
A finished problem is frozen.  With avoid_gain = 0 and cost_tol = inf this is ik.solve, exactly.

signed=True (rsim_ik_site_avoid_signed): the cost of every evaluation is clearance.collision_cost(signed=True, pen=pen) -- an overlapping pair has a depth and a
normal, so it pushes, and noverlap counts dist < 0.

Limits.  Without signed, a pair that starts in a general convex overlap (status 2) adds cost and no push: pass signed=True, or hand in several start vectors.  A listed pair that stays inside
d_safe whatever the arm does (the Panda's link0 / link1 geoms, 1 mm apart) never lets a problem finish: hand in the list without parent / child pairs.  A
6-dof arm with a pose target has no null space to use."""
import numpy as np

from . import clearance, distance, ik

AVOID_GAIN = 100.0     # include/rsim.h: chosen on the test scenes from this mirror alone (profiles/ik_avoid_parity.txt)
DEFAULTS = dict(ik.DEFAULTS, d_safe=0.05, avoid_gain=AVOID_GAIN, cost_tol=None, check_every=0)      # cost_tol None: 1/2 (d_safe / 2)^2


def options(**opts):
    """the solver's options with the defaults filled in; an unknown name raises, and so does a value the device refuses"""
    bad = set(opts) - set(DEFAULTS)
    if bad:
        raise TypeError(f"unknown IK option(s) {sorted(bad)} (have {sorted(DEFAULTS)})")
    o = dict(DEFAULTS, **opts)
    ik.options(**{k: o[k] for k in ik.DEFAULTS})
    if not o["d_safe"] > 0:
        raise ValueError(f"ik_avoid: d_safe {o['d_safe']} is not > 0")
    if o["cost_tol"] is None:
        o["cost_tol"] = 0.5 * (0.5 * o["d_safe"]) ** 2
    if not o["avoid_gain"] >= 0:
        raise ValueError(f"ik_avoid: avoid_gain {o['avoid_gain']} is not >= 0")
    if not o["cost_tol"] >= 0:
        raise ValueError(f"ik_avoid: cost_tol {o['cost_tol']} is not >= 0")
    if int(o["check_every"]) < 0:
        raise ValueError(f"ik_avoid: check_every {o['check_every']} is not >= 0")
    return o


def step(P, q, q_rest, e, J, g, o, rows):
    """the step one iteration adds to q (after the max_dq scaling, before the clamp): ik.Problem.update with v = posture_gain (q_rest - q) - avoid_gain g"""
    Jr = J[:rows]
    A = Jr @ Jr.T + o["damping"] * np.eye(rows)
    dq = Jr.T @ np.linalg.solve(A, e[:rows])
    if o["posture_gain"] > 0 or o["avoid_gain"] > 0:
        v = o["posture_gain"] * (q_rest - q) - o["avoid_gain"] * np.asarray(g, dtype=np.float64)
        dq = dq + v - Jr.T @ np.linalg.solve(A, Jr @ v)
    big = np.abs(dq).max()
    if big > o["max_dq"]:
        dq = dq * (o["max_dq"] / big)
    return dq


def solve(flat, qpos, site, dofs, pos, quat=None, q_init=None, pairs=None, overrides=None, params=None, attach=None, held=None, rel=None,
          tol=distance.DEFAULTS["tol"], dist_max_iters=distance.DEFAULTS["max_iters"], trace=None, signed=False, pen=None, **opts):
    """One problem of one env -> (q [n], err [2] = |err_pos|, |w| at q, iters, converged, finished, cost, nnear, noverlap), everything AT q.  pairs=None:
    clearance.default_pairs; params / overrides: the env's geom arrays / FK tables; attach / held / rel: its carried objects.  trace: a list that receives
    (q, e, J, cost, g) of every evaluation.  signed / pen: clearance.collision_cost's."""
    o = options(**opts)
    sg = dict(signed=True, pen=pen) if signed else {}      # (nothing is passed on without it: the unsigned call is what it was)
    P = ik.Problem(flat, qpos, site, dofs, overrides)
    p = clearance.default_pairs(flat, dofs, attach) if pairs is None else pairs
    m32 = clearance._model32(flat, overrides)
    rows = 3 if quat is None else 6
    q = P.start(q_init, o)
    q_rest = q.copy()
    it = 0
    while True:
        e, J = P.error(q, pos, quat)
        if pairs is None and attach is not None and len(attach):      # the default list: per env, only the pairs its held row makes candidate-dependent
            cost, g, nnear, nover = clearance.collision_cost(flat, qpos, dofs, q, None, o["d_safe"], tol, dist_max_iters, params, overrides, attach=attach, held=held, rel=rel,
                                                             **sg)
        else:
            xp = clearance.fk(flat, qpos, dofs, q, model32=m32, attach=attach, held=held, rel=rel)
            cost, g, nnear, nover = clearance.collision_cost(flat, qpos, dofs, q, p, o["d_safe"], tol, dist_max_iters, params, overrides, poses=xp, attach=attach, held=held,
                                                             rel=rel, frames=clearance.joint_frames(flat, qpos, dofs, q, model32=m32), **sg)
        if trace is not None:
            trace.append((q.copy(), e.copy(), J.copy(), cost, g.copy()))
        en, wn = float(np.linalg.norm(e[:3])), float(np.linalg.norm(e[3:]))
        conv = en < o["pos_tol"] and (quat is None or wn < o["rot_tol"])
        fin = bool(conv and cost <= o["cost_tol"])
        if fin or it >= o["max_iters"]:
            return q, np.array([en, wn]), it, bool(conv), fin, float(cost), int(nnear), int(nover)
        q = P.clamp(q + step(P, q, q_rest, e, J, g, o, rows), o)
        it += 1


def held_to(flat, qpos, site, dofs, pos, quat=None, q_init=None, pairs=None, **kw):
    """A case the device is held to: the mirror alone finishes it with at least five iterations to spare, and also finishes it within max_iters with
    pos_tol, rot_tol and cost_tol halved."""
    o = options(**{k: v for k, v in kw.items() if k in DEFAULTS})
    rest = {k: v for k, v in kw.items() if k not in DEFAULTS}
    r = solve(flat, qpos, site, dofs, pos, quat, q_init, pairs, **rest, **o)
    if not r[4] or r[2] > o["max_iters"] - 5:
        return False
    half = dict(o, pos_tol=0.5 * o["pos_tol"], rot_tol=0.5 * o["rot_tol"], cost_tol=0.5 * o["cost_tol"])
    return bool(solve(flat, qpos, site, dofs, pos, quat, q_init, pairs, **rest, **half)[4])


def update(flat, qpos, site, dofs, q, q_rest, pos, quat=None, pairs=None, g=None, overrides=None, params=None, attach=None, held=None, rel=None,
           tol=distance.DEFAULTS["tol"], dist_max_iters=distance.DEFAULTS["max_iters"], signed=False, pen=None, **opts):
    """clamp(q + step): the iterate one update makes of q, whatever the stopping rule says.  g: the cost's gradient to use in place of the mirror's own (the
    device tests hand the device's gradient in, to hold the step arithmetic apart from the distance layer)."""
    o = options(**opts)
    P = ik.Problem(flat, qpos, site, dofs, overrides)
    q, q_rest = np.asarray(q, dtype=np.float64), np.asarray(q_rest, dtype=np.float64)
    e, J = P.error(q, pos, quat)
    if g is None:
        g = clearance.collision_cost(flat, qpos, dofs, q, pairs, o["d_safe"], tol, dist_max_iters, params, overrides, attach=attach, held=held, rel=rel,
                                     **(dict(signed=True, pen=pen) if signed else {}))[1]
    return P.clamp(q + step(P, q, q_rest, e, J, g, o, 3 if quat is None else 6), o)
