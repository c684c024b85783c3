"""Inverse kinematics of a site over a set of hinge / slide dofs: the fp64 NumPy mirror of the device solver (csrc/rsim_ik.hip, `rsim_ik_site`,
`HipBatch.solve_ik`).  Same algorithm, same order of operations, on a compiled model (`flat`); the device tests compare the kernel with it.

Damped least squares on the site pose.  Per iteration, with q the controlled joint positions (every other joint on the path held at `qpos`):

    p, R, J = FK(q)                      site position, orientation and its rows x n Jacobian over the controlled dofs, world frame
    err     = [p* - p ; w]               w = rotation vector of q* (x) conj(q_site): axis times angle, angle in (-pi, pi] (mju_quat2Vel with dt = 1)
    stop    converged when |err_pos| < pos_tol and (with an orientation target) |w| < rot_tol; not converged after max_iters updates
    A       = J J^T + damping I,  dq = J^T A^-1 err
    posture (posture_gain > 0): v = posture_gain (q_rest - q), dq += v - J^T A^-1 (J v); q_rest is the start vector
    step    if max |dq| > max_dq: dq *= max_dq / max |dq|
    q      += dq, clamped to jnt_range where the joint is limited (clamp_range)

The posture term is projected with the DAMPED inverse, so a share damping / (sigma^2 + damping) of v leaks into the task rows: the pose error settles
near posture_gain times that share instead of falling through the tolerances when the gain is large (0.1 converges on the shipped arms, 1 mostly does not).
With clamp_range the start vector is clamped the same way, so every iterate lies inside the ranges.  FK follows the position stage of the simulator
(mjcf.kinematics_np / rsim_step.hip): qpos0 offsets, hinge anchors, bodies with several joints.  A ball joint, a free joint or a mocap body on the
path from the world to the site is refused, and so is a controlled dof that is not a hinge / slide joint on that path."""
import numpy as np

from . import mjcf

DEFAULTS = dict(damping=1e-4, max_dq=0.5, max_iters=50, pos_tol=1e-4, rot_tol=1e-3, posture_gain=0.0, clamp_range=1)
FIELDS = ("body_pos", "body_quat", "jnt_pos", "jnt_axis", "jnt_range", "qpos0", "site_pos", "site_quat")      # what FK and the clamp read of the float tables
_WIDTH = dict(body_pos=3, body_quat=4, jnt_pos=3, jnt_axis=3, jnt_range=2, qpos0=1, site_pos=3, site_quat=4)


def options(**opts):
    """the solver's options with the defaults filled in; an unknown name raises"""
    bad = set(opts) - set(DEFAULTS)
    if bad:
        raise TypeError(f"unknown IK option(s) {sorted(bad)} (have {sorted(DEFAULTS)})")
    o = dict(DEFAULTS, **opts)
    if not (o["damping"] >= 0 and o["max_dq"] > 0 and o["max_iters"] >= 0 and o["pos_tol"] >= 0 and o["rot_tol"] >= 0 and o["posture_gain"] >= 0):
        raise ValueError(f"IK options out of range: {o}")
    return o


def _tables(flat, overrides):
    t = {}
    for k in FIELDS:
        src = overrides[k] if overrides is not None and k in overrides else flat.arrays[k]
        a = np.asarray(src, dtype=np.float64)
        t[k] = a.ravel() if _WIDTH[k] == 1 else a.reshape(-1, _WIDTH[k])
    return t


def rounded(flat, overrides=None):
    """overrides holding every table FK reads rounded to float32: the model as the device sees it"""
    t = _tables(flat, overrides)
    return {k: v.astype(np.float32).astype(np.float64) for k, v in t.items()}


def chain(flat, site, dofs=None):
    """The ordered chain from the world to `site`: ("body", b) | ("joint", j, type, qpos address, column or -1) ... ("site", s), and the joint id of every
    controlled dof.  dofs=None: every dof on the path is a column, in path order.  Raises ValueError for what the solver refuses."""
    I = lambda k: np.asarray(flat.arrays[k]).ravel().astype(int)
    nsite = int(flat.nsite)
    if not 0 <= int(site) < nsite:
        raise ValueError(f"ik: site {site} out of range ({nsite} sites)")
    parent, jadr, jnum, jtype, qadr, dadr = I("body_parentid"), I("body_jntadr"), I("body_jntnum"), I("jnt_type"), I("jnt_qposadr"), I("jnt_dofadr")
    mocap = I("body_mocapid") if "body_mocapid" in flat.arrays else np.full(len(parent), -1)
    names = flat.names.get("joint", []) if hasattr(flat, "names") else []
    jn = lambda j: f"joint {j}" + (f" ({names[j]})" if j < len(names) and names[j] else "")
    path, b = [], int(I("site_bodyid")[site])
    while b > 0:
        path.append(b)
        b = int(parent[b])
    path.reverse()
    if len(path) > 64:
        raise ValueError(f"ik: the chain to site {site} passes {len(path)} bodies, more than 64")
    if dofs is not None:
        dofs = [int(d) for d in dofs]
        if not 1 <= len(dofs) <= 16:
            raise ValueError(f"ik: ndof {len(dofs)} outside 1..16")
        if len(set(dofs)) != len(dofs):
            raise ValueError(f"ik: a dof is listed twice in {dofs}")
    out, cols, found = [], [], {}
    for b in path:
        if mocap[b] >= 0:
            raise ValueError(f"ik: body {b} on the path to site {site} is a mocap body")
        out.append(("body", b))
        for j in range(jadr[b], jadr[b] + jnum[b]):
            if jtype[j] == mjcf.JNT_FREE or jtype[j] == mjcf.JNT_BALL:
                raise ValueError(f"ik: {jn(j)} on the path to site {site} is a {'free' if jtype[j] == mjcf.JNT_FREE else 'ball'} joint")
            d = int(dadr[j])
            if dofs is None:
                col = len(cols)
                cols.append(d)
            else:
                col = dofs.index(d) if d in dofs else -1
            if col >= 0:
                found[col] = j
            out.append(("joint", j, int(jtype[j]), int(qadr[j]), col))
    out.append(("site", int(site)))
    if dofs is None:
        dofs = cols
        if len(dofs) > 16:
            raise ValueError(f"ik: {len(dofs)} dofs on the path to site {site}, more than 16: name the controlled ones")
    for c, d in enumerate(dofs):
        if c not in found:
            raise ValueError(f"ik: controlled dof {d} is not a hinge or slide joint on the path to site {site}")
    return out, [found[c] for c in range(len(dofs))]


def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def _rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _walk(t, ch, qpos, q, n):
    """site position, unit quaternion and the 6 x n Jacobian [linear; angular] over the columns: the chain composed from the world outwards"""
    p, r = np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0])
    anchor, axis, kind = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=int)
    for el in ch:
        if el[0] == "body":
            b = el[1]
            p = p + _rot(r) @ t["body_pos"][b]
            r = _qmul(r, t["body_quat"][b])
            r = r / np.linalg.norm(r)
        elif el[0] == "joint":
            _, j, jt, qa, col = el
            x = (q[col] if col >= 0 else qpos[qa]) - t["qpos0"][qa]
            R = _rot(r)
            an, ax = p + R @ t["jnt_pos"][j], R @ t["jnt_axis"][j]
            if col >= 0:
                anchor[col], axis[col], kind[col] = an, ax, jt
            if jt == mjcf.JNT_HINGE:
                r = _qmul(r, np.concatenate([[np.cos(0.5 * x)], np.sin(0.5 * x) * t["jnt_axis"][j]]))
                p = an - _rot(r) @ t["jnt_pos"][j]
            else:
                p = p + ax * x
        else:
            s = el[1]
            p = p + _rot(r) @ t["site_pos"][s]
            r = _qmul(r, t["site_quat"][s])
            r = r / np.linalg.norm(r)
    J = np.zeros((6, n))
    for c in range(n):
        if kind[c] == mjcf.JNT_HINGE:
            J[:3, c], J[3:, c] = np.cross(axis[c], p - anchor[c]), axis[c]
        elif kind[c] == mjcf.JNT_SLIDE:
            J[:3, c] = axis[c]
    return p, r, J


def fk(flat, qpos, site, overrides=None):
    """(p [3], R [3, 3]) of `site` in the world frame at generalized positions `qpos`; overrides: {field: array} replacing tables of the model"""
    ch, _ = chain(flat, site)
    qpos = np.asarray(qpos, dtype=np.float64).ravel()
    held = [(e[0], e[1], e[2], e[3], -1) if e[0] == "joint" else e for e in ch]      # every joint reads qpos
    p, r, _ = _walk(_tables(flat, overrides), held, qpos, np.zeros(0), 0)
    return p, _rot(r)


def jacobian(flat, qpos, site, dofs=None, overrides=None):
    """[6, n] Jacobian [linear; angular] of `site` over `dofs` in the world frame (mj_jacSite's columns); dofs=None: over all nv dofs, zero off the path"""
    qpos = np.asarray(qpos, dtype=np.float64).ravel()
    t = _tables(flat, overrides)
    if dofs is None:
        ch, _ = chain(flat, site)
        dadr = np.asarray(flat.arrays["jnt_dofadr"]).ravel().astype(int)
        on = [e for e in ch if e[0] == "joint"]
        J = np.zeros((6, int(flat.nv)))
        for e in on:      # (one column at a time: a path may carry more dofs than a solve controls)
            one = [(x[0], x[1], x[2], x[3], 0 if x is e else -1) if x[0] == "joint" else x for x in ch]
            J[:, dadr[e[1]]] = _walk(t, one, qpos, [qpos[e[3]]], 1)[2][:, 0]
        return J
    ch, jid = chain(flat, site, dofs)
    qa = np.asarray(flat.arrays["jnt_qposadr"]).ravel().astype(int)
    return _walk(t, ch, qpos, qpos[qa[jid]], len(jid))[2]


def rotvec(qt, qs):
    """rotation vector of qt (x) conj(qs), angle in (-pi, pi]"""
    d = _qmul(qt, np.array([qs[0], -qs[1], -qs[2], -qs[3]]))
    if d[0] < 0:
        d = -d
    s = np.linalg.norm(d[1:])
    return d[1:] * (2.0 * np.arctan2(s, d[0]) / s if s > 1e-12 else 2.0)


class Problem:
    """One (site, dofs) problem on a model: the chain, the tables and the ranges, shared by `solve`, `update` and `error`."""

    def __init__(self, flat, qpos, site, dofs, overrides=None):
        self.ch, self.jid = chain(flat, site, dofs)
        self.n = len(self.jid)
        self.t = _tables(flat, overrides)
        self.qpos = np.asarray(qpos, dtype=np.float64).ravel()
        self.qadr = np.asarray(flat.arrays["jnt_qposadr"]).ravel().astype(int)[self.jid]
        lim = np.asarray(flat.arrays["jnt_limited"]).ravel().astype(bool)[self.jid]
        rng = self.t["jnt_range"][self.jid]
        self.lo, self.hi = np.where(lim, rng[:, 0], -np.inf), np.where(lim, rng[:, 1], np.inf)

    def clamp(self, q, o):
        return np.minimum(np.maximum(q, self.lo), self.hi) if o["clamp_range"] else q

    def start(self, q_init, o):
        return self.clamp(self.qpos[self.qadr].copy() if q_init is None else np.asarray(q_init, dtype=np.float64).ravel().copy(), o)

    def error(self, q, pos, quat):
        """(err [6], J [6, n]) at q; without an orientation target the angular rows are zero"""
        p, r, J = _walk(self.t, self.ch, self.qpos, q, self.n)
        e = np.zeros(6)
        e[:3] = np.asarray(pos, dtype=np.float64) - p
        if quat is not None:
            qt = np.asarray(quat, dtype=np.float64)
            e[3:] = rotvec(qt / np.linalg.norm(qt), r)
        else:
            J[3:] = 0.0
        return e, J

    def update(self, q, q_rest, e, J, o, rows):
        Jr = J[:rows]
        A = Jr @ Jr.T + o["damping"] * np.eye(rows)
        dq = Jr.T @ np.linalg.solve(A, e[:rows])
        if o["posture_gain"] > 0:
            v = o["posture_gain"] * (q_rest - q)
            dq = dq + v - Jr.T @ np.linalg.solve(A, Jr @ v)
        big = np.abs(dq).max()
        if big > o["max_dq"]:
            dq = dq * (o["max_dq"] / big)
        return dq


def update(flat, qpos, site, dofs, q, q_rest, pos, quat=None, overrides=None, **opts):
    """the step one iteration adds to q (after the max_dq scaling, before the clamp)"""
    o = options(**opts)
    P = Problem(flat, qpos, site, dofs, overrides)
    q = np.asarray(q, dtype=np.float64)
    e, J = P.error(q, pos, quat)
    return P.update(q, np.asarray(q_rest, dtype=np.float64), e, J, o, 3 if quat is None else 6)


def error(flat, qpos, site, dofs, q, pos, quat=None, overrides=None):
    """(|err_pos|, |w|) at q (0 for |w| without an orientation target)"""
    e, _ = Problem(flat, qpos, site, dofs, overrides).error(np.asarray(q, dtype=np.float64), pos, quat)
    return float(np.linalg.norm(e[:3])), float(np.linalg.norm(e[3:]))


def solve(flat, qpos, site, dofs, pos, quat=None, q_init=None, overrides=None, **opts):
    """-> (q [n], err [2] = |err_pos|, |w| at q, iters = updates made, converged).  q of a problem that did not converge is the last iterate."""
    o = options(**opts)
    P = Problem(flat, qpos, site, dofs, overrides)
    q = P.start(q_init, o)
    q_rest = q.copy()
    it = 0
    while True:
        e, J = P.error(q, pos, quat)
        en, wn = float(np.linalg.norm(e[:3])), float(np.linalg.norm(e[3:]))
        if en < o["pos_tol"] and (quat is None or wn < o["rot_tol"]):
            return q, np.array([en, wn]), it, True
        if it >= o["max_iters"]:
            return q, np.array([en, wn]), it, False
        q = P.clamp(q + P.update(q, q_rest, e, J, o, 3 if quat is None else 6), o)
        it += 1


def well_conditioned(flat, qpos, site, dofs, pos, quat=None, q_init=None, overrides=None, **opts):
    """A case the device is held to: the mirror alone converges at the stated tolerances with at least five iterations to spare, and also converges
    within max_iters with both tolerances halved."""
    o = options(**opts)
    _, _, it, ok = solve(flat, qpos, site, dofs, pos, quat, q_init, overrides, **o)
    if not ok or it > o["max_iters"] - 5:
        return False
    half = dict(o, pos_tol=0.5 * o["pos_tol"], rot_tol=0.5 * o["rot_tol"])
    return bool(solve(flat, qpos, site, dofs, pos, quat, q_init, overrides, **half)[3])
