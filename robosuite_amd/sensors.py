"""Host mirror of the sensors beyond force / torque (csrc/rsim_sensors.hip): float64 numpy, one env, written from MuJoCo's documentation [3P, docs
"XML reference: sensor"; "Computation: kinematics"] and sharing no code with csrc/ -- the idiom of dr.py and episodes.py.  The kernel is tested against this
file (tests/test_sensors.py); this file is tested against closed forms and central differences (tests/test_sensors_host.py).

Where the kernel sums MuJoCo's COM-based spatial vectors (cdof, cvel, cacc) over the dofs of a body, the mirror walks the tree with the textbook recursion
for rigid bodies in world coordinates: every body frame carries (origin p, rotation R, angular velocity w, origin velocity v, angular acceleration al,
origin acceleration a), and a point s fixed in a frame moves with v + w x s and accelerates with a + al x s + w x (w x s).

    sensor_values(flat, qpos, qvel, qacc, ctrl, contacts) -> sensordata row (float64 [nsensordata])

`contacts`: dicts with pos, frame (row 0 = normal, from geom1 to geom2), geom1, geom2, efc_address, normal_force -- what HipBatch.contacts() returns.
force / torque entries and sensors that are not carried stay zero.
"""
from __future__ import annotations

import numpy as np

from . import mjcf, raycast
from .mjcf import (SENSOR_OBJ_BODY, SENSOR_OBJ_SITE, SENSOR_OBJ_XBODY, SENSOR_TYPES)


def _quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def _rot(q):
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


class _Frame:
    """A rigid frame in world coordinates with its first and second time derivatives."""

    def __init__(self, p, q, w, v, al, a):
        self.p, self.q, self.w, self.v, self.al, self.a = (np.asarray(x, dtype=np.float64) for x in (p, q, w, v, al, a))

    @property
    def R(self):
        return _rot(self.q)

    def attached(self, lp, lq=(1.0, 0.0, 0.0, 0.0)):
        """the frame at local position lp / orientation lq, rigidly attached to this one"""
        s = self.R @ np.asarray(lp, dtype=np.float64)
        q = _quat_mul(self.q, np.asarray(lq, dtype=np.float64))
        return _Frame(self.p + s, q / np.linalg.norm(q), self.w, self.v + np.cross(self.w, s), self.al,
                      self.a + np.cross(self.al, s) + np.cross(self.w, np.cross(self.w, s)))


def body_frames(m, qpos, qvel, qacc):
    """[_Frame] of every body frame (MuJoCo's xpos / xquat and their rates) for generalized position / velocity / acceleration."""
    qpos, qvel, qacc = (np.asarray(x, dtype=np.float64).ravel() for x in (qpos, qvel, qacc))
    A = lambda name, w: np.asarray(m.arrays[name], dtype=np.float64).reshape(-1, w)
    bpos, bquat, jpos, jaxis, q0 = A("body_pos", 3), A("body_quat", 4), A("jnt_pos", 3), A("jnt_axis", 3), np.asarray(m.arrays["qpos0"], dtype=np.float64).ravel()
    I = lambda name: np.asarray(m.arrays[name]).ravel().astype(int)
    parent, jadr, jnum, jtype, qadr, dadr = I("body_parentid"), I("body_jntadr"), I("body_jntnum"), I("jnt_type"), I("jnt_qposadr"), I("jnt_dofadr")
    z3 = np.zeros(3)
    frames = [_Frame(z3, [1.0, 0, 0, 0], z3, z3, z3, z3)]
    for b in range(1, int(m.nbody)):
        if jnum[b] == 1 and jtype[jadr[b]] == mjcf.JNT_FREE:      # the joint coordinates ARE the frame: position, unit quaternion; linear rates in world axes, angular in body axes
            a, d = qadr[jadr[b]], dadr[jadr[b]]
            q = qpos[a + 3:a + 7] / np.linalg.norm(qpos[a + 3:a + 7])
            R = _rot(q)
            frames.append(_Frame(qpos[a:a + 3], q, R @ qvel[d + 3:d + 6], qvel[d:d + 3], R @ qacc[d + 3:d + 6], qacc[d:d + 3]))
            continue
        f = frames[parent[b]].attached(bpos[b], bquat[b])
        for j in range(jadr[b], jadr[b] + jnum[b]):
            R = f.R
            axis, x, xd, xdd = R @ jaxis[j], qpos[qadr[j]] - q0[qadr[j]], qvel[dadr[j]], qacc[dadr[j]]
            if jtype[j] == mjcf.JNT_SLIDE:        # origin displaced by x along an axis fixed in the frame
                s = axis * x
                f = _Frame(f.p + s, f.q, f.w, f.v + np.cross(f.w, s) + axis * xd, f.al,
                           f.a + np.cross(f.al, s) + np.cross(f.w, np.cross(f.w, s)) + 2 * np.cross(f.w, axis) * xd + axis * xdd)
            elif jtype[j] == mjcf.JNT_HINGE:      # rotation by x about an axis through the anchor, both fixed in the frame before the joint
                anchor = f.attached(jpos[j])
                h = 0.5 * x
                q = _quat_mul(f.q, np.concatenate([[np.cos(h)], np.sin(h) * jaxis[j]]))
                w = f.w + axis * xd
                al = f.al + axis * xdd + np.cross(f.w, axis) * xd
                s = -(_rot(q) @ jpos[j])          # from the anchor back to the origin, fixed in the frame behind the joint
                f = _Frame(anchor.p + s, q / np.linalg.norm(q), w, anchor.v + np.cross(w, s), al, anchor.a + np.cross(al, s) + np.cross(w, np.cross(w, s)))
            else:
                raise NotImplementedError("ball joints, and free joints below other joints, are not carried")
        frames.append(f)
    return frames


def _ray_meets(shape, size, p, d):
    """does the ray p + t d (t >= 0), in the solid's own frame, meet the sphere / ellipsoid / box?  (a start inside always does)"""
    if shape == mjcf.GEOM_BOX:
        lo, hi = 0.0, np.inf
        for k in range(3):
            if d[k] == 0.0:
                if abs(p[k]) > size[k]:
                    return False
                continue
            t = sorted(((-size[k] - p[k]) / d[k], (size[k] - p[k]) / d[k]))
            lo, hi = max(lo, t[0]), min(hi, t[1])
        return hi >= lo
    s = np.full(3, size[0]) if shape == mjcf.GEOM_SPHERE else np.asarray(size, dtype=np.float64)
    p, d = p / s, d / s                           # unit sphere
    if p @ p <= 1.0:
        return True
    t = -(p @ d) / (d @ d)                        # parameter of the closest approach of the LINE
    return t >= 0.0 and np.linalg.norm(p + t * d) <= 1.0


def sensor_values(m, qpos, qvel, qacc, ctrl, contacts=()):
    ns = int(m.nsensor)
    dims = np.asarray(m.arrays["sensor_dim"]).ravel().astype(int)
    adr = np.concatenate([[0], np.cumsum(dims)]).astype(int)
    out = np.zeros(int(adr[-1]))
    if ns == 0 or "sensor_objtype" not in m.arrays:
        return out
    I = lambda name: np.asarray(m.arrays[name]).ravel().astype(int)
    A = lambda name, w: np.asarray(m.arrays[name], dtype=np.float64).reshape(-1, w)
    stype, sobj, skind, sreason, sshape = I("sensor_type"), I("sensor_objid"), I("sensor_objtype"), I("sensor_reason"), I("sensor_shape")
    qpos, qvel, qacc, ctrl = (np.asarray(x, dtype=np.float64).ravel() for x in (qpos, qvel, qacc, ctrl))
    qadr, dadr = I("jnt_qposadr"), I("jnt_dofadr")
    T = SENSOR_TYPES
    frames = None
    g = np.asarray(m.arrays["gravity"], dtype=np.float64).ravel()
    for i in range(ns):
        t, o = stype[i], sobj[i]
        if t < 2 or sreason[i] != 0:
            continue
        sl = slice(adr[i], adr[i + 1])
        if t == T["jointpos"]:
            out[sl] = qpos[qadr[o]]
        elif t == T["jointvel"]:
            out[sl] = qvel[dadr[o]]
        elif t in (T["tendonpos"], T["tendonvel"]):
            w0, wn = I("tendon_adr")[o], I("tendon_num")[o]
            joints, coef = I("wrap_objid")[w0:w0 + wn], np.asarray(m.arrays["wrap_prm"], dtype=np.float64).ravel()[w0:w0 + wn]
            out[sl] = coef @ (qpos[qadr[joints]] if t == T["tendonpos"] else qvel[dadr[joints]])
        elif t == T["actuatorfrc"]:
            j = I("actuator_trnid")[o]
            u = ctrl[o]
            if I("actuator_ctrllimited")[o]:
                u = min(max(u, A("actuator_ctrlrange", 2)[o, 0]), A("actuator_ctrlrange", 2)[o, 1])
            f = A("actuator_gainprm", 3)[o, 0] * u
            if I("actuator_biastype")[o] == mjcf.BIAS_AFFINE:
                gear, bp = np.asarray(m.arrays["actuator_gear"], dtype=np.float64).ravel()[o], A("actuator_biasprm", 3)[o]
                f += bp[0] + bp[1] * gear * qpos[qadr[j]] + bp[2] * gear * qvel[dadr[j]]
            if I("actuator_forcelimited")[o]:
                f = min(max(f, A("actuator_forcerange", 2)[o, 0]), A("actuator_forcerange", 2)[o, 1])
            out[sl] = f
        elif t == raycast.RANGEFINDER:            # the ray kernel's sensor (csrc/rsim_ray.hip): its mirror is raycast.py
            if frames is None:
                frames = body_frames(m, qpos, qvel, qacc)
            out[sl] = raycast.rangefinder_values(m, [f.p for f in frames], [f.q for f in frames])[i]
        else:
            if frames is None:
                frames = body_frames(m, qpos, qvel, qacc)
            if skind[i] == SENSOR_OBJ_SITE:
                body = I("site_bodyid")[o]
                f = frames[body].attached(A("site_pos", 3)[o], A("site_quat", 4)[o])
            elif skind[i] == SENSOR_OBJ_BODY:
                body, f = o, frames[o].attached(A("body_ipos", 3)[o], A("body_iquat", 4)[o])
            else:
                assert skind[i] == SENSOR_OBJ_XBODY
                body, f = o, frames[o]
            R = f.R
            if t == T["framepos"]:
                out[sl] = f.p
            elif t == T["framequat"]:
                out[sl] = f.q / np.linalg.norm(f.q)
            elif t == T["framelinvel"]:
                out[sl] = f.v
            elif t == T["frameangvel"]:
                out[sl] = f.w
            elif t == T["velocimeter"]:
                out[sl] = R.T @ f.v
            elif t == T["gyro"]:
                out[sl] = R.T @ f.w
            elif t == T["accelerometer"]:
                out[sl] = R.T @ (f.a - g)
            elif t == T["touch"]:
                gb, size, total = I("geom_bodyid"), A("site_size", 3)[o], 0.0
                for c in contacts:
                    fn = float(c["normal_force"])
                    if c["efc_address"] < 0 or fn <= 0.0:
                        continue
                    b1, b2 = gb[c["geom1"]], gb[c["geom2"]]
                    if body not in (b1, b2):
                        continue
                    n = np.asarray(c["frame"], dtype=np.float64).reshape(3, 3)[0]
                    ray = -n if b2 == body else n     # through the penetration, towards the body's own surface
                    if _ray_meets(sshape[i], size, R.T @ (np.asarray(c["pos"], dtype=np.float64) - f.p), R.T @ ray):
                        total += fn
                out[sl] = total
    return out
