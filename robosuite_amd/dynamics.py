"""Dynamics at candidate configurations: the fp64 host statement, BY THE DEFINITION, of the device routines (csrc/rsim_dyn.hip, include/rsim.h
rsim_config_inverse_dynamics / rsim_config_mass_matrix / rsim_config_jacobian).

The candidate: q~ is the env's qpos with the controlled entries replaced by q; qd~ and qdd~ are zero but for the controlled entries -- every joint that is not
controlled is held, with zero velocity and zero acceleration.  Then

    tau[c] = (M(q~) qdd~)[dof_c] + qfrc_bias(q~, qd~)[dof_c] + dof_damping[dof_c] qd_c
           = sum over bodies of  Jp^T m (a - g) + Jr^T (I alpha + omega x I omega)   [dof_c]  +  dof_armature[dof_c] qdd_c  +  dof_damping[dof_c] qd_c

with Jp / Jr the Jacobian of the body's centre of mass / orientation (mjcf.body_jacobian_np on mjcf.kinematics_np), omega = Jr qd~, a = Jp qdd~ + Jp' qd~ and
alpha = Jr qdd~ + Jr' qd~, I the body's inertia about its centre of mass in the world frame.  The velocity-product terms come from differentiating the Jacobian's
columns one by one: the axis of column j turns with the frame that carries it, a_j' = omega_j x a_j, its anchor moves with that frame, and the column of a hinge
at the point c is a_j x (c - p_j).  No recursion over the tree carries a velocity, an acceleration or a force here: the kernels run recursive Newton-Euler and
composite rigid bodies, the fp64 oracle its own RNE, and this file shares an algorithm with neither.  Bodies the controlled dofs do not move have zero columns
and drop out by themselves.

Not included, as on the device: tendon springs and dampers, fluid forces, friction loss, actuator, contact, equality and applied forces.  Free and ball joints
cannot be controlled (clearance._columns refuses them, in the device's words).

CARRIED PAYLOADS (csrc/rsim_dyn_att.hip, the _attached entries of include/rsim.h): attach = [(body, carrier), ...], held = THIS env's row (None:
all held), rel = this env's [n, 7] rows or None (the env's current poses; now = (xpos, xquat) hands them in), by clearance.py's rules and refusals.  In an
env that holds attachment i the attached body and every body below it are rigid load on the carrier at X_carrier(q) o rel, the joints below held at qpos: each
such body adds its own term of the sum above,  Jp^T m (a - g) + Jr^T (I alpha + omega x I omega),  with Jp / Jr the CARRIER's mjcf.body_jacobian_np at the held
body's centre of mass, its pose from clearance.fk's attached FK, and mass, inertia, ipos and iquat from the env's own tables.  To M it adds
Jp^T m Jp + Jr^T I Jr.  The attached body's free joint has no column and no armature.  Not held: nothing is added -- as a free body it has no controlled
column and drops out by itself.  A site on a held body has the carrier's Jacobian at the point placed from the attached pose; not held: zeros.  Still no
recursion over the tree.  Not carried: a virtual payload with no body in the model, deciding what is grasped, grasp forces, an object attached to an attached
object, derivatives.

M^-1 (csrc/rsim_dyn_solve.hip, rsim_config_forward_dynamics / rsim_config_mass_solve / rsim_config_opspace): forward_dynamics, mass_solve and opspace are
numpy.linalg.solve on this file's own mass_matrix, inverse_dynamics and site_jacobian; the kernel runs a Cholesky factorisation in fp32.

DERIVATIVES (csrc/rsim_dyn_grad.hip, rsim_config_inverse_dynamics_grad / rsim_config_inverse_dynamics_jvp / rsim_config_forward_dynamics_grad):
inverse_dynamics_grad, inverse_dynamics_jvp and forward_dynamics_grad are the DEFINITION OF A DERIVATIVE on this file's own inverse_dynamics, mass_matrix and
forward_dynamics -- Richardson-extrapolated central differences in q, single central differences in qd and qdd, where they are exact -- while the kernel runs
a tangent (forward-mode) recursive Newton-Euler.  Without attach."""
from collections import OrderedDict

import numpy as np

from . import clearance, mjcf

# every float table the definition reads: what the device holds in fp32 (per-env overrides replace the model's)
FIELDS = ("body_pos", "body_quat", "body_ipos", "body_iquat", "body_mass", "body_inertia", "jnt_pos", "jnt_axis", "qpos0", "site_pos", "dof_armature",
          "dof_damping", "gravity")


def model32(flat, overrides=None):
    """the model with every table in FIELDS rounded to float32 (overrides: {field: array} of one env) -- the model as the device sees it"""
    m = mjcf.FlatModel()
    m.arrays = OrderedDict(flat.arrays)
    m.names = flat.names
    for k in FIELDS:
        src = overrides[k] if overrides is not None and k in overrides else flat.arrays[k]
        m.arrays[k] = np.asarray(src, dtype=np.float64).astype(np.float32).astype(np.float64).reshape(np.asarray(flat.arrays[k]).shape)
    return m


def _model(flat, overrides, m32):
    if m32 is not None:
        return m32
    if overrides is None:
        return flat
    m = mjcf.FlatModel()
    m.arrays = OrderedDict(flat.arrays)
    m.names = flat.names
    for k, v in overrides.items():
        m.arrays[k] = np.asarray(v, dtype=np.float64).reshape(np.asarray(flat.arrays[k]).shape)
    return m


def _full(flat, dofs, x):
    out = np.zeros(int(flat.nv))
    if x is not None:
        out[np.asarray(dofs, dtype=int)] = np.asarray(x, dtype=np.float64).ravel()
    return out


def _column_rates(m, kin, col, v):
    """{joint: (a_j', p_j')} for the controlled joints: the rate of the world axis and the velocity of the anchor of column j, both riding on the frame the
    joint is applied in -- moved by the joints before it (those of the ancestors, and the earlier ones of its own body) and by nothing else"""
    xpos, _, xmat, _, _, xanchor, xaxis = kin
    jbody = np.repeat(np.arange(int(m.nbody)), clearance._I(m, "body_jntnum"))
    dadr = clearance._I(m, "jnt_dofadr")
    out = {}
    for j in col:
        jp, jr = mjcf.body_jacobian_np(m, xpos, xmat, xanchor, xaxis, int(jbody[j]), xanchor[j])
        before = v.copy()
        before[dadr[j] + 1:] = 0.0      # dof order is joint order: later joints of the body do not carry this one (the joint itself moves neither)
        out[j] = (np.cross(jr @ before, xaxis[j]), jp @ before)
    return out


def _payload(flat, m, qpos, dofs, q, attach, held, rel, now):
    """the held bodies of one env at one candidate: ([(carrier, centre of mass, inertial frame [3, 3], mass, principal moments [3]), ...] one per held attached
    body and body below it, {body: carrier} for them, (xpos, xquat) of clearance.fk's attached FK) -- on the tables of m"""
    att = clearance._attachments(flat, dofs, attach)
    if not att:
        return [], {}, None
    xpos, xquat = clearance.fk(flat, qpos, dofs, q, model32=m, attach=att, held=held, rel=rel, now=now)
    ipos, iquat = np.asarray(m.body_ipos, dtype=np.float64).reshape(-1, 3), np.asarray(m.body_iquat, dtype=np.float64).reshape(-1, 4)
    mass, inertia = np.asarray(m.body_mass, dtype=np.float64).ravel(), np.asarray(m.body_inertia, dtype=np.float64).reshape(-1, 3)
    load, carrier_of = [], {}
    for (body, carrier), h in zip(att, clearance._held_row(att, held)):
        for b in clearance.subtree(flat, body) if h else ():
            R = mjcf.quat2mat(xquat[b])
            load.append((carrier, xpos[b] + R @ ipos[b], R @ mjcf.quat2mat(mjcf.quat_normalize(iquat[b])), float(mass[b]), inertia[b]))
            carrier_of[b] = carrier
    return load, carrier_of, (xpos, xquat)


def inverse_dynamics(flat, qpos, dofs, q, qd=None, qdd=None, overrides=None, model32=None, attach=None, held=None, rel=None, now=None):
    """tau [n] of one candidate.  qpos: the env's [nq]; q / qd / qdd: [n] of the controlled dofs (None: zeros); attach / held / rel / now: the env's carried
    payload (the module's docstring)"""
    m = _model(flat, overrides, model32)
    load = _payload(flat, m, qpos, dofs, q, attach, held, rel, now)[0]
    col = clearance._columns(flat, dofs)
    dofs = [int(d) for d in np.asarray(dofs).ravel()]
    kin = mjcf.kinematics_np(m, clearance.candidate_qpos(flat, qpos, dofs, q))
    xpos, _, xmat, xipos, ximat, xanchor, xaxis = kin
    v, a = _full(flat, dofs, qd), _full(flat, dofs, qdd)
    rates = _column_rates(m, kin, col, v) if np.any(v) else {}
    jtype, dadr = clearance._I(m, "jnt_type"), clearance._I(m, "jnt_dofadr")
    g = np.asarray(m.gravity, dtype=np.float64).ravel()
    tau = np.zeros(int(flat.nv))
    # every body with its own Jacobian at its own centre of mass; a held body with its CARRIER's Jacobian at the held body's centre of mass
    terms = [(b, xipos[b], ximat[b], float(m.body_mass[b]), m.body_inertia[b]) for b in range(1, int(m.nbody))] + load
    for jb, com, imat, mass, inertia in terms:
        jp, jr = mjcf.body_jacobian_np(m, xpos, xmat, xanchor, xaxis, jb, com)
        if not (np.any(jp[:, dofs]) or np.any(jr[:, dofs])):
            continue      # not moved
        omega, vc = jr @ v, jp @ v
        acc, alpha = jp @ a, jr @ a
        for j, (da, dp) in rates.items():      # Jp' qd~ and Jr' qd~, column by column
            d = dadr[j]
            if not (np.any(jp[:, d]) or np.any(jr[:, d])):
                continue      # the column does not move this body
            if jtype[j] == mjcf.JNT_SLIDE:
                acc += da * v[d]
            else:
                acc += (np.cross(da, com - xanchor[j]) + np.cross(xaxis[j], vc - dp)) * v[d]
                alpha += da * v[d]
        Iw = imat @ np.diag(inertia) @ imat.T
        tau += jp.T @ (mass * (acc - g)) + jr.T @ (Iw @ alpha + np.cross(omega, Iw @ omega))
    tau += np.asarray(m.dof_armature).ravel() * a + np.asarray(m.dof_damping).ravel() * v
    return tau[dofs]


def gravity_torque(flat, qpos, dofs, q, overrides=None, model32=None, attach=None, held=None, rel=None, now=None):
    return inverse_dynamics(flat, qpos, dofs, q, None, None, overrides, model32, attach, held, rel, now)


def mass_matrix(flat, qpos, dofs, q, overrides=None, model32=None, attach=None, held=None, rel=None, now=None):
    """M [n, n]: the block of the joint-space inertia at the candidate on the controlled dofs, M = sum Jp^T m Jp + Jr^T I Jr + armature; a held body's term with
    the carrier's Jacobian at its centre of mass"""
    m = _model(flat, overrides, model32)
    clearance._columns(flat, dofs)
    dofs = [int(d) for d in np.asarray(dofs).ravel()]
    M, (xpos, _, xmat, _, _, xanchor, xaxis) = mjcf.mass_matrix_np(m, clearance.candidate_qpos(flat, qpos, dofs, q))
    for carrier, com, imat, mass, inertia in _payload(flat, m, qpos, dofs, q, attach, held, rel, now)[0]:
        jp, jr = mjcf.body_jacobian_np(m, xpos, xmat, xanchor, xaxis, carrier, com)
        M = M + mass * jp.T @ jp + jr.T @ (imat @ np.diag(inertia) @ imat.T) @ jr
    return M[np.ix_(dofs, dofs)]


def site_jacobian(flat, qpos, site, dofs, q, overrides=None, model32=None, attach=None, held=None, rel=None, now=None):
    """(jacp [3, n], jacr [3, n]): mj_jacSite at the candidate in the controlled columns.  A site on a held body (or below one): the carrier's Jacobian at the
    point placed from the attached pose; on one that is not held: zeros, as for any site no controlled dof moves"""
    m = _model(flat, overrides, model32)
    clearance._columns(flat, dofs)
    if not 0 <= int(site) < int(flat.nsite):
        raise clearance.ClearanceError(f"dynamics: site {site} out of range ({int(flat.nsite)} sites)")
    dofs = [int(d) for d in np.asarray(dofs).ravel()]
    xpos, _, xmat, _, _, xanchor, xaxis = mjcf.kinematics_np(m, clearance.candidate_qpos(flat, qpos, dofs, q))
    b = int(clearance._I(m, "site_bodyid")[int(site)])
    local = np.asarray(m.site_pos, dtype=np.float64).reshape(-1, 3)[int(site)]
    _, carrier_of, poses = _payload(flat, m, qpos, dofs, q, attach, held, rel, now)
    if b in carrier_of:
        p = poses[0][b] + mjcf.quat2mat(poses[1][b]) @ local
        jp, jr = mjcf.body_jacobian_np(m, xpos, xmat, xanchor, xaxis, carrier_of[b], p)
    else:
        jp, jr = mjcf.body_jacobian_np(m, xpos, xmat, xanchor, xaxis, b, xpos[b] + xmat[b] @ local)
    return jp[:, dofs], jr[:, dofs]


def forward_dynamics(flat, qpos, dofs, q, qd=None, tau=None, overrides=None, model32=None, attach=None, held=None, rel=None, now=None):
    """qdd [n] of one candidate: M(q)^-1 (tau - qfrc_bias(q, qd) - dof_damping qd), every other joint locked -- the exact inverse of inverse_dynamics with the
    same attachment, with its limits (rsim_config_forward_dynamics).  tau None: zeros"""
    bias = inverse_dynamics(flat, qpos, dofs, q, qd, None, overrides, model32, attach, held, rel, now)
    t = np.zeros_like(bias) if tau is None else np.asarray(tau, dtype=np.float64).ravel()
    return np.linalg.solve(mass_matrix(flat, qpos, dofs, q, overrides, model32, attach, held, rel, now), t - bias)


def mass_solve(flat, qpos, dofs, q, rhs, overrides=None, model32=None, attach=None, held=None, rel=None, now=None):
    """x = M(q)^-1 rhs for rhs [n] or [n, r] (rsim_config_mass_solve)"""
    return np.linalg.solve(mass_matrix(flat, qpos, dofs, q, overrides, model32, attach, held, rel, now), np.asarray(rhs, dtype=np.float64))


def opspace(flat, qpos, site, dofs, q, overrides=None, model32=None, attach=None, held=None, rel=None, now=None):
    """(lambda_inv [6, 6], minv_jt [n, 6]) with J = [jacp; jacr] of site_jacobian: minv_jt = M^-1 J^T, lambda_inv = J M^-1 J^T (rsim_config_opspace).  The
    operational-space inertia is pinv(lambda_inv) -- lambda_inv is singular for n < 6 and at kinematic singularities -- and Jbar = minv_jt @ pinv(lambda_inv)."""
    J = np.concatenate(site_jacobian(flat, qpos, site, dofs, q, overrides, model32, attach, held, rel, now), axis=0)
    minv_jt = np.linalg.solve(mass_matrix(flat, qpos, dofs, q, overrides, model32, attach, held, rel, now), J.T)
    return J @ minv_jt, minv_jt


GRAD_H = 1e-3      # the first step of the differences in q below (rad, m); the second is half of it


def _richardson(f, h):
    """central difference of f at 0 with one Richardson step from (h, h / 2): the h^2 term of the error cancels, h^4 / 80 f^(5) is left"""
    coarse, fine = (f(h) - f(-h)) / (2.0 * h), (f(0.5 * h) - f(-0.5 * h)) / h
    return (4.0 * fine - coarse) / 3.0


def _vec(x, n):
    return np.zeros(n) if x is None else np.asarray(x, dtype=np.float64).ravel()


def inverse_dynamics_jvp(flat, qpos, dofs, q, qd=None, qdd=None, dq=None, dqd=None, dqdd=None, overrides=None, model32=None, h=GRAD_H):
    """dtau [n]: the derivative of inverse_dynamics at (q, qd, qdd) in the direction (dq, dqd, dqdd) (None: zeros), BY THE DEFINITION OF A DERIVATIVE on this
    file's own inverse_dynamics (rsim_config_inverse_dynamics_jvp; the kernel runs a tangent recursive Newton-Euler, with which this shares nothing).  Along dq:
    central differences with one Richardson step from h and h / 2.  Along dqd: one central difference, exact for any step because tau is quadratic in qd.  Along
    dqdd: one central difference, exact because tau is linear in qdd -- that share is M dqdd.
    The device differentiates with the STORED joint axis a_j (the column is a_j, the angle turns about a_j / |a_j|), so the true derivative of the statement
    differs from the device's recursion by a factor |a_j| per column j of d/dq: relative, at most about 2^-23 for an fp32-rounded unit axis (4.9e-9 of the
    scale on scene D of the tests)."""
    n = len(np.asarray(dofs).ravel())
    q, qd, qdd = _vec(q, n), _vec(qd, n), _vec(qdd, n)
    f = lambda a, b, c: inverse_dynamics(flat, qpos, dofs, a, b, c, overrides, model32)
    out = np.zeros(n)
    if dq is not None and np.any(dq):
        d = _vec(dq, n)
        out += _richardson(lambda s: f(q + s * d, qd, qdd), h)
    if dqd is not None and np.any(dqd):
        d = _vec(dqd, n)
        out += 0.5 * (f(q, qd + d, qdd) - f(q, qd - d, qdd))
    if dqdd is not None and np.any(dqdd):
        d = _vec(dqdd, n)
        out += 0.5 * (f(q, qd, qdd + d) - f(q, qd, qdd - d))
    return out


def inverse_dynamics_grad(flat, qpos, dofs, q, qd=None, qdd=None, overrides=None, model32=None, h=GRAD_H):
    """(tau [n], dtau_dq [n, n], dtau_dqd [n, n]) of one candidate, entry [i, j] = d tau_i / d q_j (resp. qd_j): column j is inverse_dynamics_jvp along e_j
    (rsim_config_inverse_dynamics_grad).  d tau / d qdd is mass_matrix."""
    n = len(np.asarray(dofs).ravel())
    eye = np.eye(n)
    gq = np.stack([inverse_dynamics_jvp(flat, qpos, dofs, q, qd, qdd, eye[j], None, None, overrides, model32, h) for j in range(n)], axis=1)
    gv = np.stack([inverse_dynamics_jvp(flat, qpos, dofs, q, qd, qdd, None, eye[j], None, overrides, model32, h) for j in range(n)], axis=1)
    return inverse_dynamics(flat, qpos, dofs, q, qd, qdd, overrides, model32), gq, gv


def forward_dynamics_grad(flat, qpos, dofs, q, qd=None, tau=None, overrides=None, model32=None, h=GRAD_H):
    """(qdd [n], dqdd_dq [n, n], dqdd_dqd [n, n]) of one candidate (rsim_config_forward_dynamics_grad): with qdd = forward_dynamics(q, qd, tau), the implicit
    function theorem on tau = inverse_dynamics(q, qd, qdd) gives dqdd/dq = -M^-1 dtau/dq and dqdd/dqd = -M^-1 dtau/dqd, both AT (q, qd, qdd); dqdd/dtau is
    M^-1 itself (mass_solve of the identity)."""
    qdd = forward_dynamics(flat, qpos, dofs, q, qd, tau, overrides, model32)
    _, gq, gv = inverse_dynamics_grad(flat, qpos, dofs, q, qd, qdd, overrides, model32, h)
    M = mass_matrix(flat, qpos, dofs, q, overrides, model32)
    return qdd, -np.linalg.solve(M, gq), -np.linalg.solve(M, gv)


def site_position(flat, qpos, site, dofs, q, overrides=None, model32=None):
    m = _model(flat, overrides, model32)
    dofs = [int(d) for d in np.asarray(dofs).ravel()]
    xpos, _, xmat = mjcf.kinematics_np(m, clearance.candidate_qpos(flat, qpos, dofs, q))[:3]
    b = int(clearance._I(m, "site_bodyid")[int(site)])
    return xpos[b] + xmat[b] @ np.asarray(m.site_pos, dtype=np.float64).reshape(-1, 3)[int(site)]


def potential_energy(flat, qpos, dofs, q, overrides=None, model32=None, attach=None, held=None, rel=None, now=None):
    """- sum m g . xipos at the candidate (its gradient along the controlled dofs is the gravity torque); a held body counts at its attached pose -- where the
    free body itself lies does not depend on q, so its own term is a constant and stays"""
    m = _model(flat, overrides, model32)
    dofs = [int(d) for d in np.asarray(dofs).ravel()]
    xipos = mjcf.kinematics_np(m, clearance.candidate_qpos(flat, qpos, dofs, q))[3]
    g = np.asarray(m.gravity, dtype=np.float64).ravel()
    held_part = sum(mass * float(com @ g) for _, com, _, mass, _ in _payload(flat, m, qpos, dofs, q, attach, held, rel, now)[0])
    return -float(np.asarray(m.body_mass).ravel() @ (xipos @ g)) - held_part


def path_derivatives(waypoints, dt):
    """(qd, qdd) of waypoints [..., W, n] spaced dt apart: central differences, one-sided at the two ends (what VecEnv.path_torques forms in torch)"""
    w = np.asarray(waypoints, dtype=np.float64)
    if w.shape[-2] < 2:
        return np.zeros_like(w), np.zeros_like(w)
    qd = np.gradient(w, dt, axis=-2)
    return qd, np.gradient(qd, dt, axis=-2)
