"""References, scales and THE BOUND shared by tests/test_dynamics_grad_host.py (CPU, the fp64 statement robosuite_amd/dynamics.py inverse_dynamics_grad /
inverse_dynamics_jvp / forward_dynamics_grad), tests/test_dynamics_grad_core_host.py (CPU, the fp32 core under sanitizers) and tests/test_dynamics_grad.py
(GPU, the kernels against both).  The scenes and the seeded draws are tests/dynamics_scenes.py's."""
import numpy as np

from robosuite_amd import clearance, dynamics, mjcf
from tests import dynamics_scenes as D

SEED_DQ, SEED_DQD, SEED_DQDD = 621, 622, 623      # the directions of the JVP: uniform in +-1


def reference(flat, qpos, dofs, q, qd=None, qdd=None, overrides=None, want=("id",), tau=None):
    """the fp64 statement at fp32-rounded model tables for qpos [B, nq], q / qd / qdd [B, K, n] (overrides: None, one dict or a list of one per env) ->
    dict(tau [B, K, n], dtau_dq, dtau_dqd [B, K, n, n]) for "id" in want; "fd": dict(qdd, dqdd_dq, dqdd_dqd) of forward dynamics at the torques tau [B, K, n]"""
    B, K, n = q.shape
    out = {k: np.zeros((B, K, n)) for k in ("tau", "qdd")}
    out.update({k: np.zeros((B, K, n, n)) for k in ("dtau_dq", "dtau_dqd", "dqdd_dq", "dqdd_dqd")})
    shared = None if isinstance(overrides, list) else dynamics.model32(flat, overrides)
    for e in range(B):
        m32 = shared if shared is not None else dynamics.model32(flat, overrides[e])
        for k in range(K):
            v = None if qd is None else qd[e, k]
            if "id" in want:
                out["tau"][e, k], out["dtau_dq"][e, k], out["dtau_dqd"][e, k] = dynamics.inverse_dynamics_grad(
                    flat, qpos[e], dofs, q[e, k], v, None if qdd is None else qdd[e, k], model32=m32)
            if "fd" in want:
                out["qdd"][e, k], out["dqdd_dq"][e, k], out["dqdd_dqd"][e, k] = dynamics.forward_dynamics_grad(
                    flat, qpos[e], dofs, q[e, k], v, None if tau is None else tau[e, k], model32=m32)
    return out


def directions(B, K, n):
    """(dq, dqd, dqdd) [B, K, n] each, uniform in +-1, rounded to float32"""
    return tuple(D.rates(B, K, n, s, 1.0) for s in (SEED_DQ, SEED_DQD, SEED_DQDD))


def reference_jvp(flat, qpos, dofs, q, qd, qdd, dq, dqd, dqdd, overrides=None):
    B, K, n = q.shape
    out = np.zeros((B, K, n))
    pick = lambda x, e, k: None if x is None else x[e, k]      # noqa: E731
    shared = None if isinstance(overrides, list) else dynamics.model32(flat, overrides)
    for e in range(B):
        m32 = shared if shared is not None else dynamics.model32(flat, overrides[e])
        for k in range(K):
            out[e, k] = dynamics.inverse_dynamics_jvp(flat, qpos[e], dofs, q[e, k], pick(qd, e, k), pick(qdd, e, k), pick(dq, e, k), pick(dqd, e, k),
                                                      pick(dqdd, e, k), model32=m32)
    return out


# the ratio of the largest intermediate of the tangent walk to the scale of its result, rounded up to a power of two: tangent_walk64 below computes the ratio in
# fp64 for one candidate, kappa_of for a scene.  The scenes of the tests reach 1.0 .. 1.6 for d / dq and 1.7 .. 3.2 for d / dqd (profiles/dyn_grad_parity.txt).
KAPPA = 4.0


def tangent_rounding_bound(nbodies, eps):
    """The error bound of dtau_dq, dtau_dqd and the JVP, relative to the per-scene scales max |dtau_dq_ref| and max |dtau_dqd_ref| (errors() below), from the
    operation count of csrc/rsim_dyn_grad_core.h -- by reasoning, not from a run.  The longest dependent chain of roundings behind one output, for a path of
    `nbodies` moved bodies:
      per body  ~20 in the pose (shared with the primal walk: dynamics_scenes.rounding_bound), ~10 in the primal V and A the tangent walk recomputes,
                ~19 in the tangent forward walk (D += S dq: 2;  dS = D x S: 4;  dV x S + V x dS: 5;  the four scaled terms summed into dA: 5;  dV: 3),
                1 in the backward sum of dW                                                                                                  = 50 per body
      once      ~8 for the joint frame, ~40 for the body's wrench tangent (inertial frame 10;  u = dV - D x V: 5;  into the body frame and back: 20;  the
                cross products and sums of the three inertia terms and D x* W: 5), ~8 for the two projections dS . W + S . dW and the diagonal terms  = 56
    Each rounding is at most eps relative to the intermediate it rounds; intermediates stay within KAPPA = 4 times the scale (kappa_of: computed in fp64
    for the scenes of the tests by the recursion written out in numpy and held to the reference -- tests/test_dynamics_grad_host.py holds every scene's figure
    to <= KAPPA; the device's output plays no part in it).  Linear accumulation, no cancellation assumed:
        bound = (50 nbodies + 56) KAPPA eps."""
    return (50 * nbodies + 56) * KAPPA * eps


def scales(ref):
    return float(np.abs(ref["dtau_dq"]).max()), float(np.abs(ref["dtau_dqd"]).max())


def jvp_scale(ref, M, n):
    """the scale a JVP along a direction with entries in +-1 is held to: the walk is linear in the direction, whose 1-norm is at most n, and the three blocks
    it combines have the scales max |dtau_dq_ref|, max |dtau_dqd_ref| and max |M_ref|"""
    return n * max(scales(ref) + (float(np.abs(M).max()),))


def errors(got, ref):
    """worst absolute errors against the per-scene scales max |dtau_dq_ref|, max |dtau_dqd_ref| (entries cross zero, so not per entry); a JVP against
    ref["jvp_scale"] (jvp_scale above)"""
    out = {}
    for k in ("dtau_dq", "dtau_dqd", "jvp"):
        if k in got and k in ref:
            scale = ref["jvp_scale"] if k == "jvp" else np.abs(ref[k]).max()
            out[k] = float(np.abs(np.asarray(got[k], dtype=np.float64) - ref[k]).max() / scale)
    return out


# the reference on env 0's tables must be off by more than this many bounds for the other envs (tests/test_dynamics_grad_host.py holds the factor from the two
# references alone)
OFF_FACTOR = 100.0


# ---- the recursion itself in fp64: where KAPPA comes from ---------------------------------------------------------------------------------------------------------
def _xm(a, b):
    """a x b of two motion vectors (w, v)"""
    return np.concatenate([np.cross(a[:3], b[:3]), np.cross(a[:3], b[3:]) + np.cross(a[3:], b[:3])])


def _xf(a, f):
    """a x* F of a motion vector and a force vector (n, f)"""
    return np.concatenate([np.cross(a[:3], f[:3]) + np.cross(a[3:], f[3:]), np.cross(a[:3], f[3:])])


def tangent_walk64(flat, qpos, dofs, q, qd=None, qdd=None, model32=None):
    """The tangent Newton-Euler recursion of csrc/rsim_dyn_grad_core.h written out in fp64 numpy on mjcf.kinematics_np, for one candidate: world vectors about
    the first moved body's position, the 2 n unit directions one after the other.  -> (dtau_dq [n, n], dtau_dqd [n, n], peak_q, peak_qd): the blocks, and the
    largest absolute value any FORCE-type intermediate of the walk takes over the directions of dq, resp. dqd -- the four terms of dW with the
    two shares of every moment the inertia forms, their partial sums, the subtree sums of dW and the two projections.  (A motion-type intermediate reaches
    the result only through the body's inertia, where its rounding is relative to one of those.)  tests/test_dynamics_grad_host.py holds the blocks to the reference, so the peaks are the peaks of the right recursion; KAPPA is
    peak over scale.  It shares the algorithm with the kernel on purpose and is no reference for it."""
    m = model32 if model32 is not None else flat
    col = clearance._columns(flat, dofs)
    dofs = [int(d) for d in np.asarray(dofs).ravel()]
    n = len(dofs)
    xpos, _, _, xipos, ximat, xanchor, xaxis = mjcf.kinematics_np(m, clearance.candidate_qpos(flat, qpos, dofs, q))
    parent, jadr, jnum, jtype = (clearance._I(m, k) for k in ("body_parentid", "body_jntadr", "body_jntnum", "jnt_type"))
    nb = int(m.nbody)
    moved = clearance.signatures(flat, dofs) != 0
    org = xpos[int(np.flatnonzero(moved)[0])]
    g = np.asarray(m.gravity, dtype=np.float64).ravel()
    mass, inertia = np.asarray(m.body_mass, dtype=np.float64).ravel(), np.asarray(m.body_inertia, dtype=np.float64).reshape(-1, 3)
    arm, damp = np.asarray(m.dof_armature, dtype=np.float64).ravel(), np.asarray(m.dof_damping, dtype=np.float64).ravel()
    x, xx = np.zeros(n) if qd is None else np.asarray(qd, dtype=np.float64), np.zeros(n) if qdd is None else np.asarray(qdd, dtype=np.float64)

    def motion(j):
        a = xaxis[j]
        return np.concatenate([np.zeros(3), a]) if jtype[j] == mjcf.JNT_SLIDE else np.concatenate([a, np.cross(xanchor[j] - org, a)])

    def imul(b, X):      # the body's spatial inertia about org applied to a motion vector
        r, R = xipos[b] - org, ximat[b]
        f = mass[b] * (X[3:] + np.cross(X[:3], r))
        parts = (R @ (inertia[b] * (R.T @ X[:3])), np.cross(r, f))
        inner[0] = max(inner[0], float(np.abs(parts[0]).max()), float(np.abs(parts[1]).max()))      # the two shares of the moment, before they are added
        return np.concatenate([parts[0] + parts[1], f])

    out, peaks = [np.zeros((n, n)), np.zeros((n, n))], [0.0, 0.0]
    for kind in (0, 1):
        for jdir in range(n):
            V, A, Dl, dV, dA, W, dW = (np.zeros((nb, 6)) for _ in range(7))
            A[0, 3:] = -g
            peak, joints, inner = 0.0, [], [0.0]
            for b in range(1, nb):
                p = parent[b]
                V[b], A[b], Dl[b], dV[b], dA[b] = V[p], A[p], Dl[p], dV[p], dA[p]
                if not moved[b]:
                    continue
                for j in range(jadr[b], jadr[b] + jnum[b]):
                    if j not in col:
                        continue
                    c = col[j]
                    S = motion(j)
                    y, yd = float(kind == 0 and c == jdir), float(kind == 1 and c == jdir)
                    dS, VS = _xm(Dl[b], S), _xm(V[b], S)
                    dA[b] = dA[b] + dS * xx[c] + (_xm(dV[b], S) + _xm(V[b], dS)) * x[c] + VS * yd
                    dV[b] = dV[b] + dS * x[c] + S * yd
                    Dl[b] = Dl[b] + S * y
                    A[b] = A[b] + S * xx[c] + VS * x[c]
                    V[b] = V[b] + S * x[c]
                    joints.append((b, c, S, dS, damp[dofs[c]] * yd))
                IV = imul(b, V[b])
                W[b] = imul(b, A[b]) + _xf(V[b], IV)
                inner[0] = 0.0      # (of the tangent's own products only: the primal's are dynamics_scenes.rounding_bound's)
                u, a = dV[b] - _xm(Dl[b], V[b]), dA[b] - _xm(Dl[b], A[b])
                terms = (_xf(Dl[b], W[b]), imul(b, a), _xf(u, IV), _xf(V[b], imul(b, u)))
                dW[b] = sum(terms)
                peak = max([peak, inner[0]] + [float(np.abs(t).max()) for t in terms + (np.cumsum(terms, axis=0),)])
            for b in range(nb - 1, 0, -1):      # the subtree sums
                if moved[b] and moved[parent[b]]:
                    W[parent[b]] += W[b]; dW[parent[b]] += dW[b]
                    peak = max(peak, float(np.abs(dW[parent[b]]).max()))
            for b, c, S, dS, diag in joints:
                two = (float(dS @ W[b]), float(S @ dW[b]))
                out[kind][c, jdir] = two[0] + two[1] + diag
                peak = max(peak, abs(two[0]), abs(two[1]))
            peaks[kind] = max(peaks[kind], peak)
    return out[0], out[1], peaks[0], peaks[1]


def kappa_of(flat, qpos, dofs, q, qd=None, qdd=None, overrides=None):
    """(peak / scale of d / dq, of d / dqd) over the candidates of a scene, qpos [B, nq], q / qd / qdd [B, K, n] (overrides: as reference): what KAPPA rounds up"""
    B, K, n = q.shape
    m32 = [dynamics.model32(flat, overrides[e] if isinstance(overrides, list) else overrides) for e in range(B if isinstance(overrides, list) else 1)]
    res = [tangent_walk64(flat, qpos[e], dofs, q[e, k], None if qd is None else qd[e, k], None if qdd is None else qdd[e, k], model32=m32[e % len(m32)])
           for e in range(B) for k in range(K)]
    return tuple(max(r[2 + i] for r in res) / max(np.abs(r[i]).max() for r in res) for i in (0, 1))


def scene_d_overrides(flat, B):
    """what tests/test_dynamics.py scene_d_batch overrides per env, formed here without a device: one link's body_mass scaled, one dof_armature raised, in
    float32 as the batch holds them -> a list of one dict per env (the GPU test holds it equal to the batch's own)"""
    from tests import clearance_scenes as S

    mass = np.tile(np.asarray(flat.arrays["body_mass"], dtype=np.float32).ravel(), (B, 1))
    arm = np.tile(np.asarray(flat.arrays["dof_armature"], dtype=np.float32).ravel(), (B, 1))
    b, d = flat.names["body"].index("l1"), S.dofs_of(flat, ("h2",))[0]
    for e in range(B):
        mass[e, b] *= 1.0 + 0.35 * (e + 1); arm[e, d] += 0.04 * (e + 1)
    return [{"body_mass": mass[e], "dof_armature": arm[e]} for e in range(B)]
