"""The fp64 statement of the dynamics queries WITH CARRIED PAYLOADS (robosuite_amd/dynamics.py: attach / held / rel) on the CPU -- the mirror is right before
the device is held to it:

  * THE WELDED TWIN.  tau, M and J(load_tip) of the mirror with attach and rel on scene P against (a) the attachment-free mirror and (b) the fp64 oracle
    (oracle/rsim_oracle.c), both on the twin model in which every held body is a jointless child of its carrier at rel with the same inertial.  The oracle
    shares no code with the mirror: a check from outside.  The same on scene J for the subtree (a jaw on a hinge, a tip on a slide, a guard; no site).
    Bound: fp64 rounding, dynamics_scenes.rounding_bound(bodies on the longest path with the attached chain, 2^-53).
  * ENERGY.  The gravity torque with the payload is the central-difference gradient of potential_energy extended by the held bodies; h and bound are
    tests/test_dynamics_host.py's (its docstring has the reasoning).
  * NOT HELD.  The mirror with held all false equals the plain mirror exactly.
  * INVERSE.  forward_dynamics(attach) followed by inverse_dynamics(attach) returns the torque."""
import numpy as np
import pytest

from robosuite_amd import clearance, dynamics
from tests import attach_scenes as A
from tests import dynamics_attach_scenes as P
from tests import dynamics_scenes as D
from tests.test_dynamics_host import FD_BOUND, FD_H

B, K = 6, 2      # envs 0 .. 5 show all four held rows of scene P


def twin_references(flat, twin_of, qpos, dofs, q, qd, qdd, attach, held, rel, site_name):
    """per env: (mirror with attach on the scene, plain mirror on the twin, oracle on the twin), each a dict of [1, K, ...] arrays, exact fp64 tables"""
    for e in range(q.shape[0]):
        rows = clearance.relative_poses(flat, qpos[e], attach, None if rel is None else rel[e], model32=flat)
        twin = twin_of(rows, held[e])
        tq, td = P.twin_qpos(flat, twin, qpos[e])[None], P.twin_dofs(flat, twin, dofs)
        site = None if site_name is None else flat.names["site"].index(site_name)
        tsite = None if site_name is None else twin.names["site"].index(site_name)
        a = (q[e:e + 1], qd[e:e + 1], qdd[e:e + 1])
        got = P.reference(flat, qpos[e:e + 1], dofs, a[0], attach, held[e:e + 1], None if rel is None else rel[e:e + 1], a[1], a[2], site, exact=True)
        yield e, got, D.reference_exact(twin, tq, td, *a, tsite), D.oracle_reference(twin, tq, td, *a, tsite)


def hold(what, got, ref, bound, with_j):
    fig = D.errors(got if with_j else {k: got[k] for k in ("tau", "M")}, ref)
    for k, v in fig.items():
        print(f"payload statement {what}: {k} {v:.3e} (bound {bound:.1e})")
        assert v <= bound, (what, k, v)


@pytest.mark.parametrize("mode", P.REL_MODES)
def test_welded_twin_scene_p(mode):
    flat = P.scene_p()
    dofs, attach, held, rel, qpos = P.dofs_p(flat), P.attach_p(flat), P.held_rows(B), P.rel_of(mode, B), P.scene_p_qpos(flat, B)
    q, qd, qdd = D.draws(flat, dofs, B, K)
    bound = D.rounding_bound(P.depth_att(flat, dofs, attach), D.EPS64)
    seen = 0.0
    for e, got, mirror, oracle in twin_references(flat, P.welded_p, qpos, dofs, q, qd, qdd, attach, held, rel, "load_tip"):
        hold(f"scene P {mode} env {e} vs the plain mirror on the twin", got, mirror, bound, True)
        hold(f"scene P {mode} env {e} vs the oracle on the twin", got, oracle, bound, True)
        plain = D.reference_exact(flat, qpos[e:e + 1], dofs, q[e:e + 1], qd[e:e + 1], qdd[e:e + 1], flat.names["site"].index("load_tip"))
        if held[e].any():
            seen = max(seen, np.abs(plain["tau"] - got["tau"]).max() / np.abs(got["tau"]).max())
        if not held[e, 0]:
            assert not got["jacp"].any() and not got["jacr"].any()      # a site on a body that is not held: zeros
        else:
            assert got["jacp"].any() and got["jacr"].any()
    assert seen > 1e-2      # the twin is not the empty-hand model: the payload shows


@pytest.mark.parametrize("mode", A.REL_MODES)
def test_welded_twin_scene_j_subtree(mode):
    flat = A.scene_j()
    dofs, attach, held, qpos = A.dofs_j(flat), A.attach_j(flat), A.held_rows_j(B), A.scene_j_qpos(flat, B)
    rel = None if mode == "state" else A.rel_given_j(B)
    q, qd, qdd = D.draws(flat, dofs, B, K)
    bound = D.rounding_bound(P.depth_att(flat, dofs, attach), D.EPS64)
    assert P.depth_att(flat, dofs, attach) == D.depth(flat, dofs) + 3      # tool, jaw, tip
    for e, got, mirror, oracle in twin_references(flat, P.welded_j, qpos, dofs, q, qd, qdd, attach, held, rel, None):
        hold(f"scene J {mode} env {e} vs the plain mirror on the twin", got, mirror, bound, False)
        hold(f"scene J {mode} env {e} vs the oracle on the twin", got, oracle, bound, False)


def test_gravity_torque_is_the_gradient_of_the_energy_with_the_held_bodies():
    flat = P.scene_p()
    dofs, attach, held, rel, qpos = P.dofs_p(flat), P.attach_p(flat), P.held_rows(B), P.rel_given(B), P.scene_p_qpos(flat, B)
    q = D.draws(flat, dofs, B, K)[0]
    n = len(dofs)
    for e in range(B):
        for r in (None, rel[e]):
            kw = dict(attach=attach, held=held[e], rel=r)
            grav = dynamics.gravity_torque(flat, qpos[e], dofs, q[e, 0], **kw)
            for c in range(n):
                dq = np.zeros(n); dq[c] = FD_H
                dU = (dynamics.potential_energy(flat, qpos[e], dofs, q[e, 0] + dq, **kw) - dynamics.potential_energy(flat, qpos[e], dofs, q[e, 0] - dq, **kw)) / (2 * FD_H)
                assert abs(dU - grav[c]) <= FD_BOUND * max(1.0, np.abs(grav).max()), (e, c, dU, grav[c])


def test_not_held_is_the_plain_mirror_exactly():
    flat = P.scene_p()
    dofs, attach, qpos = P.dofs_p(flat), P.attach_p(flat), P.scene_p_qpos(flat, 2)
    q, qd, qdd = D.draws(flat, dofs, 2, K)
    site = flat.names["site"].index("tip")
    for rel in (None, P.rel_given(2)):
        got = P.reference(flat, qpos, dofs, q, attach, np.zeros((2, 2), dtype=bool), rel, qd, qdd, site)
        ref = D.reference(flat, qpos, dofs, q, qd, qdd, site)
        assert all(np.array_equal(got[k], ref[k]) for k in ref)
    held = P.held_rows(6)      # env 5 holds the second attachment only: the first one's site reads zeros, the arm's own site is the plain one
    jp, jr = dynamics.site_jacobian(flat, qpos[0], flat.names["site"].index("load_tip"), dofs, q[0, 0], attach=attach, held=held[5])
    assert not jp.any() and not jr.any()


def test_forward_dynamics_inverts_inverse_dynamics_with_the_same_attachment():
    flat = P.scene_p()
    dofs, attach, held, rel, qpos = P.dofs_p(flat), P.attach_p(flat), P.held_rows(B), P.rel_given(B), P.scene_p_qpos(flat, B)
    q, qd, tau = D.draws(flat, dofs, B, 1)
    bound = 2 * D.rounding_bound(P.depth_att(flat, dofs, attach), D.EPS64)
    for e in range(B):
        kw = dict(attach=attach, held=held[e], rel=rel[e])
        M = dynamics.mass_matrix(flat, qpos[e], dofs, q[e, 0], **kw)
        qdd = dynamics.forward_dynamics(flat, qpos[e], dofs, q[e, 0], qd[e, 0], tau[e, 0], **kw)
        back = dynamics.inverse_dynamics(flat, qpos[e], dofs, q[e, 0], qd[e, 0], qdd, **kw)
        # one solve and one product with M: the rounding of either is amplified by at most cond(M)
        assert np.abs(back - tau[e, 0]).max() <= bound * np.linalg.cond(M) * max(1.0, np.abs(tau[e, 0]).max()), e
        plain = dynamics.forward_dynamics(flat, qpos[e], dofs, q[e, 0], qd[e, 0], tau[e, 0])
        assert (np.abs(plain - qdd).max() > 1e-3) == bool(held[e].any())      # the payload changes the acceleration exactly where something is held


def test_refusals_are_the_attached_clearance_querys():
    flat = P.scene_p()
    dofs, attach, qpos = P.dofs_p(flat), P.attach_p(flat), P.scene_p_qpos(flat, 1)
    q = D.draws(flat, dofs, 1, 1)[0]
    b = flat.names["body"].index
    with pytest.raises(clearance.ClearanceError, match="attached twice"):
        dynamics.inverse_dynamics(flat, qpos[0], dofs, q[0, 0], attach=[attach[0], (attach[0][0], b("side"))])
    arm = D.dofs_d(flat, "arm")
    with pytest.raises(clearance.ClearanceError, match="not moved by the controlled dofs"):
        dynamics.mass_matrix(flat, qpos[0], arm[1:], q[0, 0, :2], attach=[(b("load2"), b("side"))])
    with pytest.raises(clearance.ClearanceError, match="not a child of the world"):
        dynamics.site_jacobian(flat, qpos[0], 0, dofs, q[0, 0], attach=[(b("f1"), b("l2"))])
