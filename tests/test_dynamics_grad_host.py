"""The fp64 statement of the dynamics derivatives itself (robosuite_amd/dynamics.py inverse_dynamics_grad / inverse_dynamics_jvp / forward_dynamics_grad: the
definition of a derivative on the file's own inverse_dynamics, mass_matrix and forward_dynamics), on scene D (tests/dynamics_scenes.py), "all" dofs, (2, 4), on
the CPU:
  * the Richardson result from (h, h / 2) and from (h / 2, h / 4) agree to 1e-8 of max |dtau_dq|: the h^4 term that is left is below that;
  * at qd = qdd = 0, dtau_dq is the Hessian of potential_energy: symmetric to that tolerance, and equal to a second difference of that function;
  * dtau_dqd at qd = 0 is diag(dof_damping); the JVP along (0, 0, e_j) is column j of mass_matrix to 1e-12;
  * forward_dynamics_grad agrees with central differences of forward_dynamics.
And what THE BOUND of the device tests rests on (tests/dynamics_grad_scenes.py), from fp64 figures alone:
  * the recursion written out in numpy (tangent_walk64) gives the reference's blocks, and on every scene of the device tests its largest intermediate stays
    within KAPPA times the scale;
  * on scene D with per-env tables the reference on env 0's tables is off from the reference on each env's own by more than OFF_FACTOR bounds, which
    tests/test_dynamics_grad.py then asserts of the device."""
import functools

import numpy as np
import pytest

from robosuite_amd import dynamics, mjcf
from tests import clearance_scenes as S
from tests import dynamics_grad_scenes as G
from tests import dynamics_scenes as D
from tests import dynamics_solve_scenes as V

B, K = 2, 4


@functools.lru_cache(maxsize=None)
def scene():
    flat = D.scene_d()
    dofs = D.dofs_d(flat, "all")
    qpos = S.f32(D.scene_d_qpos(flat, B))
    q, qd, qdd = D.draws(flat, dofs, B, K)
    m32 = dynamics.model32(flat)
    ref = G.reference(flat, qpos, dofs, q, qd, qdd)
    return flat, dofs, qpos, q, qd, qdd, m32, ref


def each():
    return [(e, k) for e in range(B) for k in range(K)]


def test_richardson_steps_agree():
    flat, dofs, qpos, q, qd, qdd, m32, ref = scene()
    scale = np.abs(ref["dtau_dq"]).max()
    worst = 0.0
    for e, k in each():
        fine = dynamics.inverse_dynamics_grad(flat, qpos[e], dofs, q[e, k], qd[e, k], qdd[e, k], model32=m32, h=0.5 * dynamics.GRAD_H)[1]
        worst = max(worst, np.abs(fine - ref["dtau_dq"][e, k]).max() / scale)
    print(f"Richardson from (h, h/2) against (h/2, h/4): {worst:.3e} of the scale {scale:.3g}")
    assert worst <= 1e-8 and scale > 5


def test_at_rest_dtau_dq_is_the_hessian_of_the_potential_energy():
    flat, dofs, qpos, q, qd, qdd, m32, ref = scene()
    n, h = len(dofs), 2e-2
    eye = np.eye(n)
    for e, k in each()[::3]:
        H = dynamics.inverse_dynamics_grad(flat, qpos[e], dofs, q[e, k], model32=m32)[1]
        scale = np.abs(ref["dtau_dq"]).max()      # the scene's scale, as above; what is left is the stored axis being off unit length by up to 2^-24 (the column
        assert np.abs(H - H.T).max() <= 1e-8 * scale      # uses it, the angle turns about the normalised one), which makes tau a gradient only that nearly
        U = lambda x: dynamics.potential_energy(flat, qpos[e], dofs, x, model32=m32)      # noqa: E731

        def second(i, j, s):
            return (U(q[e, k] + s * (eye[i] + eye[j])) - U(q[e, k] + s * (eye[i] - eye[j])) - U(q[e, k] - s * (eye[i] - eye[j])) + U(q[e, k] - s * (eye[i] + eye[j]))) / (4 * s * s)

        H2 = np.array([[(4 * second(i, j, 0.5 * h) - second(i, j, h)) / 3 for j in range(n)] for i in range(n)])
        # a second difference with one Richardson step: h^4 times a sixth derivative of sums of sines of the angles, ~ 1e-7 / 100 of the scale; the rounding of
        # four potential energies, 4 * 2^-53 |U| / (h / 2)^2 ~ 1e-10: held to 1e-7 of the scale
        print(f"dtau_dq at rest against the second difference of potential_energy: {np.abs(H - H2).max() / scale:.3e} of the scale")
        assert np.abs(H - H2).max() <= 1e-7 * scale


def test_dtau_dqd_at_rest_is_the_damping_and_dqdd_gives_the_mass_matrix():
    flat, dofs, qpos, q, qd, qdd, m32, ref = scene()
    n = len(dofs)
    damp = np.asarray(m32.dof_damping, dtype=np.float64).ravel()[dofs]
    for e, k in each()[::3]:
        gv = dynamics.inverse_dynamics_grad(flat, qpos[e], dofs, q[e, k], None, qdd[e, k], model32=m32)[2]
        assert np.abs(gv - np.diag(damp)).max() <= 1e-12 * max(1.0, damp.max())
        M = dynamics.mass_matrix(flat, qpos[e], dofs, q[e, k], model32=m32)
        for j in range(n):
            col = dynamics.inverse_dynamics_jvp(flat, qpos[e], dofs, q[e, k], qd[e, k], qdd[e, k], dqdd=np.eye(n)[j], model32=m32)
            assert np.abs(col - M[:, j]).max() <= 1e-12 * max(1.0, np.abs(M).max())


def test_jvp_is_the_product_of_the_blocks():
    flat, dofs, qpos, q, qd, qdd, m32, ref = scene()
    dq, dqd, dqdd = G.directions(B, K, len(dofs))
    for e, k in each()[::3]:
        got = dynamics.inverse_dynamics_jvp(flat, qpos[e], dofs, q[e, k], qd[e, k], qdd[e, k], dq[e, k], dqd[e, k], dqdd[e, k], model32=m32)
        want = ref["dtau_dq"][e, k] @ dq[e, k] + ref["dtau_dqd"][e, k] @ dqd[e, k] + dynamics.mass_matrix(flat, qpos[e], dofs, q[e, k], model32=m32) @ dqdd[e, k]
        assert np.abs(got - want).max() <= 1e-7 * np.abs(want).max()      # two Richardson results of one derivative: the h^4 terms differ


def test_forward_dynamics_grad_against_central_differences():
    flat, dofs, qpos, q, qd, qdd, m32, ref = scene()
    n, h = len(dofs), dynamics.GRAD_H
    tau = V.tau_draw(B, K, n)
    eye = np.eye(n)
    for e, k in each()[::3]:
        x, Xq, Xv = dynamics.forward_dynamics_grad(flat, qpos[e], dofs, q[e, k], qd[e, k], tau[e, k], model32=m32)
        assert np.abs(x - dynamics.forward_dynamics(flat, qpos[e], dofs, q[e, k], qd[e, k], tau[e, k], model32=m32)).max() == 0
        f = lambda a, b: dynamics.forward_dynamics(flat, qpos[e], dofs, a, b, tau[e, k], model32=m32)      # noqa: E731
        Dq = np.stack([dynamics._richardson(lambda s: f(q[e, k] + s * eye[j], qd[e, k]), h) for j in range(n)], axis=1)
        Dv = np.stack([0.5 * (f(q[e, k], qd[e, k] + eye[j]) - f(q[e, k], qd[e, k] - eye[j])) for j in range(n)], axis=1)      # qdd is quadratic in qd
        # both sides carry the h^4 term of a Richardson step (1e-8 of the scale above), one of them through M^-1: held to 1e-7 of the scale
        print(f"forward_dynamics_grad against differences of forward_dynamics: {np.abs(Xq - Dq).max() / np.abs(Dq).max():.3e}, {np.abs(Xv - Dv).max() / np.abs(Dv).max():.3e}")
        assert np.abs(Xq - Dq).max() <= 1e-7 * np.abs(Dq).max() and np.abs(Xv - Dv).max() <= 1e-7 * np.abs(Dv).max()


# ---- what the bound of the device tests rests on ---------------------------------------------------------------------------------------------------------------
def test_the_recursion_in_fp64_gives_the_reference():
    flat, dofs, qpos, q, qd, qdd, m32, ref = scene()
    sq, sv = G.scales(ref)
    for e, k in each():
        gq, gv, _, _ = G.tangent_walk64(flat, qpos[e], dofs, q[e, k], qd[e, k], qdd[e, k], model32=m32)
        # the recursion differentiates with the stored axis, the statement with the normalised one: a factor |axis_j| per column, 2^-23 of dtau_dq; 1e-7 covers it
        assert np.abs(gq - ref["dtau_dq"][e, k]).max() <= 1e-7 * sq and np.abs(gv - ref["dtau_dqd"][e, k]).max() <= 1e-9 * sv


def scenes():
    from tests import raycast_scenes as R
    from tests.dynamics_solve_scenes import chain16

    flat = D.scene_d()
    yield "scene D arm", flat, S.f32(D.scene_d_qpos(flat, 5)), D.dofs_d(flat, "arm"), 5, 13
    yield "scene D all", flat, S.f32(D.scene_d_qpos(flat, 5)), D.dofs_d(flat, "all"), 5, 13
    flat, cfg = R.lift()
    yield "Lift", flat, S.f32(np.tile(R.lift_init_qpos(flat, cfg), (2, 1))), list(range(7)), 2, 5
    flat, dofs = chain16()
    yield "16-hinge chain", flat, np.tile(np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel(), (2, 1)), dofs, 2, 3


def test_kappa_covers_every_scene_of_the_device_tests():
    import os

    assets = os.path.join(os.path.dirname(os.path.abspath(mjcf.__file__)), "assets")
    bax = mjcf.load_model(os.path.join(assets, "peg_baxter_joint_velocity.rsim"))
    more = [("Baxter, both arms", bax, S.f32(np.tile(np.asarray(bax.arrays["qpos0"], dtype=np.float64).ravel(), (2, 1))), list(range(14)), 2, 5)]
    for name, flat, qpos, dofs, b, k in list(scenes()) + more:
        kq, kv = G.kappa_of(flat, qpos, dofs, *D.draws(flat, dofs, b, k))
        print(f"largest intermediate of the tangent walk over the scale, {name}: d/dq {kq:.2f}, d/dqd {kv:.2f} (KAPPA {G.KAPPA:g})")
        assert max(kq, kv) <= G.KAPPA


@pytest.mark.parametrize("which", ("arm", "all"))
def test_env_zeros_tables_are_off_by_many_bounds(which):
    flat = D.scene_d()
    dofs = D.dofs_d(flat, which)
    qpos = S.f32(D.scene_d_qpos(flat, 5))
    q, qd, qdd = D.draws(flat, dofs, 5, 13)
    over = G.scene_d_overrides(flat, 5)
    right, wrong = G.reference(flat, qpos, dofs, q, qd, qdd, overrides=over), G.reference(flat, qpos, dofs, q, qd, qdd, overrides=over[0])
    off, bound = G.errors(right, wrong), G.tangent_rounding_bound(D.depth(flat, dofs), D.EPS32)
    print(f"scene D {which}: env 0's tables against each env's own: dtau_dq {off['dtau_dq'] / bound:.0f} bounds, dtau_dqd {off['dtau_dqd'] / bound:.0f} bounds")
    assert min(off["dtau_dq"], off["dtau_dqd"]) > (G.OFF_FACTOR + 1) * bound      # one bound is the device's own share
