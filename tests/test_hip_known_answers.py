"""The fused kernel against closed forms of MuJoCo's DOCUMENTED model -- not against the oracle: the same one-body systems tests/test_oracle.py holds the
fp64 restatement to (soft-constraint resting depths of a contact and a joint limit, implicit joint damping, soft friction loss, torsional slip on the
elliptic cone), run through the C-ABI's B = 1 entries (rsim_step / rsim_forward) on the MI355X.  What agrees here agrees with the documentation itself,
whatever the oracle does.  The second half holds the terms that no fixture or generated model moves, on the cases of tests/known_answer_cases.py: fluid forces
and wind, contact margin and gap, limit margins, the contact-parameter mixing rules, frictionless contacts, velocity and affine actuators."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from robosuite_amd import mjcf  # noqa: E402
from tests import known_answer_cases as K  # noqa: E402
from tests.util import make_hip  # noqa: E402

H, G0 = 0.002, 9.81


def _batch(xml):
    flat = mjcf.compile_mjcf(xml)
    hm, hb = make_hip(flat, None, B=1)
    hb.set("qpos", np.asarray(flat.qpos0, dtype=np.float64)[None]); hb.set("qvel", 0.0); hb.set("ctrl", 0.0); hb.set("qacc_warmstart", 0.0)
    return flat, hb


_depth = K.resting_depth           # r = a0 (1 - d(r)) / (k d(r)^2) by fixed-point iteration on the documented impedance and spring


@pytest.mark.parametrize("solref,solimp", (((0.02, 1.0), (0.9, 0.95, 0.001, 0.5, 2)), ((0.01, 0.7), (0.8, 0.8, 0.002, 0.5, 2)), ((0.003, 1.0), (0.95, 0.99, 0.0005, 0.3, 3))))
def test_resting_depths_of_a_contact_and_a_joint_limit(solref, solimp):
    sr, si = " ".join(map(str, solref)), " ".join(map(str, solimp))
    flat, hb = _batch(f"""<mujoco><option timestep="{H}" cone="elliptic"/><worldbody><geom name="floor" type="plane" size="1 1 0.1" solref="{sr}" solimp="{si}"/>
        <body name="ball" pos="0 0 0.05"><freejoint/><geom name="ball" type="sphere" size="0.05" density="1000" solref="{sr}" solimp="{si}"/></body></worldbody></mujoco>""")
    for _ in range(3000):
        hb.step()
    hb.forward()
    q, v = hb.get("qpos")[0], hb.get("qvel")[0]
    want = _depth(G0, solref, solimp)
    assert np.abs(v).max() < 1e-4 and hb.get("ncon")[0] == 1
    assert 0.05 - q[2] == pytest.approx(want, rel=2e-3, abs=2e-7)               # fp32 position of a 5 cm ball: 4e-9 m of rounding on depths of 1e-5 .. 4e-4 m
    assert hb.contacts(0)[0]["normal_force"] == pytest.approx(1000 * 4 / 3 * np.pi * 0.05**3 * G0, rel=1e-3)   # measured 2e-4 (fp32)
    # a pendulum pushed against its joint limit by a motor
    flat, hb = _batch(f"""<mujoco><compiler angle="radian"/><option timestep="{H}" gravity="0 0 0"/><worldbody><body name="p"><joint name="h" type="hinge" axis="0 1 0" range="-0.3 0.3" solreflimit="{sr}" solimplimit="{si}"/>
        <geom type="sphere" size="0.02" pos="0.2 0 0" mass="0.5" contype="0" conaffinity="0"/></body></worldbody><actuator><motor joint="h" gear="1"/></actuator></mujoco>""")
    hb.set("qpos", np.array([[0.25]])); hb.set("ctrl", np.array([[0.4]]))
    for _ in range(6000):
        hb.step()
    hb.forward()
    inertia = float(hb.get("qM")[0].ravel()[0])
    assert abs(hb.get("qvel")[0][0]) < 1e-4 and hb.get("nefc")[0] == 1
    assert hb.get("qpos")[0][0] - 0.3 == pytest.approx(_depth(0.4 / inertia, solref, solimp), rel=5e-3, abs=3e-7)


def test_damping_friction_loss_and_torsional_slip():
    pend = """<mujoco><compiler angle="radian"/><option timestep="%g" gravity="0 0 0"/><worldbody><body><joint name="h" type="hinge" axis="0 0 1" %s/>
              <geom type="box" size="0.1 0.02 0.02" mass="1.5" contype="0" conaffinity="0"/></body></worldbody><actuator><motor joint="h" gear="1"/></actuator></mujoco>"""
    # implicit joint damping: one step takes v to v I / (I + h b)
    b = 0.7
    flat, hb = _batch(pend % (H, 'damping="%g"' % b))
    hb.forward(); inertia = float(hb.get("qM")[0].ravel()[0])
    hb.set("qvel", np.array([[2.0]]))
    v = 2.0
    for _ in range(50):
        hb.step(); v *= inertia / (inertia + H * b)
        assert hb.get("qvel")[0][0] == pytest.approx(v, rel=2e-5)            # fp32 over 50 steps: measured 2e-6
    # soft friction loss: creep at tau R / b below the bound, (tau - F) / I above it
    flat, hb = _batch(pend % (H, 'frictionloss="0.3"'))
    hb.set("ctrl", np.array([[0.25]]))
    for _ in range(400):
        hb.step()
    creep = 0.25 * (0.1 / 0.9) * (1.0 / inertia) / (2.0 / (0.95 * 0.02))
    assert hb.get("qvel")[0][0] == pytest.approx(creep, rel=1e-4)
    hb.set("ctrl", np.array([[0.8]])); hb.forward()
    assert hb.get("qacc")[0][0] == pytest.approx((0.8 - 0.3) / inertia, rel=2e-3)
    # torsional slip: the force on the elliptic cone, Newton's and Euler's equations for it
    mu_t, r = 0.02, 0.05
    flat, hb = _batch(f"""<mujoco><option timestep="{H}" cone="elliptic" impratio="1"/><worldbody><geom type="plane" size="1 1 0.1" condim="4" friction="1 {mu_t} 0.0001"/>
        <body name="ball" pos="0 0 {r}"><freejoint/><geom type="sphere" size="{r}" density="1000" condim="4" friction="1 {mu_t} 0.0001"/></body></worldbody></mujoco>""")
    for _ in range(1500):
        hb.step()
    m_ball = 1000 * 4 / 3 * np.pi * r**3
    v = np.zeros((1, 6)); v[0, 5] = 30.0
    hb.set("qvel", v); hb.forward()
    c = hb.contacts(0)[0]
    f = hb.get("efc_force")[0][c["efc_address"]:c["efc_address"] + c["dim"]]
    a = hb.get("qacc")[0]
    assert c["dim"] == 4 and abs(f[1]) < 1e-4 and abs(f[2]) < 1e-4
    assert abs(f[3]) == pytest.approx(mu_t * f[0], rel=1e-5)
    assert a[5] == pytest.approx(f[3] / (0.4 * m_ball * r * r), rel=1e-4)
    assert m_ball * a[2] == pytest.approx(f[0] - m_ball * G0, rel=1e-3)


def test_free_flight_and_coulomb_threshold():
    """Mechanics, no simulator: (a) a box in free flight follows the semi-implicit Euler recursion of constant gravity exactly (v_n = v_0 - g h n,
    z_n = z_0 + v_0 h n - g h^2 n (n + 1) / 2) and keeps its angular velocity (isotropic inertia); (b) a flat box on a plane under gravity tilted by theta stays put
    while tan(theta) < mu (elliptic cone, impratio 20, four corner contacts); above it every slipping contact's force sits on the cone, |f_t| = mu f_n against
    the motion, and the box obeys Newton's equation for those forces."""
    flat, hb = _batch(f"""<mujoco><option timestep="{H}"/><worldbody><body pos="0 0 1"><freejoint/><geom type="box" size="0.03 0.03 0.03" density="400"/></body></worldbody></mujoco>""")
    v0 = np.array([[0.1, -0.2, 0.3, 1.0, 2.0, -1.5]])
    hb.set("qvel", v0)
    n = 200
    for _ in range(n):
        hb.step()
    q, v = hb.get("qpos")[0], hb.get("qvel")[0]
    assert v[:3] == pytest.approx([0.1, -0.2, 0.3 - G0 * H * n], rel=1e-5, abs=1e-6)
    assert q[:3] == pytest.approx([0.1 * H * n, -0.2 * H * n, 1.0 + 0.3 * H * n - G0 * H * H * n * (n + 1) / 2], abs=2e-6)
    assert v[3:] == pytest.approx(v0[0, 3:], rel=1e-5)
    mu = 0.3
    m_box = 400 * 0.2 * 0.2 * 0.02
    for fac in (0.5, 0.9, 1.5):
        th = np.arctan(fac * mu)
        gx, gz = G0 * np.sin(th), -G0 * np.cos(th)
        flat, hb = _batch(f"""<mujoco><option timestep="{H}" cone="elliptic" impratio="20" gravity="{gx} 0 {gz}"/><worldbody><geom type="plane" size="5 5 0.1" friction="{mu} 0.005 0.0001"/>
            <body pos="0 0 0.01"><freejoint/><geom type="box" size="0.1 0.1 0.01" density="400" friction="{mu} 0.005 0.0001"/></body></worldbody></mujoco>""")
        if fac < 1.0:                                           # below the Coulomb threshold: stays put (soft contacts creep at ~3e-5 m/s)
            for _ in range(300):
                hb.step()
            assert abs(hb.get("qvel")[0][0]) < 1e-3 and hb.get("ncon")[0] == 4, fac
            continue
        # above it: settle under the normal component alone, then give it the downhill velocity and evaluate one forward(): every corner contact slips, its
        # force lies ON the cone (|f_t| = mu f_n) against the motion, and the box obeys Newton's equation along the plane for exactly those forces.
        # (A sustained slide is no clean known answer in this model: the primal cone couples friction into the normal direction and the box hops.)
        flat0, hb0 = _batch(f"""<mujoco><option timestep="{H}" cone="elliptic" impratio="20" gravity="0 0 {gz}"/><worldbody><geom type="plane" size="5 5 0.1" friction="{mu} 0.005 0.0001"/>
            <body pos="0 0 0.01"><freejoint/><geom type="box" size="0.1 0.1 0.01" density="400" friction="{mu} 0.005 0.0001"/></body></worldbody></mujoco>""")
        for _ in range(1500):
            hb0.step()
        hb.set("qpos", hb0.get("qpos").astype(np.float64))
        v = np.zeros((1, 6)); v[0, 0] = 0.5
        hb.set("qvel", v); hb.forward()
        ft_sum, fn_sum = 0.0, 0.0
        cons = hb.contacts(0)
        assert len(cons) == 4
        for c in cons:
            f = hb.get("efc_force")[0][c["efc_address"]:c["efc_address"] + c["dim"]]
            t_world = c["frame"][1] * f[1] + c["frame"][2] * f[2]
            assert np.linalg.norm(f[1:3]) == pytest.approx(mu * f[0], rel=1e-4)
            assert t_world[0] < 0 and abs(t_world[1]) < 1e-3 * abs(t_world[0])       # against the motion
            ft_sum += t_world[0]; fn_sum += f[0]
        a = hb.get("qacc")[0]
        assert m_box * a[0] == pytest.approx(m_box * gx + ft_sum, rel=1e-3)
        assert m_box * a[2] == pytest.approx(m_box * gz + fn_sum, rel=1e-3, abs=1e-3)


def test_actuator_models_and_clamps():
    """fwd_actuation as documented (XML reference: actuator/motor, position, velocity, general, ctrlrange, forcerange, gear): force = gain x clamp(ctrl) + bias .
    [1, length, velocity], clamped to forcerange, times the gear on the joint -- one joint per actuator (K.actuator_xml: motor, three position servos, a
    velocity servo and an affine general actuator with gear 2, the last two at non-zero qvel), forward() accelerations against I^-1 x the expected force."""
    flat, hb = _batch(K.actuator_xml())
    hb.set("qpos", np.array([K.ACT_Q])); hb.set("qvel", np.array([K.ACT_QVEL])); hb.set("ctrl", np.array([K.ACT_CTRL]))
    hb.forward()
    M = hb.get("qM")[0].reshape(6, 6)
    inertia, mass = float(M[0, 0]), float(M[3, 3])
    assert inertia == pytest.approx(K.ACT_INERTIA, rel=1e-5) and mass == pytest.approx(K.ACT_MASS, rel=1e-6)
    assert np.diag(M)[4:] == pytest.approx([K.ACT_INERTIA] * 2, rel=1e-5)
    frc = K.actuator_forces()
    assert hb.get("qacc")[0] == pytest.approx(frc / np.array([inertia, inertia, inertia, mass, inertia, inertia]), rel=2e-5)
    assert hb.get("qfrc_actuator")[0] == pytest.approx(frc, rel=2e-5)


def test_planar_two_link_arm_has_the_textbook_mass_matrix_and_bias():
    """The kernel's CRBA (incidence-matrix MFMAs) and RNE against the closed-form dynamics of the planar elbow manipulator, eight random states in one batch."""
    from tests.test_oracle import planar_2r_closed_form, planar_2r_xml
    flat = mjcf.compile_mjcf(planar_2r_xml())
    hm, hb = make_hip(flat, None, B=8)
    rng = np.random.default_rng(0)
    q, qd = rng.uniform(-2, 2, (8, 2)), rng.uniform(-3, 3, (8, 2))
    hb.set("qpos", q); hb.set("qvel", qd); hb.set("ctrl", 0.0); hb.set("qacc_warmstart", 0.0)
    hb.forward()
    for e in range(8):
        M, bias = planar_2r_closed_form(q[e], qd[e])
        assert hb.get("qM")[e].reshape(2, 2) == pytest.approx(M, rel=2e-6, abs=1e-7)
        assert hb.get("qfrc_bias")[e] == pytest.approx(bias, rel=1e-5, abs=2e-6)
        assert hb.get("qacc")[e] == pytest.approx(np.linalg.solve(M, -bias), rel=2e-5, abs=1e-4)


def test_narrow_phase_against_elementary_geometry():
    """The kernel's plane-box, plane-convex, box-box and MPR paths on the geometry cases of tests/test_oracle.py: depths, midpoints and normals of the contacts
    in fp32 (support points relative to the first geom keep MPR's rounding at ~1e-8 m)."""
    from tests.test_oracle import check_narrow_phase, narrow_phase_cases, narrow_phase_scene
    for name, bodies, expected in narrow_phase_cases():
        flat, hb = _batch(narrow_phase_scene(bodies))
        hb.forward()
        mpr = "sphere" in name and "plane" not in name or "capsule" in name
        # MPR stops when the portal is within 1e-6 m of the surface of the Minkowski difference: on curved shapes that leaves the normal free by about
        # sqrt(2 tol / r) ~ 6e-3 rad (measured 4e-3 on the two spheres; the fp64 oracle happens to start on the centre line and is exact) and the
        # point by r times that; depths are good to the tolerance itself
        check_narrow_phase(hb.contacts(0), expected, 3e-6, 1e-3 if mpr else 5e-6, 2e-2 if mpr else 1e-5, name)


def test_contact_conventions_on_the_kernel():
    """Contact COUNT and PLACEMENT per pair type on the canonical poses of tests/test_contact_conventions.py (what MuJoCo documents per pair and where this project's
    narrow phase deviates is written there): plane-box corners, one contact for plane-convex, the clipped-face manifold of box-box up to its eight vertices, one
    contact inside the patch for the MPR pairs -- the kernel's answers in fp32."""
    from tests.test_contact_conventions import check_conventions, convention_cases
    from tests.test_oracle import narrow_phase_scene
    for name, bodies, expected in convention_cases():
        flat, hb = _batch(narrow_phase_scene(bodies))
        hb.forward()
        mpr = "MPR" in name
        check_conventions(hb.contacts(0), expected, 3e-6, 5e-6, 2e-3 if mpr else 1e-5, name)


def test_mesh_narrow_phase_against_elementary_geometry(tmp_path):
    """The kernel's plane-hull and MPR-on-hull paths (hull vertices in registers, support scans as wave arg-max, coordinates relative to the first geom) on the
    mesh cases of tests/test_oracle.py: a hull vertex in the plane and in a box face, a hull flat on a box, two hulls edge on edge, a 64-gon prism, a geodesic
    sphere of 642 vertices (scanned from global memory: more than 256), a sphere primitive on a hull.  One contact per convex pair; depth, normal and -- where
    the geometry determines it -- the point, in fp32."""
    from tests.test_oracle import check_mesh_contacts, check_mesh_patch, mesh_narrow_phase_cases, mesh_scene
    for name, bodies, expected, tol in mesh_narrow_phase_cases(tmp_path):
        flat, hb = _batch(mesh_scene(str(tmp_path), bodies))
        hb.forward()
        cs = hb.contacts(0)
        # fp32: depths to 3e-6 m (MPR's own tolerance is 1e-6), points of vertex / edge contacts to 1e-4 m, normals to 2e-3
        check_mesh_contacts(cs, expected, (max(tol[0], 3e-6), None if tol[1] is None else max(tol[1], 2e-4), max(tol[2], 2e-3)), name)
        check_mesh_patch(cs, bodies, name, tol=2e-5)


# ---- terms that no fixture or generated model moves (tests/known_answer_cases.py; the fp64 oracle is held to the same cases in tests/test_known_answers_host.py) --------
# Worst |got - want| / max |want| of one MI355X run per fluid case against the closed form (profiles/known_answers_parity.txt); each test holds four times its
# figure (one box, one run, pose-dependent rounding), which must stay below the 1e-4 every parity test holds qfrc_passive to.
FLUID_MEASURED = {"free_box_qfrc": 3.483e-7, "free_box_qacc": 7.574e-7, "density_qfrc": 3.944e-7, "density_qacc": 8.344e-7, "viscosity_qfrc": 2.179e-7, "viscosity_qacc": 1.708e-7,
                  "wind_at_rest_qfrc": 2.996e-7, "wind_at_rest_qacc": 2.104e-7, "chain_qfrc": 9.901e-7, "per_env_qfrc": 2.631e-7, "per_env_qacc": 4.040e-7,
                  "cfg0_top_qfrc": 1.828e-7, "cfg4_top_qfrc": 2.484e-7}     # *_qacc: the linear part, the acceleration of the body origin


def _hold_fluid(name, got, want):
    """Worst over the batch of |got - want| / max |want| per env, printed beside its bound, then held."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    worst = float((np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)).max())
    bound = 4 * FLUID_MEASURED[name]
    print(f"known-answer fluid {name}: measured {worst:.3e} bound {bound:.3e} (largest reference entry {np.abs(want).max():.3g})")
    assert bound <= 1e-4 and worst <= bound, (name, worst, bound)


def _hold_free_box(name, hb, qpos, ref):
    """qfrc_passive and the linear qacc (the acceleration of the body origin) at their measured bounds.  The angular qacc comes out of an fp32 solve with a mass
    matrix that mixes 0.27 kg with 2e-4 kg m^2 (condition number 1500, computed from the closed form), so it is held to the textbook forward error of that
    solve, n u cond(M) = 6 x 2^-24 x 1500 = 5e-4 of the solution's largest entry -- loose for a fluid term, tight for a wrong gyroscopic or lever-arm term."""
    qacc = hb.get("qacc")
    _hold_fluid(name + "_qfrc", hb.get("qfrc_passive"), [r[0] for r in ref])
    _hold_fluid(name + "_qacc", qacc[:, :3], [r[1][:3] for r in ref])
    bound = min(6 * 2.0 ** -24 * np.linalg.cond(K.free_box_mass_matrix(q)) for q in qpos)
    worst = max(np.abs(qacc[e, 3:] - r[1][3:]).max() / np.abs(r[1]).max() for e, r in enumerate(ref))     # a body at rest has no angular acceleration
    print(f"known-answer fluid {name}_qacc angular: measured {worst:.3e} bound {bound:.3e}")
    assert worst <= bound, (name, worst, bound)


def _states(xml, qpos, qvel, per_env=False):
    flat = mjcf.compile_mjcf(xml)
    hm, hb = make_hip(flat, None, B=len(qpos), per_env=per_env)
    hb.set("qpos", qpos); hb.set("qvel", qvel); hb.set("ctrl", 0.0); hb.set("qacc_warmstart", 0.0)
    return flat, hb


@pytest.mark.parametrize("name,rho,mu,wind,rest", (("free_box", K.RHO, K.MU, K.WIND, False), ("density", K.RHO, 0.0, (0, 0, 0), False), ("viscosity", 0.0, K.MU, (0, 0, 0), False),
                                                   ("wind_at_rest", K.RHO, K.MU, K.WIND, True)), ids=("free_box", "density", "viscosity", "wind_at_rest"))
def test_fluid_forces_on_a_free_box_follow_the_documented_inertia_model(name, rho, mu, wind, rest):
    """The inertia-box fluid model in a water-like medium with wind (forces of up to 0.7 N on a weight of 2.6 N), on a free box whose geom is offset and rotated
    inside its body: eight seeded poses and 6-velocities in one batch, qfrc_passive and qacc (origin acceleration of a spinning body: Newton at the COM, Euler
    about it, shifted to the origin) against the closed form; then density alone, viscosity alone, and wind on a body at rest."""
    qpos, qvel = K.free_box_states(rest=rest)
    flat, hb = _states(K.free_box_xml(rho, mu, wind), qpos, qvel)
    hb.forward()
    _hold_free_box(name, hb, qpos, [K.free_box_reference(q, v, rho, mu, wind) for q, v in zip(qpos, qvel)])


def test_fluid_forces_on_a_hinge_hinge_slide_chain():
    """Three offset, rotated boxes behind tilted joint axes with non-zero anchors: qfrc_passive against the closed-form wrenches at velocities from central
    differences of an fp64 FK, projected on the joints by central differences of the same FK -- no cdof / cvel of any implementation in the reference."""
    q, qd = K.chain_states()
    flat, hb = _states(K.chain_xml(), q, qd)
    hb.forward()
    _hold_fluid("chain_qfrc", hb.get("qfrc_passive"), [K.chain_reference(a, b) for a, b in zip(q, qd)])


def test_fluid_medium_per_env():
    """The per-env option table the randomisation kernel writes: four envs, each with its own density, viscosity and wind, each against its own closed form."""
    qpos, qvel = K.free_box_states(4)
    flat, hb = _states(K.free_box_xml(), qpos, qvel, per_env=True)
    media = K.per_env_media()
    for e, (rho, mu, wind) in enumerate(media):
        hb.param_set("opt", np.concatenate([[H], [0, 0, -G0], [rho, mu, 1.0], wind]), env0=e)
    hb.forward()
    ref = [K.free_box_reference(q, v, *md) for q, v, md in zip(qpos, qvel, media)]
    assert np.abs(ref[0][0] - ref[1][0]).max() > 0.05          # the media differ by far more than any tolerance
    _hold_free_box("per_env", hb, qpos, ref)


@pytest.mark.parametrize("name", ("cfg0_top", "cfg4_top"))
def test_fluid_forces_through_both_force_propagation_paths(name):
    """The smallest and the largest kernel configuration propagate body forces to the joints differently (subtree bit masks / incidence-matrix products): the
    capacity models at their top dof edge in water with wind, qfrc_passive against the fp64 oracle relative to its largest entry.  The one oracle comparison
    among these tests; the oracle's fluid block is held to the closed forms above in tests/test_known_answers_host.py."""
    from tests import capacity_models
    from tests.util import make_oracle
    cfg, flat = capacity_models.build(name)
    flat.arrays["density"][0] = K.RHO; flat.arrays["viscosity"][0] = K.MU; flat.arrays["wind"][:] = K.WIND
    q, v = capacity_models.start_state(flat, 1)
    om, od, _ = make_oracle(flat)
    od.qpos[:] = q; od.qvel[:] = v; od.forward()
    want = np.array(od.qfrc_passive)
    hm, hb = make_hip(flat, None, B=1)
    assert hm.kernel_config()[0] == cfg
    hb.set("qpos", q[None]); hb.set("qvel", v[None]); hb.set("ctrl", 0.0); hb.set("qacc_warmstart", 0.0)
    hb.forward()
    _hold_fluid(name + "_qfrc", hb.get("qfrc_passive"), want[None])


def _settled(hb, n, ctrl=None):
    if ctrl is not None:
        hb.set("ctrl", np.array([[ctrl]]))
    for _ in range(n):
        hb.step()
    hb.forward()
    assert np.abs(hb.get("qvel")[0]).max() < 1e-4


@pytest.mark.parametrize("gap", (0.0, K.GAP))
def test_ball_rests_above_the_plane_inside_the_margin(gap):
    """Margin 2 mm on both geoms: the ball rests ABOVE the plane, the violation (margin - gap) - dist being the documented resting violation r; one contact,
    its normal force the weight."""
    mg = f'{K.sol_attrs()} margin="{K.MARGIN}" gap="{gap}"'
    flat, hb = _batch(K.ball_plane_xml(mg, mg))
    _settled(hb, K.SETTLE["margin_ball"])
    r = _depth(G0, K.SOLREF, K.SOLIMP)
    z = float(hb.get("qpos")[0][2])
    assert hb.get("ncon")[0] == 1 and hb.get("nefc")[0] == 3 and z - K.BALL_R > 1e-3
    assert (K.MARGIN - gap) - (z - K.BALL_R) == pytest.approx(r, rel=2e-3, abs=2e-7)
    c = hb.contacts(0)[0]
    assert (K.MARGIN - gap) - c["dist"] == pytest.approx(r, rel=2e-3, abs=2e-7)
    assert c["normal_force"] == pytest.approx(K.BALL_MASS * G0, rel=1e-3)


class _HipState:
    def __init__(self, xml):
        self.flat, self.hb = _batch(xml)

    def forward(self):
        self.hb.forward()

    def contacts(self):
        return self.hb.contacts(0)

    nefc = property(lambda self: int(self.hb.get("nefc")[0]))
    qacc = property(lambda self: self.hb.get("qacc")[0])


@pytest.mark.parametrize("pair", ("plane_box", "box_box"))
def test_contact_and_row_creation_inside_margin_and_gap(pair):
    """A box over the plane and over a fixed box (face to face), margin 2 mm and gap 0.5 mm, at separations of 2.1, 1.75, 1.0 and -0.1 mm: no contact; contacts
    listed without rows (efc_address -1, nefc 0, qacc = g); rows active with positive normal forces (the kernel activates a row at dist < margin - gap - 1e-7);
    every reported dist is the constructed one; contact counts as MuJoCo documents them (at most 4 / 8) and exactly the oracle's."""
    from tests.test_known_answers_host import check_margin_states, oracle_margin_counts
    xml_of, most = (K.box_over_plane_xml, 4) if pair == "plane_box" else (K.box_over_box_xml, 8)
    assert check_margin_states(_HipState, xml_of, most) == oracle_margin_counts(xml_of, most)


def test_hinge_and_tendon_limits_rest_inside_their_margin():
    """The limit pendulum with a margin of 0.05 rad on its joint rests INSIDE the range with the row active, at q - hi = r - margin; its twin under a limited
    fixed tendon of length 2 q (the lim_only pattern of tests/golden/coupled_fingers.xml, with a margin) rests at len - hi = r - margin, r the documented
    resting violation for the constraint-space acceleration coef tau / I."""
    flat, hb = _batch(K.limit_pendulum_xml())
    hb.set("qpos", np.array([[0.2]]))
    _settled(hb, K.SETTLE["limit_pendulum"], K.LIMIT_TORQUE)
    assert float(hb.get("qM")[0].ravel()[0]) == pytest.approx(K.PENDULUM_INERTIA, rel=1e-5) and hb.get("nefc")[0] == 1
    q = float(hb.get("qpos")[0][0])
    assert q < K.LIMIT_HI
    assert q - K.LIMIT_HI + K.LIMIT_MARGIN == pytest.approx(_depth(K.LIMIT_TORQUE / K.PENDULUM_INERTIA, K.SOLREF, K.SOLIMP), rel=2e-3, abs=2e-7)
    flat, hb = _batch(K.tendon_limit_xml())
    hb.set("qpos", np.array([[0.1]]))
    _settled(hb, K.SETTLE["limit_tendon"], K.LIMIT_TORQUE)
    q = float(hb.get("qpos")[0][0])
    assert hb.get("nefc")[0] == 1 and K.TENDON_COEF * q < K.LIMIT_HI
    assert K.TENDON_COEF * q - K.LIMIT_HI + K.LIMIT_MARGIN == pytest.approx(_depth(K.TENDON_COEF * K.LIMIT_TORQUE / K.PENDULUM_INERTIA, K.SOLREF, K.SOLIMP), rel=2e-3, abs=2e-7)


@pytest.mark.parametrize("row", K.MIX_ROWS, ids=lambda r: "solmix_%g_%g_priority_%d_%d" % r)
def test_resting_depth_of_the_documented_parameter_mix(row):
    """Plane and ball carry different solref / solimp: the ball's resting depth is the documented one of the MIXED parameters (the higher priority's; at equal
    priority the solmix-weighted average, weights below 1e-15 counting as zero) -- depths from 0.022 to 0.37 mm over the six rows."""
    flat, hb = _batch(K.mix_xml(row))
    _settled(hb, K.SETTLE["mix"])
    assert hb.get("ncon")[0] == 1
    assert K.BALL_R - float(hb.get("qpos")[0][2]) == pytest.approx(_depth(G0, *K.documented_mix(row)), rel=2e-3, abs=2e-7)
    assert hb.contacts(0)[0]["normal_force"] == pytest.approx(K.BALL_MASS * G0, rel=1e-3)


@pytest.mark.parametrize("row,mu", K.FRICTION_ROWS, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else None)
def test_sliding_friction_is_the_larger_one_or_the_higher_priority(row, mu):
    """The flat box of the Coulomb test with sliding friction 0.2 / 0.5 at equal priority, with the 0.2 geom at higher priority, and 0.6 / 0.3 with the 0.3 geom
    at higher priority: settled, then given 0.5 m/s, every corner contact slips with |f_t| / f_n = 0.5, 0.2, 0.3."""
    from tests.test_known_answers_host import check_friction_mix
    flat, hb = _batch(K.friction_xml(row))
    _settled(hb, K.SETTLE["friction"])
    v = np.zeros((1, 6)); v[0, 0] = 0.5
    hb.set("qvel", v); hb.forward()
    check_friction_mix(hb.contacts(0), hb.get("efc_force")[0], mu, 1e-4)


@pytest.mark.parametrize("row,dim", K.CONDIM_ROWS, ids=lambda v: "condim_%d_%d_priority_%d" % v if isinstance(v, tuple) else None)
def test_frictionless_contact_lets_the_ball_slide_freely(row, dim):
    """Gravity tilted by 0.3 rad; condim (1, 1), (1, 3) at equal priority (the larger wins), (1, 3) with the condim-1 geom at priority 1: contact dim and row
    count 1, 3, 1; the normal force is m g cos(theta); a frictionless contact leaves the tangential velocity to the Euler recursion g sin(theta) h n, with
    friction the ball is strictly slower."""
    flat, hb = _batch(K.condim_xml(row))
    n = K.SETTLE["condim"]
    for _ in range(n):
        hb.step()
    hb.forward()
    free = G0 * np.sin(K.THETA) * H * n
    c, v = hb.contacts(0), hb.get("qvel")[0]
    assert len(c) == 1 and c[0]["dim"] == dim and hb.get("nefc")[0] == dim
    assert abs(v[2]) < 1e-4
    assert c[0]["normal_force"] == pytest.approx(K.BALL_MASS * G0 * np.cos(K.THETA), rel=1e-3)
    if dim == 1:
        assert v[0] == pytest.approx(free, rel=1e-5)
    else:
        assert v[0] < free * (1 - 1e-3)
