"""Sensors beyond force / torque on the MI355X (csrc/rsim_sensors.hip): the kernel against its fp64 host mirror (robosuite_amd/sensors.py, itself held to
closed forms in tests/test_sensors_host.py), known answers on the kernel alone, the stages of step1 / step2, per-env model tables, the 64-sensor edge and
the batched accessors.  Every value test here fails on a build without the kernel: the entries read zero there.

Parity bounds (profiles/sensors_parity.txt): per stage, the worst |kernel - mirror| relative to max(|mirror|, stage scale) over every env and entry of the
two scenes below was measured on the MI355X; the bound is three times that measurement.  The mirror is fed the batch's own qpos / qvel / qacc / ctrl /
contacts, so only sensor arithmetic (fp32 kinematics against fp64) is compared.  Stage scales: 1 (m, unit quaternions, rad), 1 (m/s, rad/s), 9.81 (m/s^2, N).

The acceleration stage includes the accelerometer on a free body that spins while it translates (`s_acc_box` in the envs where the box tumbles): the entry
whose cdof_dot terms must cancel the frame's own w x v."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
from robosuite_amd import mjcf, sensors  # noqa: E402
from tests import sensors_scenes as S  # noqa: E402
from tests.util import load_golden, make_hip  # noqa: E402

G = 9.81
SCALE = {"pos": 1.0, "vel": 1.0, "acc": G}
# measured on the MI355X (profiles/sensors_parity.txt), worst over the two scenes and the states of the stage test: pos 8.33e-08, vel 3.56e-07, acc 4.75e-07 -> x 3
BOUND = {"pos": 2.5e-7, "vel": 1.07e-6, "acc": 1.43e-6}


def _stage(code):
    return "pos" if code <= 5 else ("vel" if code <= 11 else "acc")


def _layout(flat):
    adr = np.concatenate([[0], np.cumsum(np.asarray(flat.arrays["sensor_dim"]).ravel())]).astype(int)
    sl = {n: slice(adr[i], adr[i + 1]) for i, n in enumerate(flat.names["sensor"])}
    stage = {n: _stage(int(t)) for n, t in zip(flat.names["sensor"], flat.sensor_type) if int(t) >= 2}
    return sl, stage


def _mirror(flat, hb, env, qpos=None, qvel=None, ctrl=None):
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    return sensors.sensor_values(flat, f64(hb.get("qpos")[env] if qpos is None else qpos), f64(hb.get("qvel")[env] if qvel is None else qvel), f64(hb.get("qacc")[env]),
                                 f64(hb.get("ctrl")[env] if ctrl is None else ctrl), hb.contacts(env))


def _errors(flat, got, want, only=None):
    """worst error per stage, relative to max(|reference|, stage scale)"""
    sl, stage = _layout(flat)
    worst = {}
    for n, st in stage.items():
        if only and st not in only:
            continue
        e = np.abs(got[sl[n]] - want[sl[n]]) / np.maximum(np.abs(want[sl[n]]), SCALE[st])
        worst[st] = max(worst.get(st, 0.0), float(e.max()))
    return worst


def _unit(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def arm_states(flat, B, seed=11, resting=(1, 4, 7)):
    """B different states of the arm2_box scene; in the `resting` envs the box lies on the floor (yawed, pressed 0.4 mm in), elsewhere it tumbles in the air"""
    rng = np.random.default_rng(seed)
    nq, nv = int(flat.nq), int(flat.nv)
    qpos, qvel, ctrl = np.zeros((B, nq)), np.zeros((B, nv)), np.zeros((B, int(flat.nu)))
    for e in range(B):
        qpos[e, :3] = [rng.uniform(-2, 2), rng.uniform(-1, 0.6), rng.uniform(0, 0.1)]
        if e in resting:
            yaw = rng.uniform(-3, 3)
            qpos[e, 3:10] = [rng.uniform(-0.3, 0.3), rng.uniform(0.6, 0.9), 0.0496, np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]
        else:
            qpos[e, 3:10] = np.concatenate([[rng.uniform(-0.3, 0.3), rng.uniform(0.6, 0.9), rng.uniform(0.3, 0.6)], _unit(rng)])
            qvel[e, 3:9] = rng.uniform(-2, 2, 6)
        qpos[e, 10:17] = np.concatenate([[-0.6, -0.5, rng.uniform(0.3, 0.5)], _unit(rng)])
        qvel[e, :3] = rng.uniform(-2, 2, 3)
        qvel[e, 9:15] = rng.uniform(-1, 1, 6)
        ctrl[e] = [rng.uniform(-25, 25), rng.uniform(-20, 20), rng.uniform(-0.05, 0.15)]
    return qpos, qvel, ctrl


def _set_state(hb, qpos, qvel, ctrl):
    hb.set("qpos", qpos); hb.set("qvel", qvel); hb.set("ctrl", ctrl); hb.set("qacc_warmstart", 0.0)


@pytest.fixture(scope="module")
def arm():
    flat = mjcf.compile_mjcf(S.ARM_XML)
    hm, hb = make_hip(flat, None, B=9)
    return flat, hm, hb


# ---- 1. kernel = mirror ---------------------------------------------------------------------------------------------------------------------------
def test_kernel_equals_mirror_on_the_arm_scene(arm):
    flat, hm, hb = arm
    sl, _ = _layout(flat)
    _set_state(hb, *arm_states(flat, 9))
    hb.forward()
    sd = hb.get("sensordata").astype(np.float64)
    worst, touched = {}, 0
    for e in range(9):
        want = _mirror(flat, hb, e)
        for k, v in _errors(flat, sd[e], want).items():
            worst[k] = max(worst.get(k, 0.0), v)
        for n in ("s_acc", "s_acc_box", "s_touch", "s_af", "s_af1"):
            print(f"  env {e} {n:10s} kernel {np.round(sd[e][sl[n]], 5)} mirror {np.round(want[sl[n]], 5)}")
        touched += want[sl["s_touch"]][0] > 1.0
        assert want[sl["s_touch_far"]][0] == 0.0 == sd[e][sl["s_touch_far"]][0]
        assert np.abs(sd[e][sl["s_force"]]).max() > 0          # force / torque are still there beside the new entries
    print("sensors parity arm2_box B=9:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert touched == 3                                         # the three resting boxes press on the pad (two of the four corner contacts lie in it)
    assert not np.array_equal(sd[0], sd[1]) and np.abs(sd).max() > 1
    for k in ("pos", "vel", "acc"):
        assert worst[k] <= BOUND[k], (k, worst)


def test_kernel_equals_mirror_on_the_tendon_scene():
    flat = mjcf.compile_mjcf(S.FINGERS_XML)
    hm, hb = make_hip(flat, None, B=3)
    rng = np.random.default_rng(3)
    _set_state(hb, rng.uniform(-0.15, 0.6, (3, 3)), rng.uniform(-2, 2, (3, 3)), rng.uniform(0, 1, (3, 2)))
    hb.forward()
    sd = hb.get("sensordata").astype(np.float64)
    worst = {}
    for e in range(3):
        for k, v in _errors(flat, sd[e], _mirror(flat, hb, e)).items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("sensors parity coupled_fingers B=3:", {k: f"{v:.2e}" for k, v in worst.items()})
    sl, _ = _layout(flat)
    assert np.abs(sd[:, sl["t_pos"]]).min() > 1e-3 and np.abs(sd[:, sl["t_vel"]]).min() > 1e-3
    for k in ("pos", "vel", "acc"):
        assert worst[k] <= BOUND[k], (k, worst)


# ---- 2. known answers on the kernel itself --------------------------------------------------------------------------------------------------------
def _b1(xml):
    flat = mjcf.compile_mjcf(xml)
    hm, hb = make_hip(flat, None, B=1)
    hb.set("qpos", np.asarray(flat.qpos0, dtype=np.float64)[None]); hb.set("qvel", 0.0); hb.set("ctrl", 0.0); hb.set("qacc_warmstart", 0.0)
    return flat, hm, hb


BALL = """<mujoco><option timestep="0.002" cone="elliptic"/><worldbody><geom name="floor" type="plane" size="1 1 0.1"/>
    <body name="ball" pos="0 0 %g"><freejoint/><geom name="ball" type="sphere" size="0.05" density="1000"/><site name="imu" pos="0.01 0.02 0"/>
    <site name="sole" type="box" size="0.02 0.02 0.02" pos="0 0 -0.05"/></body></worldbody>
    <sensor><accelerometer name="acc" site="imu"/><touch name="touch" site="sole"/></sensor></mujoco>"""


def test_free_fall_reads_zero_and_rest_reads_g_and_the_weight():
    flat, hm, hb = _b1(BALL % 1.0)
    hb.set("qvel", np.array([[0.3, -0.2, 0.5, 0, 0, 0]]))
    hb.forward()
    hb.sync()
    # |qacc - g| in fp32: a few roundings of 9.81 (6e-7 each) -> 1e-4 m/s^2 is more than ten of them
    assert np.abs(hb.sensor("acc").cpu().numpy()).max() < 1e-4 and hb.get("qacc")[0][2] == pytest.approx(-G, rel=1e-6)
    assert hb.sensor("touch").cpu().numpy()[0, 0] == 0.0
    flat, hm, hb = _b1(BALL % 0.05)
    for _ in range(3000):          # the resting-depth scene of tests/test_hip_known_answers.py
        hb.step()
    hb.forward()
    hb.sync()
    assert np.abs(hb.get("qvel")[0]).max() < 1e-4 and hb.get("ncon")[0] == 1
    R = mjcf.quat2mat(hb.get("qpos")[0][3:7].astype(np.float64))
    acc = R @ hb.sensor("acc").cpu().numpy()[0].astype(np.float64)
    assert acc[2] == pytest.approx(G, rel=1e-3) and np.abs(acc[:2]).max() < 1e-3 * G
    assert hb.sensor("touch").cpu().numpy()[0, 0] == pytest.approx(1000 * 4 / 3 * np.pi * 0.05**3 * G, rel=1e-3)


def test_pendulum_gyro_is_rate_times_axis():
    axis = np.array([1.0, 2.0, 2.0]) / 3.0
    flat, hm, hb = _b1("""<mujoco><compiler angle="radian"/><worldbody><body name="p" pos="0 0 1"><joint name="h" type="hinge" axis="1 2 2"/>
        <geom type="sphere" size="0.02" pos="0.2 0 0" mass="0.5"/><site name="tip" pos="0.2 0 0"/></body></worldbody><sensor><gyro name="gy" site="tip"/></sensor></mujoco>""")
    hb.set("qpos", np.array([[0.9]])); hb.set("qvel", np.array([[-1.7]]))
    hb.forward()
    hb.sync()
    assert np.abs(hb.sensor("gy").cpu().numpy()[0] - (-1.7) * axis).max() < 1e-5 * 1.7        # the axis is fixed in the site frame; fp32 rotation there and back


# ---- 3. stages ------------------------------------------------------------------------------------------------------------------------------------
def test_step1_refreshes_position_and_velocity_and_step2_all(arm):
    flat, hm, hb = arm
    sl, stage = _layout(flat)
    qa, va, ca = arm_states(flat, 9, seed=21)
    qb, vb, cb = arm_states(flat, 9, seed=22)
    _set_state(hb, qa, va, ca)
    hb.forward()
    sd_a = hb.get("sensordata")
    _set_state(hb, qb, vb, cb)
    hb.step1()
    sd_1 = hb.get("sensordata")
    q32, v32, c32 = hb.get("qpos"), hb.get("qvel"), hb.get("ctrl")
    acc_names = [n for n in flat.names["sensor"] if stage.get(n, "acc") == "acc"]      # force / torque included
    for n in acc_names:
        assert np.array_equal(sd_1[:, sl[n]], sd_a[:, sl[n]]), n                       # acceleration stage: still the previous values, bit for bit
    for e in range(9):
        want = _mirror(flat, hb, e)
        w = _errors(flat, sd_1[e].astype(np.float64), want, only=("pos", "vel"))
        print(f"sensors parity after step1, env {e}:", {k: f"{v:.2e}" for k, v in w.items()})
        assert w["pos"] <= BOUND["pos"] and w["vel"] <= BOUND["vel"], (e, w)
    assert np.abs(sd_1[:, sl["s_fp_site"]] - sd_a[:, sl["s_fp_site"]]).max() > 1e-2
    hb.step2()
    sd_2 = hb.get("sensordata").astype(np.float64)
    assert np.abs(hb.get("qpos") - q32).max() > 1e-4                                   # the state moved on ...
    for e in range(9):                                                                 # ... the sensors are those of the substep before its integration
        w = _errors(flat, sd_2[e], _mirror(flat, hb, e, qpos=q32[e], qvel=v32[e], ctrl=c32[e]))
        print(f"sensors parity after step2, env {e}:", {k: f"{v:.2e}" for k, v in w.items()})
        for k in ("pos", "vel", "acc"):
            assert w[k] <= BOUND[k], (e, w)
    assert np.abs(sd_2[:, sl["s_acc"]] - sd_a[:, sl["s_acc"]].astype(np.float64)).max() > 1e-2


# ---- 4. force / torque untouched ------------------------------------------------------------------------------------------------------------------------
def test_force_and_torque_are_bitwise_what_they_were(arm):
    flat, hm, hb = arm
    plain = mjcf.compile_mjcf(S.ARM_FT_PAD)
    _, hp = make_hip(plain, None, B=9)
    state = arm_states(flat, 9, seed=31)
    _set_state(hb, *state); _set_state(hp, *state)
    hb.forward(); hp.forward()
    sl, _ = _layout(flat)
    a, b = hb.get("sensordata"), hp.get("sensordata")
    assert np.array_equal(a[:, sl["s_force"]], b[:, 0:3]) and np.array_equal(a[:, sl["s_torque"]], b[:, 3:6])
    assert np.abs(b).max() > 0.1
    for k in ("qacc", "xpos", "efc_force"):
        assert np.array_equal(hb.get(k), hp.get(k)), k


# ---- 5. per-env tables ----------------------------------------------------------------------------------------------------------------------------
def test_frames_follow_the_envs_own_model_tables():
    flat = mjcf.compile_mjcf(S.ARM_XML)
    hm, hb = make_hip(flat, None, B=2, per_env=True)
    sl, _ = _layout(flat)
    q, v, c = arm_states(flat, 2, seed=41)
    q[1], v[1], c[1] = q[0], v[0], c[0]
    _set_state(hb, q, v, c)
    hb.forward()
    before = hb.get("sensordata")
    assert np.array_equal(before[0], before[1])
    link3 = flat.names["body"].index("link3")
    bp = hb.param_get("body_pos", 1, 1)
    bp[0, link3] += [0.04, -0.03, 0.02]
    hb.param_set("body_pos", bp, env0=1)
    hb.forward()
    after = hb.get("sensordata")
    assert np.array_equal(after[0][sl["s_fp_xbody"]], before[0][sl["s_fp_xbody"]]) and np.array_equal(after[0][sl["s_fp_site"]], before[0][sl["s_fp_site"]])
    moved = flat.copy()
    moved.arrays["body_pos"][link3] += [0.04, -0.03, 0.02]
    want = _mirror(moved, hb, 1)
    assert np.abs(after[1][sl["s_fp_xbody"]] - before[1][sl["s_fp_xbody"]]).max() > 0.02
    for n in ("s_fp_xbody", "s_fp_site", "s_fp_body"):
        assert np.abs(after[1][sl[n]] - want[sl[n]]).max() <= BOUND["pos"], n


# ---- 6. edges -------------------------------------------------------------------------------------------------------------------------------------
def test_sixty_four_sensors_and_a_model_that_carries_none():
    block = "".join(f'<jointpos name="p{i}" joint="{"ab"[i % 2]}"/>' for i in range(64))
    flat, hm, hb = _b1(f"""<mujoco><compiler angle="radian"/><worldbody><body pos="0 0 1"><joint name="a" type="hinge" axis="0 1 0"/><geom type="sphere" size="0.05"/>
        <body pos="0 0 -0.2"><joint name="b" type="slide" axis="1 0 0"/><geom type="sphere" size="0.05"/></body></body></worldbody><sensor>{block}</sensor></mujoco>""")
    assert hm.int("nsensordata") == 64 and hm.sensor_slice("p63") == (63, 1, True)
    hb.set("qpos", np.array([[0.25, -0.125]]))
    hb.forward()
    assert np.array_equal(hb.get("sensordata")[0], np.tile(np.float32([0.25, -0.125]), 32))
    flat, hm, hb = _b1(S.ONLY_ZERO_XML)
    assert hm.int("nsensor_zero") == hm.int("nsensor") == 3
    hb.set("qpos", np.array([[0.4]])); hb.set("qvel", np.array([[1.5]]))
    hb.forward()
    assert hb.get("sensordata").shape == (1, 5) and not hb.get("sensordata").any()


# ---- 7. batched use -------------------------------------------------------------------------------------------------------------------------------
def _lift_with_sensors(tag):
    g, cfg, flat = load_golden(tag)
    site, jnt = flat.names["site"].index("gripper0_right_grip_site"), int(cfg["qpos_idx"][3])
    j = int(np.flatnonzero(np.asarray(flat.jnt_qposadr) == jnt)[0])
    return cfg, S.add_sensors(flat, [("hand_gyro", "gyro", mjcf.SENSOR_OBJ_SITE, site, 3), ("elbow_pos", "jointpos", mjcf.SENSOR_OBJ_JOINT, j, 1),
                                     ("hand_acc", "accelerometer", mjcf.SENSOR_OBJ_SITE, site, 3)]), jnt


def test_batch_state_sensor_inside_a_host_controlled_step():
    from robosuite_amd import lift
    from robosuite_amd.controllers import HostControlledEnv
    from tests.test_controllers_plugin import _parts
    B = 4
    cfg, flat, jnt = _lift_with_sensors("ctl_joint_torque")
    task = lift.LiftBatch(flat, cfg, np.arange(B), seed0=4)
    st, parts = _parts(task, cfg, flat)
    seen = []
    run = parts[0].controller.run_controller

    def spy():
        gy, jp = st.sensor("hand_gyro"), st.sensor("elbow_pos")
        adr, dim, _ = task.model.sensor_slice("hand_gyro")
        seen.append((tuple(gy.shape), tuple(jp.shape), torch.equal(gy, task.batch.tensor("sensordata")[:, adr:adr + dim]), torch.equal(jp[:, 0], st.qpos[:, jnt]), gy.abs().max().item()))
        return run()

    parts[0].controller.run_controller = spy
    env = HostControlledEnv(task, parts, n_sub=5)
    env.step(torch.zeros(B, 8, device="cuda").uniform_(-1, 1))
    env.step(torch.zeros(B, 8, device="cuda").uniform_(-1, 1))
    assert len(seen) == 10 and all(s[:4] == ((B, 3), (B, 1), True, True) for s in seen)
    assert seen[-1][4] > 0.0                                   # the arm moves: the gyro at the hand reads it, per substep, between step1 and step2


def test_vec_env_sensor_after_a_fused_step_is_a_fresh_forward():
    from robosuite_amd.vec_env import VecEnv
    B = 4
    cfg, flat, jnt = _lift_with_sensors("seed1_full")
    env = VecEnv("Lift", B, flat, cfg, horizon=50, bank_episodes=2)
    env.reset()
    for _ in range(2):
        env.step(torch.zeros(B, env.action_dim, device="cuda").uniform_(-1, 1))
    got = {n: env.sensor(n).clone() for n in ("hand_gyro", "elbow_pos", "hand_acc")}
    assert tuple(got["hand_gyro"].shape) == (B, 3) and got["hand_gyro"].abs().max().item() > 1e-4
    b = env.env.batch
    b.forward(); b.sync()
    sd = b.get("sensordata")
    for n, t in got.items():
        adr, dim, _ = b.model.sensor_slice(n)
        if n == "hand_acc":      # the read's forward runs the narrow phase cold, forward() warm-started: the same contacts to the MPR tolerance, the same accelerations to ~1e-4
            assert np.abs(t.cpu().numpy() - sd[:, adr:adr + dim]).max() <= 1e-3 * G, n
        else:
            assert np.array_equal(t.cpu().numpy(), sd[:, adr:adr + dim]), n
    assert np.array_equal(got["elbow_pos"].cpu().numpy()[:, 0], b.get("qpos")[:, jnt])
    assert np.abs(got["hand_acc"].cpu().numpy()).max() > 1.0   # gravity at least
