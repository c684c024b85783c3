"""External forces in the fused control step (rsim_set_applied_forces): mjData.qfrc_applied and xfrc_applied, off by default, honoured by every body that
steps an env once enabled.  Closed forms (a hovering cube, a pure torque), the fp64 oracle driven with the same generalised forces, the force / torque
sensor, the capacity-tier hand-over, opt-in neutrality and the episode-restart semantics of mj_resetData."""
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from robosuite_amd import mjcf  # noqa: E402
from tests.test_applied_forces_host import xfrc_to_qfrc  # noqa: E402
from tests.util import load_golden, make_hip, make_oracle  # noqa: E402

ADIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robosuite_amd", "assets")


def _assets(task):
    name = {"lift": "lift_panda", "stack": "stack_panda"}[task]
    return mjcf.load_model(os.path.join(ADIR, name + ".rsim")), json.load(open(os.path.join(ADIR, name + ".cfg.json")))


def _hover_batch(B, enable):
    """Lift (golden model + controller), arm at the fixture's start, cube 0.2 m above the table at y = 0.3, away from the arm, at rest, unit quaternion."""
    g, cfg, flat = load_golden("seed1_full")
    nq, cube = flat.nq, flat.name2id("body", "cube_main")
    qa = int(flat.arrays["jnt_qposadr"][flat.arrays["body_jntadr"][cube]])
    q = g["states"][0][1:1 + nq].copy()
    q[qa:qa + 7] = [0.0, 0.3, 1.03, 1.0, 0.0, 0.0, 0.0]
    hm, hb = make_hip(flat, cfg, B=B)
    hb.set("qpos", q[None].repeat(B, 0)); hb.set("qvel", 0); hb.set("qacc_warmstart", 0); hb.set("ctrl", 0)
    hb.forward(); hb.ctrl_reset()
    hb.set_applied_forces(enable)
    return flat, hb, cube, qa, q


def _zero_actions(hb, B):
    return torch.zeros((B, hb.model.action_dim), dtype=torch.float32, device="cuda")


def test_xfrc_applied_holds_a_cube_against_gravity():
    """xfrc_applied[cube] = (0, 0, m g, 0, 0, 0): after one control step (25 substeps) the cube has not moved; without the switch it falls 1/2 g t^2."""
    B = 4
    for enable in (True, False):
        flat, hb, cube, qa, q0 = _hover_batch(B, enable)
        m, g = float(flat.arrays["body_mass"][cube]), -float(np.asarray(flat.arrays["gravity"]).ravel()[2])
        x = hb.tensor("xfrc_applied")
        x[:, cube, 2] = m * g
        hb.control_step(_zero_actions(hb, B), 25)
        qp, qv = hb.get("qpos")[:, qa:qa + 7], hb.get("qvel")[:, 9:15]
        t = 25 * float(flat.arrays["timestep"][0])
        if enable:
            assert np.abs(qp - q0[qa:qa + 7]).max() < 2e-6 and np.abs(qv).max() < 2e-5, (qp[0], qv[0])
        else:
            drop = q0[qa + 2] - qp[:, 2]
            # semi-implicit Euler: the position uses the velocity of the end of each substep, 1/2 g t^2 (1 + 1/n)
            np.testing.assert_allclose(drop, 0.5 * g * t * t * (1 + 1 / 25), rtol=1e-3)
            assert drop.min() > 0.01
        assert np.array_equal(hb.get("qpos")[0], hb.get("qpos")[B - 1])


def test_pure_torque_spins_the_hovering_cube():
    """A torque on the hovering cube: omega after one control step ~ I^-1 tau t (unit quaternion: body frame = world frame, free-joint angular dofs are
    body-frame).  Second-order (gyroscopic) terms are below 1e-3 of it for this torque."""
    B = 2
    flat, hb, cube, qa, q0 = _hover_batch(B, True)
    m, g = float(flat.arrays["body_mass"][cube]), -float(np.asarray(flat.arrays["gravity"]).ravel()[2])
    tau = np.array([2e-5, -1e-5, 3e-5])
    w = np.zeros(6); w[2] = m * g; w[3:] = tau
    hb.tensor("xfrc_applied")[:, cube] = torch.tensor(w, dtype=torch.float32, device="cuda")
    hb.control_step(_zero_actions(hb, B), 25)
    t = 25 * float(flat.arrays["timestep"][0])
    I = np.asarray(flat.arrays["body_inertia"]).reshape(-1, 3)[cube]
    iq = np.asarray(flat.arrays["body_iquat"]).reshape(-1, 4)[cube]
    R = mjcf.quat2mat(iq)
    want = R @ ((R.T @ tau) / I) * t
    om = hb.get("qvel")[0, 9 + 3:9 + 6]
    np.testing.assert_allclose(om, want, rtol=5e-3, atol=1e-6 * np.abs(want).max())


def _oracle_parity(qfrc_fn, xfrc_fn, steps=3):
    """Lift golden fixture, B = 3 identical envs; the kernel with the switch on against the oracle driven substep by substep with the same generalised force."""
    g, cfg, flat = load_golden("seed1_full")
    nq, B = flat.nq, 3
    s0 = g["states"][0]
    om, od, oc = make_oracle(flat, cfg)
    hm, hb = make_hip(flat, cfg, B=B)
    od.qpos[:] = s0[1:1 + nq]; od.qvel[:] = s0[1 + nq:]; od.qacc_warmstart[:] = 0; od.forward(); oc.reset(od)
    hb.set("qpos", s0[1:1 + nq][None].repeat(B, 0)); hb.set("qvel", s0[1 + nq:][None].repeat(B, 0)); hb.set("qacc_warmstart", 0); hb.set("ctrl", 0)
    hb.forward(); hb.ctrl_reset()
    hb.set_applied_forces(True)
    qf, xf = qfrc_fn(flat), xfrc_fn(flat)
    hb.set("qfrc_applied", qf[None].astype(np.float32).repeat(B, 0)); hb.set("xfrc_applied", xf[None].astype(np.float32).repeat(B, 0))
    qf32, xf32 = qf.astype(np.float32).astype(np.float64), xf.astype(np.float32).astype(np.float64)
    errs = []
    for t in range(steps):
        a = g["actions"][t]
        hb.control_step(torch.tensor(np.repeat(a[None], B, 0), dtype=torch.float32, device="cuda"), 25)
        for i in range(25):
            od.step1()
            if i == 0:
                oc.set_goal(od, a)
            oc.run(od)
            od.qfrc_applied[:] = qf32 + xfrc_to_qfrc(od, xf32)
            od.step2()
        hq, hv = hb.get("qpos"), hb.get("qvel")
        errs.append((np.abs(hq[0] - od.qpos).max(), np.abs(hv[0] - od.qvel).max()))
        assert np.array_equal(hq[0], hq[B - 1])
    return errs, flat, od


def test_qfrc_applied_matches_the_oracle():
    rng = np.random.default_rng(5)
    scale = np.r_[np.full(7, 0.5), np.full(2, 0.05), np.full(6, 0.05)]      # arm / fingers / cube dofs (Lift: nv = 15)
    errs, flat, od = _oracle_parity(lambda f: rng.uniform(-1, 1, f.nv) * scale, lambda f: np.zeros((f.nbody, 6)))
    print("qfrc_applied, 3 control steps vs oracle |dq| |dv|:", errs)
    assert all(e[0] < 5e-5 and e[1] < 5e-4 for e in errs), errs        # fp32 against fp64: measured 8e-6 / 2.1e-4 after the third step
    assert np.abs(od.qvel).max() > 0.01


def test_xfrc_applied_matches_the_oracle():
    rng = np.random.default_rng(6)

    def xf(f):
        w = np.zeros((f.nbody, 6))
        for name, s in (("cube_main", 0.05), ("robot0_link3", 2.0), ("robot0_link6", 2.0)):
            w[f.name2id("body", name)] = rng.uniform(-s, s, 6) * np.array([1, 1, 1, 0.1, 0.1, 0.1])
        return w
    errs, flat, od = _oracle_parity(lambda f: np.zeros(f.nv), xf)
    print("xfrc_applied, 3 control steps vs oracle |dq| |dv|:", errs)
    assert all(e[0] < 5e-5 and e[1] < 5e-4 for e in errs), errs


def test_force_torque_sensor_sees_the_wrench_on_a_finger():
    """rsim_forward with a wrench on a finger body (cube lifted off the table: no contact anywhere) against the fp64 oracle under the equivalent
    qfrc_applied (from the oracle's own Jacobian, xfrc_to_qfrc): the same accelerations, and the force / torque sensors at ft_frame differ from the oracle's
    by minus the wrench moved to the site and rotated into the site frame (mj_rnePostConstraint puts xfrc_applied in cfrc_ext, the oracle's qfrc_applied
    does not), at the bounds of tests/test_hip_parity.py's contact-free sensor check.  Within the kernel, the same wrench as xfrc_applied and as the
    equivalent qfrc_applied differ in the sensors by exactly that term (1e-4)."""
    from oracle.oracle import OracleData, OracleModel
    flat, hb, cube, qa, q = _hover_batch(1, False)
    fb = flat.name2id("body", "gripper0_right_leftfinger")
    site = flat.name2id("site", "gripper0_right_ft_frame")
    w = np.zeros((flat.nbody, 6)); w[fb] = [0.7, -0.4, 1.1, 0.03, 0.02, -0.05]
    w32 = w.astype(np.float32)
    hb.set("xfrc_applied", w32[None]); hb.forward()
    assert int(hb.get("ncon")[0]) == 0
    s_x, a_x = hb.get("sensordata")[0].astype(np.float64), hb.get("qacc")[0].astype(np.float64)
    od = OracleData(OracleModel(mjcf.to_blob(flat)))
    od.qpos[:] = hb.get("qpos")[0]; od.qvel[:] = hb.get("qvel")[0]; od.ctrl[:] = hb.get("ctrl")[0]; od.qacc_warmstart[:] = 0
    od.forward()
    qeq = xfrc_to_qfrc(od, w32.astype(np.float64))
    od.qfrc_applied[:] = qeq; od.forward()
    assert od.ncon == 0
    R = np.asarray(od.site_xmat).reshape(-1, 3, 3)[site]
    sp, xip = np.asarray(od.site_xpos).reshape(-1, 3)[site], np.asarray(od.xipos).reshape(-1, 3)[fb]
    term = np.concatenate([R.T @ w32[fb, :3], R.T @ (w32[fb, 3:] + np.cross(xip - sp, w32[fb, :3]))])
    ref_a, ref_s = np.array(od.qacc), np.array(od.sensordata) - term
    assert np.abs(a_x - ref_a).max() < 1e-4 * max(1.0, np.abs(ref_a).max()), (a_x, ref_a)
    for a in range(0, len(ref_s), 3):
        assert np.abs(s_x[a:a + 3] - ref_s[a:a + 3]).max() < 2e-4 * max(1.0, np.abs(ref_s[a:a + 3]).max()), (a, s_x, ref_s)
    hb.set("xfrc_applied", 0); hb.set("qfrc_applied", qeq[None].astype(np.float32)); hb.forward()
    s_q = hb.get("sensordata")[0].astype(np.float64)
    np.testing.assert_allclose(s_x - s_q, -term, atol=1e-4)


def _lift_env(n, horizon=0, bank=0, groups=1):
    from robosuite_amd.vec_env import VecEnv
    flat, cfg = _assets("lift")
    return VecEnv("Lift", n, flat, cfg, horizon=horizon, bank_episodes=bank, stream_groups=groups)


def _rollout(env, T, setup):
    from robosuite_amd import lift
    env.reset()
    setup(env)
    tape = torch.tensor(lift.env_actions(np.arange(env.n_envs), T), device="cuda")
    for t in range(T):
        env.step(tape[t])
    b = env.env.batch
    b.sync()
    return {k: b.get(k).copy() for k in ("qpos", "qvel", "ctrl", "cstate")}


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def test_switch_off_ignores_the_arrays_and_on_with_zeros_changes_nothing():
    n, T = 16, 20

    def nonzero(env):
        env.qfrc_applied[:] = 3.0
        env.set_body_wrench("cube_main", [0, 0, 5.0, 0, 0, 0])

    def enable_zero(env):
        env.enable_applied_forces()

    base = _rollout(_lift_env(n), T, lambda env: None)
    assert _same(_rollout(_lift_env(n), T, nonzero), base)
    assert _same(_rollout(_lift_env(n), T, enable_zero), base)
    on = _rollout(_lift_env(n), T, lambda env: (env.enable_applied_forces(), nonzero(env)))
    assert not _same(on, base)


def test_stream_groups_step_the_same_forces():
    n, T = 16, 6

    def setup(env):
        env.enable_applied_forces()
        rng = np.random.default_rng(1)
        env.set_body_wrench("cube_main", torch.tensor(rng.uniform(-1, 1, (n, 6)), dtype=torch.float32))
        env.qfrc_applied[:, :7] = torch.tensor(rng.uniform(-1, 1, (n, 7)), dtype=torch.float32, device="cuda")

    assert _same(_rollout(_lift_env(n, groups=2), T, setup), _rollout(_lift_env(n), T, setup))


def test_episode_restart_zeroes_the_forces_and_a_later_write_acts():
    """Horizon 3, env 0 one step ahead: the launch in which env 0 reports `done` zeroes env 0's rows only; a wrench written after that acts in env 0's new
    episode; the others keep theirs until their own episodes end one step later."""
    from robosuite_amd import lift
    n = 8
    env = _lift_env(n, horizon=3, bank=3)
    env.reset()
    env.enable_applied_forces()
    b = env.env.batch
    b.set("ep_step", np.array([1] + [0] * (n - 1), np.int32))
    tape = torch.tensor(lift.env_actions(np.arange(n), 8), device="cuda")
    with pytest.raises(KeyError):
        env.set_body_wrench("nope", [0] * 6)
    with pytest.raises(ValueError):
        env.set_body_wrench("cube_main", [0] * 5)
    cube = env.env.model.name2id("body", "cube_main")
    env.set_body_wrench("cube_main", [0, 0, 0.3, 0, 0, 0])
    env.qfrc_applied[:] = 0.1
    _, _, done, _ = env.step(tape[0])
    assert not done.any()
    assert (env.xfrc_applied[:, cube, 2] == 0.3).all() and (env.qfrc_applied == 0.1).all()   # rows stay while the episodes run
    _, _, done, _ = env.step(tape[1])
    assert done.tolist() == [1] + [0] * (n - 1)
    x, qf = b.get("xfrc_applied"), b.get("qfrc_applied")
    assert np.abs(x[0]).max() == 0 and np.abs(qf[0]).max() == 0                              # env 0 restarted: its rows are zero ...
    assert (x[1:, cube, 2] == 0.3).all() and np.abs(np.delete(x[1:], cube, axis=1)).max() == 0 and (qf[1:] == 0.1).all()   # ... the others' untouched
    # a wrench written after `done` acts on env 0's new episode: its cube (reset 1 cm above the table) is lifted instead of falling
    env.set_body_wrench("cube_main", [0, 0, 5.0, 0, 0, 0], envs=[0])
    z0 = b.get("qpos")[:, 9 + 2].copy()
    _, _, done, _ = env.step(tape[2])
    dz = b.get("qpos")[:, 9 + 2] - z0
    assert dz[0] > 1e-2, dz
    assert done.tolist() == [0] + [1] * (n - 1)
    x = b.get("xfrc_applied")
    assert x[0, cube, 2] == 5.0 and np.abs(x[1:]).max() == 0 and np.abs(b.get("qfrc_applied")).max() == 0


def test_alternating_halves_step_the_same_forces():
    """AlternatingVecEnv: each half is a VecEnv of its own; with forces on, env i (its own wrench and qfrc_applied rows) is env i of one big batch, bitwise,
    through on-device episode restarts (which zero the rows in both)."""
    from robosuite_amd import lift
    from robosuite_amd.vec_env import AlternatingVecEnv, VecEnv
    flat, cfg = _assets("lift")
    B, T, H = 32, 12, 5
    rng = np.random.default_rng(4)
    w = torch.tensor(rng.uniform(-1, 1, (B, 6)) * np.array([0.3, 0.3, 0.5, 0.01, 0.01, 0.01]), dtype=torch.float32)
    qf = torch.tensor(rng.uniform(-0.3, 0.3, (B, 7)), dtype=torch.float32, device="cuda")
    whole = VecEnv("Lift", B, flat, cfg, seed=5, horizon=H, bank_episodes=3)
    alt = AlternatingVecEnv("Lift", B, flat, cfg, seed=5, horizon=H, bank_episodes=3)
    whole.reset(); alt.reset()
    h = B // 2
    halves = ((whole, slice(0, B)), (alt.halves[0], slice(0, h)), (alt.halves[1], slice(h, B)))
    for e, sl in halves:
        e.enable_applied_forces()
    tape = torch.tensor(lift.env_actions(np.arange(B), T), device="cuda")
    for t in range(T):
        if t % H == 0:     # (re)apply after the restarts zeroed them
            for e, sl in halves:
                e.set_body_wrench("cube_main", w[sl]); e.qfrc_applied[:, :7] = qf[sl]
        o, r, d, _ = whole.step(tape[t])
        for k, sl in ((0, slice(0, h)), (1, slice(h, B))):
            alt.step_half(k, tape[t][sl])
        for k, sl in ((0, slice(0, h)), (1, slice(h, B))):
            ok, rk, dk, _ = alt.wait_half(k)
            assert torch.equal(ok, o[sl]) and torch.equal(rk, r[sl]) and torch.equal(dk, d[sl]), (t, k)
    assert int(whole.env.batch.get("ep_index").min()) >= 2


@pytest.mark.parametrize("task", ("lift", "stack"))
def test_hand_over_keeps_the_forces(monkeypatch, task):
    """An env handed to the wide body in mid-step (RSIM_FORCE_HANDOVER=k) keeps its external forces for the rest of the step: the forced run ends where the
    native body alone takes it, at the tolerances of tests/test_hip_edge_cases.py::test_fused_tier_hand_over_in_mid_step_carries_the_step_on."""
    from robosuite_amd import lift, stack
    flat, cfg = _assets(task)
    cls, n = {"lift": (lift.LiftBatch, 16), "stack": (stack.StackBatch, 16)}[task]
    ids = np.arange(n)
    tape = torch.tensor(lift.env_actions(ids, 6), device="cuda")
    rng = np.random.default_rng(2)
    # the last body is the (last) cube: a push below its weight and small joint forces.  Wrenches of several times a cube's weight throw it around, and the
    # fp32 noise of the two bodies' row layouts then grows through the impacts (4.4e-2 in |dv| after four steps with 2 N); these keep the run as contact-rich
    # as the plain workload, so the bounds are those of the existing hand-over test
    w = rng.uniform(-1, 1, (n, 6)).astype(np.float32) * np.array([0.3, 0.3, 0.3, 0.005, 0.005, 0.005], np.float32)
    qf = rng.uniform(-0.2, 0.2, (n, flat.nv)).astype(np.float32)

    def run(force):
        monkeypatch.delenv("RSIM_FORCE_HANDOVER", raising=False)
        env = cls(flat, cfg, ids, seed0=0)
        b = env.batch
        b.set_applied_forces(True)
        x = np.zeros((n, flat.nbody, 6), np.float32); x[:, flat.nbody - 1] = w
        b.set("xfrc_applied", x); b.set("qfrc_applied", qf)
        t0 = b.tier_stats()
        out = []
        for t in range(4):
            if force is not None:
                monkeypatch.setenv("RSIM_FORCE_HANDOVER", str(force[t]))
            env.step(tape[t])
            b.sync()
            out.append((b.get("qpos").copy(), b.get("qvel").copy()))
        monkeypatch.delenv("RSIM_FORCE_HANDOVER", raising=False)
        t1 = b.tier_stats()
        return out, t1[1] - t0[1]

    ref, _ = run(None)
    got, handed = run([7, 1, 24, 12])
    assert handed >= 3 * n, handed            # (an env the wide tier steps from the start of a step has no hand-over)
    for t in range(4):
        dq, dv = np.abs(got[t][0] - ref[t][0]).max(), np.abs(got[t][1] - ref[t][1]).max()
        print(f"{task}: forced hand-over, control step {t}: |dq| {dq:.1e} |dv| {dv:.1e}")
        assert dq < 2e-4 * (t + 1) and dv < 5e-3 * (t + 1), (t, dq, dv)
    # and the forces act: the same run without them ends elsewhere
    monkeypatch.delenv("RSIM_FORCE_HANDOVER", raising=False)
    env = cls(flat, cfg, ids, seed0=0)
    for t in range(4):
        env.step(tape[t])
    env.batch.sync()
    assert np.abs(env.batch.get("qpos") - ref[3][0]).max() > 10 * np.abs(got[3][0] - ref[3][0]).max()



def _oracle_step_with_forces(od, flat, cfg, pre, e, action, n_sub, qf, xf=None):
    """ONE control step of env `e` on the fp64 oracle data `od` (the env's live model) from the kernel's state `pre` (positions, velocities, warm start,
    commands, controller record, as tests/test_full_size_parity.py copies them), with qfrc_applied = qf + J^T xf set after every mj_step1 (the wrench's
    Jacobian at that substep's kinematics)."""
    from tests.util import make_oracle
    _, _, oc = make_oracle(flat, cfg)
    od.qpos[:] = pre["qpos"][e]; od.qvel[:] = pre["qvel"][e]; od.qacc_warmstart[:] = pre["qacc_warmstart"][e]; od.ctrl[:] = pre["ctrl"][e]
    od.qfrc_applied[:] = 0
    od.forward(); oc.reset(od)
    st = oc.state
    st[:20] = pre["cstate"][e][:20]; st[20:24] = pre["cstate"][e][20:24]; st[24:28] = pre["cstate"][e][20:24]
    a = np.asarray(action, dtype=np.float64)
    for i in range(n_sub):
        od.step1()
        if i == 0:
            oc.set_goal(od, a)
        oc.run(od)
        od.qfrc_applied[:] = qf + (xfrc_to_qfrc(od, xf) if xf is not None else 0.0)
        od.step2()
    return np.array(od.qpos), np.array(od.qvel)


def test_stack_over_capacity_step_with_forces_matches_the_oracle(monkeypatch):
    """Stack (J, M and the contact block in the per-env global buffer; fused wide body): the 16 named over-capacity states of
    tests/golden/stack_over_capacity.npz, random qfrc_applied on every dof and a wrench on cubeA.  One control step through the fused kernel -- every env
    handed to the wide body at substep 12, which carries it on, forces included -- against the oracle driven with the same generalised forces,
    at the bounds of tests/test_full_size_parity.py::test_stack_over_capacity_states_three_control_steps_against_the_oracle."""
    from oracle.oracle import OracleData, OracleModel
    from tests.test_full_size_parity import STACK_OVER_DQ, STACK_OVER_DV, STACK_OVER_TAIL_ENVS, STACK_STEP_DQ_TAIL, STACK_STEP_DV_TAIL
    flat, cfg = _assets("stack")
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stack_over_capacity.npz"))
    n, n_sub = len(z["envs"]), int(z["n_sub"])
    F = ("qpos", "qvel", "qacc_warmstart", "ctrl", "cstate")
    rng = np.random.default_rng(8)
    scale = np.full(flat.nv, 0.02); scale[np.asarray(cfg["dof_idx"])] = 0.5
    qf = (rng.uniform(-1, 1, (n, flat.nv)) * scale).astype(np.float32)
    ca = flat.name2id("body", "cubeA_main")
    xf = np.zeros((n, flat.nbody, 6), np.float32)
    xf[:, ca] = rng.uniform(-1, 1, (n, 6)) * np.array([0.05, 0.05, 0.05, 0.002, 0.002, 0.002])

    def run(forces):
        # with the forces some envs no longer outgrow the native rows; RSIM_FORCE_HANDOVER=12 hands every env to the wide body in mid-step, as the
        # over-capacity ones go there (tests/test_hip_edge_cases.py: the step ends where the native body alone takes it)
        monkeypatch.setenv("RSIM_FORCE_HANDOVER", "12")
        hm, hb = make_hip(flat, cfg, B=n)
        for k in F:
            hb.set(k, z[k])
        if forces:
            hb.set_applied_forces(True); hb.set("qfrc_applied", qf); hb.set("xfrc_applied", xf)
        t0 = hb.tier_stats()
        hb.control_step(torch.tensor(z["actions"][:, 0], dtype=torch.float32, device="cuda"), n_sub)
        t1 = hb.tier_stats()
        monkeypatch.delenv("RSIM_FORCE_HANDOVER")
        assert int(hb.get("overflow").sum()) == 0 and int(hb.get("diverged").sum()) == 0
        return hb.get("qpos").copy(), hb.get("qvel").copy(), (t1[0] - t0[0], t1[1] - t0[1])

    q1, v1, stats = run(True)
    assert stats == (n, n), stats                       # every env was carried on by the wide body after a hand-over
    q0, _, _ = run(False)
    om = OracleModel(mjcf.to_blob(flat))
    pre = {k: z[k] for k in F}
    e = np.zeros((n, 2))
    for i in range(n):
        q, v = _oracle_step_with_forces(OracleData(om), flat, cfg, pre, i, z["actions"][i, 0], n_sub, qf[i].astype(np.float64), xf[i].astype(np.float64))
        e[i] = np.abs(q1[i] - q).max(), np.abs(v1[i] - v).max()
    moved = np.abs(q1 - q0).max(1)
    print("Stack over capacity with forces, per env |dq| / |dv| vs oracle:", [f"{a:.1e}/{b:.1e}" for a, b in e], "; forces moved the state by", [f"{x:.1e}" for x in moved])
    tail = np.isin(z["envs"], STACK_OVER_TAIL_ENVS)
    assert (e[~tail, 0] < STACK_OVER_DQ).all() and (e[~tail, 1] < STACK_OVER_DV).all(), e[~tail].max(0)
    assert (e[tail, 0] < STACK_STEP_DQ_TAIL).all() and (e[tail, 1] < STACK_STEP_DV_TAIL).all(), e[tail].max(0)
    assert np.median(moved) > 10 * np.median(e[:, 0]), (np.median(moved), np.median(e[:, 0]))   # the forces acted, and are what the oracle saw


def test_pickplace_tier_list_kernel_steps_with_forces():
    """PickPlace: its capacity tier is NOT fused -- envs near or beyond the 128-row native capacity are stepped by k_step_list (the 256-row configuration),
    from the tier list or the redo list.  2048 envs under per-step dynamics randomisation with qfrc_applied on the arm joints of every env; after 30 control
    steps, one more, and the envs the tier stepped in it (plus some spread over the batch) on the oracle with the same qfrc_applied and the env's live model, at
    the bounds of tests/test_full_size_parity.py::test_pickplace_one_whole_control_step_of_the_fused_path_against_the_oracle.  For the tier-stepped envs the
    oracle WITHOUT the forces lands several times farther from the kernel: the list kernel applied them."""
    from robosuite_amd import lift, pick_place
    from tests.test_full_size_parity import PP_STEP_DQ_ARM, PP_STEP_DQ_MAX, PP_STEP_DQ_MEDIAN, oracle_for_env, spread
    g, cfg, flat = load_golden("seed0_full", "pickplace_iiwa")
    B = 2048
    ids = np.arange(B)
    env = pick_place.PickPlaceBatch(flat, cfg, ids, seed0=0, horizon=500, bank_episodes=2, per_env_params=True)
    b = env.batch
    b.dr_save_defaults()
    arm = np.asarray(cfg["dof_idx"])
    rng = np.random.default_rng(9)
    qf = np.zeros((B, flat.nv), np.float32)
    qf[:, arm] = rng.uniform(-2, 2, (B, len(arm)))
    b.set_applied_forces(True)
    b.set("qfrc_applied", qf)
    tape = torch.tensor(lift.env_actions(ids, 31), device="cuda")
    for t in range(30):
        b.randomize_dynamics(seed=11, step=t)
        env.step(tape[t])
    b.randomize_dynamics(seed=11, step=30)
    pre = {k: b.get(k) for k in ("qpos", "qvel", "qacc_warmstart", "ctrl", "cstate")}
    on_tier = b.tier_snapshot().astype(bool)
    b.set("cap_need", 0)
    t0 = b.tier_stats()
    env.step(tape[30])
    t1 = b.tier_stats()
    q1, need = b.get("qpos"), b.get("cap_need")
    tiered = np.nonzero(on_tier | (need[:, 0] > b.maxcon) | (need[:, 1] > b.maxefc))[0]
    print(f"PickPlace with forces: wide-tier env-steps in the compared step {t1[0] - t0[0]} (redone {t1[1] - t0[1]}), envs {tiered.tolist()[:16]}")
    assert t1[0] - t0[0] > 0 and len(tiered) > 0
    pick = np.unique(np.concatenate([tiered[:8], spread(B, 4)]))
    armq = np.asarray(cfg["qpos_idx"])
    rows = []
    for e in pick:
        e = int(e)
        _, od = oracle_for_env(flat, b, e)
        q, _ = _oracle_step_with_forces(od, flat, cfg, pre, e, tape[30][e].cpu().numpy(), env.n_sub, qf[e].astype(np.float64))
        r = dict(env=e, tier=e in tiered, dq=np.abs(q1[e] - q), finite=bool(np.isfinite(q).all()))
        if r["tier"]:
            q0, _ = _oracle_step_with_forces(od, flat, cfg, pre, e, tape[30][e].cpu().numpy(), env.n_sub, np.zeros(flat.nv))
            r["dq_without"] = np.abs(q1[e] - q0)[armq].max()
        rows.append(r)
        print(f"   env {e}{' (tier)' if r['tier'] else ''}: |dq| {r['dq'].max():.1e} arm {r['dq'][armq].max():.1e}" + (f"; oracle without the forces: arm {r['dq_without']:.1e}" if r["tier"] else ""))
    dq_all = np.array([r["dq"].max() for r in rows]); dq_arm = np.array([r["dq"][armq].max() for r in rows])
    assert all(r["finite"] for r in rows) and int((b.get("diverged")[pick] > 0).sum()) == 0 and int(b.get("overflow")[pick].sum()) == 0
    assert np.median(dq_all) < PP_STEP_DQ_MEDIAN and dq_arm.max() < PP_STEP_DQ_ARM and dq_all.max() < PP_STEP_DQ_MAX, (np.median(dq_all), dq_arm.max(), dq_all.max())
    for r in rows:
        if r["tier"]:
            assert r["dq_without"] > 3 * r["dq"][armq].max(), r["env"]
