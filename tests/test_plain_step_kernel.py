"""The fused-tier builds (configurations 0-2) hold the control step twice (csrc/rsim_step.hip fused_step): k_step, the plain form a default launch runs, without
the profiler, the MPR restart cone and the applied forces; and k_full_step, with all three behind their run-time switches, which the host launches while one of
them is in use (csrc/rsim_api.cpp step_launch) or always under RSIM_FULL_STEP_KERNEL=1 at batch creation.  The plain form removes code a default step reaches
and skips, no arithmetic and no branch of any run, so the standard is equality to the bit: two batches of one build, one of each kind, identical seeds and
actions, compared after every control step in everything a step leaves, the narrow phase's warm-start records included."""
import json
import os
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("obs", "terminal_obs", "reward", "done", "success", "qpos", "qvel", "qacc_warmstart", "ctrl", "cstate", "time", "ep_step", "ep_index", "bank_stale", "diverged")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "robosuite_amd", "assets")


def _assets(stem):
    from robosuite_amd import mjcf
    return mjcf.load_model(os.path.join(ASSETS, stem + ".rsim")), json.load(open(os.path.join(ASSETS, stem + ".cfg.json")))


def _snap(b):
    b.sync()
    s = {k: b.get(k).copy() for k in FIELDS if b.shapes[k][-1] > 0}
    s["needs_reset"] = b.restart_flags()
    s["tier_stats"] = np.array(b.tier_stats(), dtype=np.int64)
    s["mpr_records"] = b.mpr_records()
    return s


def _assert_same(a, b, t):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (t, k)
        assert a[k].tobytes() == b[k].tobytes(), (t, k, np.nonzero(np.atleast_1d(a[k] != b[k]).reshape(len(a[k]), -1).any(1))[0][:8])


def _pair(monkeypatch, make):
    """(full, plain): the switch is read once, when the batch is created."""
    monkeypatch.setenv("RSIM_FULL_STEP_KERNEL", "1")
    full = make()
    monkeypatch.delenv("RSIM_FULL_STEP_KERNEL")
    return full, make()


def _run(monkeypatch, make, steps, step, batch=lambda e: e, force=None, close=None, prepare=None, launches=1):
    """Steps the pair side by side and asserts bitwise equality after every control step, and that each batch ran its own kernel only.  Returns the per-step
    snapshots of the plain batch and the batch itself."""
    full, plain = _pair(monkeypatch, make)
    if prepare:
        prepare(full); prepare(plain)
    if force is not None:
        monkeypatch.setenv("RSIM_FORCE_HANDOVER", str(force))      # read by every launch
    out = []
    try:
        for t in range(steps):
            step(full, t); step(plain, t)
            a, b = _snap(batch(full)), _snap(batch(plain))
            _assert_same(a, b, t)
            out.append(b)
    finally:
        monkeypatch.delenv("RSIM_FORCE_HANDOVER", raising=False)
        if close:
            close(full); close(plain)
    assert batch(plain).step_kernel_launches() == (launches * steps, 0) and batch(full).step_kernel_launches() == (0, launches * steps)
    assert sum(int(s["bank_stale"].sum()) for s in out) == 0
    return out, batch(plain)


def _env_run(monkeypatch, make, n, steps, force=None, groups=1):
    from robosuite_amd import lift
    tape = {}

    def step(e, t):
        if "a" not in tape:
            tape["a"] = torch.tensor(lift.env_actions(np.arange(n), steps, action_dim=e.model.action_dim), device="cuda")
        e.step(tape["a"][t])

    def close(e):
        e.bank_quiesce(); e._bank_stop()

    out, b = _run(monkeypatch, make, steps, step, batch=lambda e: e.batch, force=force, close=close, launches=groups,
                  prepare=(lambda e: e.batch.set_stream_groups(groups)) if groups > 1 else None)
    assert sum(int(s["done"].sum()) for s in out) > 0           # episodes did end inside the kernel: no empty comparison
    return out, b


def _lift():
    from robosuite_amd import lift
    flat, cfg = _assets("lift_panda")
    return lambda: lift.LiftBatch(flat, cfg, np.arange(24), seed0=0, per_env_cube=True, horizon=3, bank_episodes=4)


def test_lift_episodes_ending_in_the_kernel(monkeypatch):
    """Configuration 0, 24 envs, horizon 3, 4 control steps: every env restarts once inside the kernel (constant block rebuilt, reset observation taken)."""
    out, b = _env_run(monkeypatch, _lift(), 24, 4)
    assert [int(s["done"].sum()) for s in out] == [0, 0, 24, 0]


def test_lift_handed_to_the_wide_body(monkeypatch):
    """The same under RSIM_FORCE_HANDOVER=7: every env is carried on by the wide body of the plain kernel from substep 7 of every step."""
    out, b = _env_run(monkeypatch, _lift(), 24, 4, force=7)
    assert [int(s["done"].sum()) for s in out] == [0, 0, 24, 0]
    assert out[-1]["tier_stats"][1] >= 24 * 3, out[-1]["tier_stats"]


def test_lift_stream_groups(monkeypatch):
    """Two env blocks on their own streams: the launch of each block makes the same choice (two launches per control step)."""
    out, b = _env_run(monkeypatch, _lift(), 24, 4, groups=2)
    assert [int(s["done"].sum()) for s in out] == [0, 0, 24, 0]


def test_stack_over_capacity(monkeypatch):
    """Configuration 1: the 16 recorded Stack states whose control step outgrows the native body (tests/golden/stack_over_capacity.npz, the stack_over recipe of
    tools/cand_desc_states.py), four copies of each = 64 envs, 3 control steps: both bodies of the kernel run their narrow phase and solver."""
    from tests.util import make_hip
    flat, cfg = _assets("stack_panda")
    z = np.load(os.path.join(ROOT, "tests", "golden", "stack_over_capacity.npz"))
    n_sub, rep = int(z["n_sub"]), 4
    n = rep * len(z["envs"])

    def make():
        hm, hb = make_hip(flat, cfg, B=n)
        for k in ("qpos", "qvel", "qacc_warmstart", "ctrl", "cstate"):
            hb.set(k, np.tile(z[k], (rep, 1)))
        return hb

    acts = torch.tensor(np.tile(z["actions"], (rep, 1, 1)), dtype=torch.float32, device="cuda")
    out, b = _run(monkeypatch, make, 3, lambda hb, t: hb.control_step(acts[:, t].contiguous(), n_sub))
    assert out[-1]["tier_stats"][0] > 0 and out[-1]["tier_stats"][1] > 0, out[-1]["tier_stats"]       # envs were stepped by, and handed to, the wide body
    assert (b.get("ncon") > 0).all() and int(b.get("overflow").sum()) == 0 and int(out[-1]["diverged"].sum()) == 0
    # (no single pair holds a record in all 64 envs; every env holds some)
    nrec = (out[-1]["mpr_records"][:, :, 3] != 0).sum(1)
    print("stack_over: pairs with a warm-start record, per env:", nrec.tolist())
    assert (nrec > 0).all()       # every env holds records: that comparison is not one of zeros


def test_peg(monkeypatch):
    """Configuration 2 (TwoArmPegInHole / Baxter, JOINT_VELOCITY), per-episode peg radius: 16 envs, horizon 2, 3 control steps."""
    from robosuite_amd import peg_in_hole
    from tests.util import load_golden
    g, cfg, flat = load_golden("ctl_joint_velocity", "peg_baxter")
    out, b = _env_run(monkeypatch, lambda: peg_in_hole.PegBatch(flat, cfg, np.arange(16), seed0=0, horizon=2, bank_episodes=4, per_env_peg=True), 16, 3)
    assert [int(s["done"].sum()) for s in out] == [0, 16, 0]


def _press(B):
    """The press scene of tools/mpr_touch_states.py (tests/test_mpr_touch_record.py): a 42-vertex hull flies into the side of a cylinder and is pulled off again
    by a spring.  That test steps it with rsim_step -- the debug kernel; here the sled carries a motor driven by a JOINT_TORQUE part with zero actions (no
    gravity in the scene: zero torque), so that control steps of ten substeps run it through k_step / k_full_step: four steps = the forty substeps of the
    recipe.  Returns make() -> a batch at the recipe's start."""
    from robosuite_amd import mjcf
    from tests.util import make_hip
    from tools.mpr_touch_states import press_inputs, press_xml
    with tempfile.TemporaryDirectory() as tmp:
        flat = mjcf.compile_mjcf(press_xml(tmp).replace("</mujoco>", '<actuator><motor name="push" joint="in"/></actuator></mujoco>'))
    cfg = {"type": "JOINT_TORQUE", "qpos_idx": [0], "dof_idx": [0], "act_idx": [0], "input_min": [-1.0], "input_max": [1.0], "output_min": [-0.1], "output_max": [0.1],
           "torque_limits": [[-1.0], [1.0]]}
    q0, v0 = press_inputs(B)

    def make():
        hm, hb = make_hip(flat, cfg, B=B)
        hb.set("qpos", q0); hb.set("qvel", v0); hb.set("qacc_warmstart", 0); hb.set("ctrl", 0)
        hb.forward(); hb.ctrl_reset()
        return hb

    return make


def _press_step(hb):
    hb.control_step(torch.zeros((hb.B, hb.model.action_dim), dtype=torch.float32, device="cuda"), 10)


def test_a_hull_pressed_onto_a_cylinder_and_pulled_off(monkeypatch):
    """The press scene (_press): contact after steps one and two (MPR's refinement on a curved shape every substep, the flag-4 record), none after step four."""
    B = 8
    ncon = []

    def step(hb, t):
        _press_step(hb)
        ncon.append(hb.get("ncon").copy())

    out, b = _run(monkeypatch, _press(B), 4, step)
    print("press ncon per control step (full, plain):", [c.tolist() for c in ncon])
    for t in range(4):
        assert np.array_equal(ncon[2 * t], ncon[2 * t + 1])
    assert (ncon[1] > 0).all() and (ncon[3] > 0).all() and (ncon[7] == 0).all()
    assert (out[0]["mpr_records"][:, :, 3] == 4.0).any()      # touched, this deep: the record of a contact next to a smooth shape
    assert all(np.isfinite(s["qpos"]).all() and np.isfinite(s["qvel"]).all() for s in out)


def _hover(B):
    """Lift at the golden fixture's start with the cube 0.2 m above the table, at rest (tests/test_applied_forces.py)."""
    from tests.util import load_golden, make_hip
    g, cfg, flat = load_golden("seed1_full")
    nq, cube = flat.nq, flat.name2id("body", "cube_main")
    qa = int(flat.arrays["jnt_qposadr"][flat.arrays["body_jntadr"][cube]])
    q = g["states"][0][1:1 + nq].copy()
    q[qa:qa + 7] = [0.0, 0.3, 1.03, 1.0, 0.0, 0.0, 0.0]
    hm, hb = make_hip(flat, cfg, B=B)
    hb.set("qpos", q[None].repeat(B, 0)); hb.set("qvel", 0); hb.set("qacc_warmstart", 0); hb.set("ctrl", 0)
    hb.forward(); hb.ctrl_reset()
    return flat, hb, cube, g


def test_the_profiler_runs_on_the_full_kernel_and_disarming_returns_to_the_plain_one():
    """The press scene (_press): the hull lies against the cylinder throughout the second control step, so every env's narrow phase runs MPR there and the armed
    profiler has support evaluations to count."""
    B = 8
    hb = _press(B)()
    _press_step(hb)
    assert hb.step_kernel_launches() == (1, 0)
    hb.profile(True)
    _press_step(hb)
    assert hb.step_kernel_launches() == (1, 1)
    wl = hb.wavelog()              # (before any read of a derived field: that runs a forward pass, a launch of its own while the profiler is armed)
    print("wave log of the profiled step (start, end, mpr, supports, newton, candidates):", wl[:, 2:8].tolist())
    assert (wl[:, 5] > 0).all() and (wl[:, 3] > wl[:, 2]).all(), wl[:, 2:8]      # non-zero support counts, every env's end after its start
    p = hb.profile(False)
    assert p["n_support"] > 0 and p["n_sub"] == 10 * B, p
    assert (hb.get("ncon") > 0).all()
    _press_step(hb)
    assert hb.step_kernel_launches() == (2, 1)


def test_applied_forces_switch_to_the_full_kernel_in_mid_run(monkeypatch):
    """Two plain steps, the forces enabled, two steps (full kernel), disabled, one step (plain again): bitwise the batch that ran the full kernel throughout."""
    B = 8
    monkeypatch.setenv("RSIM_FULL_STEP_KERNEL", "1")
    flat, ref, cube, g = _hover(B)
    monkeypatch.delenv("RSIM_FULL_STEP_KERNEL")
    _, hb, _, _ = _hover(B)
    w = np.zeros((B, flat.nbody, 6), np.float32)
    w[:, cube, 2] = 0.5 * float(flat.arrays["body_mass"][cube]) * 9.81 * (1 + np.arange(B)) / B
    qf = (np.random.default_rng(3).uniform(-0.3, 0.3, (B, flat.nv)) * (np.arange(flat.nv) < 7)).astype(np.float32)
    moved = []
    for t in range(5):
        if t == 2:
            for b in (ref, hb):
                b.set_applied_forces(True); b.set("xfrc_applied", w); b.set("qfrc_applied", qf)
        if t == 4:
            for b in (ref, hb):
                b.set_applied_forces(False)
        a = torch.tensor(np.repeat(g["actions"][t][None], B, 0), dtype=torch.float32, device="cuda")
        ref.control_step(a, 25); hb.control_step(a, 25)
        _assert_same(_snap(ref), _snap(hb), t)
        moved.append(hb.get("qpos").copy())
    assert hb.step_kernel_launches() == (3, 2) and ref.step_kernel_launches() == (0, 5)
    assert np.array_equal(moved[1][0], moved[1][B - 1]) and not np.array_equal(moved[3][0], moved[3][B - 1])      # the per-env wrenches acted once enabled
