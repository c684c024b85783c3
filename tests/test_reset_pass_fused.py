"""The reset pass inside the control-step kernel (csrc/rsim_step.hip k_step, RF_RESET_INKERNEL): in the fused-tier builds (configurations 0-2) the workgroup
that ended an env's episode rebuilds the env's constant block and takes its reset observation itself; RSIM_SEPARATE_RESET_PASS=1 at batch creation keeps the
k_step -> k_prepare(reset_only) -> k_reset_obs chain of launches.  Both are the same body under the same flags on the same reloaded state, so the standard is
equality to the bit: two batches of one build, one of each kind, identical seeds and actions, compared after every control step in everything a step leaves."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("obs", "terminal_obs", "reward", "done", "success", "qpos", "qvel", "qacc_warmstart", "ctrl", "cstate", "time", "ep_step", "ep_index", "bank_stale", "diverged")
ASSETS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robosuite_amd", "assets")


def _assets(stem):
    from robosuite_amd import mjcf
    return mjcf.load_model(os.path.join(ASSETS, stem + ".rsim")), json.load(open(os.path.join(ASSETS, stem + ".cfg.json")))


def _snap(env):
    b = env.batch
    b.sync()
    s = {k: b.get(k).copy() for k in FIELDS}
    s["needs_reset"] = b.restart_flags()
    s["tier_stats"] = np.array(b.tier_stats(), dtype=np.int64)
    return s


def _pair(monkeypatch, make):
    """(separate, fused): the switch is read once, when the batch is created."""
    monkeypatch.setenv("RSIM_SEPARATE_RESET_PASS", "1")
    sep = make()
    monkeypatch.delenv("RSIM_SEPARATE_RESET_PASS")
    return sep, make()


def _run(monkeypatch, make, n, steps, prepare=None, force=None):
    """Steps the pair side by side and asserts bitwise equality after every control step.  Returns the per-step snapshots of the fused batch."""
    from robosuite_amd import lift
    sep, fus = _pair(monkeypatch, make)
    if prepare:
        prepare(sep); prepare(fus)
    tape = torch.tensor(lift.env_actions(np.arange(n), steps, action_dim=fus.model.action_dim), device="cuda")
    if force is not None:
        monkeypatch.setenv("RSIM_FORCE_HANDOVER", str(force))      # read by every launch
    out = []
    try:
        for t in range(steps):
            sep.step(tape[t]); fus.step(tape[t])
            a, b = _snap(sep), _snap(fus)
            for k in a:
                assert np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f"), (t, k, np.nonzero(np.atleast_1d(a[k] != b[k]))[0][:8])
            out.append(b)
    finally:
        monkeypatch.delenv("RSIM_FORCE_HANDOVER", raising=False)
        for e in (sep, fus):
            e.bank_quiesce(); e._bank_stop()
    assert sum(int(s["done"].sum()) for s in out) > 0           # episodes did end: no empty comparison
    assert sum(int(s["bank_stale"].sum()) for s in out) == 0
    return out


def _lift(per_env_cube):
    from robosuite_amd import lift
    flat, cfg = _assets("lift_panda")
    return lambda: lift.LiftBatch(flat, cfg, np.arange(24), seed0=0, per_env_cube=per_env_cube, horizon=3, bank_episodes=4)


def test_lift_per_env_cube_rebuilds_the_constant_block_in_the_kernel(monkeypatch):
    """24 envs, horizon 3, ring of 4, 8 control steps: every env restarts twice, each time with another cube size -- a block that was not rebuilt (or was read
    back stale) changes the cube's geometry and with it the reset observation and every later step."""
    out = _run(monkeypatch, _lift(True), 24, 8)
    assert [int(s["done"].sum()) for s in out] == [0, 0, 24, 0, 0, 24, 0, 0]
    assert out[-1]["ep_index"].tolist() == [2] * 24
    assert out[2]["needs_reset"].all() and not out[3]["needs_reset"].any()      # left set for the next step's fresh controllers, consumed by it
    # the premise: the reset observation depends on the episode (another cube, another placement), so a skipped or stale pass would be seen
    assert not np.array_equal(out[2]["obs"], out[5]["obs"]) and not np.array_equal(out[2]["obs"], out[2]["terminal_obs"])


def test_lift_shared_constant_block_takes_the_observation_only(monkeypatch):
    """per_env_cube=False: no per-env blocks, nothing patched -- the kernel re-enters the body without a rebuild."""
    out = _run(monkeypatch, _lift(False), 24, 8)
    assert [int(s["done"].sum()) for s in out] == [0, 0, 24, 0, 0, 24, 0, 0]


def test_stack_episode_ending_on_the_wide_body(monkeypatch):
    """Every env hands over to the wide body at substep 5 of every step (RSIM_FORCE_HANDOVER), so the steps that end episodes are committed by the wide body and
    the re-entry of the native body follows it in the same workgroup."""
    from robosuite_amd import stack
    flat, cfg = _assets("stack_panda")
    out = _run(monkeypatch, lambda: stack.StackBatch(flat, cfg, np.arange(64), seed0=0, horizon=3, bank_episodes=4), 64, 7, force=5)
    assert [int(s["done"].sum()) for s in out] == [0, 0, 64, 0, 0, 64, 0]
    for t in (2, 5):      # the steps that end episodes: all 64 env-steps went through the wide body, by a hand-over unless the env was on the tier already
        d = out[t]["tier_stats"] - out[t - 1]["tier_stats"]
        assert d[0] == 64 and d[1] > 0, (t, d)
    assert out[-1]["tier_stats"][1] > 0


def test_peg_per_env_peg(monkeypatch):
    """Configuration 2 (TwoArmPegInHole / Baxter, JOINT_VELOCITY: controller state beyond LDS, no tier), per-episode peg radius: 16 envs, horizon 2, 6 steps."""
    from robosuite_amd import peg_in_hole
    from tests.util import load_golden
    g, cfg, flat = load_golden("ctl_joint_velocity", "peg_baxter")
    out = _run(monkeypatch, lambda: peg_in_hole.PegBatch(flat, cfg, np.arange(16), seed0=0, horizon=2, bank_episodes=4, per_env_peg=True), 16, 6)
    assert [int(s["done"].sum()) for s in out] == [0, 16, 0, 16, 0, 16]


def test_early_end_rule_armed_keeps_the_separate_launches_and_agrees(monkeypatch):
    """terminate_on_success with min_episode_steps = 1: k_end_episodes restarts envs after k_step, so both batches run the launches behind the step."""
    out = _run(monkeypatch, _lift(True), 24, 8, prepare=lambda e: e.set_early_end(success=True, min_steps=1))
    assert sum(int(s["done"].sum()) for s in out) >= 48


def test_stream_groups(monkeypatch):
    """Two env blocks on their own streams: each block's k_step finishes its own restarts."""
    out = _run(monkeypatch, _lift(True), 24, 8, prepare=lambda e: e.batch.set_stream_groups(2))
    assert [int(s["done"].sum()) for s in out] == [0, 0, 24, 0, 0, 24, 0, 0]
