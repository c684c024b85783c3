"""Ending episodes early on the device (include/rsim.h rsim_set_early_end / rsim_end_episodes, csrc/rsim_episode.hip): on success, on a bad-state guard
hit, on request.  The standard is the one the horizon restart is held to (test_hip_parity.py test_on_device_episode_reset_equals_a_fresh_host_reset):
an env that ended is BITWISE the env a host reset builds for its next episode, and goes on bitwise like it; every other env is bit-unchanged."""
import functools

import numpy as np
import pytest

from tests.util import load_golden, make_oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STATE = ("qpos", "qvel", "qacc_warmstart", "ctrl", "time", "cstate", "obs", "reward", "success", "done", "ep_step", "ep_index", "terminal_obs", "task_object",
         "bank_stale", "diverged", "overflow", "end_reason")
IDS = np.array([3, 11, 200])
TABLE = 0.8            # Lift: table_height; success = cube centre above TABLE + 0.04 (lift.py lift_task)
HORIZON, RING = 50, 3


def _snap(env, keys=STATE):
    return {k: env.batch.get(k).copy() for k in keys}


def _patched(env):
    """float32 [B, P]: the float-table entries the env's reset ring patches per episode (Lift: what depends on the cube size; Peg: on the peg radius)."""
    slots = env._bank_slots() if hasattr(env, "_bank_slots") else []
    if not slots:
        return np.zeros((env.B, 0), np.float32)
    rows = {k: env.batch.param_get(k).reshape(env.B, -1) for k in {k for k, _, _ in slots}}
    return np.stack([rows[k][:, e] for k, e, _ in slots], axis=1).astype(np.float32)


def _lift(ids=IDS, **kw):
    from robosuite_amd import lift
    g, cfg, flat = load_golden("seed1_full")
    return lift.LiftBatch(flat, cfg, ids, seed0=0, **kw)


def _raise_cube(env, k, height):
    """Env k's cube `height` above the table top, written into the state before the first step."""
    z = int(env.spec["sampler"]["objects"][0]["qposadr"]) + 2
    q = env.batch.get("qpos")
    q[k, z] = TABLE + height
    env.batch.set("qpos", q)


def _acts(ids, n):
    from robosuite_amd import lift
    return torch.tensor(lift.env_actions(ids, n), device="cuda")


def _oracle_success(qpos_rows, actions, steps):
    """Lift's success check after `steps` control steps on the CPU oracle, per row."""
    g, cfg, flat = load_golden("seed1_full")
    cube = flat.names["body"].index("cube_main")
    out = []
    for q, a in zip(qpos_rows, actions):
        om, od, oc = make_oracle(flat, cfg)
        od.qpos[:] = q; od.qvel[:] = 0; od.qacc_warmstart[:] = 0; od.forward(); oc.reset(od)
        for t in range(steps):
            oc.env_step(od, a[t], 25)
        out.append(bool(od.xpos[3 * cube + 2] > TABLE + 0.04))
    return out


@functools.lru_cache(maxsize=None)
def _scenario():
    """Scenario 1, computed once: envs [3, 11, 200], horizon 50, ring of 3, env 11's cube 0.10 m above the table, success rule armed (`auto`); the same
    batch without the rule (`plain`); a host reset of episode 1 (`fresh`).  One step, then three more of auto and fresh.  Returns host snapshots."""
    acts = _acts(IDS, 4)
    auto, plain = _lift(horizon=HORIZON, bank_episodes=RING), _lift(horizon=HORIZON, bank_episodes=RING)
    auto.set_early_end(success=True)
    for e in (auto, plain):
        _raise_cube(e, 1, 0.10)
    q_start = plain.batch.get("qpos").copy()
    bank = dict(rows=np.stack([np.concatenate([np.asarray(x, np.float32) for x in plain._bank_rows(np.arange(3), ep)], axis=1) for ep in range(RING)], axis=1),
                tags=np.tile(np.arange(RING), (3, 1)), patch_idx=np.arange(len(plain._bank_patch_offsets())))
    auto.step(acts[0]); plain.step(acts[0])
    s = dict(acts=acts.cpu().numpy(), q_start=q_start, bank=bank, auto=_snap(auto), plain=_snap(plain), auto_ft=_patched(auto), plain_ft=_patched(plain))
    fresh = _lift()
    fresh.reset(block=1)
    fresh.batch.observe()
    s["fresh"], s["fresh_ft"] = _snap(fresh, ("qpos", "obs")), _patched(fresh)
    fresh.reset(block=1)
    s["auto_next"], s["fresh_next"] = [], []
    for t in range(1, 4):
        auto.step(acts[t]); fresh.step(acts[t])
        s["auto_next"].append(_snap(auto)); s["fresh_next"].append(_snap(fresh, ("qpos", "qvel", "obs")))
    return s


def test_success_ends_the_episode_and_the_env_restarts_as_a_fresh_host_reset():
    s = _scenario()
    a, p, f = s["auto"], s["plain"], s["fresh"]
    # the premise, on the CPU: after one control step the raised cube is above the success height, the other two are not
    assert _oracle_success(s["q_start"], s["acts"].transpose(1, 0, 2), 1) == [False, True, False]
    assert p["success"].tolist() == [0, 1, 0] and p["done"].tolist() == [0, 0, 0]
    assert a["done"].tolist() == [0, 1, 0] and a["end_reason"].tolist() == [0, 2, 0]
    assert a["ep_index"].tolist() == [0, 1, 0] and a["ep_step"].tolist() == [1, 0, 1]
    # env 11 is a fresh host reset of its episode 1: state, patched model entries (cube size), the observation reset() returns
    assert np.array_equal(a["qpos"][1], f["qpos"][1]) and np.array_equal(a["obs"][1], f["obs"][1]) and np.array_equal(s["auto_ft"][1], s["fresh_ft"][1])
    assert s["auto_ft"].shape[1] > 0 and not np.array_equal(s["auto_ft"][1], s["plain_ft"][1])
    assert not np.any(a["qvel"][1]) and not np.any(a["qacc_warmstart"][1]) and not np.any(a["ctrl"][1]) and a["time"][1] == 0
    # the finished episode's last record, reward and success are the step's own
    assert np.array_equal(a["terminal_obs"][1], p["obs"][1]) and a["reward"][1] == p["reward"][1] and a["success"][1] == p["success"][1] == 1
    # the other envs never noticed
    for k in ("qpos", "qvel", "obs", "qacc_warmstart", "ctrl", "time", "cstate", "reward", "ep_step", "ep_index"):
        assert np.array_equal(a[k][[0, 2]], p[k][[0, 2]]), k
    assert np.array_equal(s["auto_ft"][[0, 2]], s["plain_ft"][[0, 2]])
    # fresh controller state, cold narrow phase, rebuilt constant block: three more steps bitwise like the host-reset batch
    for t, (x, y) in enumerate(zip(s["auto_next"], s["fresh_next"])):
        for k in ("qpos", "qvel", "obs"):
            assert np.array_equal(x[k][1], y[k][1]), (t, k)
    assert int(s["auto_next"][-1]["bank_stale"].sum()) == 0 and s["auto_next"][-1]["ep_step"].tolist() == [4, 3, 4]


def test_device_state_equals_the_host_mirror():
    from robosuite_amd import episodes
    s = _scenario()
    before = dict(s["plain"], ft=s["plain_ft"], seen_diverged=np.zeros(3, np.int32), needs_reset=np.zeros(3, np.int32))
    want = episodes.end_episodes_reference(before, s["bank"], episodes.RULE_SUCCESS, min_steps=1)
    got = dict(s["auto"], ft=s["auto_ft"])
    for k in want:
        if k in ("seen_diverged", "needs_reset"):       # not readable from the device
            continue
        rows = [0, 2] if k == "obs" else [0, 1, 2]      # the ended env's RSIM_OBS is replaced by the reset observation after the kernel
        assert np.array_equal(want[k][rows], got[k][rows]), k
    assert want["end_reason"].tolist() == [0, 2, 0]


def test_success_waits_for_min_steps():
    """min_steps = 3: the success of steps 1 and 2 ends nothing.  The cube starts 0.25 m up (0.10 m would be back on the table by step 3: it falls
    0.11 m in 0.15 s) -- checked on the oracle."""
    acts = _acts(IDS, 3)
    env = _lift(horizon=HORIZON, bank_episodes=RING)
    env.set_early_end(success=True, min_steps=3)
    _raise_cube(env, 1, 0.25)
    q0 = env.batch.get("qpos")[1:2].copy()
    assert _oracle_success(q0, acts.cpu().numpy().transpose(1, 0, 2)[1:2], 3) == [True]
    log = []
    for t in range(3):
        env.step(acts[t])
        log.append((env.batch.get("success").tolist(), env.batch.get("done").tolist(), env.batch.get("end_reason").tolist(), env.batch.get("ep_index").tolist()))
    assert [x[0] for x in log] == [[0, 1, 0]] * 3
    assert [x[1] for x in log] == [[0, 0, 0], [0, 0, 0], [0, 1, 0]] and [x[2] for x in log] == [[0, 0, 0], [0, 0, 0], [0, 2, 0]]
    assert [x[3] for x in log] == [[0, 0, 0], [0, 0, 0], [0, 1, 0]] and env.batch.get("ep_step").tolist() == [3, 0, 3]


def _make(name, ids, **kw):
    from robosuite_amd import factory, lift, peg_in_hole, pick_place, stack
    if name == "Lift":
        g, cfg, flat = load_golden("seed1_full")
        return lift.LiftBatch(flat, cfg, ids, seed0=2, **kw)
    if name == "PickPlaceSingle":
        g, cfg, flat = load_golden("seed3", "pickplace_single_iiwa")
        return pick_place.PickPlaceBatch(flat, cfg, ids, seed0=2, **kw)
    stem, cls = {"Stack": ("stack_panda", stack.StackBatch), "TwoArmPegInHole": ("peg_baxter_joint_velocity", peg_in_hole.PegBatch),
                 "PickPlace": ("pickplace_iiwa", pick_place.PickPlaceBatch)}[name]
    flat, cfg = factory.load_shipped(stem)
    return cls(flat, cfg, ids, seed0=2, **kw)


CONFIGS = ("Lift", "Stack", "TwoArmPegInHole", "PickPlace", "PickPlaceSingle")
ENDED, OTHERS = [0, 2], [1, 3]


@functools.lru_cache(maxsize=None)
def _requested(name):
    """Per configuration, computed once: two steps of four envs, end_episodes(mask) for two of them; a host reset of episode 1 beside it; the same two
    steps on a batch whose horizon is 2 (the restart the control step itself performs).  Returns (env, fresh, snapshots)."""
    ids = np.array([5, 77, 1030, 4000])
    env, fresh, hz = _make(name, ids, horizon=HORIZON, bank_episodes=2), _make(name, ids), _make(name, ids, horizon=2, bank_episodes=2)
    adim = env.model.action_dim
    a = torch.tensor(np.random.default_rng(9).uniform(-0.3, 0.3, (2, 4, adim)).astype(np.float32), device="cuda")
    for e in (env, hz):
        e.step(a[0]); e.step(a[1])
    s = dict(before=_snap(env), before_ft=_patched(env), horizon_obs=hz.batch.get("obs").copy())
    env.end_episodes(torch.tensor([1, 0, 1, 0], dtype=torch.bool, device="cuda"))
    s["after"], s["after_ft"] = _snap(env), _patched(env)
    fresh.reset(block=1)
    fresh.batch.observe()
    s["fresh"], s["fresh_ft"] = _snap(fresh, ("qpos", "obs", "task_object")), _patched(fresh)
    return env, fresh, s


@pytest.mark.parametrize("name", CONFIGS)
def test_requested_end_in_every_configuration(name):
    """end_episodes(mask) after two steps, two of four envs: the ended envs hold the state a fresh host reset of episode 1 builds (qpos, patched table
    entries, task object), the others are bit-unchanged in every state array; ten such calls walk episodes 1 .. 10 of the env's own stream through a
    ring of two, never stale.  (The reset observation: the next test.)"""
    env, fresh, s = _requested(name)
    before, after, f = s["before"], s["after"], s["fresh"]
    assert np.array_equal(after["qpos"][ENDED], f["qpos"][ENDED])
    assert np.array_equal(s["after_ft"][ENDED], s["fresh_ft"][ENDED]) and np.array_equal(after["task_object"][ENDED], f["task_object"][ENDED])
    assert np.array_equal(after["terminal_obs"][ENDED], before["obs"][ENDED])
    assert after["done"][ENDED].tolist() == [1, 1] and after["end_reason"][ENDED].tolist() == [4, 4] and after["ep_step"][ENDED].tolist() == [0, 0]
    assert after["ep_index"].tolist() == [1, 0, 1, 0] and not np.any(after["qvel"][ENDED]) and not np.any(after["time"][ENDED])
    for k in STATE:
        assert np.array_equal(after[k][OTHERS], before[k][OTHERS]), k
    assert np.array_equal(s["after_ft"][OTHERS], s["before_ft"][OTHERS])
    mask = torch.tensor([1, 0, 1, 0], dtype=torch.bool, device="cuda")
    for k in range(2, 11):
        env.end_episodes(mask)
        q, pv = fresh._bank_rows(np.arange(4), k)
        assert env.batch.get("ep_index").tolist() == [k, 0, k, 0]
        assert np.array_equal(env.batch.get("qpos")[ENDED], np.asarray(q, np.float32)[ENDED]), k
        if name == "PickPlaceSingle":
            assert np.array_equal(env.batch.get("task_object")[ENDED], np.asarray(pv)[ENDED, 0].astype(np.int32)), k
        else:
            assert np.array_equal(_patched(env)[ENDED], np.asarray(pv, np.float32).reshape(4, -1)[ENDED]), k
    assert int(env.batch.get("bank_stale").sum()) == 0
    for k in ("qpos", "qvel", "cstate", "obs", "ep_step"):
        assert np.array_equal(env.batch.get(k)[OTHERS], before[k][OTHERS]), k


@pytest.mark.parametrize("name", CONFIGS)
def test_requested_end_returns_the_reset_observation_of_a_fresh_host_reset(name):
    """RSIM_OBS of an env ended on request is bitwise the record a fresh host reset of its next episode returns (reset(block=1) + observe()), in every
    configuration.  (The restart a control step performs takes its record with k_reset_obs, the control-step build of the same body: bitwise the same
    for the one-tile configurations -- asserted here against a horizon restart -- and equal up to the last bits of robot0_joint_acc, 5e-5 at most, in
    the 64 x 48 one, which is why rsim_end_episodes uses the entry a host reset uses.)"""
    env, fresh, s = _requested(name)
    got, want = s["after"]["obs"][ENDED], s["fresh"]["obs"][ENDED]
    if name in ("Lift", "Stack", "TwoArmPegInHole"):
        assert np.array_equal(got, s["horizon_obs"][ENDED])
    dims, keys = np.cumsum([0] + list(env.cfg["obs_dims"])), env.cfg["obs_keys"]
    d = np.abs(got - want)
    print(name, "keys that differ from the host reset:", [(keys[k], float(d[:, dims[k]:dims[k + 1]].max())) for k in range(len(keys)) if d[:, dims[k]:dims[k + 1]].max() > 0])
    assert np.array_equal(got, want)


def test_requested_end_right_after_a_horizon_restart_leaves_the_other_restarted_envs_alone():
    """All three envs restart at the horizon (step 2); before their next step one of them is ended on request.  The two others keep everything the
    horizon restart left -- record included -- and still get their fresh controllers at the next step, exactly as on a twin batch nobody asked anything
    of; the ended env moves on to episode 2 and steps like a host reset of it."""
    acts = _acts(IDS, 3)
    env, twin, fresh = _lift(horizon=2, bank_episodes=RING), _lift(horizon=2, bank_episodes=RING), _lift()
    for t in range(2):
        env.step(acts[t]); twin.step(acts[t])
    before = _snap(env)
    assert before["done"].tolist() == [1, 1, 1]
    env.end_episodes(torch.tensor([0, 1, 0], dtype=torch.bool, device="cuda"))
    after = _snap(env)
    for k in STATE:
        assert np.array_equal(after[k][[0, 2]], before[k][[0, 2]]), k
    assert after["ep_index"].tolist() == [1, 2, 1] and after["end_reason"][1] == 4
    fresh.reset(block=2)
    fresh.batch.observe()
    assert np.array_equal(after["qpos"][1], fresh.batch.get("qpos")[1]) and np.array_equal(after["obs"][1], fresh.batch.get("obs")[1])
    fresh.reset(block=2)
    env.step(acts[2]); twin.step(acts[2]); fresh.step(acts[2])
    for k in ("qpos", "qvel", "obs", "cstate"):
        assert np.array_equal(env.batch.get(k)[[0, 2]], twin.batch.get(k)[[0, 2]]), k
    for k in ("qpos", "qvel", "obs"):
        assert np.array_equal(env.batch.get(k)[1], fresh.batch.get(k)[1]), k


def test_horizon_and_success_in_the_same_step_restart_once():
    env = _lift(horizon=1, bank_episodes=RING)
    env.set_early_end(success=True)
    _raise_cube(env, 1, 0.10)
    env.step(_acts(IDS, 1)[0])
    assert env.batch.get("success").tolist() == [0, 1, 0] and env.batch.get("done").tolist() == [1, 1, 1]
    assert env.batch.get("ep_index").tolist() == [1, 1, 1] and env.batch.get("end_reason").tolist() == [1, 1, 1]


def test_a_guard_hit_ends_the_episode_when_the_rule_is_armed():
    """A cube velocity of 1e11 m/s trips the bad-state guard in the first substep (|qvel| >= 1e10: the env is put back to qpos0 and counted in
    RSIM_DIVERGED).  Rule armed: the step reports done / reason 3 and the env holds episode 1's drawn reset.  Rule off: as ever, it carries on in episode 0."""
    acts = _acts(IDS, 1)
    out = {}
    for armed in (True, False):
        env = _lift(horizon=HORIZON, bank_episodes=RING)
        if armed:
            env.set_early_end(diverged=True)
        v = env.batch.get("qvel")
        v[1, 9] = 1.0e11
        env.batch.set("qvel", v)
        env.step(acts[0])
        out[armed] = _snap(env)
    fresh = _lift()
    fresh.reset(block=1)
    fresh.batch.observe()
    on, off = out[True], out[False]
    assert on["diverged"][1] >= 1 and on["diverged"][[0, 2]].tolist() == [0, 0] and np.array_equal(on["diverged"], off["diverged"])
    assert on["end_reason"].tolist() == [0, 3, 0] and on["done"].tolist() == [0, 1, 0] and on["ep_index"].tolist() == [0, 1, 0]
    assert np.array_equal(on["qpos"][1], fresh.batch.get("qpos")[1]) and np.array_equal(on["obs"][1], fresh.batch.get("obs")[1])
    assert off["end_reason"].tolist() == [0, 0, 0] and off["done"].tolist() == [0, 0, 0] and off["ep_index"].tolist() == [0, 0, 0]
    assert not np.array_equal(off["qpos"][1], fresh.batch.get("qpos")[1])
    for k in ("qpos", "qvel", "obs"):
        assert np.array_equal(on[k][[0, 2]], off[k][[0, 2]]), k


def test_a_guard_hit_ends_the_episode_on_the_list_tier_configuration():
    """The same rule behind PickPlace's control step (64 x 48 configuration: native pass, list-tier passes 1 and 2, then k_end_episodes): the env whose
    last object is thrown at 1e11 m/s restarts from episode 1's drawn reset, the other envs step exactly as on a batch without the rule."""
    ids = np.array([5, 77, 1030, 4000])
    out = {}
    for armed in (True, False):
        env = _make("PickPlace", ids, horizon=HORIZON, bank_episodes=2)
        if armed:
            env.set_early_end(diverged=True)
        v = env.batch.get("qvel")
        v[2, v.shape[1] - 6] = 1.0e11
        env.batch.set("qvel", v)
        env.step(torch.zeros(4, env.model.action_dim, device="cuda"))
        out[armed] = _snap(env)
    fresh = _make("PickPlace", ids)
    fresh.reset(block=1)
    on, off = out[True], out[False]
    assert on["diverged"][2] >= 1 and np.array_equal(on["diverged"], off["diverged"]) and on["diverged"][[0, 1, 3]].tolist() == [0, 0, 0]
    assert on["end_reason"].tolist() == [0, 0, 3, 0] and on["done"].tolist() == [0, 0, 1, 0] and on["ep_index"].tolist() == [0, 0, 1, 0]
    assert np.array_equal(on["qpos"][2], fresh.batch.get("qpos")[2]) and not np.any(on["qvel"][2]) and on["ep_step"].tolist() == [1, 1, 0, 1]
    assert np.array_equal(on["terminal_obs"][2], off["obs"][2]) and int(on["bank_stale"].sum()) == 0
    for k in ("qpos", "qvel", "obs", "cstate", "reward"):
        assert np.array_equal(on[k][[0, 1, 3]], off[k][[0, 1, 3]]), k


def test_not_armed_means_nothing_changes():
    from robosuite_amd.vec_env import VecEnv
    acts = _acts(IDS, 8)
    plain, disarmed = _lift(horizon=4, bank_episodes=RING), _lift(horizon=4, bank_episodes=RING)
    disarmed.set_early_end(success=False, diverged=False, min_steps=1)
    for t in range(8):
        plain.step(acts[t]); disarmed.step(acts[t])
        x, y = _snap(plain), _snap(disarmed)
        for k in STATE:
            assert np.array_equal(x[k], y[k]), (t, k)
        assert not np.any(x["end_reason"])              # not maintained: the horizon is reported by `done` alone
    assert plain.batch.get("ep_index").tolist() == [2, 2, 2]
    g, cfg, flat = load_golden("seed1_full")
    env = VecEnv("Lift", 3, flat, cfg, horizon=4, bank_episodes=RING, env_ids=IDS)
    env.reset()
    obs, rew, done, info = env.step(acts[0])
    assert sorted(info) == ["success", "terminal_obs"] and not env.early_end_armed


def test_stream_groups_and_the_alternating_env_compute_the_same_bits():
    from robosuite_amd.vec_env import AlternatingVecEnv
    s = _scenario()
    acts = _acts(IDS, 4)
    env = _lift(horizon=HORIZON, bank_episodes=RING)
    env.batch.set_stream_groups(2)
    env.set_early_end(success=True)
    _raise_cube(env, 1, 0.10)
    env.step(acts[0])
    x = _snap(env)
    for k in STATE:
        assert np.array_equal(x[k], s["auto"][k]), k
    assert np.array_equal(_patched(env), s["auto_ft"])
    for t in range(1, 4):
        env.step(acts[t])
        x = _snap(env)
        for k in STATE:
            assert np.array_equal(x[k], s["auto_next"][t - 1][k]), (t, k)
    # two half-batches stepped alternately: envs [3, 11] and [200, 7]
    ids4 = np.array([3, 11, 200, 7])
    g, cfg, flat = load_golden("seed1_full")
    alt = AlternatingVecEnv("Lift", 4, flat, cfg, env_ids=ids4, seed=0, horizon=HORIZON, bank_episodes=RING, terminate_on_success=True)
    alt.reset()
    _raise_cube(alt.halves[0].env, 1, 0.10)
    a4 = _acts(ids4, 4)
    log = []
    for t in range(4):
        alt.step_half(0, a4[t, :2]); alt.step_half(1, a4[t, 2:])
        rec = [alt.wait_half(k) for k in (0, 1)]
        log.append({"obs": torch.cat([r[0] for r in rec]).cpu().numpy(), "done": torch.cat([r[2] for r in rec]).cpu().numpy(),
                    "end_reason": torch.cat([r[3]["end_reason"] for r in rec]).cpu().numpy(), "terminal_obs": torch.cat([r[3]["terminal_obs"] for r in rec]).cpu().numpy()})
    want = [s["auto"]] + s["auto_next"]
    for t in range(4):
        for k in ("obs", "done", "end_reason"):
            assert np.array_equal(log[t][k][:3], want[t][k]), (t, k)
    assert log[0]["end_reason"].tolist() == [0, 2, 0, 0] and np.array_equal(log[0]["terminal_obs"][1], s["auto"]["terminal_obs"][1])


def test_host_controller_path_restarts_on_request():
    """HostControlledEnv (controllers evaluated in torch between rsim_step1 and rsim_step2): a requested end reaches the part controllers'
    reset_goal(mask) through `done`, and the env continues bitwise like a host-reset one."""
    from robosuite_amd import lift
    from robosuite_amd.controllers import HostControlledEnv
    from tests.test_controllers_plugin import _lift_joint_torque, _parts
    B = 4
    g, cfg, flat, task = _lift_joint_torque(B, horizon=HORIZON, bank=RING)
    _, _, _, ftask = _lift_joint_torque(B)
    env, fresh = HostControlledEnv(task, _parts(task, cfg, flat)[1]), HostControlledEnv(ftask, _parts(ftask, cfg, flat)[1])
    acts = torch.tensor(lift.env_actions(np.arange(B), 5, action_dim=8), device="cuda")
    env.reset(); env.step(acts[0]); env.step(acts[1])
    before = _snap(task)
    mask = torch.tensor([0, 1, 0, 0], dtype=torch.bool, device="cuda")
    obs = env.end_episodes(mask)
    fresh.reset(block=1)
    ftask.batch.observe()
    assert task.batch.get("done").tolist() == [0, 1, 0, 0] and task.batch.get("end_reason").tolist() == [0, 4, 0, 0] and env._restarted.tolist() == [False, True, False, False]
    assert np.array_equal(task.batch.get("qpos")[1], ftask.batch.get("qpos")[1]) and np.array_equal(obs.cpu().numpy()[1], ftask.batch.get("obs")[1])
    for k in ("qpos", "qvel", "obs", "ctrl", "time"):
        assert np.array_equal(task.batch.get(k)[[0, 2, 3]], before[k][[0, 2, 3]]), k
    for t in range(2, 5):
        env.step(acts[t]); fresh.step(acts[t])
        for k in ("qpos", "qvel", "obs", "ctrl"):
            assert np.array_equal(task.batch.get(k)[1], ftask.batch.get(k)[1]), (t, k)
    assert task.batch.get("ep_step").tolist() == [5, 3, 5, 5] and int(task.batch.get("bank_stale").sum()) == 0


def test_gym_face_reports_terminated_and_the_final_observation():
    from robosuite_amd.vec_env import GymVecEnv, VecEnv
    s = _scenario()
    g, cfg, flat = load_golden("seed1_full")
    venv = VecEnv("Lift", 3, flat, cfg, env_ids=IDS, seed=0, horizon=HORIZON, bank_episodes=RING, terminate_on_success=True)
    env = GymVecEnv(venv)
    env.reset()
    _raise_cube(venv.env, 1, 0.10)
    obs, rew, term, trunc, info = env.step(_acts(IDS, 1)[0])
    assert term.tolist() == [False, True, False] and trunc.tolist() == [False, False, False] and info["_final_observation"].tolist() == [False, True, False]
    assert info["end_reason"].tolist() == [0, 2, 0] and info["success"].tolist() == [0, 1, 0]
    flat_of = lambda rec: venv.flat_obs(torch.as_tensor(rec)).numpy()   # noqa: E731  (GymWrapper layout: object keys, then proprioception)
    assert np.array_equal(info["final_observation"].cpu().numpy()[1], flat_of(s["plain"]["obs"])[1]) and np.array_equal(obs.cpu().numpy(), flat_of(s["auto"]["obs"]))
    assert np.array_equal(rew.cpu().numpy(), s["plain"]["reward"])
    # the env's own reset clears the reason and re-arms the rule
    env.reset()
    assert not np.any(venv.env.batch.get("end_reason")) and venv.env.batch.get("ep_index").tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        VecEnv("Lift", 3, flat, cfg, env_ids=IDS, bank_episodes=0, terminate_on_success=True)
