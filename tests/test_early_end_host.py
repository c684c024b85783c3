"""Ending episodes early, host side (no GPU): the numpy mirror of k_end_episodes (robosuite_amd/episodes.py) on hand-made arrays, the gymnasium mapping
of RSIM_END_REASON, the reset ring's upkeep cadence once episodes can be shorter than the horizon, the new entries of the C-ABI, and the lock around
lift.prepared()'s cache (which the ring's upkeep threads share)."""
import os
import re
import threading

import numpy as np
import pytest

from robosuite_amd import episodes, lift
from tests.test_reset_bank_host import FakeTask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rsim.h")).read()
B, NQ, NV, NU, NOBS, E, NPAIR = 5, 4, 3, 2, 6, 3, 2


def _state(seed=0):
    r = np.random.default_rng(seed)
    f32 = lambda *shape: r.standard_normal(shape).astype(np.float32)   # noqa: E731
    return dict(done=np.zeros(B, np.int32), success=np.zeros(B, np.int32), ep_step=np.full(B, 7, np.int32), ep_index=np.array([0, 1, 2, 3, 4], np.int32),
                diverged=np.zeros(B, np.int32), seen_diverged=np.zeros(B, np.int32), end_reason=np.full(B, 9, np.int32), bank_stale=np.zeros(B, np.int32),
                needs_reset=np.zeros(B, np.int32), task_object=np.full(B, 3, np.int32), obs=f32(B, NOBS), terminal_obs=f32(B, NOBS), qpos=f32(B, NQ),
                qvel=f32(B, NV), qacc_warmstart=f32(B, NV), ctrl=f32(B, NU), time=f32(B), reward=f32(B), ft=f32(B, 10), ft_base=f32(B, 10),
                mprc=f32(B, NPAIR, 12), qfrc_applied=f32(B, NV), xfrc_applied=f32(B, 2, 6))


def _bank(seed=1):
    """Slot s of env e holds the episode above the env's own whose number is s modulo E -- a ring the host kept filled."""
    r = np.random.default_rng(seed)
    rows = r.standard_normal((B, E, NQ + 3)).astype(np.float32)
    rows[:, :, NQ + 1] = r.integers(0, 4, (B, E))          # the RSIM_PATCH_TASK_OBJECT column carries small integers
    tags = np.zeros((B, E), np.int32)
    for e in range(B):
        for k in range(e + 1, e + 1 + E):
            tags[e, k % E] = k
    return dict(rows=rows, tags=tags, patch_idx=np.array([7, episodes.PATCH_TASK_OBJECT, 2]))


def _untouched(before, after, envs, skip=("end_reason", "seen_diverged")):
    for k in before:
        if k not in skip:
            assert np.array_equal(before[k][envs], after[k][envs]), k


def test_mirror_restart_writes_what_the_horizon_branch_writes():
    s, bank = _state(), _bank()
    s["success"][:] = [1, 1, 0, 0, 0]
    s["done"][0] = 1                                        # env 0: restarted at the horizon by the step itself, success or not
    out = episodes.end_episodes_reference(s, bank, episodes.RULE_SUCCESS, applied=True)
    assert out["end_reason"].tolist() == [1, 2, 0, 0, 0]
    assert out["ep_index"].tolist() == [0, 2, 2, 3, 4]      # env 0 not restarted a second time: no episode skipped
    _untouched(s, out, [0, 2, 3, 4])
    row = bank["rows"][1, 2 % E]
    assert np.array_equal(out["qpos"][1], row[:NQ]) and np.array_equal(out["terminal_obs"][1], s["obs"][1]) and np.array_equal(out["obs"][1], s["obs"][1])
    for k in ("qvel", "qacc_warmstart", "ctrl", "time", "qfrc_applied", "xfrc_applied"):
        assert not np.any(out[k][1]), k
    assert out["ft"][1, 7] == row[NQ] and out["ft_base"][1, 7] == row[NQ] and out["ft"][1, 2] == row[NQ + 2] and out["ft_base"][1, 2] == row[NQ + 2]
    assert out["task_object"][1] == int(row[NQ + 1])        # the RSIM_PATCH_TASK_OBJECT column lands in task_object, not in the float table
    keep = [i for i in range(10) if i not in (2, 7)]
    assert np.array_equal(out["ft"][1, keep], s["ft"][1, keep])
    assert not np.any(out["mprc"][1, :, 3]) and np.array_equal(np.delete(out["mprc"][1], 3, axis=1), np.delete(s["mprc"][1], 3, axis=1))
    assert (out["ep_step"][1], out["done"][1], out["needs_reset"][1], out["bank_stale"][1]) == (0, 1, 1, 0)
    assert out["reward"][1] == s["reward"][1] and out["success"][1] == 1          # the terminal step's values stay
    # with the applied forces not read by the control step, a restart leaves them alone
    out2 = episodes.end_episodes_reference(s, bank, episodes.RULE_SUCCESS)
    assert np.array_equal(out2["qfrc_applied"], s["qfrc_applied"]) and np.array_equal(out2["xfrc_applied"], s["xfrc_applied"])
    assert not np.array_equal(s["qpos"][1], out["qpos"][1]) and s["ep_index"][1] == 1     # the input is not modified


def test_mirror_success_before_min_steps_is_ignored():
    s, bank = _state(), _bank()
    s["success"][:] = 1
    s["ep_step"][:] = [1, 2, 3, 4, 5]
    out = episodes.end_episodes_reference(s, bank, episodes.RULE_SUCCESS, min_steps=3)
    assert out["end_reason"].tolist() == [0, 0, 2, 2, 2] and out["done"].tolist() == [0, 0, 1, 1, 1]
    _untouched(s, out, [0, 1])
    assert episodes.end_episodes_reference(s, bank, 0, min_steps=1)["end_reason"].tolist() == [0] * B      # rule not armed


def test_mirror_cause_priority_and_divergence_bookkeeping():
    s, bank = _state(), _bank()
    s["success"][:] = [1, 0, 0, 1, 0]
    s["diverged"][:] = [2, 2, 0, 0, 0]
    s["seen_diverged"][:] = [1, 1, 0, 0, 0]
    mask = np.array([1, 1, 1, 0, 0], np.uint8)
    both = episodes.RULE_SUCCESS | episodes.RULE_DIVERGED
    out = episodes.end_episodes_reference(s, bank, both, mask)
    assert out["end_reason"].tolist() == [2, 3, 4, 2, 0]     # success before diverged before requested
    assert np.array_equal(out["seen_diverged"], s["diverged"])      # updated for every env on every launch
    again = dict(out, done=np.zeros(B, np.int32), success=np.zeros(B, np.int32))
    assert episodes.end_episodes_reference(again, bank, both)["end_reason"].tolist() == [0] * B     # a guard hit ends one episode, not every later one
    # only the divergence rule armed: success is not a cause
    assert episodes.end_episodes_reference(s, bank, episodes.RULE_DIVERGED, mask)["end_reason"].tolist() == [3, 3, 4, 0, 0]
    # outside a control step the mask alone decides; done / end_reason of the other envs stay
    s["done"][:] = [0, 0, 0, 1, 0]
    alone = episodes.end_episodes_reference(s, bank, both, mask, standalone=True)
    assert alone["end_reason"].tolist() == [4, 4, 4, 9, 9] and alone["done"].tolist() == [1, 1, 1, 1, 0] and alone["ep_index"].tolist() == [1, 2, 3, 3, 4]
    assert np.array_equal(alone["seen_diverged"], s["seen_diverged"])
    _untouched(s, alone, [3, 4], skip=())


def test_mirror_counts_a_stale_slot_and_still_uses_it():
    s, bank = _state(), _bank()
    bank["tags"][2, 3 % E] = 0                              # env 2 is about to start episode 3; its slot still holds episode 0
    out = episodes.end_episodes_reference(s, bank, 0, np.array([0, 0, 1, 1, 0]))
    assert out["bank_stale"].tolist() == [0, 0, 1, 0, 0] and out["end_reason"].tolist() == [0, 0, 4, 4, 0]
    assert np.array_equal(out["qpos"][2], bank["rows"][2, 3 % E, :NQ])


class _StubVecEnv:
    """What GymVecEnv needs of a VecEnv."""
    n_envs, action_dim, obs_dim = 5, 7, 4
    action_spec = (-np.ones(7), np.ones(7))

    def __init__(self, armed, reason):
        self.early_end_armed, self._reason = armed, reason

    def flat_obs(self, obs, keys=None):
        return obs

    def step(self, actions):
        torch = pytest.importorskip("torch")
        reason = torch.tensor(self._reason, dtype=torch.int32)
        info = {"success": reason == 2, "terminal_obs": torch.zeros(5, 4)}
        if self.early_end_armed:
            info["end_reason"] = reason
        return torch.zeros(5, 4), torch.zeros(5), (reason > 0).to(torch.int32), info


def test_gym_face_maps_the_end_reason():
    torch = pytest.importorskip("torch")
    from robosuite_amd.vec_env import GymVecEnv, gym_flags
    reason = [0, 1, 2, 3, 4]
    obs, rew, term, trunc, info = GymVecEnv(_StubVecEnv(True, reason)).step(None)
    assert term.tolist() == [False, False, True, False, True] and trunc.tolist() == [False, True, False, True, False]
    assert info["_final_observation"].tolist() == [False, True, True, True, True] and info["end_reason"].tolist() == reason
    # not armed: as ever -- `done` is passed on as terminated, nothing is truncated, no new key
    obs, rew, term, trunc, info = GymVecEnv(_StubVecEnv(False, reason)).step(None)
    assert term.tolist() == [False, True, True, True, True] and not trunc.any() and sorted(info) == ["_final_observation", "final_observation", "success"]
    t, u = gym_flags(np.array(reason))
    assert t.tolist() == [False, False, True, False, True] and u.tolist() == [False, True, False, True, False]


class _CountingTask(FakeTask):
    refills = 0

    def refill_bank(self):
        self.refills += 1
        return super().refill_bank()


def test_ring_upkeep_cadence_follows_the_shortest_possible_episode():
    # not armed: exactly the parent's rule -- sync below a horizon of 32, every horizon // 2 steps when synchronous, horizon // 4 otherwise
    for horizon, want in ((4, (True, 2)), (40, (False, 10)), (500, (False, 125))):
        t = FakeTask(3, horizon)
        t.install_reset_bank(4)
        assert t.early_min_steps == 0 and t._bank_cadence() == want, horizon
    # armed with min_steps = 1 and a ring of 4: three stored episodes last three steps -- synchronous upkeep, every step
    t = _CountingTask(3, 500)
    t.install_reset_bank(4)
    t.early_min_steps = 1
    assert t._bank_cadence() == (True, 1)
    for _ in range(5):
        t._bank_tick()
    assert t.refills == 5 and getattr(t, "_bank_thread", None) is None
    # longer minimum episodes buy slack back; the horizon still bounds it
    t.early_min_steps = 50
    assert t._bank_cadence() == (False, 150 // 4)
    t.early_min_steps = 400
    assert t._bank_cadence() == (False, 125)
    # the invariant: no reset finds a stale slot although every env ends its episode on every step
    t = FakeTask(4, 500)
    t.install_reset_bank(2)
    t.early_min_steps = 1
    for _ in range(40):
        t.batch.device_reset(range(4))
        t._bank_tick()
    assert t.batch.stale.sum() == 0 and t.batch.ep_index.tolist() == [40] * 4


def test_new_entries_are_declared_exported_and_bound():
    from robosuite_amd import backend
    assert re.search(r"int rsim_set_early_end\(rsim_batch\* b, int rules, int min_steps\);", HEADER)
    assert re.search(r"int rsim_end_episodes\(rsim_batch\* b, const uint8_t\* mask_dev\);", HEADER)
    body = HEADER[HEADER.index("enum rsim_field {"):]
    body = re.sub(r"/\*.*?\*/", "", body[:body.index("};")], flags=re.S)
    names = re.findall(r"\b(RSIM_[A-Z_]+)\b", body)
    assert names[-2:] == ["RSIM_END_REASON", "RSIM_FIELD_COUNT"] and names[-3] == "RSIM_XFRC_APPLIED"     # appended: no existing value moves
    assert backend.FIELD_ID["end_reason"] == len(names) - 2 == len(backend.FIELDS) and "end_reason" in backend.INT_FIELDS
    lib = os.path.join(ROOT, "robosuite_amd", "librsim_hip.so")
    if os.path.exists(lib):
        L = backend.lib()
        assert hasattr(L, "rsim_set_early_end") and hasattr(L, "rsim_end_episodes")
        # a per-batch switch, off unless armed: the string the PMC evidence is keyed to is what it was
        assert b"early" not in L.rsim_tuning_defaults()


def test_prepared_cache_survives_two_threads():
    """lift.prepared() is called from the stepping thread and from every env's ring-upkeep thread; its LRU reshuffle (delete, re-insert, evict) is
    guarded by a lock.  Two threads walking more specs than the cache holds: every call returns its own spec's arrays, nothing raises, the bound holds."""
    specs = [dict(arm_init_qpos=[float(i)] * 7, cube=dict(size_min=[0.02 + i * 1e-4] * 3, size_max=[0.03] * 3)) for i in range(lift._PREPARED_MAX + 8)]
    errors = []

    def hammer(order):
        try:
            for _ in range(30):
                for i in order:
                    p = lift.prepared(specs[i])
                    if p["arm"][0] != float(i) or p["size_min"][0] != 0.02 + i * 1e-4:
                        errors.append(("wrong entry", i))
        except Exception as exc:   # noqa: BLE001
            errors.append(exc)

    n = len(specs)
    threads = [threading.Thread(target=hammer, args=(list(range(n)),)), threading.Thread(target=hammer, args=(list(range(n - 1, -1, -1)),))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert errors == [] and len(lift._PREPARED) <= lift._PREPARED_MAX
    assert isinstance(lift._PREPARED_LOCK, type(threading.Lock()))
