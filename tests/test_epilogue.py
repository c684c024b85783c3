"""-m gpu: the observation / reward / success epilogue of the step kernels (Sim::obs_reward, csrc/rsim_step.hip) against the fp64 statement of
tests/epilogue_cases.py at constructed states that realise every reward and success branch (tests/test_epilogue_host.py holds the statement and the cases).

Per task one batch of B cases, run under every (reward_scale, reward_shaping) variant:
  debug path   set(qpos, qvel = 0), rsim_observe: reward, success, the Peg scalars
  fused path   forward, ctrl_reset, ONE control_step(zero action, n_sub = 1), in a batch created normally (the plain kernel) and in one created under
               RSIM_FULL_STEP_KERNEL=1: the epilogue reads the frames and the contact list of that substep's position stage, i.e. of the constructed state
Before rewards are compared the device's own contact list must give the oracle's grasp / touching facts: a mismatch there is a narrow-phase finding.

Bounds: success and the integers the reward carries (objects in bins, the 2.25 / 2 / 1 plateaus) exact; reward 1e-4 (Lift, Stack) and 2e-4 (TwoArmPegInHole,
PickPlace) -- the bounds the fixture comparisons of tests/test_hip_parity.py hold against the reference, now at the same state, where the reasoned error is a
frame error of 2e-6 times a slope of at most 15 plus fp32 tanhf; Peg scalars, relative positions and quaternions 5e-4, the observation bound.
"""
import numpy as np
import pytest
import torch

from tests import epilogue_cases as ec

pytestmark = pytest.mark.gpu

BOUND = {"lift": 1e-4, "stack": 1e-4, "peg": 2e-4, "pickplace": 2e-4, "pickplace_can": 2e-4, "pickplace_single": 2e-4}
NORM = {"lift": 2.25, "stack": 2.0, "peg": 5.0, "pickplace": 4.0, "pickplace_can": 1.0, "pickplace_single": 1.0}
OBS_BOUND = 5e-4


def _task_desc(task, flat, cfg, scale, shaping):
    from robosuite_amd import lift, peg_in_hole, pick_place, stack
    build = {"lift": lift.lift_task, "stack": stack.stack_task, "peg": peg_in_hole.peg_task}.get(task, pick_place.pick_place_task)
    return build(flat, cfg, reward_scale=scale, reward_shaping=shaping)


def _batch(task, S, scale, shaping, B, full, monkeypatch):
    from robosuite_amd.backend import HipBatch, HipModel
    hm = HipModel(S["flat"])
    hm.set_controller(S["cfg"])
    hm.set_task(_task_desc(task, S["flat"], S["cfg"], scale, shaping))
    if full:
        monkeypatch.setenv("RSIM_FULL_STEP_KERNEL", "1")
    try:
        hb = HipBatch(hm, B, 0, False)
    finally:
        if full:
            monkeypatch.delenv("RSIM_FULL_STEP_KERNEL")
    return hm, hb


def _set(hb, qpos, task_objects=None):
    hb.set("qpos", qpos); hb.set("qvel", 0); hb.set("qacc_warmstart", 0); hb.set("ctrl", 0)
    if task_objects is not None:
        hb.set("task_object", np.asarray(task_objects, dtype=np.int32))


def _one_substep(hm, hb):
    hb.forward(); hb.ctrl_reset()
    hb.control_step(torch.zeros(hb.B, hm.action_dim, dtype=torch.float32, device="cuda"), 1)
    assert int(np.abs(hb.get("diverged")).sum()) == 0 and int(np.abs(hb.get("overflow")).sum()) == 0
    return hb.get("reward").astype(np.float64), hb.get("success"), hb.get("obs").astype(np.float64)


def _device_contact_facts(task, S, hb, ev):
    """the oracle's grasp / touching facts from the device's own contact list, case by case"""
    info = S["info"]
    ncon, rec = hb.get("ncon"), hb.get("contact")
    for e, (c, (_, _, f)) in enumerate(zip(S["cases"], ev)):
        if "grasp" not in f:
            continue
        pairs = {}
        for r in rec[e][:ncon[e]]:
            k = (min(int(r[13]), int(r[14])), max(int(r[13]), int(r[14])))
            pairs[k] = max(pairs.get(k, -np.inf), -float(r[0]))
        obj = [g for i in f.get("active", [0]) for g in info["geoms"][i]] if task.startswith("pickplace") else info["geoms"][0]
        left, right = ec.group_depth(pairs, info["left_pad"], obj), ec.group_depth(pairs, info["right_pad"], obj)
        assert (left is not None and right is not None) == f["grasp"], \
            f"narrow phase, not epilogue: {c['name']}: device pad depths {left}, {right} against the oracle's {f['pad_depths']}"
        if task == "stack":
            touch = ec.group_depth(pairs, info["geoms"][0], info["geoms"][1])
            assert (touch is not None) == f["touching"], f"narrow phase, not epilogue: {c['name']}: device cubeA-cubeB depth {touch} against the oracle's {f['touch_depth']}"


def _compare(task, scale, shaping, path, S, ev, reward, success, worst):
    norm = NORM[task]
    for e, (c, (r, s, f)) in enumerate(zip(S["cases"], ev)):
        tag = (task, path, scale, shaping, c["name"])
        assert int(success[e]) == int(s), (tag, int(success[e]), s)
        raw = reward[e] * norm / scale                     # the reference's sum before normalisation: its integer part is the plateau
        if task.startswith("pickplace"):
            assert int(np.floor(raw + 1e-3)) == int(f["plateau"]), (tag, raw, f["plateau"])
        if f["plateau"] > 0 and (task in ("lift", "stack") or not shaping):
            assert reward[e] == np.float32(f["plateau"] * (5.0 if task == "peg" else 1.0) * scale / norm), (tag, reward[e], f["plateau"])
        err = abs(reward[e] - r)
        worst[path] = max(worst.get(path, 0.0), err)
        assert err < BOUND[task], (tag, reward[e], r)


def _obs_slices(cfg):
    dims = np.cumsum([0] + cfg["obs_dims"])
    return {k: slice(dims[i], dims[i + 1]) for i, k in enumerate(cfg["obs_keys"])}


def _compare_peg_scalars(S, ev, obs, worst, path):
    sl = _obs_slices(S["cfg"])
    for e, (_, _, f) in enumerate(ev):
        got = np.array([obs[e][sl["angle"]][0], obs[e][sl["t"]][0], obs[e][sl["d"]][0]])
        err = np.abs(got - (f["cos"], f["t"], f["d"])).max()
        worst[path + " scalars"] = max(worst.get(path + " scalars", 0.0), err)
        assert err < OBS_BOUND, (path, S["cases"][e]["name"], got, f["cos"], f["t"], f["d"])


def _compare_relative_pose(task, S, ev, obs0, obs1, worst, path):
    """obs0: the record rsim_observe left (relative entries zero, object poses cached); obs1: the record of the control step after it"""
    info, sl = S["info"], _obs_slices(S["cfg"])
    names = S["cfg"]["task"]["objects"]
    for e, (c, (_, _, f)) in enumerate(zip(S["cases"], ev)):
        fr = f["frames"]
        if task == "pickplace":
            keys = [(i, n) for i, n in enumerate(names)]
        elif task == "pickplace_can":
            keys = [(3, "Can")]
        else:
            keys = [(int(c["want"]["task_object"]), "obj")]
            assert obs1[e][sl["obj_id"]][0] == c["want"]["task_object"] and obs0[e][sl["obj_id"]][0] == c["want"]["task_object"]
        for i, n in keys:
            kp, kq = f"{n}_to_robot0_eef_pos", f"{n}_to_robot0_eef_quat"
            assert np.all(obs0[e][sl[kp]] == 0) and np.all(obs0[e][sl[kq]] == 0), (path, c["name"], n)
            b = info["bodies"][i]
            cached_p, cached_q = obs0[e][sl[f"{n}_pos"]], obs0[e][sl[f"{n}_quat"]]
            wxyz = fr["xquat"][4 * b:4 * b + 4]
            assert np.abs(cached_p - fr["xpos"][3 * b:3 * b + 3]).max() < OBS_BOUND and np.abs(cached_q - wxyz[[1, 2, 3, 0]]).max() < OBS_BOUND, (path, c["name"], n)
            hand = info["hand"]
            rp, rq = ec.rel_pose_statement(fr["xquat"][4 * hand:4 * hand + 4], fr["site_xpos"][3 * info["site"]:3 * info["site"] + 3], cached_p, cached_q)
            gp, gq = obs1[e][sl[kp]], obs1[e][sl[kq]]
            assert gq[3] >= 0, (path, c["name"], n, gq)                      # canonical w >= 0
            ep, eq = np.abs(gp - rp).max(), min(np.abs(gq - rq).max(), np.abs(gq + rq).max())
            worst[path + " rel pos"] = max(worst.get(path + " rel pos", 0.0), ep)
            worst[path + " rel quat"] = max(worst.get(path + " rel quat", 0.0), eq)
            assert ep < OBS_BOUND and eq < OBS_BOUND, (path, c["name"], n, gp, rp, gq, rq)


@pytest.mark.parametrize("task", list(ec.TASKS))
def test_epilogue_matches_the_statement_on_every_branch(task, monkeypatch):
    S = ec.TASKS[task]()
    qpos = np.array([c["qpos"] for c in S["cases"]])
    B = len(qpos)
    tobj = [c["want"]["task_object"] for c in S["cases"]] if task == "pickplace_single" else None
    for scale, shaping in ec.VARIANTS:
        ev = ec.evaluate(S, scale, shaping)
        worst = {}
        for full in (False, True):
            hm, hb = _batch(task, S, scale, shaping, B, full, monkeypatch)
            path = "fused full" if full else "fused plain"
            _set(hb, qpos, tobj)
            hb.observe()
            obs0 = hb.get("obs").astype(np.float64)
            if not full:
                _device_contact_facts(task, S, hb, ev)
                _compare(task, scale, shaping, "debug", S, ev, hb.get("reward").astype(np.float64), hb.get("success"), worst)
                if task == "peg":
                    _compare_peg_scalars(S, ev, obs0, worst, "debug")
            reward, success, obs1 = _one_substep(hm, hb)
            _compare(task, scale, shaping, path, S, ev, reward, success, worst)
            if task == "peg":
                _compare_peg_scalars(S, ev, obs1, worst, path)
            if task.startswith("pickplace"):
                _compare_relative_pose(task, S, ev, obs0, obs1, worst, path)
        print(f"{task} scale {scale} shaping {int(shaping)} B {B}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items())
              + f"  (bounds: reward {BOUND[task]:.0e}, observations {OBS_BOUND:.0e})")


@pytest.mark.parametrize("task", ("lift", "stack"))
def test_epilogue_of_the_wide_body_with_the_fingers_closed_on_the_cube(task, monkeypatch):
    """More contacts / rows than the native body carries: the env is handed to the fused wide body, whose copy of the epilogue decides the reward."""
    S = ec.TASKS[task]()
    (r, s, f), = ec.evaluate(S, wide=True)
    base = S["cases"][0]["qpos"]
    for full in (False, True):
        hm, hb = _batch(task, S, 1.0, True, 2, full, monkeypatch)
        lim = hm.kernel_config()[1]
        _set(hb, np.array([base, base]))
        hb.forward(); hb.ctrl_reset()                                        # the controller starts from a state within the native capacity
        _set(hb, np.array([S["wide"]["qpos"]] * 2))
        hb.control_step(torch.zeros(2, hm.action_dim, dtype=torch.float32, device="cuda"), 1)
        need = hb.get("cap_need")
        assert np.all((need[:, 0] > lim["ncon"]) | (need[:, 1] > lim["nefc"])), (need, lim)
        assert int(np.abs(hb.get("overflow")).sum()) == 0 and int(np.abs(hb.get("diverged")).sum()) == 0
        reward, success = hb.get("reward").astype(np.float64), hb.get("success")
        print(f"{task} wide body ({'full' if full else 'plain'} kernel): needs {need[0].tolist()} of {lim['ncon']} / {lim['nefc']}, oracle {f['ncon']} / {f['nefc']}, "
              f"|reward - statement| {np.abs(reward - r).max():.2e} (bound {BOUND[task]:.0e})")
        assert np.all(success == int(s)) and np.abs(reward - r).max() < BOUND[task], (reward, r, success, s)
