"""CPU: the fp64 statement of the task epilogue (tests/epilogue_cases.py) pinned to the rewards the reference returned, and the caps on the constructed
cases that tests/test_epilogue.py holds the kernel to.  Nothing here touches the kernel.

Pin: for every step of the fixtures the five epilogue tests of tests/test_hip_parity.py use, the statement is evaluated on the oracle at the state whose
kinematics the reference sampled -- the last substep's, from `sub_qpos` where the fixture records it (Lift, TwoArmPegInHole), else after the oracle's own
replay of the control step, whose frames and contact list are still those of the last substep's position stage -- at the bounds of those tests.

Caps: every required branch fact is realised by the required number of cases; every compared quantity is 1e-3 off its threshold; every contact a case relies
on is 0.3 .. 1 mm deep; every "no grasp" / "not touching" case keeps the groups 1 mm apart by the fp64 distance mirror; every relative rotation is 0.05 off a
mat2quat branch switch and off w = 0; contacts and rows stay within the configuration's native capacity except in the named over-capacity cases; no case is
left out.
"""
import numpy as np
import pytest

from tests import epilogue_cases as ec
from tests.util import load_golden, make_oracle

PINS = (("lift_panda", "seed0_gentle", "lift", 1e-4), ("lift_panda", "seed1_full", "lift", 1e-4), ("stack_panda", "seed0_full", "stack", 1e-4),
        ("peg_baxter", "ctl_joint_torque", "peg", 2e-4), ("pickplace_iiwa", "seed0_full", "pickplace", 2e-4), ("pickplace_can_iiwa", "seed2_full", "pickplace", 2e-4))


@pytest.mark.parametrize("model,tag,task,bound", PINS)
def test_statement_matches_the_recorded_reference_rewards(model, tag, task, bound):
    g, cfg, flat = load_golden(tag, model)
    nq = flat.nq
    if task == "lift":
        info, statement = ec.panda_ids(flat, cfg, ["cube"]), ec.lift_statement
    elif task == "stack":
        info, statement = ec.panda_ids(flat, cfg, ["cubeA", "cubeB"]), ec.stack_statement
    elif task == "peg":
        info, statement = ec.peg_ids(flat), ec.peg_statement
    else:
        info, statement = ec.pickplace_ids(flat, cfg), ec.pickplace_statement
    n = len(g["actions"])
    worst = 0.0
    if "sub_qpos" in g.files:
        om, od, _ = make_oracle(flat)
        n_sub = len(g["sub_qpos"]) // n
        for t in range(n):
            ec.set_state(od, g["sub_qpos"][n_sub * t + n_sub - 1])          # the state the last substep's position stage saw
            r, s, _ = statement(info, od)
            worst = max(worst, abs(r - g["rewards"][t]))
            assert abs(r - g["rewards"][t]) < bound, (t, r, g["rewards"][t])
            assert not s                                                     # these fixtures never succeed (tests/test_hip_parity.py asserts 0 on the device)
    else:
        om, od, oc = make_oracle(flat, cfg)
        s0 = g["states"][0]
        od.qpos[:] = s0[1:1 + nq]; od.qvel[:] = s0[1 + nq:]; od.qacc_warmstart[:] = 0; od.ctrl[:] = 0; od.forward(); oc.reset(od)
        for t in range(n):
            oc.env_step(od, g["actions"][t], 25)                             # frames and contacts stay those of the last substep's position stage
            r, s, _ = statement(info, od)
            worst = max(worst, abs(r - g["rewards"][t]))
            assert abs(r - g["rewards"][t]) < bound, (t, r, g["rewards"][t])
            assert int(s) == (int(g["success"][t]) if "success" in g.files else 0), t
    print(f"{model} {tag}: {n} steps, worst |statement - recorded reward| {worst:.2e} (bound {bound:.0e})")


def _count(ev, cases, pred):
    return sum(1 for c, (r, s, f) in zip(cases, ev) if pred(f, s, c["want"]))


REQUIRED = {
    "lift": (("far reach", lambda f, s, w: not f["grasp"] and not f["lifted"] and f["dist"] > 0.15, 2),
             ("near reach without grasp", lambda f, s, w: not f["grasp"] and not f["lifted"] and f["dist"] < 0.08, 2),
             ("grasp below the margin", lambda f, s, w: f["grasp"] and not f["lifted"], 2),
             ("grasp above the margin", lambda f, s, w: f["grasp"] and s, 2),
             ("above the margin without the gripper", lambda f, s, w: not f["grasp"] and s and f["dist"] > 0.15, 2)),
    "stack": (("reach without grasp", lambda f, s, w: not f["grasp"] and not f["lifted"] and not f["touching"], 2),
              ("reach with grasp", lambda f, s, w: f["grasp"] and not f["lifted"], 2),
              ("lifted and far from cubeB", lambda f, s, w: f["lifted"] and not f["touching"] and f["dxy"] > 0.1, 2),
              ("lifted and aligned", lambda f, s, w: f["lifted"] and not f["touching"] and f["r_lift"] > 1.49, 2),
              ("stacked and released", lambda f, s, w: s and f["touching"] and not f["grasp"], 2),
              ("stacked, still grasped", lambda f, s, w: f["touching"] and f["grasp"] and f["lifted"] and not s, 2),
              ("touching, not lifted", lambda f, s, w: f["touching"] and not f["lifted"] and not f["grasp"] and not s, 2)),
    "peg": (("success", lambda f, s, w: s, 2), ("far", lambda f, s, w: f["d"] > 0.2, 2),
            ("only d fails", lambda f, s, w: f["checks"] == (False, True, True, True), 2), ("only t low fails", lambda f, s, w: f["checks"] == (True, False, True, True), 2),
            ("only t high fails", lambda f, s, w: f["checks"] == (True, True, False, True), 2), ("only cos fails", lambda f, s, w: f["checks"] == (True, True, True, False), 2)),
    "pickplace": (("nothing near", lambda f, s, w: f["nin"] == 0 and not any(f["near"]) and not any(f["inside"]) and not any(f["above"]) and not f["grasp"], 2),)
    + tuple((f"object {i} alone in its quadrant", lambda f, s, w, i=i: f["nin"] == 1 and f["in_bin"][i] and not any(f["near"]), 1) for i in range(4))
    + (("inside another object's quadrant, not counted", lambda f, s, w: f["nin"] == 0 and any(f["other_quadrant"]), 2),
       ("in its quadrant with the gripper near", lambda f, s, w: any(i and n for i, n in zip(f["inside"], f["near"])) and f["nin"] == 0, 2),
       ("over its target but above the bin", lambda f, s, w: f["nin"] == 0 and any(f["above"]) and not any(f["inside"]) and not f["grasp"], 2),
       ("two in", lambda f, s, w: f["nin"] == 2, 1), ("three in", lambda f, s, w: f["nin"] == 3, 1), ("all four in", lambda f, s, w: f["nin"] == 4 and s, 2),
       ("grasp at different heights", lambda f, s, w: f["grasp"] and f.get("zmin_from") in f["grasped"], 2),
       ("grasp while a closer object sets the reach distance", lambda f, s, w: f["grasp"] and f["reach_from"] not in f["grasped"], 1),
       ("grasp while another object sets the lift height", lambda f, s, w: f["grasp"] and f.get("zmin_from") not in f["grasped"], 1),
       ("ungrasped object above its target", lambda f, s, w: not f["grasp"] and any(f["above"]) and f["r_hover"] > 0.5, 2),
       ("grasped object beside the region above its target", lambda f, s, w: f["grasp"] and not any(f["above"]) and f["r_hover"] > f["r_lift"] + 0.02, 2),
       ("hover maximum from another object than the reach minimum", lambda f, s, w: f["active"] and f["hover_from"] != f["reach_from"], 2),
       ("an object in its bin closer to the gripper than every active one", lambda f, s, w: f["nin"] > 0 and f["active"] and min(f["dist"]) < min(f["dist"][i] for i in f["active"]) - 0.05, 2)),
    "pickplace_can": (("object in", lambda f, s, w: f["in_bin"][3] and s, 1), ("object out", lambda f, s, w: f["nin"] == 0 and not s, 2),
                      ("success on another object", lambda f, s, w: s and not f["in_bin"][3], 1), ("two in", lambda f, s, w: f["nin"] == 2, 1)),
    "pickplace_single": (("object in", lambda f, s, w: f["nin"] == 1 and s, 2), ("object out", lambda f, s, w: f["nin"] == 0 and not s, 2)),
}


@pytest.mark.parametrize("task", list(ec.TASKS))
def test_cases_realise_every_branch_within_the_caps(task):
    from robosuite_amd.backend import HipModel
    S = ec.TASKS[task]()
    flat, info, cases = S["flat"], S["info"], S["cases"]
    ev = ec.evaluate(S)
    lim = HipModel(flat).kernel_config()[1]
    om, od, _ = make_oracle(flat)
    assert len(ev) == len(cases) and 2 <= len(cases) <= 48
    for c, (r, s, f) in zip(cases, ev):
        for k, v in c["want"].items():                       # what the builder meant is what the statement finds
            if k in f:
                assert f[k] == v, (c["name"], k, f[k], v)
        for name, m in f["margins"]:
            assert m >= ec.MARGIN, (c["name"], name, m)
        assert f["ncon"] <= lim["ncon"] and f["nefc"] <= lim["nefc"], (c["name"], f["ncon"], f["nefc"])
        if task == "peg":
            continue
        ec.set_state(od, c["qpos"])
        active = f.get("active", [0])
        obj = [g for i in active for g in info["geoms"][i]] if task.startswith("pickplace") else info["geoms"][0]
        if f["grasp"]:
            assert all(ec.DEPTH[0] <= d <= ec.DEPTH[1] for d in f["pad_depths"]), (c["name"], f["pad_depths"])
        elif obj:
            # no grasp: both pad groups are 1 mm clear of the object geoms
            gaps = [ec.group_gap(flat, od, info[p], obj) for p in ("left_pad", "right_pad")]
            assert min(gaps) >= 1e-3, (c["name"], gaps)
        if task == "stack":
            if f["touching"]:
                assert ec.DEPTH[0] <= f["touch_depth"] <= ec.DEPTH[1], (c["name"], f["touch_depth"])
            else:
                assert ec.group_gap(flat, od, info["geoms"][0], info["geoms"][1]) >= 1e-3, c["name"]
    for label, pred, need in REQUIRED[task]:
        got = _count(ev, cases, pred)
        assert got >= need, (task, label, got, need)
    if task == "pickplace_single":                          # mode 1: two different RSIM_TASK_OBJECT values among the envs
        assert len({c["want"]["task_object"] for c in cases}) >= 2
    # the sparse and the half-scale forms: every case is run under every variant; sparse must see both outcomes
    sparse = ec.evaluate(S, 1.0, False)
    assert {s for _, s, _ in sparse} == {True, False} and {r > 0 for r, _, _ in sparse} == {True, False}
    for (r1, s1, _), (r2, s2, _) in zip(ev, ec.evaluate(S, 0.5, True)):
        assert s1 == s2 and abs(r2 - 0.5 * r1) < 1e-15
    if S["wide"] is not None:
        (r, s, f), = ec.evaluate(S, wide=True)
        assert f["ncon"] > lim["ncon"] or f["nefc"] > lim["nefc"], (f["ncon"], f["nefc"], lim)
        for k, v in S["wide"]["want"].items():
            assert f[k] == v, (S["wide"]["name"], k)
        # headroom: the device's box-box contact counts may differ from the oracle's by a point or two
        assert f["ncon"] >= lim["ncon"] + 3 or f["nefc"] >= lim["nefc"] + 9, (f["ncon"], f["nefc"], lim)


def test_relative_rotations_cover_every_mat2quat_branch():
    S = ec.pickplace_cases()
    seen = {}
    for c in S["cases"]:
        for q in c["want"].get("rel", []):
            R = ec.q2m(q)
            branch, dist, w = ec.mat2quat_branch(R)
            assert dist >= 0.05 and w >= 0.05, (c["name"], q, branch, dist, w)
            seen[branch] = seen.get(branch, 0) + 1
            x, y, z, w_ = ec.mat2quat_xyzw(R)
            assert np.abs(ec.q2m([w_, x, y, z]) - R).max() < 1e-12
    assert set(seen) == {0, 1, 2, 3} and sum(seen.values()) >= 6, seen
