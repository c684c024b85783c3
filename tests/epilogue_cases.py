"""Constructed states for the observation / reward / success epilogue (Sim::obs_reward, csrc/rsim_step.hip) and the fp64 statement they are held to.

The statement: one function per task that reads oracle data after forward() (xpos, xquat, site_xpos, contacts()) and returns (reward, success, branch facts),
written from the reference's formulas as include/rsim.h cites them -- Lift.reward / _check_success (lift.py:224-273, 433-444), Stack.staged_rewards
(stack.py:268-312), TwoArmPegInHole._compute_orientation / reward (two_arm_peg_in_hole.py:240-290, 513-560), PickPlace.staged_rewards / not_in_bin /
_check_success (pick_place.py:274-429, 737-762) -- and the relative-pose sensors of PickPlace (manipulation_env.py:244-303).  numpy float64, no device call.

The cases: qpos rows (qvel = 0) built on the CPU oracle from fixture states.  Objects are teleported through their free joints, grasps close the fingers by
bisection until both pad contacts are 0.3 .. 1 mm deep, arm poses are damped least-squares updates on oracle Jacobians.  tests/test_epilogue_host.py pins the
statement to the recorded reference rewards and asserts the caps on the cases; tests/test_epilogue.py holds the kernel to the statement at these states.
"""
import functools

import numpy as np

from robosuite_amd import distance
from tests.util import load_golden, make_oracle

MARGIN = 1e-3                 # every compared quantity stays this far from its threshold (device frames are good to 2e-6)
DEPTH = (3e-4, 1e-3)          # a contact a case relies on is this deep
VARIANTS = ((1.0, True), (1.0, False), (0.5, True))   # (reward_scale, reward_shaping) every task batch is run under


# ---- small fp64 helpers --------------------------------------------------------------------------------------------------------------------
def q2m(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def qmul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw])


def axis_quat(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a / np.linalg.norm(a)])


def mat2quat_xyzw(R):
    """transform_utils.mat2quat up to sign, canonical w >= 0: the eigenvector of the largest eigenvalue of the symmetric 4 x 4 matrix built from R
    (Bar-Itzhack), which has no branches to get wrong."""
    m = np.asarray(R, dtype=np.float64)
    K = np.array([[m[0, 0] - m[1, 1] - m[2, 2], 0, 0, 0], [m[0, 1] + m[1, 0], m[1, 1] - m[0, 0] - m[2, 2], 0, 0],
                  [m[0, 2] + m[2, 0], m[1, 2] + m[2, 1], m[2, 2] - m[0, 0] - m[1, 1], 0],
                  [m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1], m[0, 0] + m[1, 1] + m[2, 2]]]) / 3.0
    w, V = np.linalg.eigh(K)
    q = V[:, np.argmax(w)]
    return q if q[3] >= 0 else -q


def mat2quat_branch(R):
    """(branch the textbook mat2quat takes: 0 trace, 1 x, 2 y, 3 z; distance of the rotation from the nearest branch switch; |w|)"""
    m = np.asarray(R, dtype=np.float64)
    tr, d = np.trace(m), np.diag(m)
    if tr > 0:
        return 0, tr, abs(mat2quat_xyzw(m)[3])
    k = int(np.argmax(d))
    others = [d[j] for j in range(3) if j != k]
    return 1 + k, min(-tr, d[k] - max(others)), abs(mat2quat_xyzw(m)[3])


def rel_pose_statement(eef_quat, grip, o_pos, o_quat_xyzw):
    """{obj}_to_eef_pos / _quat: pose of the object (as cached, quaternion xyzw) in the frame {grip site position, eef body orientation}."""
    Re = q2m(eef_quat)
    x, y, z, w = o_quat_xyzw
    Ro = q2m([w, x, y, z])
    return Re.T @ (np.asarray(o_pos, dtype=np.float64) - grip), mat2quat_xyzw(Re.T @ Ro)


# ---- oracle access -------------------------------------------------------------------------------------------------------------------------
def set_state(od, qpos):
    od.qpos[:] = qpos; od.qvel[:] = 0; od.qacc_warmstart[:] = 0; od.ctrl[:] = 0
    od.forward()


def contact_depths(od):
    """{(geom a, geom b) with a < b: deepest penetration (m, positive) among the oracle's contacts of that pair}"""
    out = {}
    for c in od.contacts():
        k = (min(c["geom1"], c["geom2"]), max(c["geom1"], c["geom2"]))
        out[k] = max(out.get(k, -np.inf), -c["dist"])
    return out


def group_depth(depths, ga, gb):
    """deepest contact between geom groups ga and gb, None when they share no contact"""
    d = [v for (a, b), v in depths.items() if (a in ga and b in gb) or (a in gb and b in ga)]
    return max(d) if d else None


def group_gap(flat, od, ga, gb):
    """smallest distance between two geom groups by the fp64 mirror (0 when they overlap)"""
    pairs = [(a, b) for a in ga for b in gb]
    return float(distance.geom_distance(flat, od.xpos, od.xquat, pairs, distmax=0.5)[0].min())


def body_p(od, b):
    return np.array(od.xpos[3 * b:3 * b + 3])


def body_q(od, b):
    return np.array(od.xquat[4 * b:4 * b + 4])


def site_p(od, s):
    return np.array(od.site_xpos[3 * s:3 * s + 3])


def geom_p(od, g):
    return np.array(od.geom_xpos[3 * g:3 * g + 3])


def move_site(od, qpos, site, target, dofs, iters=60, damping=1e-3, cap=0.2):
    """damped least squares on the oracle's site Jacobian: joints `dofs` (qpos address = dof address) until `site` is at `target`"""
    q = np.array(qpos, dtype=np.float64)
    for _ in range(iters):
        set_state(od, q)
        e = np.asarray(target) - site_p(od, site)
        if np.linalg.norm(e) < 1e-10:
            break
        J = od.jac("site", site)[0][:, dofs]
        dq = J.T @ np.linalg.solve(J @ J.T + damping * np.eye(3), e)
        n = np.abs(dq).max()
        q[dofs] += dq * min(1.0, cap / n) if n > 0 else 0
    set_state(od, q)
    return q


def put_free(qpos, adr, pos, quat):
    qpos[adr:adr + 3] = pos
    qpos[adr + 3:adr + 7] = np.asarray(quat) / np.linalg.norm(quat)


def close_fingers(od, qpos, fingers, place, lpad, rpad, obj, lo, hi, target=6.5e-4):
    """Bisection on the finger closure c in [lo (open), hi (closed)]: `fingers(q, c)` writes the finger joints, `place(od, q)` teleports the object between
    the pads of the pose just set; until the shallower of the two pad contacts is `target` deep.  Returns the qpos row."""
    def depth(c):
        q = np.array(qpos, dtype=np.float64)
        fingers(q, c)
        set_state(od, q)
        place(od, q)
        set_state(od, q)
        d = contact_depths(od)
        a, b = group_depth(d, lpad, obj), group_depth(d, rpad, obj)
        return q, (-1.0 if a is None or b is None else min(a, b))
    for _ in range(40):
        c = 0.5 * (lo + hi)
        q, d = depth(c)
        if abs(d - target) < 5e-5:
            break
        lo, hi = (c, hi) if d < target else (lo, c)
    return q


# ---- the statement -------------------------------------------------------------------------------------------------------------------------
def _margin(facts, name, value, threshold):
    facts["margins"].append((name, abs(float(value) - threshold)))


def _grasp(info, depths, obj_geoms, facts):
    a, b = group_depth(depths, info["left_pad"], obj_geoms), group_depth(depths, info["right_pad"], obj_geoms)
    facts["pad_depths"] = (a, b)
    return a is not None and b is not None


def panda_ids(flat, cfg, objects):
    n = flat.names
    return dict(site=int(cfg["eef_site"]), hand=n["body"].index("robot0_right_hand"), left_pad=[n["geom"].index("gripper0_right_finger1_pad_collision")],
                right_pad=[n["geom"].index("gripper0_right_finger2_pad_collision")], table_height=float(cfg.get("table_height", 0.8)),
                bodies=[n["body"].index(f"{o}_main") for o in objects], geoms=[[n["geom"].index(f"{o}_g0")] for o in objects],
                qadr=[int(flat.jnt_qposadr[n["joint"].index(f"{o}_joint0")]) for o in objects])


def lift_statement(info, od, scale=1.0, shaping=True):
    """Lift.reward (lift.py:224-273): 2.25 on success, else reaching 1 - tanh(10 d) + 0.25 for a grasp; x scale / 2.25.  Success: cube above table + 0.04."""
    facts = dict(margins=[])
    cube, grip = body_p(od, info["bodies"][0]), site_p(od, info["site"])
    facts["grasp"] = _grasp(info, contact_depths(od), info["geoms"][0], facts)
    facts["lifted"] = success = bool(cube[2] > info["table_height"] + 0.04)
    _margin(facts, "cube height", cube[2], info["table_height"] + 0.04)
    facts["dist"] = float(np.linalg.norm(cube - grip))
    r = 0.0
    if success:
        r = 2.25
    elif shaping:
        r = 1 - np.tanh(10.0 * facts["dist"]) + (0.25 if facts["grasp"] else 0.0)
    facts["plateau"] = 2.25 if success else 0.0
    return r * scale / 2.25, success, facts


def stack_statement(info, od, scale=1.0, shaping=True):
    """Stack.staged_rewards (stack.py:268-312): max(reach + grasp, lift + align, stack) x scale / 2; sparse: the stack term alone.  Success: r_stack > 0."""
    facts = dict(margins=[])
    A, B, grip = body_p(od, info["bodies"][0]), body_p(od, info["bodies"][1]), site_p(od, info["site"])
    depths = contact_depths(od)
    facts["grasp"] = grasp = _grasp(info, depths, info["geoms"][0], facts)
    facts["touch_depth"] = group_depth(depths, info["geoms"][0], info["geoms"][1])
    facts["touching"] = touching = facts["touch_depth"] is not None
    facts["dist"] = float(np.linalg.norm(A - grip))
    r_reach = (1 - np.tanh(10.0 * facts["dist"])) * 0.25 + (0.25 if grasp else 0.0)
    facts["lifted"] = lifted = bool(A[2] > info["table_height"] + 0.04)
    _margin(facts, "cubeA height", A[2], info["table_height"] + 0.04)
    facts["dxy"] = float(np.linalg.norm(A[:2] - B[:2]))
    r_lift = 1.0 + 0.5 * (1 - np.tanh(facts["dxy"])) if lifted else 0.0
    r_stack = 2.0 if (not grasp and r_lift > 0 and touching) else 0.0
    facts["r_lift"], facts["plateau"] = r_lift, r_stack
    r = max(r_reach, r_lift, r_stack) if shaping else r_stack
    return r * scale / 2.0, r_stack > 0, facts


def peg_ids(flat):
    b = flat.names["body"]
    return dict(peg=b.index("peg_main"), hole=b.index("hole_main"))


def peg_scalars(od, info):
    """TwoArmPegInHole._compute_orientation (two_arm_peg_in_hole.py:523-560) -> (t, d, cos)"""
    Rp, Rh = q2m(body_q(od, info["peg"])), q2m(body_q(od, info["hole"]))
    pp, hp = body_p(od, info["peg"]), body_p(od, info["hole"])
    v = Rp @ np.array([0.0, 0.0, 1.0])
    v /= np.linalg.norm(v)
    center = hp + Rh @ np.array([0.1, 0.0, 0.0])
    t = (center - pp) @ v / np.linalg.norm(v) ** 2
    d = np.linalg.norm(np.cross(v, pp - center)) / np.linalg.norm(v)
    hn = Rh @ np.array([0.0, 0.0, 1.0])
    return float(t), float(d), float(abs(hn @ v / np.linalg.norm(hn) / np.linalg.norm(v)))


def peg_statement(info, od, scale=1.0, shaping=True):
    """TwoArmPegInHole.reward (two_arm_peg_in_hole.py:240-290): success (d < 0.06, -0.12 <= t <= 0.14, cos > 0.95) + reaching + perpendicular + parallel + alignment
    terms, x scale / 5; sparse: 5 x success."""
    facts = dict(margins=[])
    t, d, c = peg_scalars(od, info)
    facts.update(t=t, d=d, cos=c, checks=(d < 0.06, t >= -0.12, t <= 0.14, c > 0.95))
    for name, v, th in (("d", d, 0.06), ("t low", t, -0.12), ("t high", t, 0.14), ("cos", c, 0.95)):
        _margin(facts, name, v, th)
    success = all(facts["checks"])
    r = 1.0 if success else 0.0
    if shaping:
        dist = np.linalg.norm(body_p(od, info["peg"]) - body_p(od, info["hole"]))
        r += (1 - np.tanh(dist)) + (1 - np.tanh(d)) + (1 - np.tanh(abs(t))) + c
    else:
        r *= 5.0
    facts["plateau"] = 1.0 if success else 0.0
    return r * scale / 5.0, success, facts


def pickplace_ids(flat, cfg):
    n, t = flat.names, cfg["task"]
    return dict(site=n["site"].index(t["grip_site"]), hand=n["body"].index(t["eef_body"]), left_pad=[n["geom"].index(g) for g in t["left_pad"]],
                right_pad=[n["geom"].index(g) for g in t["right_pad"]], bodies=[n["body"].index(b) for b in t["object_bodies"]],
                geoms=[[n["geom"].index(g) for g in gs] for gs in t["object_geoms"]], qadr=[int(o["qposadr"]) for o in t["placement"]["objects"]],
                bin2_pos=np.array(t["bin2_pos"], dtype=np.float64), bin_size=np.array(t["bin_size"], dtype=np.float64),
                targets=np.array(t["target_bin_placements"], dtype=np.float64), single=int(t.get("single_object_mode", 0)))


def pickplace_statement(info, od, scale=1.0, shaping=True):
    """PickPlace._check_success / not_in_bin / staged_rewards / reward (pick_place.py:274-429, 737-762)."""
    facts = dict(margins=[])
    bp, bs, n = info["bin2_pos"], info["bin_size"], len(info["bodies"])
    grip = site_p(od, info["site"])
    pos = [body_p(od, b) for b in info["bodies"]]
    dist = [float(np.linalg.norm(grip - p)) for p in pos]
    inside, in_bin, elsewhere = [], [], []

    def bounds(j):                    # not_in_bin (pick_place.py:403-429): the quadrant of bin 2 that belongs to object j
        xl, yl = bp[0], bp[1]
        if j in (0, 2):
            xl -= bs[0] / 2
        if j < 2:
            yl -= bs[1] / 2
        return xl, xl + bs[0] / 2, yl, yl + bs[1] / 2
    for i, p in enumerate(pos):
        xl, xh, yl, yh = bounds(i)
        ins = bool(xl < p[0] < xh and yl < p[1] < yh and bp[2] < p[2] < bp[2] + 0.1)
        elsewhere.append(any(bounds(j)[0] < p[0] < bounds(j)[1] and bounds(j)[2] < p[1] < bounds(j)[3] and bp[2] < p[2] < bp[2] + 0.1 for j in range(n) if j != i))
        for name, v, th in (("x low", p[0], xl), ("x high", p[0], xh), ("y low", p[1], yl), ("y high", p[1], yh), ("z low", p[2], bp[2]), ("z high", p[2], bp[2] + 0.1)):
            _margin(facts, f"object {i} {name}", v, th)
        _margin(facts, f"object {i} reach", 1 - np.tanh(10.0 * dist[i]), 0.6)
        inside.append(ins)
        in_bin.append(ins and (1 - np.tanh(10.0 * dist[i])) < 0.6)
    active = [i for i in range(n) if not in_bin[i]]
    nin = sum(in_bin)
    facts.update(inside=inside, in_bin=in_bin, nin=nin, other_quadrant=elsewhere, near=[(1 - np.tanh(10.0 * d)) >= 0.6 for d in dist], dist=dist, active=active)
    r_reach = r_grasp = r_lift = r_hover = 0.0
    above = [False] * n
    if active:
        facts["reach_from"] = active[int(np.argmin([dist[i] for i in active]))]
        r_reach = (1 - np.tanh(10.0 * min(dist[i] for i in active))) * 0.1
    depths = contact_depths(od)
    facts["grasp"] = grasp = bool(active) and _grasp(info, depths, [g for i in active for g in info["geoms"][i]], facts)
    facts["grasped"] = [i for i in active if grasp and group_depth(depths, info["left_pad"], info["geoms"][i]) is not None
                        and group_depth(depths, info["right_pad"], info["geoms"][i]) is not None]
    r_grasp = 0.35 if grasp else 0.0
    if active and grasp:
        zd = [max(bp[2] + 0.25 - pos[i][2], 0.0) for i in active]
        facts["zmin"], facts["zmin_from"] = min(zd), active[int(np.argmin(zd))]
        r_lift = 0.35 + (1 - np.tanh(15.0 * min(zd))) * 0.15
    if active:
        hov = []
        for i in active:
            dx, dy = pos[i][0] - info["targets"][i][0], pos[i][1] - info["targets"][i][1]
            above[i] = bool(abs(dx) < bs[0] / 4 and abs(dy) < bs[1] / 4)
            _margin(facts, f"object {i} above x", abs(dx), bs[0] / 4)
            _margin(facts, f"object {i} above y", abs(dy), bs[1] / 4)
            hov.append((0.5 if above[i] else r_lift) + (1 - np.tanh(10.0 * np.hypot(dx, dy))) * 0.2)
        r_hover = max(hov)
        facts["hover_from"] = active[int(np.argmax(hov))]
    facts.update(above=above, r_lift=r_lift, r_hover=r_hover, plateau=float(nin))
    r = float(nin) + (max(r_reach, r_grasp, r_lift, r_hover) if shaping else 0.0)
    r *= scale
    if info["single"] == 0:
        r /= 4.0
    return r, (nin > 0 if info["single"] else nin == n), facts


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
def _case(cases, name, q, **want):
    cases.append(dict(name=name, qpos=np.array(q, dtype=np.float64), want=want))


def _panda_grasp(od, info, q, k=0, c=None):
    """cube k between the Panda's pads with the hand's orientation; fingers +-c, or closed by bisection until both pad contacts are DEPTH deep"""
    adr, lp, rp = info["qadr"][k], info["left_pad"], info["right_pad"]

    def fingers(q, c):
        q[7], q[8] = c, -c

    def place(od, q):
        put_free(q, adr, 0.5 * (geom_p(od, lp[0]) + geom_p(od, rp[0])), body_q(od, info["hand"]))
    if c is not None:
        q = np.array(q, dtype=np.float64)
        fingers(q, c); set_state(od, q); place(od, q); set_state(od, q)
        return q
    return close_fingers(od, q, fingers, place, lp, rp, info["geoms"][k], 0.04, 0.0)


def _panda_pose(od, info, q0, mid_target):
    """arm pose that puts the midpoint of the two pads at `mid_target` (two rounds: the pad midpoint sits a few mm off the grip site)"""
    q, arm = np.array(q0, dtype=np.float64), list(range(7))
    tgt = np.array(mid_target, dtype=np.float64)
    for _ in range(3):
        set_state(od, q)
        mid = 0.5 * (geom_p(od, info["left_pad"][0]) + geom_p(od, info["right_pad"][0]))
        q = move_site(od, q, info["site"], site_p(od, info["site"]) + tgt - mid, arm)
    return q


@functools.lru_cache(maxsize=None)
def lift_cases():
    g, cfg, flat = load_golden("seed1_full", "lift_panda")
    om, od, _ = make_oracle(flat, cfg)
    info = panda_ids(flat, cfg, ["cube"])
    q0 = g["states"][0][1:1 + flat.nq].copy()
    adr, th = info["qadr"][0], info["table_height"]
    cases = []
    _case(cases, "far: fixture state", q0, grasp=False, lifted=False)
    q = q0.copy(); put_free(q, adr, (-0.05, 0.15, th + 0.0209), axis_quat((0, 0, 1), 0.7))
    _case(cases, "far: cube elsewhere on the table", q, grasp=False, lifted=False)
    low = [_panda_pose(od, info, q0, (0.0, 0.0, th + 0.026)), _panda_pose(od, info, q0, (-0.05, 0.1, th + 0.038))]
    for i, (qa, off) in enumerate(zip(low, (0.035, 0.06))):         # open fingers, the cube `off` beside the pads along the hand's x axis (across the fingers' plane)
        q = qa.copy(); q[7], q[8] = 0.04, -0.04
        set_state(od, q)
        mid = 0.5 * (geom_p(od, info["left_pad"][0]) + geom_p(od, info["right_pad"][0]))
        p = mid + off * q2m(body_q(od, info["hand"]))[:, 0]
        p[2] = min(p[2], th + 0.036)
        put_free(q, adr, p, body_q(od, info["hand"]))
        _case(cases, f"near, no grasp {i}", q, grasp=False, lifted=False, near=True)
    for i, qa in enumerate(low):
        _case(cases, f"grasp below the margin {i}", _panda_grasp(od, info, qa), grasp=True, lifted=False)
    high = [q0, _panda_pose(od, info, q0, (0.0, 0.0, th + 0.042))]
    for i, qa in enumerate(high):
        _case(cases, f"grasp above the margin {i}", _panda_grasp(od, info, qa), grasp=True, lifted=True)
    for i, p in enumerate(((0.1, 0.1, th + 0.1), (0.0, -0.1, th + 0.042))):
        q = q0.copy(); put_free(q, adr, p, axis_quat((1, 1, 0), 0.4 * i))
        _case(cases, f"cube above the margin, no gripper {i}", q, grasp=False, lifted=True)
    q = q0.copy(); put_free(q, adr, (0.05, -0.1, th + 0.038), (1, 0, 0, 0))
    _case(cases, "cube in the air below the margin", q, grasp=False, lifted=False)
    # over the native capacity: fingers fully closed (they meet each other and sink 2 cm into the cube), the cube flat and 0.65 mm deep in the table,
    # turned about the vertical to the hand's heading
    q = _panda_grasp(od, info, low[1], c=0.0)
    set_state(od, q)
    x = q2m(body_q(od, info["hand"]))[:, 0] * (1, 1, 0)
    x /= np.linalg.norm(x)
    qx, qy, qz, qw = mat2quat_xyzw(np.column_stack([x, np.cross((0, 0, 1), x), (0, 0, 1)]))
    half = np.asarray(flat.arrays["geom_size"], dtype=np.float64).reshape(-1, 3)[info["geoms"][0][0]]
    put_free(q, adr, (q[adr], q[adr + 1], th + half[2] - 6.5e-4), (qw, qx, qy, qz))
    wide = dict(name="fingers fully closed on the cube, the cube touching the table", qpos=q, want=dict(grasp=True, lifted=False))
    return dict(flat=flat, cfg=cfg, info=info, cases=cases, wide=wide, statement=lift_statement)


@functools.lru_cache(maxsize=None)
def stack_cases():
    g, cfg, flat = load_golden("seed0_full", "stack_panda")
    om, od, _ = make_oracle(flat, cfg)
    info = panda_ids(flat, cfg, ["cubeA", "cubeB"])
    q0 = g["states"][0][1:1 + flat.nq].copy()
    (aA, aB), th = info["qadr"], info["table_height"]
    hA, hB = 0.02, 0.025                                           # cube half sizes of the fixture's model
    cases = []
    _case(cases, "reach: fixture state", q0, grasp=False, lifted=False, touching=False)
    q0 = q0.copy(); put_free(q0, aB, (0.12, 0.2, th + hB), axis_quat((0, 0, 1), 0.2))     # from here on cubeB starts out of the gripper's way
    low = [_panda_pose(od, info, q0, (0.0, 0.0, th + 0.026)), _panda_pose(od, info, q0, (-0.05, 0.1, th + 0.038))]
    q = low[0].copy(); q[7], q[8] = 0.04, -0.04
    set_state(od, q)
    put_free(q, aA, 0.5 * (geom_p(od, info["left_pad"][0]) + geom_p(od, info["right_pad"][0])) + (0, 0, 0.005), body_q(od, info["hand"]))
    _case(cases, "reach: cubeA between the open fingers", q, grasp=False, lifted=False, touching=False)
    for i, qa in enumerate(low):
        _case(cases, f"reach with grasp {i}", _panda_grasp(od, info, qa), grasp=True, lifted=False, touching=False)
    held = _panda_grasp(od, info, q0)
    _case(cases, "lifted in the grasp, far from cubeB", held, grasp=True, lifted=True, touching=False)
    q = q0.copy(); put_free(q, aA, (0.1, -0.15, th + 0.042), axis_quat((0, 0, 1), 0.3))
    _case(cases, "lifted without the gripper, far from cubeB", q, grasp=False, lifted=True, touching=False)
    set_state(od, held)
    pA, qA = held[aA:aA + 3].copy(), held[aA + 3:aA + 7].copy()
    down = q2m(qA)[:, 2] * np.sign(-q2m(qA)[2, 2])               # cubeA's own axis that points towards the table
    for i, off in enumerate(((0.0, 0.0), (0.004, -0.003))):
        q = held.copy(); put_free(q, aB, (pA[0] + off[0], pA[1] + off[1], pA[2] - 0.12), axis_quat((0, 0, 1), 0.5 * i))
        _case(cases, f"lifted and aligned over cubeB {i}", q, grasp=True, lifted=True, touching=False, aligned=True)
    for i, (xy, yaw) in enumerate((((0.05, 0.05), 0.0), ((-0.08, 0.12), 0.6))):
        q = q0.copy()
        put_free(q, aB, (xy[0], xy[1], th + hB), axis_quat((0, 0, 1), yaw))
        put_free(q, aA, (xy[0] + 0.003 * i, xy[1], th + 2 * hB + hA - 6.5e-4), axis_quat((0, 0, 1), yaw))
        _case(cases, f"cubeA resting in cubeB's top, released {i}", q, grasp=False, lifted=True, touching=True)
    for i, side in enumerate((0.0, 0.004)):                       # cubeB pushed 0.65 mm into the held cubeA's lower face, same orientation
        q = held.copy(); put_free(q, aB, pA + (hA + hB - 6.5e-4) * down + side * q2m(qA)[:, 0], qA)
        _case(cases, f"cubeA in cubeB's top, still grasped {i}", q, grasp=True, lifted=True, touching=True)
    q = q0.copy()
    put_free(q, aB, (0.05, 0.05, th + hB), (1, 0, 0, 0)); put_free(q, aA, (0.05 + hA + hB - 6.5e-4, 0.05, th + hA), (1, 0, 0, 0))
    _case(cases, "side by side on the table, touching", q, grasp=False, lifted=False, touching=True)
    q = q0.copy()
    put_free(q, aB, (0.05, 0.05, th + hB), (1, 0, 0, 0)); put_free(q, aA, (0.05, 0.05 - (hA + hB - 6.5e-4), th + 0.038), (1, 0, 0, 0))
    _case(cases, "touching cubeB's side below the margin", q, grasp=False, lifted=False, touching=True)
    # over the native capacity: fingers fully closed on the lifted cubeA while cubeB sits 0.65 mm in its lower face: released it would be success
    q = _panda_grasp(od, info, q0, c=0.0)
    put_free(q, aB, q[aA:aA + 3] + (hA + hB - 6.5e-4) * down, q[aA + 3:aA + 7])
    wide = dict(name="fingers fully closed on cubeA, cubeB in its lower face", qpos=q, want=dict(grasp=True, lifted=True, touching=True))
    return dict(flat=flat, cfg=cfg, info=info, cases=cases, wide=wide, statement=stack_statement)


def _peg_pose(od, flat, info, q, t, d, angle, phi=0.0, iters=60):
    """damped least squares on the oracle's body Jacobians (peg minus hole, both arms move) until the peg sits at parallel distance t and perpendicular
    distance d from the hole centre with its axis `angle` off the hole normal (tilted towards the hole's in-plane direction phi)"""
    q = np.array(q, dtype=np.float64)
    rng_ = np.asarray(flat.jnt_range, dtype=np.float64)[:flat.nq]
    for _ in range(iters):
        set_state(od, q)
        Rp, Rh = q2m(body_q(od, info["peg"])), q2m(body_q(od, info["hole"]))
        pp, hp = body_p(od, info["peg"]), body_p(od, info["hole"])
        v = Rp[:, 2]
        n = Rh[:, 2] * np.sign(Rh[:, 2] @ v)
        e1 = Rh[:, 0] * np.cos(phi) + Rh[:, 1] * np.sin(phi)
        vt = np.cos(angle) * n + np.sin(angle) * e1
        u = np.cross(vt, e1)
        target = hp + Rh[:, 0] * 0.1 - t * vt + d * u / np.linalg.norm(u)
        e = np.concatenate([target - pp, np.cross(v, vt)])
        if np.abs(e).max() < 1e-10:
            break
        (jp1, jr1), (jp2, jr2) = od.jac("body", info["peg"]), od.jac("body", info["hole"])
        J = np.vstack([jp1 - jp2, jr1 - jr2])
        dq = J.T @ np.linalg.solve(J @ J.T + 1e-3 * np.eye(6), e)
        q = np.clip(q + dq * min(1.0, 0.2 / np.abs(dq).max()), rng_[:, 0] + 0.01, rng_[:, 1] - 0.01)
    set_state(od, q)
    return q


@functools.lru_cache(maxsize=None)
def peg_cases():
    g, cfg, flat = load_golden("ctl_joint_torque", "peg_baxter")
    om, od, _ = make_oracle(flat)
    info = peg_ids(flat)
    q0 = g["states"][0][1:1 + flat.nq].copy()
    cases = []
    ok = (True, True, True, True)
    inside, outside = np.arccos(0.953), np.arccos(0.947)
    _case(cases, "far: fixture state", q0, checks=(False, True, False, False))
    _case(cases, "far: a later fixture state", g["states"][20][1:1 + flat.nq], checks=(False, True, False, False))
    _case(cases, "success: centred", _peg_pose(od, flat, info, q0, 0.0, 0.0016, 0.0), checks=ok)
    _case(cases, "success: every comparison 3e-3 inside, t high", _peg_pose(od, flat, info, q0, 0.137, 0.057, inside), checks=ok)
    _case(cases, "success: every comparison 3e-3 inside, t low", _peg_pose(od, flat, info, q0, -0.117, 0.057, inside, phi=1.0), checks=ok)
    for k, (d, tl, th_, a) in enumerate(((0.063, -0.123, 0.143, outside), (0.09, -0.16, 0.18, np.arccos(0.90)))):
        _case(cases, f"d over 0.06 ({k})", _peg_pose(od, flat, info, q0, 0.0, d, 0.0), checks=(False, True, True, True))
        _case(cases, f"t under -0.12 ({k})", _peg_pose(od, flat, info, q0, tl, 0.01, 0.0), checks=(True, False, True, True))
        _case(cases, f"t over 0.14 ({k})", _peg_pose(od, flat, info, q0, th_, 0.01, 0.0), checks=(True, True, False, True))
        _case(cases, f"cos under 0.95 ({k})", _peg_pose(od, flat, info, q0, 0.0, 0.01, a, phi=2.0 * k), checks=(True, True, True, False))
    return dict(flat=flat, cfg=cfg, info=info, cases=cases, wide=None, statement=peg_statement)


def _robotiq(q, c):
    """Robotiq 140: outer knuckles +-c, inner fingers +c (the pads stay parallel), inner knuckles -c"""
    q[7], q[10], q[8], q[11], q[9], q[12] = c, -c, c, c, -c, -c


def _iiwa_grasp(od, info, q, k, local=(1.0, 0.0, 0.0, 0.0), shift=(0.0, 0.0, 0.0), target=6.5e-4):
    """object k between the Robotiq pads, orientation = hand x `local`, centre `shift` (hand frame) off the pad midpoint; closed by bisection"""
    def place(od, q):
        R = q2m(body_q(od, info["hand"]))
        mid = 0.5 * (geom_p(od, info["left_pad"][0]) + geom_p(od, info["right_pad"][0]))
        put_free(q, info["qadr"][k], mid + R @ np.asarray(shift), qmul(body_q(od, info["hand"]), np.asarray(local)))
    return close_fingers(od, q, _robotiq, place, info["left_pad"], info["right_pad"], info["geoms"][k], 0.0, 0.7, target)


def _pickplace_fixture(model, tag):
    g, cfg, flat = load_golden(tag, model)
    om, od, _ = make_oracle(flat, cfg)
    return g, cfg, flat, od, pickplace_ids(flat, cfg)


@functools.lru_cache(maxsize=None)
def pickplace_cases():
    g, cfg, flat, od, info = _pickplace_fixture("pickplace_iiwa", "seed0_full")
    fixture = g["states"][0][1:1 + flat.nq].copy()
    T, bp, adr, arm = info["targets"], info["bin2_pos"], info["qadr"], list(range(7))
    q0 = fixture.copy()
    q0[adr[2] + 2] += 0.005          # the fixture's Cereal box sits at bin2_pos[2] + 0.1 to the last digit: off that threshold for every constructed case
    up = (1.0, 0.0, 0.0, 0.0)
    corner = lambda i, z=0.098: (bp[0] + (-0.002 if i in (0, 2) else 0.002), bp[1] + (-0.002 if i < 2 else 0.002), bp[2] + z)   # noqa: E731
    centre = lambda i, z=0.05: (T[i][0] + 0.03, T[i][1] - 0.02, bp[2] + z)                                                      # noqa: E731
    cases = []

    def put(q, i, pos, quat=up):
        q = q.copy(); put_free(q, adr[i], pos, quat)
        return q
    _case(cases, "nothing near: fixture state, Cereal 5 mm up", q0, nin=0, grasp=False)
    _case(cases, "nothing near: a later fixture state", g["states"][10][1:1 + flat.nq], nin=0, grasp=False)
    for i in range(4):
        _case(cases, f"object {i} alone in its quadrant", put(q0, i, centre(i)), nin=1, in_bin=[j == i for j in range(4)])
        _case(cases, f"object {i} alone, 2 mm inside its quadrant's inner corner and top", put(q0, i, corner(i)), nin=1, in_bin=[j == i for j in range(4)])
    _case(cases, "Milk in Bread's quadrant", put(q0, 0, centre(1)), nin=0)
    _case(cases, "Can 2 mm across the corner in Milk's quadrant", put(q0, 3, corner(0)), nin=0)
    _case(cases, "Bread 2 mm across the corner in Can's quadrant", put(q0, 1, corner(3)), nin=0)
    for k, (i, z) in enumerate(((3, 0.102), (0, 0.15))):
        _case(cases, f"object {i} over its target but above the bin ({k})", put(q0, i, (T[i][0], T[i][1] + 0.01 * k, bp[2] + z)), nin=0, above_i=i)
    over = {i: move_site(od, q0, info["site"], (T[i][0], T[i][1], bp[2] + 0.04), arm) for i in (3, 0)}
    for i, qa in over.items():                                    # the gripper, open, around / beside an object that sits inside its quadrant
        set_state(od, qa)
        R, s = q2m(body_q(od, info["hand"])), site_p(od, info["site"])
        mid = 0.5 * (geom_p(od, info["left_pad"][0]) + geom_p(od, info["right_pad"][0]))
        _case(cases, f"object {i} in its quadrant, gripper around it", put(qa, i, mid, body_q(od, info["hand"])), nin=0, near_i=i, grasp=False)
        _case(cases, f"object {i} in its quadrant, gripper 0.08 beside it", put(qa, i, s + 0.08 * R[:, 0], body_q(od, info["hand"])), nin=1, grasp=False)
    q = put(put(q0, 0, centre(0)), 3, corner(3))
    _case(cases, "two in", q, nin=2)
    _case(cases, "three in", put(q, 2, centre(2, 0.09)), nin=3)
    for k in range(2):
        q = q0
        for i in range(4):
            q = put(q, i, centre(i, 0.06 + 0.03 * k) if (i + k) % 2 else (T[i][0] - 0.05, T[i][1] + 0.06, bp[2] + 0.07), axis_quat((0, 0, 1), 0.4 * i))
        _case(cases, f"all four in ({k})", q, nin=4)
    high = [q0, move_site(od, q0, info["site"], (0.0, -0.2, bp[2] + 0.2), arm),
            move_site(od, q0, info["site"], (0.05, -0.15, bp[2] + 0.27), arm)]
    for k, (i, qa) in enumerate(zip((0, 3, 1), high)):
        _case(cases, f"object {i} grasped, height {k}", _iiwa_grasp(od, info, qa, i), nin=0, grasp=True, grasped=[i])
    held = _iiwa_grasp(od, info, q0, 0)
    _case(cases, "Milk grasped while the Can floats above the lift height", put(held, 3, (0.3, -0.4, bp[2] + 0.3)), nin=0, grasp=True, zmin_from=3)
    # the Cereal box held by one end, its centre 0.06 along the hand's x axis; the Can, axis along the hand's x, 0.05 beyond the grip site: closer than the held one
    qc = _iiwa_grasp(od, info, high[1], 2, local=axis_quat((0, 1, 0), np.pi / 2), shift=(0.06, 3.4e-4, 0.0))   # 0.34 mm towards one pad: evens out the two depths
    set_state(od, qc)
    R, s = q2m(body_q(od, info["hand"])), site_p(od, info["site"])
    _case(cases, "Cereal grasped by one end while the Can is closer to the grip site", put(qc, 3, s + 0.05 * R[:, 2], qmul(body_q(od, info["hand"]), axis_quat((0, 1, 0), np.pi / 2))),
          nin=0, grasp=True, grasped=[2], reach_from=3)
    for k, (i, off) in enumerate(((0, (0.11, 0.0)), (1, (0.0, -0.14)))):
        qa = move_site(od, q0, info["site"], (T[i][0] + off[0], T[i][1] + off[1], bp[2] + 0.17), arm)
        _case(cases, f"object {i} grasped beside the region above its target ({k})", _iiwa_grasp(od, info, qa, i), nin=0, grasp=True, grasped=[i], hover_from=i)
    # relative pose: one object orientation per mat2quat branch, in the hand's frame
    set_state(od, q0)
    qh = body_q(od, info["hand"])
    rels = [axis_quat((1, 2, 3), 0.3), axis_quat((1, 0.05, -0.03), 2.97), axis_quat((0.04, 1, 0.06), 2.97), axis_quat((-0.05, 0.03, 1), 2.97),
            axis_quat((1, -1, 0.5), 1.9), axis_quat((0.3, 1, 0.4), 2.5), axis_quat((1, 0.1, 0.9), 2.8), axis_quat((-1, 1, 0.2), 1.2)]
    for k in range(2):
        q = q0
        for i in range(4):
            q = put(q, i, q0[adr[i]:adr[i] + 3], qmul(qh, rels[4 * k + i]))
        _case(cases, f"relative orientations {k}", q, rel=[rels[4 * k + i] for i in range(4)])
    return dict(flat=flat, cfg=cfg, info=info, cases=cases, wide=None, statement=pickplace_statement)


@functools.lru_cache(maxsize=None)
def pickplace_single_cases(mode):
    """single-object modes: 2 = PickPlaceCan (the other objects were cleared to (10, 10, 10)), 1 = PickPlaceSingle (the object changes per episode:
    every case names the env's RSIM_TASK_OBJECT)"""
    g, cfg, flat, od, info = _pickplace_fixture(*(("pickplace_can_iiwa", "seed2_full") if mode == 2 else ("pickplace_single_iiwa", "seed3")))
    assert info["single"] == mode
    q0 = (g["states"][0] if mode == 2 else g["states"][0][0])[1:1 + flat.nq].copy()
    T, bp, adr = info["targets"], info["bin2_pos"], info["qadr"]
    for i in range(4):                # a fixture object that happens to sit within 2 mm of a quadrant's x bound is moved 3 mm off it
        if abs(q0[adr[i]] - bp[0]) < 2e-3:
            q0[adr[i]] += 0.003
    cases = []

    def put(q, i, pos):
        q = q.copy(); put_free(q, adr[i], pos, axis_quat((0, 0, 1), 0.3 * i))
        return q
    at = lambda i, z=0.06: (T[i][0] - 0.04, T[i][1] + 0.05, bp[2] + z)     # noqa: E731
    objs = (3, 3, 0, 1) if mode == 2 else (int(g["ep_object"][0]), (int(g["ep_object"][0]) + 1) % 4, 0, 2)
    _case(cases, "object out: fixture state", q0, nin=0, task_object=objs[0])
    _case(cases, "object out: above its bin", put(q0, objs[0], at(objs[0], 0.13)), nin=0, task_object=objs[1])
    _case(cases, "object in", put(q0, objs[0], at(objs[0])), nin=1, task_object=objs[0])
    _case(cases, "another object in its bin", put(q0, objs[2], at(objs[2])), nin=1, task_object=objs[1])
    _case(cases, "two objects in", put(put(q0, objs[2], at(objs[2])), objs[3], at(objs[3], 0.08)), nin=2, task_object=objs[0])
    return dict(flat=flat, cfg=cfg, info=info, cases=cases, wide=None, statement=pickplace_statement)


TASKS = {"lift": lift_cases, "stack": stack_cases, "peg": peg_cases, "pickplace": pickplace_cases,
         "pickplace_can": functools.partial(pickplace_single_cases, 2), "pickplace_single": functools.partial(pickplace_single_cases, 1)}


def evaluate(S, scale=1.0, shaping=True, wide=False):
    """[(reward, success, facts)] of the statement over the task's cases (or its over-capacity case) on a fresh oracle"""
    om, od, _ = make_oracle(S["flat"], S["cfg"] if "eef_site" in S["cfg"] else None)
    out = []
    for c in ([S["wide"]] if wide else S["cases"]):
        set_state(od, c["qpos"])
        r, s, f = S["statement"](S["info"], od, scale, shaping)
        f["ncon"], f["nefc"] = od.ncon, od.nefc
        f["frames"] = dict(xpos=np.array(od.xpos), xquat=np.array(od.xquat), site_xpos=np.array(od.site_xpos))
        out.append((float(r), bool(s), f))
    return out
