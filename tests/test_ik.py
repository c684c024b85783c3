"""Inverse kinematics on the device (csrc/rsim_ik.hip, rsim_ik_site) against the fp64 host mirror (robosuite_amd/ik.py): achieved pose, one update, limits,
unreachable targets, purity, the Python entry points and the IK_POSE plugin controller.

q_out is never compared with the mirror's q: a redundant arm's solution set is a manifold, and the fp32 and fp64 paths may end at different points of it.
What is compared is the pose ik.fk finds, in fp64, at the device's q_out.  On well-conditioned cases (ik.well_conditioned, the mirror alone; at most 10 % of
a scene's cases may be left out, asserted here and in tests/test_ik_host.py) the device reports converged and that pose meets pos_tol + m_p / rot_tol + m_r,
where m_p / m_r are FOUR TIMES the worst |err_dev - err_fp64(q_out)| one GPU run measured per scene -- the fp32 kinematics error of the kernel
(profiles/ik_parity.txt; the margin is for one box, one run and pose-dependent rounding, as in tests/test_raycast.py).  One update (max_iters = 1, damping
1e-2, a step cap that binds) and two updates with the posture term (its v is zero at the first) are held to the mirror's at the fp32-rounded inputs, relative
to max(|dq|, 1e-3), again at four times the measured worst."""
import numpy as np
import pytest
import torch

from robosuite_amd import backend, ik
from tests import ik_scenes as S
from tests.util import load_golden, make_hip

pytestmark = pytest.mark.gpu

B, NCASE = 3, 40
# scene -> worst measured (|err_pos,dev - err_pos,fp64|, |w_dev - w_fp64|, error of two updates with posture_gain = 1, of one update with a binding max_dq): profiles/ik_parity.txt
MEASURED = {"panda": (3.399e-7, 3.738e-7, 7.288e-6, 6.425e-6), "baxter_left": (3.421e-7, 3.399e-7, 4.511e-6, 1.322e-5), "chain3": (1.865e-7, 0.0, 5.526e-6, 5.862e-6),
            "hinge1": (8.495e-8, 0.0, 9.058e-5, 4.948e-5), "chain16": (1.925e-7, 2.510e-7, 5.410e-6, 4.753e-6), "panda_per_env": (3.020e-7, 3.488e-7, None, None)}
BOUND = {k: tuple(None if x is None else 4 * x for x in v) for k, v in MEASURED.items()}
POS_TOL, ROT_TOL = ik.DEFAULTS["pos_tol"], ik.DEFAULTS["rot_tol"]


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def solve_cases(hb, site, dofs, C, K, with_init=True, **opts):
    """C: one case dict per env (tests/ik_scenes.py cases).  Device solves in calls of K problems per env (the last call repeats the last case to fill up)
    -> q [B, n, ndof], err [B, n, 2], iters [B, n], converged [B, n] as numpy"""
    n = len(C[0]["pos"])
    parts = []
    for a in range(0, n, K):
        idx = [min(a + k, n - 1) for k in range(K)]
        pos = _dev(np.stack([c["pos"][idx] for c in C]))
        quat = None if C[0]["quat"] is None else _dev(np.stack([c["quat"][idx] for c in C]))
        qi = _dev(np.stack([c["q_init"][idx] for c in C])) if with_init else None
        r = hb.solve_ik(site, dofs, pos, quat, qi, **opts)
        assert r[0].shape == (len(C), K, len(dofs)) and r[1].shape == (len(C), K, 2) and r[2].shape == r[3].shape == (len(C), K)
        assert r[0].dtype == r[1].dtype == torch.float32 and r[2].dtype == torch.int32 and r[3].dtype == torch.bool
        parts.append([x[:, :min(K, n - a)].cpu().numpy() for x in r])
    return tuple(np.concatenate([p[i] for p in parts], axis=1) for i in range(4))


def limits32(flat, dofs, ov):
    """the ranges the kernel clamps to: float32, infinite where the joint is not limited"""
    jid = S._joints_of(flat, dofs)
    lim = np.asarray(flat.arrays["jnt_limited"]).ravel().astype(bool)[jid]
    r = np.asarray(ov["jnt_range"], dtype=np.float64).reshape(-1, 2)[jid].astype(np.float32)
    return np.where(lim, r[:, 0], -np.inf).astype(np.float32), np.where(lim, r[:, 1], np.inf).astype(np.float32)


class Scene:
    """a scene's batch, its cases per env and the mirror's verdict on them: built once, shared by the tests"""

    def __init__(self, name, per_env=False):
        s = S.scene("panda" if name == "panda_per_env" else name)
        self.name, self.flat, self.site, self.dofs, self.quat = name, s["flat"], s["site"], s["dofs"], s["quat"]
        self.hm, self.hb = make_hip(self.flat, s["cfg"], B=B, per_env=per_env)
        self.qpos = np.tile(np.asarray(self.flat.arrays["qpos0"], dtype=np.float64).ravel(), (B, 1)).astype(np.float32)
        self.hb.set("qpos", self.qpos)
        self.ov = [ik.rounded(self.flat) for _ in range(B)]
        self.C = self.ok = None

    def draw(self):
        self.C = [S.cases(self.flat, self.site, self.dofs, NCASE, seed=S.case_seed(self.name, e), overrides=self.ov[e], quat=self.quat) for e in range(B)]
        self.ok = np.stack([S.well(self.flat, self.qpos[e].astype(np.float64), self.site, self.dofs, self.C[e], self.ov[e]) for e in range(B)])
        return self

    def err64(self, e, q, i, C=None):
        c = (C or self.C)[e]
        return ik.error(self.flat, self.qpos[e].astype(np.float64), self.site, self.dofs, np.asarray(q, dtype=np.float64), c["pos"][i],
                        None if c["quat"] is None else c["quat"][i], self.ov[e])


_SCENES = {}


def get_scene(name):
    if name not in _SCENES:
        _SCENES[name] = Scene(name).draw()
    return _SCENES[name]


def check_pose(sc, q, err, it, conv, C=None, ok=None):
    """checks 1 and 3 on one run over a scene's cases; returns the worst (|err_pos| gap, |w| gap) between the device's report and fp64 at its q_out"""
    C, ok = C or sc.C, sc.ok if ok is None else ok
    m_p, m_r = BOUND[sc.name][:2]
    worst = [0.0, 0.0]
    for e in range(B):
        lo, hi = limits32(sc.flat, sc.dofs, sc.ov[e])
        assert np.isfinite(q[e]).all() and (q[e] >= lo).all() and (q[e] <= hi).all(), (sc.name, e)      # limits, in fp32, converged or not
        for i in range(len(C[e]["pos"])):
            e64 = sc.err64(e, q[e, i], i, C)
            worst = [max(worst[0], abs(err[e, i, 0] - e64[0])), max(worst[1], abs(err[e, i, 1] - e64[1]))]
            if ok[e, i]:
                assert conv[e, i] and it[e, i] <= ik.DEFAULTS["max_iters"], (sc.name, e, i, it[e, i], err[e, i])
                assert e64[0] <= POS_TOL + m_p and e64[1] <= ROT_TOL + m_r, (sc.name, e, i, e64)
            if conv[e, i]:
                assert err[e, i, 0] < POS_TOL and (not sc.quat or err[e, i, 1] < ROT_TOL)
            if not sc.quat:
                assert err[e, i, 1] == 0.0
    print(f"ik parity {sc.name}: {int(ok.sum())}/{ok.size} well-conditioned, {int(conv.sum())} converged, median iterations {np.median(it):.0f}, "
          f"worst |err_dev - err_fp64(q_out)| pos {worst[0]:.3e} rot {worst[1]:.3e} (margins {m_p:.1e} / {m_r:.1e})")
    assert (~ok).sum() <= 0.10 * ok.size, (sc.name, int((~ok).sum()))
    return worst


# ---- check 1 (achieved pose) and 3 (limits) ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (1, 2, 5))
def test_panda_achieved_pose(K):
    sc = get_scene("panda")
    check_pose(sc, *solve_cases(sc.hb, sc.site, sc.dofs, sc.C, K))


@pytest.mark.parametrize("name", ("baxter_left", "chain3", "hinge1", "chain16"))
def test_achieved_pose(name):
    sc = get_scene(name)
    check_pose(sc, *solve_cases(sc.hb, sc.site, sc.dofs, sc.C, 5))


# ---- check 2: one update --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("panda", "baxter_left", "chain3", "hinge1", "chain16"))
@pytest.mark.parametrize("variant", ("posture", "max_dq"))
def test_one_update_equals_the_mirror(name, variant):
    sc = get_scene(name)
    """max_dq: ONE update with a step cap that binds.  posture: TWO updates with posture_gain = 1 -- the first is made at q == q_rest, where v is exactly zero and
    the posture branch adds nothing; the second starts from q_rest + dq_1, so v = -dq_1 is as large as the first step (nonzero in every case: asserted) and J v, the second pair of
    solves and the projection all take part.  Both tolerances are 0 there, so neither side stops after one update."""
    n_up = 2 if variant == "posture" else 1
    opts = dict(max_iters=n_up, damping=1e-2, **(dict(posture_gain=1.0, pos_tol=0.0, rot_tol=0.0) if variant == "posture" else dict(max_dq=0.02)))
    q, err, it, conv = solve_cases(sc.hb, sc.site, sc.dofs, sc.C, 5, **opts)
    worst, bound, capped, vmin, shift = 0.0, BOUND[name][2 if variant == "posture" else 3], 0, np.inf, 0.0
    for e in range(B):
        for i in range(NCASE):
            c = sc.C[e]
            ref = ik.solve(sc.flat, sc.qpos[e].astype(np.float64), sc.site, sc.dofs, c["pos"][i], None if c["quat"] is None else c["quat"][i], c["q_init"][i], sc.ov[e], **opts)
            start = np.minimum(np.maximum(c["q_init"][i], limits32(sc.flat, sc.dofs, sc.ov[e])[0]), limits32(sc.flat, sc.dofs, sc.ov[e])[1])
            dq_ref, dq_dev = ref[0] - start, q[e, i].astype(np.float64) - start
            assert it[e, i] == n_up == ref[2]
            if variant == "posture":
                one = ik.solve(sc.flat, sc.qpos[e].astype(np.float64), sc.site, sc.dofs, c["pos"][i], None if c["quat"] is None else c["quat"][i], c["q_init"][i], sc.ov[e], **dict(opts, max_iters=1))
                v = 1.0 * (start - one[0])                      # posture_gain (q_rest - q) as the second update sees it
                plain = ik.solve(sc.flat, sc.qpos[e].astype(np.float64), sc.site, sc.dofs, c["pos"][i], None if c["quat"] is None else c["quat"][i], c["q_init"][i], sc.ov[e], **dict(opts, posture_gain=0.0))
                vmin, shift = min(vmin, float(np.abs(v).max())), max(shift, float(np.abs(ref[0] - plain[0]).max()))
            worst = max(worst, float(np.abs(dq_dev - dq_ref).max() / max(np.abs(dq_ref).max(), 1e-3)))
            capped += bool(np.isclose(np.abs(dq_ref).max(), 0.02, rtol=1e-9))
    print(f"ik one update {name} / {variant}: worst relative error {worst:.3e} (bound {bound:.1e}); step cap bound in {capped}/{B * NCASE} cases"
          + (f"; smallest max|v| at the second update {vmin:.3e}, largest change of q through the posture term {shift:.3e}" if variant == "posture" else ""))
    if variant == "posture":
        assert vmin > 0.0 and shift > 1e-3       # v is nonzero in every case, and the term moves q by 1e-3 and more: a thousand times what the bound lets an error be
    assert worst <= bound
    if variant == "max_dq":
        assert capped >= B * NCASE // 2      # small enough to bind


# ---- check 4: unreachable target --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("panda", "chain3", "hinge1"))
def test_unreachable_target(name):
    sc = get_scene(name)
    C = [{k: (None if v is None else v[:5].copy()) for k, v in c.items()} for c in sc.C]
    for c in C:
        c["pos"] = (c["pos"] + [5.0, 0.0, 0.0]).astype(np.float32).astype(np.float64)
    q, err, it, conv = solve_cases(sc.hb, sc.site, sc.dofs, C, 5)
    assert not conv.any() and (it == ik.DEFAULTS["max_iters"]).all()
    for e in range(B):
        lo, hi = limits32(sc.flat, sc.dofs, sc.ov[e])
        assert np.isfinite(q[e]).all() and (q[e] >= lo).all() and (q[e] <= hi).all()
        for i in range(5):
            e64 = sc.err64(e, q[e, i], i, C)
            assert abs(err[e, i, 0] - e64[0]) <= 0.01 * e64[0] and abs(err[e, i, 1] - e64[1]) <= 0.01 * e64[1] + (0.0 if sc.quat else 1e-30), (name, e, i, err[e, i], e64)
            assert e64[0] > 3.0


# ---- per-env model parameters -----------------------------------------------------------------------------------------------------------------------------
def test_per_env_params_are_honoured():
    """env 1's robot base is moved 5 cm, env 2's joint 4 is narrowed to +- 0.3 rad so that the clamp acts; targets come from the mirror with the same overrides"""
    sc = _SCENES.get("panda_per_env")
    if sc is None:
        sc = _SCENES["panda_per_env"] = Scene("panda_per_env", per_env=True)
        base = sc.flat.names["body"].index("robot0_base")
        bp = sc.hb.param_get("body_pos")
        bp[1, base] += [0.05, 0.0, 0.0]
        sc.hb.param_set("body_pos", bp[1:2], env0=1)
        jr = sc.hb.param_get("jnt_range")
        jr[2, 4] = [-0.3, 0.3]
        sc.hb.param_set("jnt_range", jr[2:3], env0=2)
        live_bp, live_jr = sc.hb.param_get("body_pos"), sc.hb.param_get("jnt_range")
        assert np.allclose(live_bp[1, base] - live_bp[0, base], [0.05, 0, 0], atol=1e-6) and np.allclose(live_jr[2, 4], [-0.3, 0.3], atol=1e-6)
        sc.ov = [ik.rounded(sc.flat, {"body_pos": live_bp[e], "jnt_range": live_jr[e]}) for e in range(B)]
        sc.draw()
    q, err, it, conv = solve_cases(sc.hb, sc.site, sc.dofs, sc.C, 5)
    check_pose(sc, q, err, it, conv)
    lo2, hi2 = limits32(sc.flat, sc.dofs, sc.ov[2])
    assert lo2[4] == np.float32(-0.3) and hi2[4] == np.float32(0.3) and (q[2, :, 4] >= lo2[4]).all() and (q[2, :, 4] <= hi2[4]).all()
    # the clamp acts: without it the mirror's answer leaves env 2's narrowed range in some case
    left = 0
    for i in range(NCASE):
        c = sc.C[2]
        qf = ik.solve(sc.flat, sc.qpos[2].astype(np.float64), sc.site, sc.dofs, c["pos"][i], c["quat"][i], c["q_init"][i], sc.ov[2], clamp_range=0)[0]
        left += bool(abs(qf[4]) > 0.3)
    assert left >= 1
    # the same target in every env: env 1 (base moved) needs other joint angles than env 0, whose answer is the one it gave before
    C0 = [sc.C[0]] * B
    qs, errs, its, convs = solve_cases(sc.hb, sc.site, sc.dofs, C0, 5)
    assert np.array_equal(qs[0], q[0]) and np.array_equal(its[0], it[0])
    both = convs[0] & convs[1]
    assert both.sum() >= NCASE // 2 and (np.abs(qs[1] - qs[0]).max(axis=1)[both] > 1e-3).all()
    for i in np.flatnonzero(both)[:10]:
        e1 = ik.error(sc.flat, sc.qpos[1].astype(np.float64), sc.site, sc.dofs, qs[1, i].astype(np.float64), sc.C[0]["pos"][i], sc.C[0]["quat"][i], sc.ov[1])
        e0 = ik.error(sc.flat, sc.qpos[1].astype(np.float64), sc.site, sc.dofs, qs[1, i].astype(np.float64), sc.C[0]["pos"][i], sc.C[0]["quat"][i], sc.ov[0])
        assert e1[0] <= POS_TOL + BOUND["panda_per_env"][0] and e0[0] > 0.04      # right on env 1's model, 5 cm off on env 0's


def test_a_joint_on_the_path_that_is_not_controlled_is_held_at_the_envs_qpos():
    sc = get_scene("panda")
    dofs = sc.dofs[1:]
    qpos = sc.qpos.copy()
    qpos[:, 0] = [0.0, 0.4, -0.7]
    hm, hb = make_hip(sc.flat, None, B=B)
    hb.set("qpos", qpos)
    C = [S.cases(sc.flat, sc.site, dofs, 10, seed=77 + e, qpos=qpos[e].astype(np.float64), overrides=sc.ov[e]) for e in range(B)]
    q, err, it, conv = solve_cases(hb, sc.site, dofs, C, 5)
    assert conv.mean() >= 0.8
    for e in range(B):
        for i in np.flatnonzero(conv[e]):
            e64 = ik.error(sc.flat, qpos[e].astype(np.float64), sc.site, dofs, q[e, i].astype(np.float64), C[e]["pos"][i], C[e]["quat"][i], sc.ov[e])
            assert e64[0] <= POS_TOL + BOUND["panda"][0] and e64[1] <= ROT_TOL + BOUND["panda"][1], (e, i, e64)


# ---- check 5: purity ----------------------------------------------------------------------------------------------------------------------------------------
def _lift(Bn=4, tag="seed0_gentle"):
    from robosuite_amd import lift

    g, cfg, flat = load_golden(tag)
    return flat, cfg, lift.LiftBatch(flat, cfg, np.arange(Bn), seed0=4, horizon=50, bank_episodes=3)


def test_a_solve_leaves_the_state_alone():
    flat, cfg, task = _lift()
    _, _, twin = _lift()
    task.reset(); twin.reset()
    a = torch.zeros((4, task.model.action_dim), device="cuda"); a[:, 0] = 0.5; a[:, 4] = -0.3
    task.step(a); twin.step(a)
    hb = task.batch
    keys = ("qpos", "qvel", "time", "ctrl", "cstate")
    before = {k: hb.get(k).copy() for k in keys}
    site, dofs = cfg["eef_site"], cfg["dof_idx"]
    st = hb.tensor("qpos")[:, cfg["qpos_idx"]].clone()
    pos = torch.tensor([[0.1, 0.05, 1.0]], device="cuda").repeat(4, 1)
    quat = torch.tensor([[0.0, 1.0, 0.0, 0.0]], device="cuda").repeat(4, 1)
    r_none = hb.solve_ik(site, dofs, pos, quat)
    r_expl = hb.solve_ik(site, dofs, pos, quat, st)
    for x, y in zip(r_none, r_expl):
        assert torch.equal(x, y)                                    # q_init=None is the current joint positions
    assert r_none[0].shape == (4, 7) and r_none[1].shape == (4, 2) and r_none[2].shape == r_none[3].shape == (4,)      # 2-D in, 2-D out
    for k in keys:
        assert np.array_equal(hb.get(k), before[k]), k
    task.step(a); twin.step(a)
    assert torch.equal(task.obs(), twin.obs()) and np.array_equal(hb.get("qpos"), twin.batch.get("qpos"))


# ---- check 6: interface -------------------------------------------------------------------------------------------------------------------------------------
def test_vecenv_and_batchstate_calls_and_bad_arguments():
    import ctypes as C

    from robosuite_amd.controllers import BatchState
    from robosuite_amd.vec_env import VecEnv

    g, cfg, flat = load_golden("seed0_gentle")
    env = VecEnv("Lift", 2, flat, cfg, horizon=50)
    env.reset()
    env.step(torch.zeros((2, env.action_dim), device="cuda"))
    pos = torch.tensor([[[0.05, 0.1, 1.0], [-0.1, 0.0, 1.1]]], device="cuda").repeat(2, 1, 1)
    quat = torch.tensor([0.0, 1.0, 0.0, 0.0], device="cuda").expand(2, 2, 4)
    hb = env.env.batch
    a = env.solve_ik(pos, quat)
    b = hb.solve_ik(cfg["eef_site"], cfg["dof_idx"], pos, quat)
    c = BatchState(hb).solve_ik(cfg["eef_site"], cfg["dof_idx"], pos, quat)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert a[3].all() and a[0].shape == (2, 2, 7)
    with pytest.raises(ValueError):
        env.solve_ik(pos, quat, arm=1)
    site, dofs = cfg["eef_site"], cfg["dof_idx"]
    for bad in (lambda: hb.solve_ik(site, dofs, pos[:, :, :2]), lambda: hb.solve_ik(site, dofs, pos, quat[:, :1]), lambda: hb.solve_ik(site, dofs, pos.cpu()),
                lambda: hb.solve_ik(site, dofs, pos, quat, torch.zeros((2, 2, 6), device="cuda")), lambda: hb.solve_ik(site, dofs, pos[:1]),
                lambda: hb.solve_ik(site, dofs, pos, damping=-1.0), lambda: hb.solve_ik(site, dofs, pos, tolerance=1.0),
                lambda: hb.solve_ik(site, [0, 1, 7], pos), lambda: hb.solve_ik(site, list(range(17)), pos), lambda: hb.solve_ik(99, dofs, pos),
                lambda: hb.solve_ik(flat.names["site"].index("cube_default_site"), [0], pos)):
        with pytest.raises(backend.RsimError):
            bad()
    # the C boundary names what it refuses
    L = backend.lib()
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    q, err, it = torch.zeros((2, 2, 7), device="cuda"), torch.zeros((2, 2, 2), device="cuda"), torch.zeros((2, 2), dtype=torch.int32, device="cuda")
    d7 = (C.c_int32 * 7)(*dofs)
    cube = flat.names["site"].index("cube_default_site")
    for args, word in (((hb.ptr, site, 0, d7, 2, P(pos), None, None, None, P(q), P(err), P(it)), b"ndof 0"),
                       ((hb.ptr, site, 17, d7, 2, P(pos), None, None, None, P(q), P(err), P(it)), b"ndof 17"),
                       ((hb.ptr, site, 7, d7, 0, P(pos), None, None, None, P(q), P(err), P(it)), b"k 0"),
                       ((hb.ptr, site, 7, d7, 2, P(pos), None, None, None, None, P(err), P(it)), b"q_out_dev"),
                       ((hb.ptr, site, 7, d7, 2, P(pos), None, None, None, P(q), None, P(it)), b"err_dev"),
                       ((hb.ptr, site, 7, d7, 2, P(pos), None, None, None, P(q), P(err), None), b"iters_dev"),
                       ((hb.ptr, 99, 7, d7, 2, P(pos), None, None, None, P(q), P(err), P(it)), b"site 99"),
                       ((hb.ptr, cube, 1, d7, 2, P(pos), None, None, None, P(q), P(err), P(it)), b"free joint"),
                       ((hb.ptr, site, 3, (C.c_int32 * 3)(0, 1, 7), 2, P(pos), None, None, None, P(q), P(err), P(it)), b"dof 7 is not a hinge or slide joint on the path"),
                       ((hb.ptr, site, 2, (C.c_int32 * 2)(1, 1), 2, P(pos), None, None, None, P(q), P(err), P(it)), b"twice")):
        assert L.rsim_ik_site(*args) != 0 and word in L.rsim_last_error(), (word, L.rsim_last_error())
    # opts == NULL is the defaults
    assert L.rsim_ik_site(hb.ptr, site, 7, d7, 2, P(pos), P(quat.contiguous()), None, None, P(q), P(err), P(it)) == 0
    hb.sync()
    assert torch.equal(q, b[0]) and torch.equal(err, b[1])


def test_ball_joint_and_mocap_body_on_the_path_are_refused_by_the_library():
    """the two refusals of the chain builder in rsim_api.cpp that no shipped model reaches: batches of a generated chain that ends in a ball joint, and of a model
    whose site sits on a mocap body"""
    import ctypes as C

    from robosuite_amd import mjcf
    from tests import capacity_models

    L = backend.lib()
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    pos, q, err, it = torch.zeros((1, 1, 3), device="cuda"), torch.zeros((1, 1, 1), device="cuda"), torch.zeros((1, 1, 2), device="cuda"), torch.zeros((1, 1), dtype=torch.int32, device="cuda")
    ball = mjcf.compile_mjcf(capacity_models.model_xml(3, 0, n_ball=1))
    mocap = mjcf.compile_mjcf('<mujoco><worldbody><geom type="plane" size="1 1 0.1"/><body name="a" pos="0 0 1"><joint name="h" type="hinge" axis="0 1 0"/>'
                              '<geom type="sphere" size="0.05"/></body><body name="m" mocap="true" pos="0.5 0 1"><geom type="sphere" size="0.05" contype="0" conaffinity="0"/>'
                              '<site name="tip"/></body></worldbody></mujoco>')
    for flat, word in ((ball, b"(b0) on the path to site 1 is a ball joint"), (mocap, b"is a mocap body")):
        hm, hb = make_hip(flat, None, B=1)
        site = flat.names["site"].index("tip")
        assert L.rsim_ik_site(hb.ptr, site, 1, (C.c_int32 * 1)(0), 1, P(pos), None, None, None, P(q), P(err), P(it)) != 0 and word in L.rsim_last_error(), L.rsim_last_error()
        with pytest.raises(ValueError):
            ik.chain(flat, site, [0])               # the mirror refuses the same


def test_vecenv_solves_for_the_second_arm_of_a_two_arm_description():
    """arm=1 on the Baxter two-arm OSC description: the second part's site and dofs (eef_site2, the entries at offset 8 of the controller description)"""
    from robosuite_amd.controllers import BatchState, TorchIKPoseController
    from robosuite_amd.vec_env import VecEnv

    g, cfg, flat = load_golden("ctl_osc_pose", "peg_baxter")
    env = VecEnv("TwoArmPegInHole", 2, flat, cfg, horizon=50)
    env.reset()
    env.step(torch.zeros((2, env.action_dim), device="cuda"))
    hb = env.env.batch
    hb.forward()
    st = BatchState(hb)
    out = []
    for arm, part in enumerate(cfg["parts"]):
        p, R = st.site_pose(part["eef_site"])
        pos, quat = p + torch.tensor([0.02, -0.01, 0.015], device="cuda"), TorchIKPoseController.mat2quat(R)
        a = env.solve_ik(pos, quat, arm=arm)
        b = hb.solve_ik(part["eef_site"], part["dof_idx"], pos, quat)
        for x, y in zip(a, b):
            assert torch.equal(x, y)
        assert a[3].all() and a[0].shape == (2, 7)
        qpos = hb.get("qpos").astype(np.float64)
        for e in range(2):          # the answer puts THIS arm's site at the target, on the mirror
            e64 = ik.error(flat, qpos[e], part["eef_site"], part["dof_idx"], a[0][e].cpu().numpy().astype(np.float64), pos[e].cpu().numpy().astype(np.float64),
                           quat[e].cpu().numpy().astype(np.float64), ik.rounded(flat))
            assert e64[0] <= POS_TOL + BOUND["baxter_left"][0] and e64[1] <= ROT_TOL + BOUND["baxter_left"][1], (arm, e, e64)
        out.append(a[0])
    assert cfg["parts"][0]["eef_site"] != cfg["parts"][1]["eef_site"] and set(cfg["parts"][0]["dof_idx"]).isdisjoint(cfg["parts"][1]["dof_idx"])
    with pytest.raises(ValueError):
        env.solve_ik(pos, quat, arm=2)


# ---- check 7: the IK_POSE plugin ------------------------------------------------------------------------------------------------------------------------------
def _ik_env(Bn=4):
    from robosuite_amd.controllers import BatchState, HostControlledEnv, Part, TorchGripController, TorchIKPoseController

    flat, cfg, task = _lift(Bn, "ctl_joint_position")
    st = BatchState(task.batch)
    cr = np.asarray(flat.actuator_ctrlrange)
    ji = dict(joints=cfg["qpos_idx"], qpos=cfg["qpos_idx"], qvel=cfg["dof_idx"])
    arm = TorchIKPoseController(st, ji, (cr[cfg["act_idx"], 0], cr[cfg["act_idx"], 1]), cfg["eef_site"], cfg["base_site"], kp=cfg["kp"], damping_ratio=cfg["damping_ratio"])
    grip = TorchGripController(st, dict(joints=cfg["grip_qpos_idx"], qpos=cfg["grip_qpos_idx"], qvel=cfg["grip_dof_idx"]),
                               (cr[cfg["grip_act"], 0], cr[cfg["grip_act"], 1]), signs=cfg["grip_sign"], speed=cfg["grip_speed"])
    env = HostControlledEnv(task, [Part(arm, slice(0, 6), cfg["act_idx"]), Part(grip, slice(6, 7), cfg["grip_act"])])
    return flat, cfg, task, st, ji, cr, arm, env


def test_ik_pose_plugin_goal_and_torques():
    from robosuite_amd.controllers import TorchJointPositionController

    flat, cfg, task, st, ji, cr, arm, env = _ik_env()
    assert arm.name == "IK_POSE" and arm.control_dim == 6 and env.action_dim == 7
    env.reset()
    task.batch.step1()
    a = torch.tensor([[0.5, -0.2, 0.3, 0.1, -0.2, 0.3]], device="cuda").repeat(4, 1)
    a[1] *= -1; a[2, 3:] = 0
    arm.set_goal(a)
    q, err, it, conv = st.solve_ik(cfg["eef_site"], cfg["dof_idx"], arm.target_pos, arm.target_quat, arm.joint_pos.contiguous())
    assert conv.all() and torch.equal(arm.goal_qpos, q) and arm.ik_failures == 0
    # the target is the scaled delta, in the base frame, on the achieved pose: 2.5 cm along base x for action 0.5
    ep, eR = st.site_pose(cfg["eef_site"]); op, oR = st.site_pose(cfg["base_site"])
    d = torch.einsum("bji,bj->bi", oR, arm.target_pos - ep)
    assert torch.allclose(d[0], torch.tensor([0.025, -0.01, 0.015], device="cuda"), atol=2e-6)
    ref = TorchJointPositionController(st, ji, (cr[cfg["act_idx"], 0], cr[cfg["act_idx"], 1]), kp=cfg["kp"], damping_ratio=cfg["damping_ratio"])
    ref.goal_qpos = q.clone()
    assert torch.equal(arm.run_controller(), ref.run_controller())
    # an env whose solve does not converge keeps its goal and is counted
    arm.ik_opts = dict(max_iters=0)
    arm.set_goal(a)
    assert torch.equal(arm.goal_qpos, q) and arm.ik_failures == 4


def test_ik_pose_plugin_moves_the_gripper_along_x():
    flat, cfg, task, st, ji, cr, arm, env = _ik_env()
    env.reset()
    task.batch.forward()
    p0, _ = st.site_pose(cfg["eef_site"])
    p0 = p0.clone()
    a = torch.zeros((4, 7), device="cuda"); a[:, 0] = 1.0
    for _ in range(10):
        env.step(a)
    task.batch.forward()
    p1, _ = st.site_pose(cfg["eef_site"])
    d = (p1 - p0).cpu().numpy()
    print("IK_POSE, ten steps of +x: displacement per env", d.round(4).tolist(), "failures", arm.ik_failures)
    assert (d[:, 0] > 0.01).all() and (np.abs(d[:, 1]) < d[:, 0]).all() and (np.abs(d[:, 2]) < d[:, 0]).all()
