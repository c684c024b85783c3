"""Configuration clearance on the device (csrc/rsim_clear.hip: rsim_config_fk, rsim_config_pairs, rsim_config_clearance) against the fp64 host mirror
(robosuite_amd/clearance.py), with the model's parameters rounded to fp32 as the device holds them.

  * FK: config_fk against clearance.fk for every body -- position error in metres, rotation angle in radians; a body the dofs do not move equals
    get("xpos") / get("xquat") bit for bit.  Also against the step path's own FK: the candidate written into a second batch's qpos, forward(), xpos.
  * clearance, held to the distance layer: the device's OWN config_fk poses go to the mirror's geom_distance over the same list, so the FK error stays out of
    it.  |dist - min_ref| <= BOUND; the chosen pair satisfies ref_dist[pair] <= min_ref + 2 BOUND (this holds at ties and in the touching band alike, so no
    pair is left out); where status is 0 or 2 the witnesses lie in their solids (distance_scenes.outside_by) and |p2 - p1| = |dist|, each within BOUND; a
    candidate with everything beyond distmax reads (distmax, -1, zeros, FAR).
  * chunking: chunks = 1, 2, the list length and automatic agree within BOUND (a near-tie may resolve differently by an ulp, so not bit for bit); a repeat call
    is bit-identical.
  * the shapes are chosen for the lane mapping (lane = env * K + k): (3, 5) one partial wavefront over three envs, (65, 3) three full wavefronts that straddle
    env boundaries and a partial one, (2, 70) K larger than a wavefront, and 2-D tensors for K = 1.

BOUND is four times the worst figure of one GPU run per scene (MEASURED, profiles/clearance_parity.txt, written by tools/clearance_parity.py from the
functions below; the margin is for one box, one run and pose-dependent rounding) -- the convention of tests/test_distance.py."""
import numpy as np
import pytest
import torch

from robosuite_amd import backend, clearance, distance
from tests import clearance_scenes as S
from tests import distance_scenes as D
from tests.util import make_hip

pytestmark = pytest.mark.gpu

# worst figures of one GPU run (profiles/clearance_parity.txt): FK position (m) and rotation (rad) against the mirror, FK position against the step path's
# forward(), |dist - min_ref| (m) at the device's own poses, and K = 1 at the env's own joints against torch.min over geom_distance.  The tests assert 4 x.
MEASURED = {
    "T": {"fk_pos": 3.503e-7, "fk_rot": 3.936e-7, "fk_step": 2.021e-7, "dist": 8.161e-7, "ident": 3.725e-9},
    "panda": {"fk_pos": 3.016e-7, "fk_rot": 4.577e-7, "fk_step": 5.127e-7, "dist": 4.489e-7, "ident": 0.0},
    "baxter": {"fk_pos": 3.766e-7, "fk_rot": 4.872e-7, "fk_step": 4.974e-7, "dist": 7.395e-7, "ident": 8.941e-8},
}
# ... with a floor under the identity bound, as tests/test_distance.py has one under its gap allowance: the two answers come from two fp32 evaluations of the
# same poses (this kernel's FK, the step path's forward()), coordinates up to 2 m whose ulp is 2^-23 m; one run that measured 0 (Panda) or a few 1e-9 promises
# no more than that a few of those roundings may differ elsewhere
IDENT_FLOOR = 4 * 2.0 ** -23
BOUND = {s: {k: max(4 * v, IDENT_FLOOR) if k == "ident" else 4 * v for k, v in m.items()} for s, m in MEASURED.items()}
SHAPES = ((3, 5), (65, 3), (2, 70))


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def state(hb):
    return hb.get("qpos").astype(np.float64), hb.get("xpos").astype(np.float64), hb.get("xquat").astype(np.float64)


# ---- the figures (also what tools/clearance_parity.py prints) ------------------------------------------------------------------------------------------
def fk_figures(flat, hb, dofs, q, overrides=None):
    """config_fk at q [B, K, n] -> (xpos, xquat float64 [B, K, nbody, .], {"fk_pos", "fk_rot"} against the mirror); unmoved bodies are asserted bitwise"""
    xp, xq = (t.cpu().numpy() for t in hb.config_fk(dofs, dev(q)))
    B, K = q.shape[:2]
    assert xp.shape == (B, K, int(flat.nbody), 3) and xq.shape == (B, K, int(flat.nbody), 4) and xp.dtype == np.float32
    still = clearance.signatures(flat, dofs) == 0
    now_p, now_q = hb.get("xpos"), hb.get("xquat")
    assert np.array_equal(xp[:, :, still], np.broadcast_to(now_p[:, None, still], xp[:, :, still].shape))      # bit for bit the env's pose
    assert np.array_equal(xq[:, :, still], np.broadcast_to(now_q[:, None, still], xq[:, :, still].shape))
    rp, rq = S.fk_reference(flat, hb.get("qpos").astype(np.float64), dofs, q, overrides)
    xp, xq = xp.astype(np.float64), xq.astype(np.float64)
    return xp, xq, {"fk_pos": float(np.linalg.norm(xp - rp, axis=-1).max()), "fk_rot": float(S.rot_angle(xq, rq).max())}


def step_fk_figure(flat, cfg, hb, dofs, q, xp):
    """the candidates written into a second batch's qpos, forward(), xpos: worst position difference to config_fk's xp"""
    hm2, hb2 = make_hip(flat, cfg, B=q.shape[0])
    qa = np.asarray(flat.arrays["jnt_qposadr"]).ravel()[[int(np.flatnonzero(np.asarray(flat.arrays["jnt_dofadr"]).ravel() == d)[0]) for d in dofs]]
    worst = 0.0
    for k in range(q.shape[1]):
        qpos = hb.get("qpos")
        qpos[:, qa] = q[:, k].astype(np.float32)
        hb2.set("qpos", qpos); hb2.forward()
        worst = max(worst, float(np.linalg.norm(hb2.get("xpos").astype(np.float64) - xp[:, k], axis=-1).max()))
    return worst


def clear_figures(flat, out, xp, xq, pairs, distmax, bound, params=None, ref=None):
    """device (dist, pair, fromto, status) [B, K(, 6)] against the mirror at poses xp / xq [B, K, nbody, .] (the device's own).  Asserted here: shapes, no
    iteration cap, what a far candidate reads, and that far is far outside 2 `bound` of distmax.  Returned with the reference, for check(): "dist" = worst
    |dist - min_ref|, "witness" = how far a reported point lies outside its solid or |p2 - p1| is off |dist| (status 0 or 2), "pick" = how far the chosen
    pair's reference distance lies above the minimum."""
    dist, pair, ft, st = (o.cpu().numpy() for o in out)
    params = S.params32(flat) if params is None else params
    d_ref = ref if ref is not None else S.pair_reference(flat, xp, xq, pairs, params)[0]
    m_ref = d_ref.min(axis=-1)
    far = m_ref >= distmax
    err = np.abs(dist.astype(np.float64) - np.where(far, distmax, m_ref))
    assert dist.shape == pair.shape == st.shape == m_ref.shape and ft.shape == m_ref.shape + (6,)
    assert not (st & distance.CAP).any()
    none = pair < 0
    edge = np.abs(m_ref - distmax) <= 2 * bound
    assert (none == far)[~edge].all(), np.argwhere((none != far) & ~edge)[:8]
    assert (dist[none] == np.float32(distmax)).all() and (ft[none] == 0).all() and (st[none] == distance.FAR).all()
    assert (pair[~none] < len(pairs)).all() and ((st[~none] & distance.FAR) == 0).all()
    ee, kk = np.nonzero(~none)
    pick = float((d_ref[ee, kk, pair[~none]] - m_ref[~none]).max()) if len(ee) else 0.0      # how far the chosen pair's distance is above the minimum
    wit = 0.0
    for e, k in zip(ee, kk):
        if st[e, k] in (distance.OK, distance.OVERLAP):
            pe = params[e] if isinstance(params, list) else params
            pr = pairs[pair[e, k]]
            G = distance.world_geoms(flat, xp[e, k], xq[e, k], pr, pe)
            o1, o2 = D.outside_by(G[int(pr[0])], ft[e, k, :3]), D.outside_by(G[int(pr[1])], ft[e, k, 3:])
            length = float(np.linalg.norm(ft[e, k, 3:].astype(np.float64) - ft[e, k, :3]))
            wit = max(wit, o1, o2, abs(length - abs(float(dist[e, k]))))
    return {"dist": float(err.max()), "witness": wit, "pick": pick}, d_ref


def ident_figure(hb, flat, dofs, pairs, distmax):
    """K = 1 at the env's own controlled joints, 2-D tensors, against torch.min over geom_distance of the same list"""
    qa = np.asarray(flat.arrays["jnt_qposadr"]).ravel()[[int(np.flatnonzero(np.asarray(flat.arrays["jnt_dofadr"]).ravel() == d)[0]) for d in dofs]]
    q = dev(hb.get("qpos")[:, qa])
    d, pair, ft, st = hb.config_clearance(dofs, q, pairs=pairs, distmax=distmax)
    assert d.shape == (hb.B,) and pair.shape == (hb.B,) and ft.shape == (hb.B, 6) and st.shape == (hb.B,)
    full = hb.geom_distance(pairs, distmax=distmax)
    m = full[0].min(dim=1).values
    return float((d - m).abs().max())


def bound_of(scene, key):
    """witnesses are held to the distance bound, the chosen pair to twice that (it holds at ties and in the touching band alike)"""
    return BOUND[scene]["dist"] if key == "witness" else 2 * BOUND[scene]["dist"] if key == "pick" else BOUND[scene][key]


def check(scene, fig):
    for k, v in fig.items():
        print(f"clearance parity scene {scene}: {k} {v:.3e} (bound {bound_of(scene, k):.1e})")
    for k, v in fig.items():
        assert v <= bound_of(scene, k), (scene, k, v)


# ---- scene T -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_t(tmp_path_factory):
    return S.scene_t(tmp_path_factory.mktemp("clear_t")), {}


def batch_t(scene_t, B, K, which="all"):
    """the batch of B envs at the seeded state, the candidates, the device's poses at them and the mirror's pair distances there -- made once per shape"""
    flat, cache = scene_t
    key = (B, K, which)
    if key not in cache:
        hm, hb = make_hip(flat, None, B=B)
        hb.set("qpos", S.scene_t_qpos(flat, B).astype(np.float32)); hb.forward()
        dofs = S.dofs_t(flat, which)
        q = S.candidates(flat, dofs, B, K)
        pairs = clearance.default_pairs(flat, dofs)
        xp, xq, fig = fk_figures(flat, hb, dofs, q)
        cache[key] = dict(hm=hm, hb=hb, dofs=dofs, q=q, pairs=pairs, xp=xp, xq=xq, fk=fig, ref=S.pair_reference(flat, xp, xq, pairs, S.params32(flat))[0])
    return cache[key]


@pytest.mark.parametrize("B,K", SHAPES)
def test_fk_scene_t(scene_t, B, K):
    flat, _ = scene_t
    c = batch_t(scene_t, B, K)
    check("T", c["fk"])
    if (B, K) == SHAPES[0]:
        check("T", {"fk_step": step_fk_figure(flat, None, c["hb"], c["dofs"], c["q"], c["xp"])})
        arm = batch_t(scene_t, B, K, "arm")      # the other dof list: the side link is then held
        check("T", arm["fk"])


@pytest.mark.parametrize("B,K", SHAPES)
def test_clearance_scene_t(scene_t, B, K):
    flat, _ = scene_t
    c = batch_t(scene_t, B, K)
    hb = c["hb"]
    assert np.array_equal(hb.config_pairs(c["dofs"]), c["pairs"])
    out = hb.config_clearance(c["dofs"], dev(c["q"]), distmax=S.DISTMAX_T)      # the default list
    assert out[0].dtype == torch.float32 and out[1].dtype == torch.int32 and out[3].dtype == torch.int32 and out[0].shape == (B, K)
    fig, _ = clear_figures(flat, out, c["xp"], c["xq"], c["pairs"], S.DISTMAX_T, BOUND["T"]["dist"], ref=c["ref"])
    check("T", fig)
    pair, st = out[1].cpu().numpy(), out[3].cpu().numpy()
    assert (pair < 0).any() and (st == distance.OK).any() and (st == distance.OVERLAP).any()      # far, separated, overlapping
    assert (out[0] < 0).any() == bool((c["ref"].min(axis=-1) < -2 * BOUND["T"]["dist"]).any())     # ... and signed where the mirror has one (not at 15 candidates)
    given = hb.config_clearance(c["dofs"], dev(c["q"]), pairs=c["pairs"], distmax=S.DISTMAX_T)      # the same list, given: the same answer
    assert all(torch.equal(a, b) for a, b in zip(out, given))
    d_only = hb.config_clearance(c["dofs"], dev(c["q"]), distmax=S.DISTMAX_T, fromto=False)
    assert d_only[2] is None and torch.equal(d_only[0], out[0]) and torch.equal(d_only[1], out[1])


def test_explicit_list_with_static_pairs_scene_t(scene_t):
    flat, _ = scene_t
    c = batch_t(scene_t, *SHAPES[0])
    pairs = D.all_pairs(flat)      # every pair the distance query accepts: static pairs and pairs no candidate changes included
    out = c["hb"].config_clearance(c["dofs"], dev(c["q"]), pairs=pairs, distmax=1.0)
    fig, _ = clear_figures(flat, out, c["xp"], c["xq"], pairs, 1.0, BOUND["T"]["dist"])
    check("T", fig)


def test_chunking_scene_t(scene_t):
    flat, _ = scene_t
    B, K = SHAPES[1]
    c = batch_t(scene_t, B, K)
    hb, q = c["hb"], dev(c["q"])
    base = hb.config_clearance(c["dofs"], q, distmax=S.DISTMAX_T, chunks=1)
    for chunks in (2, len(c["pairs"]), 0, 7):
        out = hb.config_clearance(c["dofs"], q, distmax=S.DISTMAX_T, chunks=chunks)
        fig, _ = clear_figures(flat, out, c["xp"], c["xq"], c["pairs"], S.DISTMAX_T, BOUND["T"]["dist"], ref=c["ref"])
        check("T", fig)
        assert float((out[0] - base[0]).abs().max()) <= BOUND["T"]["dist"]
        again = hb.config_clearance(c["dofs"], q, distmax=S.DISTMAX_T, chunks=chunks)      # a repeat call: bit-identical
        assert all(torch.equal(a, b) for a, b in zip(out, again))


def test_identity_with_geom_distance_scene_t(scene_t):
    flat, _ = scene_t
    c = batch_t(scene_t, *SHAPES[0])
    check("T", {"ident": ident_figure(c["hb"], flat, c["dofs"], c["pairs"], S.DISTMAX_T)})
    q2 = dev(c["q"][:, 0])      # the 2-D convention against the same candidates as [B, 1, n]
    a = c["hb"].config_clearance(c["dofs"], q2, distmax=S.DISTMAX_T)
    b = c["hb"].config_clearance(c["dofs"], q2[:, None], distmax=S.DISTMAX_T)
    assert all(torch.equal(x, y[:, 0]) for x, y in zip(a, b))
    f2, f3 = c["hb"].config_fk(c["dofs"], q2), c["hb"].config_fk(c["dofs"], q2[:, None])
    assert f2[0].shape == (3, int(flat.nbody), 3) and torch.equal(f2[0], f3[0][:, 0]) and torch.equal(f2[1], f3[1][:, 0])


def test_per_env_parameters_scene_t(tmp_path):
    flat = S.scene_t(tmp_path)
    B, K = 3, 5
    hm, hb = make_hip(flat, None, B=B, per_env=True)
    hb.set("qpos", np.repeat(S.scene_t_qpos(flat, 1), B, axis=0).astype(np.float32)); hb.forward()      # the same state in every env
    dofs = S.dofs_t(flat, "all")
    q = np.repeat(S.candidates(flat, dofs, 1, K), B, axis=0)                                              # ... and the same candidates
    pairs = clearance.default_pairs(flat, dofs)
    before = hb.config_clearance(dofs, dev(q), distmax=1.0)
    bp, gs = hb.param_get("body_pos"), hb.param_get("geom_size")
    b, g = flat.names["body"].index("l1"), flat.names["geom"].index("g_cyl")
    bp[1, b] += [0.05, -0.03, 0.04]; gs[1, g] = gs[1, g] * [1.6, 1.3, 1.0]
    hb.param_set("body_pos", bp[1:2], env0=1); hb.param_set("geom_size", gs[1:2], env0=1)
    hb.forward()
    live = {k: hb.param_get(k) for k in ("body_pos", "geom_size", "geom_pos", "geom_quat")}
    over = [{"body_pos": S.f32(live["body_pos"][e])} for e in range(B)]
    params = [{k: S.f32(live[k][e]) for k in ("geom_size", "geom_pos", "geom_quat")} for e in range(B)]
    xp, xq, fig = fk_figures(flat, hb, dofs, q, over)
    check("T", fig)
    assert np.abs(xp[1] - xp[0]).max() > 0.03 and np.array_equal(xp[0], xp[2])      # env 1's link moved, the others are as one another
    after = hb.config_clearance(dofs, dev(q), distmax=1.0)
    fig, _ = clear_figures(flat, after, xp, xq, pairs, 1.0, BOUND["T"]["dist"], params=params)
    check("T", fig)
    for a, c in zip(before, after):
        assert torch.equal(a[0], c[0]) and torch.equal(a[2], c[2])                   # the other envs' results are unchanged
    assert not torch.equal(before[0][1], after[0][1])


def test_python_level_refusals_scene_t(scene_t):
    flat, _ = scene_t
    c = batch_t(scene_t, *SHAPES[0])
    hb, dofs, q = c["hb"], c["dofs"], dev(c["q"])
    free_dof = int(np.asarray(flat.arrays["jnt_dofadr"]).ravel()[flat.names["joint"].index("fsj")])
    for call in (lambda *a, **k: hb.config_clearance(*a, **k), lambda *a, **k: hb.config_fk(*a, **k)):
        with pytest.raises(backend.RsimError, match="CUDA tensor"):
            call(dofs, q.cpu())                                                     # wrong device
        with pytest.raises(backend.RsimError, match="shape"):
            call(dofs, q[:, :, :3])                                                 # wrong shape
        with pytest.raises(backend.RsimError, match="shape"):
            call(dofs, q[:, :0])                                                    # K = 0
        with pytest.raises(backend.RsimError, match="free joint"):
            call([free_dof] + dofs[1:], q)
        with pytest.raises(backend.RsimError, match="listed twice"):
            call([dofs[0]] + dofs[:3], q)
        with pytest.raises(backend.RsimError, match="out of range"):
            call([999] + dofs[1:], q)
    with pytest.raises(backend.RsimError, match="ndof"):
        hb.config_pairs([])
    gn = flat.names["geom"].index
    for bad, word in (([[0, 99]], "out of range"), ([[gn("g_cap"), gn("g_cap")]], "against itself"), (np.zeros((0, 2), dtype=np.int32), "npair < 1")):
        with pytest.raises(backend.RsimError, match=word):
            hb.config_clearance(dofs, q, pairs=bad)
    with pytest.raises(backend.RsimError, match="max_iters"):
        hb.config_clearance(dofs, q, max_iters=0)


# ---- Panda and Baxter: the default list, both classes present ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("panda", "baxter_right", "baxter_left", "baxter_both"))
def test_arms_default_list(name):
    s = S.arm(name)
    flat, cfg, dofs = s["flat"], s["cfg"], s["dofs"]
    scene = "panda" if name == "panda" else "baxter"
    B, K = SHAPES[0]
    hm, hb = make_hip(flat, cfg, B=B)
    hb.set("qpos", np.tile(s["qpos"], (B, 1)).astype(np.float32)); hb.set("qvel", 0); hb.forward()
    q = S.candidates(flat, dofs, B, K)
    pairs = clearance.default_pairs(flat, dofs)
    assert np.array_equal(hb.config_pairs(dofs), pairs)
    xp, xq, fig = fk_figures(flat, hb, dofs, q)
    check(scene, fig)
    if name in ("panda", "baxter_both"):
        check(scene, {"fk_step": step_fk_figure(flat, cfg, hb, dofs, q, xp)})
    out = hb.config_clearance(dofs, dev(q), distmax=S.DISTMAX_ARM)
    fig, d_ref = clear_figures(flat, out, xp, xq, pairs, S.DISTMAX_ARM, BOUND[scene]["dist"])
    check(scene, fig)
    m_ref = d_ref.min(axis=-1)
    assert (m_ref > 1e-4).any() and (m_ref <= 0).any()      # free and colliding candidates: both classes are present
    d = out[0].cpu().numpy()
    assert (d > 1e-4).any() and (d <= 0).any()
    check(scene, {"ident": ident_figure(hb, flat, dofs, pairs, S.DISTMAX_ARM)})


# ---- purity ----------------------------------------------------------------------------------------------------------------------------------------------
def _actions(hm, B, t):
    a = torch.zeros((B, hm.action_dim), device="cuda")
    a[:, 0] = 0.5; a[1, 2] = -0.8; a[2, 1] = 0.6; a[:, -1] = 1.0 if t % 2 else -1.0
    return a


def _lift():
    """the shipped Lift / Panda asset, its arm's dofs"""
    from tests import raycast_scenes as R

    flat, cfg = R.lift()
    return dict(flat=flat, cfg=cfg, dofs=list(range(7)), qpos=R.lift_init_qpos(flat, cfg))


def _lift_batch(B=3):
    s = _lift()
    hm, hb = make_hip(s["flat"], s["cfg"], B=B)
    hb.set("qpos", np.tile(s["qpos"], (B, 1)).astype(np.float32)); hb.set("qvel", 0)
    hb.forward(); hb.ctrl_reset()
    return s, hm, hb


def test_state_is_bitwise_unchanged_by_both_calls():
    s, hm, hb = _lift_batch()
    q = dev(S.candidates(s["flat"], s["dofs"], 3, 5))
    names = ("qpos", "qvel", "time", "xpos", "xquat")
    before = [hb.get(n).copy() for n in names]
    hb.config_fk(s["dofs"], q); hb.config_clearance(s["dofs"], q)
    for n, a in zip(names, before):
        assert np.array_equal(a, hb.get(n)), n


def test_a_query_between_control_steps_changes_nothing_ten_steps_later():
    got = []
    for ask in (False, True):
        s, hm, hb = _lift_batch()
        q = dev(S.candidates(s["flat"], s["dofs"], 3, 5))
        for t in range(10):
            hb.control_step(_actions(hm, 3, t), 25)
            if ask and t in (0, 4):
                hb.config_clearance(s["dofs"], q); hb.config_fk(s["dofs"], q)
        got.append((hb.get("qpos").copy(), hb.get("qvel").copy()))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


def test_unmoved_bodies_are_current_behind_a_fused_step():
    s, hm, hb = _lift_batch()
    flat = s["flat"]
    dofs = [s["dofs"][-1]]      # the last arm joint alone: the links before it are not moved by the candidate, and they move in the step
    xp0 = hb.get("xpos").copy()
    hb.control_step(_actions(hm, 3, 0), 25)      # the derived arrays are stale now: the query brings them up first
    q = dev(np.zeros((3, 2, 1)))
    xp, xq = (t.cpu().numpy() for t in hb.config_fk(dofs, q))
    still = clearance.signatures(flat, dofs) == 0
    now = hb.get("xpos")
    assert np.abs(now - xp0).max() > 1e-4
    assert np.array_equal(xp[:, :, still], np.broadcast_to(now[:, None, still], xp[:, :, still].shape))
    hb.control_step(_actions(hm, 3, 1), 25)
    d, pair, ft, st = hb.config_clearance(dofs, q)      # ... and so does the clearance entry: it equals the query on the refreshed poses
    again = hb.config_clearance(dofs, q)
    assert torch.equal(d, again[0]) and np.abs(hb.get("xpos") - now).max() > 1e-4


def test_vec_env_composition():
    from robosuite_amd.vec_env import VecEnv

    s = _lift()
    env = VecEnv("Lift", 3, s["flat"], s["cfg"], horizon=50)
    env.reset()
    q = dev(S.candidates(s["flat"], s["dofs"], 3, 5))
    d, pair, ft, st = env.config_clearance(q)
    ref = env.env.batch.config_clearance(s["dofs"], q)
    assert all(torch.equal(a, b) for a, b in zip((d, pair, ft, st), ref))
    xp, xq = env.config_fk(q)
    assert xp.shape == (3, 5, int(s["flat"].nbody), 3)
    named = [("gripper0_right_finger1_pad_collision", "cube_g0"), ("table_collision", s["flat"].names["geom"].index("gripper0_right_hand_collision"))]
    d2, pair2, _, _ = env.config_clearance(q, pairs=named)
    assert d2.shape == (3, 5) and int(pair2.max()) <= 1
    with pytest.raises(KeyError):
        env.config_clearance(q, pairs=[("no_such_geom", "cube_g0")])
    with pytest.raises(ValueError):
        env.config_clearance(q, arm=1)
