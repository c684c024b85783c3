"""Geom distance on the device (csrc/rsim_dist.hip, rsim_geom_distance) against the fp64 host mirror (robosuite_amd/distance.py) on the state read back from the
device, with the model's geometry rounded to fp32 as the device holds it.

  * dist is compared on EVERY pair of every env: |d - d_ref| in metres stays under BOUND, four times the worst value one GPU run measured per scene
    (profiles/distance_parity.txt; the margin is for one box, one run and pose-dependent rounding).  dist is 1-Lipschitz in every translation, so nothing is
    left out.
  * status is compared, and fromto goes through the certificate (it is NOT compared to the mirror's points: witnesses are not unique on parallel faces),
    only outside the band the mirror alone defines: |d| and |d - distmax| above 1e-4 m, an overlap of general convex shapes deeper than that
    (distance_scenes.reference).  At most 10 % of a scene's pairs may be left out (asserted here and, on the mirror alone, in tests/test_distance_host.py).
    Certificate: both witnesses inside their solids and |p2 - p1| = dist, each within BOUND; the certified gap -- |p2 - p1| minus the separation of the solids
    along the witnesses' direction -- within tol plus GAP_ALLOW, four times the worst excess over tol that run measured.
  * no result carries the iteration-cap bit at the default max_iters (the host rehearsal, tests/test_distance_core_host.py, shows the same on the same inputs).

The common point of a status-2 overlap is held inside both solids within the same BOUND.  Figures: profiles/distance_parity.txt."""
import numpy as np
import pytest
import torch

from robosuite_amd import backend, distance
from tests import distance_scenes as S
from tests import raycast_scenes as R
from tests.util import make_hip

pytestmark = pytest.mark.gpu

TOL = distance.DEFAULTS["tol"]
# worst |d - d_ref| per scene of one GPU run (profiles/distance_parity.txt), and the worst certified gap beyond tol; the tests assert 4 x
# (one run of the build the Makefile makes: rsim_dist.o without the SLP packer.  With the packer on the same source measured A 9.210e-7 / 3.304e-5: the gap of
# a pair a few 1e-4 m apart is decided by which rounding ends its iteration, the distance is not)
MEASURED = {"A": 9.015e-7, "H": 4.406e-8, "L": 9.455e-7}
GAP_MEASURED = {"A": 1.0702e-3, "H": 0.0, "L": 4.215e-9}
BOUND = {k: 4 * v for k, v in MEASURED.items()}
# ... with a floor under the gap allowance: the certificate is evaluated on fp32 witnesses, whose coordinates (up to 2 m here) carry 2^-23 m each, so an excess of
# a few of those is rounding of the check itself, whatever one run measured (scene H measured 0: four times that would leave no margin at all)
GAP_FLOOR = 4 * 2.0 ** -23
GAP_ALLOW = {k: max(4 * v, GAP_FLOOR) for k, v in GAP_MEASURED.items()}
WORST, WORST_GAP = {}, {}


def hold(scene, flat, pairs, xp, xq, out, distmax, params=None, ref=None, cap=True):
    """device (dist, fromto, status) [B, P(, 6)] of `pairs` against the mirror; returns the reference"""
    dist, ft, st = (o.cpu().numpy() for o in out)
    ref = ref if ref is not None else S.reference(flat, xp, xq, pairs, distmax, S.params32(flat) if params is None else params)
    assert dist.shape == st.shape == ref["dist"].shape and ft.shape == ref["fromto"].shape
    err = np.abs(dist.astype(np.float64) - ref["dist"])
    band = ref["band"]
    WORST[scene] = max(WORST.get(scene, 0.0), float(err.max()))
    print(f"distance parity scene {scene}: {err.size} pairs, worst |d - d_ref| {err.max():.3e} (bound {BOUND[scene]:.1e}), {band.sum()} in the band")
    assert not (st & distance.CAP).any(), (scene, np.argwhere(st & distance.CAP)[:8])
    assert err.max() <= BOUND[scene], (scene, np.unravel_index(err.argmax(), err.shape), float(err.max()))
    if cap:
        assert band.mean() <= S.BAND_SHARE, (scene, int(band.sum()), band.size)
    off = np.argwhere(~band & (st != ref["status"]))
    assert len(off) == 0, (scene, [(int(e), int(k), int(st[e, k]), int(ref["status"][e, k]), float(ref["d"][e, k])) for e, k in off[:8]])
    far = (st & distance.FAR) != 0
    assert (dist[far] == np.float32(distmax)).all() and (ft[far] == 0).all()
    over = ~band & ((st & distance.OVERLAP) != 0)
    assert (dist[over] == 0).all() and (ft[over][:, :3] == ft[over][:, 3:]).all()          # one common point, twice
    worst_gap, worst_out = 0.0, 0.0
    for e in range(len(xp)):
        G = None
        for k in np.flatnonzero(~band[e] & ~far[e]):
            if G is None:
                pe = params[e] if isinstance(params, list) else (S.params32(flat) if params is None else params)
                G = distance.world_geoms(flat, xp[e], xq[e], pairs.ravel(), pe)
            g1, g2 = G[int(pairs[k][0])], G[int(pairs[k][1])]
            o1, o2 = S.outside_by(g1, ft[e, k, :3]), S.outside_by(g2, ft[e, k, 3:])
            # containment within the scene's dist bound: the witnesses of a reported distance, the deepest points of a signed overlap, and the common point
            # of a status-2 overlap alike
            worst_out = max(worst_out, o1, o2)
            assert max(o1, o2) <= BOUND[scene], (scene, e, k, int(st[e, k]), o1, o2)
            if st[e, k] == distance.OK:
                length = float(np.linalg.norm(ft[e, k, 3:].astype(np.float64) - ft[e, k, :3]))
                assert abs(length - abs(float(dist[e, k]))) <= BOUND[scene], (scene, e, k, length, dist[e, k])
                if dist[e, k] > 0:
                    _, _, up, low = S.certificate(g1, g2, ft[e, k])
                    worst_gap = max(worst_gap, up - low - TOL)
    WORST_GAP[scene] = max(WORST_GAP.get(scene, 0.0), worst_gap)
    print(f"   certified gap beyond tol: worst {worst_gap:.3e} (allowance {GAP_ALLOW[scene]:.1e}); worst point outside its solid {worst_out:.3e}")
    assert worst_gap <= GAP_ALLOW[scene], (scene, worst_gap)
    return ref


def poses(hb):
    return hb.get("xpos").astype(np.float64), hb.get("xquat").astype(np.float64)


# ---- Scene A: every geom type, every pair ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flat_a(tmp_path_factory):
    flat = S.scene_a(tmp_path_factory.mktemp("dist_a"))
    return flat, S.all_pairs(flat), {}


def batch_a(flat_a, B):
    """the batch of B envs at the seeded poses (env e is the same in every B), its poses read back, and the mirror's reference -- made once per B"""
    flat, pairs, cache = flat_a
    if B not in cache:
        hm, hb = make_hip(flat, None, B=B)
        hb.set("qpos", S.scene_a_qpos(flat, B).astype(np.float32))
        hb.forward()
        xp, xq = poses(hb)
        cache[B] = (hm, hb, xp, xq, S.reference(flat, xp, xq, pairs, S.DISTMAX, S.params32(flat)))
    return cache[B]


@pytest.mark.parametrize("B", (3, 65, 130))      # one partial wavefront; a second and a third env block, the last one partial
def test_every_pair_scene_a(flat_a, B):
    flat, pairs, _ = flat_a
    hm, hb, xp, xq, ref = batch_a(flat_a, B)
    out = hb.geom_distance(pairs, distmax=S.DISTMAX)
    assert out[0].shape == (B, len(pairs)) and out[1].shape == (B, len(pairs), 6) and out[2].shape == (B, len(pairs))
    assert out[0].dtype == torch.float32 and out[2].dtype == torch.int32
    hold("A", flat, pairs, xp, xq, out, S.DISTMAX, ref=ref)
    st = out[2].cpu().numpy()
    assert (st == distance.OK).any() and (st == distance.FAR).any() and (st == distance.OVERLAP).any() and (out[0] < -S.BAND).any()
    again = hb.geom_distance(pairs, distmax=S.DISTMAX)                                     # a repeat call with the same list: bit-identical
    assert all(torch.equal(a, b) for a, b in zip(out, again))
    d_only = hb.geom_distance(pairs, distmax=S.DISTMAX, fromto=False)
    assert d_only[1] is None and torch.equal(d_only[0], out[0]) and torch.equal(d_only[2], out[2])


@pytest.mark.parametrize("B", (3, 130))
def test_one_pair_scene_a(flat_a, B):
    flat, pairs, _ = flat_a
    hm, hb, xp, xq, ref = batch_a(flat_a, B)
    names = flat.names["geom"]
    for a, b in (("cyl", "box"), ("box2", "box"), ("cyl2", "floor"), ("floor", "msh")):      # P = 1, either order of a plane pair
        one = np.array([[names.index(a), names.index(b)]], dtype=np.int32)
        hold("A", flat, one, xp, xq, hb.geom_distance(one, distmax=S.DISTMAX), S.DISTMAX, cap=False)


def test_distmax_scene_a(flat_a):
    flat, pairs, _ = flat_a
    hm, hb, xp, xq, ref = batch_a(flat_a, 3)
    e, k = np.argwhere((ref["d"] > 0.2) & (ref["d"] < 0.5))[0]
    one = pairs[k:k + 1]
    d, ft, st = (o.cpu().numpy() for o in hb.geom_distance(one, distmax=0.1))
    assert d[e, 0] == np.float32(0.1) and (ft[e, 0] == 0).all() and st[e, 0] == distance.FAR       # beyond distmax: (distmax, zeros, 1)
    d, ft, st = (o.cpu().numpy() for o in hb.geom_distance(one, distmax=2.0))
    assert abs(d[e, 0] - ref["d"][e, k]) <= BOUND["A"] and st[e, 0] == distance.OK and np.abs(ft[e, 0]).max() > 0      # a larger distmax: its distance


def test_refusals_by_name(flat_a):
    flat, pairs, _ = flat_a
    hm, hb, xp, xq, ref = batch_a(flat_a, 3)
    for bad, word in (([[0, 99]], "out of range"), ([[3, 3]], "against itself"), (np.zeros((0, 2), dtype=np.int32), "npair < 1")):
        with pytest.raises(backend.RsimError, match=word):
            hb.geom_distance(bad)
    with pytest.raises(backend.RsimError, match="max_iters"):
        hb.geom_distance(pairs, max_iters=0)


def test_per_env_box_size(tmp_path):
    flat = S.scene_a(tmp_path)
    hm, hb = make_hip(flat, None, B=2, per_env=True)
    hb.set("qpos", np.repeat(S.scene_a_qpos(flat, 1), 2, axis=0).astype(np.float32))       # the same pose twice
    g = flat.names["geom"].index("box")
    pairs = np.array([p for p in S.all_pairs(flat) if g in p], dtype=np.int32)
    size = hb.param_get("geom_size")
    size[1, g] = size[1, g] * [1.5, 0.5, 1.25]
    hb.param_set("geom_size", size[1:2], env0=1)
    hb.forward()
    xp, xq = poses(hb)
    live = hb.param_get("geom_size")
    params = [dict(S.params32(flat), geom_size=S.f32(live[e])) for e in range(2)]
    out = hb.geom_distance(pairs, distmax=S.DISTMAX)
    hold("A", flat, pairs, xp, xq, out, S.DISTMAX, params=params, cap=False)
    d = out[0].cpu().numpy()
    same = S.reference(flat, xp[:1], xq[:1], pairs, S.DISTMAX, S.params32(flat))["dist"][0]
    assert np.abs(d[0] - same).max() <= BOUND["A"] and np.abs(d[1] - d[0]).max() > 1e-3       # env 1's override changes env 1's distances only


# ---- Scene H: hulls of 4 and of more than 256 vertices -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (3, 65))
def test_hull_sizes_scene_h(tmp_path, B):
    flat = S.scene_h(tmp_path)
    assert sorted(int(n) for n in np.asarray(flat.arrays["mesh_vertnum"]).ravel()) == [4, S.N_BIG]
    hm, hb = make_hip(flat, None, B=B)
    hb.set("qpos", S.scene_h_qpos(flat, B).astype(np.float32))
    hb.forward()
    xp, xq = poses(hb)
    pairs = S.all_pairs(flat)
    hold("H", flat, pairs, xp, xq, hb.geom_distance(pairs, distmax=S.DISTMAX_H), S.DISTMAX_H)
    hold("H", flat, pairs[::-1, ::-1].copy(), xp, xq, hb.geom_distance(pairs[::-1, ::-1].copy(), distmax=S.DISTMAX_H), S.DISTMAX_H)      # another list, geoms swapped


# ---- Scene L: Lift / Panda --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_l():
    flat, cfg = R.lift()
    hm, hb = make_hip(flat, cfg, B=3)
    hb.set("qpos", np.tile(R.lift_init_qpos(flat, cfg), (3, 1)).astype(np.float32)); hb.set("qvel", 0)
    hb.forward(); hb.ctrl_reset()
    return flat, cfg, hm, hb, distance.body_pairs(flat, *S.lift_bodies(flat))


def _actions(hm, t):
    a = torch.zeros((3, hm.action_dim), device="cuda")
    a[:, 0] = 0.5; a[1, 2] = -0.8; a[2, 1] = 0.6; a[:, -1] = 1.0 if t else -1.0
    return a


def test_reset_pose_and_after_three_fused_steps_scene_l(scene_l):
    flat, cfg, hm, hb, pairs = scene_l
    out = hb.geom_distance(pairs, distmax=S.DISTMAX_L)
    xp0, xq0 = poses(hb)
    hold("L", flat, pairs, xp0, xq0, out, S.DISTMAX_L)
    for t in range(3):
        hb.control_step(_actions(hm, t), 25)
    out = hb.geom_distance(pairs, distmax=S.DISTMAX_L)          # the derived arrays are stale behind a fused step: the query brings them up first
    xp, xq = poses(hb)
    assert np.abs(xp - xp0).max() > 1e-3
    hold("L", flat, pairs, xp, xq, out, S.DISTMAX_L)
    assert not torch.equal(out[0][0], out[0][1])
    with pytest.raises(backend.RsimError, match="visual-only mesh"):
        hb.geom_distance([[flat.names["geom"].index("robot0_g0_vis"), flat.names["geom"].index("table_collision")]])


def test_pure_query_scene_l():
    flat, cfg = R.lift()
    pairs = distance.body_pairs(flat, *S.lift_bodies(flat))
    got = []
    for ask in (False, True):
        hm, hb = make_hip(flat, cfg, B=3)
        hb.set("qpos", np.tile(R.lift_init_qpos(flat, cfg), (3, 1)).astype(np.float32)); hb.set("qvel", 0)
        hb.forward(); hb.ctrl_reset()
        hb.control_step(_actions(hm, 0), 25)
        if ask:
            hb.geom_distance(pairs, distmax=S.DISTMAX_L)
        q1, v1 = hb.get("qpos").copy(), hb.get("qvel").copy()
        hb.control_step(_actions(hm, 1), 25)
        got.append((q1, v1, hb.get("qpos").copy(), hb.get("qvel").copy()))
    for a, b in zip(*got):
        assert np.array_equal(a, b)      # bit-identical with and without a query in between


def test_vec_env_by_name_and_body_distance_scene_l():
    from robosuite_amd.vec_env import VecEnv

    flat, cfg = R.lift()
    env = VecEnv("Lift", 3, flat, cfg, horizon=50)
    env.reset()
    env.step(torch.zeros((3, env.action_dim), device="cuda"))
    named = [("gripper0_right_finger1_pad_collision", "cube_g0"), ("table_collision", flat.names["geom"].index("gripper0_right_hand_collision"))]
    d, ft, st = env.geom_distance(named, distmax=S.DISTMAX_L)
    hb = env.env.batch
    xp, xq = poses(hb)
    live = {k: hb.param_get(k) for k in ("geom_size", "geom_pos", "geom_quat")}      # a Lift env has its own cube: the geometry each env holds
    params = [{k: S.f32(v[e]) for k, v in live.items()} for e in range(3)]
    ids = np.array([[flat.names["geom"].index(g) if isinstance(g, str) else g for g in pr] for pr in named], dtype=np.int32)
    hold("L", flat, ids, xp, xq, (d, ft, st), S.DISTMAX_L, params=params, cap=False)
    with pytest.raises(KeyError):
        env.geom_distance([("no_such_geom", "cube_g0")])
    dm, fm, k, pairs = env.body_distance(S.L_ROBOT, S.L_SCENE, distmax=S.DISTMAX_L)
    assert np.array_equal(pairs, distance.body_pairs(flat, *S.lift_bodies(flat))) and dm.shape == (3,) and fm.shape == (3, 6) and k.shape == (3,)
    ref = S.reference(flat, xp, xq, pairs, S.DISTMAX_L, params)
    rd, rf, rk = distance.reduce_min(ref["dist"], ref["fromto"])
    assert np.abs(dm.cpu().numpy() - rd).max() <= BOUND["L"]
    full = hb.geom_distance(pairs, distmax=S.DISTMAX_L)
    assert torch.equal(dm, full[0].min(dim=1).values) and torch.equal(fm, full[1][torch.arange(3), k])      # the reduction is torch.min over the pair list
