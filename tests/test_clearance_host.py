"""The fp64 mirror of the configuration clearance query (robosuite_amd/clearance.py) on its own, on the CPU: FK against mjcf.kinematics_np and ik.fk, the
default pair list's rule on Panda, the minimum against brute force, the share of free and of colliding candidates among the seeded Panda draws (the property
tests/test_clearance.py relies on on the device), and the refusals by name."""
import numpy as np
import pytest

from robosuite_amd import clearance, distance, ik, mjcf
from tests import clearance_scenes as S
from tests import ik_scenes


@pytest.fixture(scope="module")
def scene_t(tmp_path_factory):
    flat = S.scene_t(tmp_path_factory.mktemp("clear_t"))
    return flat, S.scene_t_qpos(flat, 4)


def test_fk_at_the_envs_own_q_is_kinematics_np(scene_t):
    flat, qpos = scene_t
    m32 = clearance._model32(flat)
    qa = np.asarray(flat.arrays["jnt_qposadr"]).ravel().astype(int)
    dadr = np.asarray(flat.arrays["jnt_dofadr"]).ravel().astype(int)
    for which in ("arm", "all"):
        dofs = S.dofs_t(flat, which)
        own = [int(qa[np.flatnonzero(dadr == d)[0]]) for d in dofs]
        for e in range(len(qpos)):
            xp, xq = clearance.fk(flat, qpos[e], dofs, qpos[e][own])
            ref = mjcf.kinematics_np(m32, qpos[e])
            assert np.array_equal(xp, ref[0]) and np.array_equal(xq, ref[1])


@pytest.mark.parametrize("name", ("chain3", "panda"))
def test_fk_agrees_with_ik_fk_on_the_sites_body(name):
    s = ik_scenes.scene(name)
    flat, site, dofs = s["flat"], s["site"], s["dofs"]
    qpos = np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel()
    body = int(np.asarray(flat.arrays["site_bodyid"]).ravel()[site])
    t = ik.rounded(flat)
    lo, hi, qa = ik_scenes.ranges(flat, dofs)
    for k in range(5):
        q = np.random.default_rng([3, k]).uniform(lo, hi)
        xp, xq = clearance.fk(flat, qpos, dofs, q)
        full = qpos.copy(); full[qa] = q
        p, Rs = ik.fk(flat, full, site, overrides=t)
        Rb = mjcf.quat2mat(xq[body])
        # the two fp64 statements differ in one thing: kinematics_np renormalises a hinge axis, ik.fk takes the fp32-rounded axis as it is.  A rounded unit
        # axis is off unit length by at most sqrt(3) 2^-24 ~ 1e-7; over at most seven hinges turning through up to 3 rad with a reach under 1.5 m that is
        # 7 x 3 x 1e-7 rad and 1.5 m times it: 3.2e-6 -- held to 4e-6 (seen: 1.5e-8)
        assert np.abs(xp[body] + Rb @ t["site_pos"][site] - p).max() < 4e-6
        assert np.abs(Rb @ mjcf.quat2mat(mjcf.quat_normalize(t["site_quat"][site])) - Rs).max() < 4e-6


def test_signatures_and_moved_bodies_scene_t(scene_t):
    flat, _ = scene_t
    bn = flat.names["body"].index
    arm, both = S.dofs_t(flat, "arm"), S.dofs_t(flat, "all")
    sig = clearance.signatures(flat, arm)
    assert sig[bn("l0")] == sig[bn("side")] == 0b001 and sig[bn("l1")] == 0b011 and sig[bn("l2")] == sig[bn("f1")] == sig[bn("f2")] == 0b111
    assert sig[0] == sig[bn("fsb")] == sig[bn("fbb")] == 0
    assert clearance.moved_bodies(flat, arm) == sorted(bn(b) for b in ("l0", "side", "l1", "l2", "f1", "f2"))
    sig = clearance.signatures(flat, both)      # columns: hs, h2, h0, s1
    assert sig[bn("l0")] == 0b0100 and sig[bn("side")] == 0b0101 and sig[bn("l1")] == 0b1100 and sig[bn("l2")] == 0b1110
    gb = np.asarray(flat.arrays["geom_bodyid"]).ravel()
    for dofs in (arm, both):
        sig = clearance.signatures(flat, dofs)
        pairs = clearance.default_pairs(flat, dofs)
        every = list(zip(np.asarray(flat.arrays["pair_geom1"]).ravel(), np.asarray(flat.arrays["pair_geom2"]).ravel()))
        assert [tuple(p) for p in pairs] == [(a, b) for a, b in every if sig[gb[a]] != sig[gb[b]]]      # the collision list's order, nothing else dropped
        assert len(pairs) < len(every)


def test_default_pairs_on_panda():
    s = S.arm("panda")
    flat, dofs = s["flat"], s["dofs"]
    gn, bn = flat.names["geom"], flat.names["body"]
    gb = np.asarray(flat.arrays["geom_bodyid"]).ravel()
    pairs = [tuple(int(x) for x in p) for p in clearance.default_pairs(flat, dofs)]
    every = [(int(a), int(b)) for a, b in zip(np.asarray(flat.arrays["pair_geom1"]).ravel(), np.asarray(flat.arrays["pair_geom2"]).ravel())]
    body = lambda g: bn[gb[g]]      # noqa: E731
    finger = lambda g: "finger" in body(g)      # noqa: E731
    link = lambda g: body(g).startswith("robot0_link")      # noqa: E731
    dropped = [p for p in every if p not in pairs]
    assert dropped and set(pairs) <= set(every)
    assert not any(finger(a) and finger(b) for a, b in pairs) and any(finger(a) and finger(b) for a, b in dropped)      # every finger-against-finger pair
    static = lambda g: body(g) in ("world", "table", "cube_main")      # noqa: E731
    assert not any(static(a) and static(b) for a, b in pairs)                                                           # floor / table against the cube
    assert {("world", "cube_main"), ("table", "cube_main")} <= {(body(a), body(b)) for a, b in dropped}
    assert any(link(a) and link(b) for a, b in pairs)                                                                   # link against link stays
    assert any((link(a) and body(b) == "table") or (link(b) and body(a) == "table") for a, b in pairs)                 # ... and link against table
    assert len(gn) > 0


def test_clearance_is_the_brute_force_minimum(scene_t):
    flat, qpos = scene_t
    dofs = S.dofs_t(flat, "all")
    pairs = clearance.default_pairs(flat, dofs)
    q = S.candidates(flat, dofs, len(qpos), 4)
    seen = set()
    for e in range(len(qpos)):
        for k in range(4):
            xp, xq = clearance.fk(flat, qpos[e], dofs, q[e, k])
            d, ft, st = distance.geom_distance(flat, xp, xq, pairs, S.DISTMAX_T)
            got = clearance.clearance(flat, qpos[e], dofs, q[e, k], pairs, distmax=S.DISTMAX_T)
            near = [i for i in range(len(pairs)) if not st[i] & distance.FAR and d[i] < S.DISTMAX_T]
            if not near:
                assert got[0] == S.DISTMAX_T and got[1] == -1 and not got[2].any() and got[3] == distance.FAR
                seen.add("far")
                continue
            best = min(near, key=lambda i: (d[i], i))
            assert got[0] == d[best] and got[1] == best and np.array_equal(got[2], ft[best]) and got[3] == st[best]
            seen.add("near")
    assert seen == {"far", "near"}
    # ties: the same pair listed twice, and two overlaps at 0 -- the lowest index wins
    twice = np.concatenate([pairs, pairs])
    for k in range(4):
        a = clearance.clearance(flat, qpos[0], dofs, q[0, k], pairs, distmax=1.0)
        b = clearance.clearance(flat, qpos[0], dofs, q[0, k], twice, distmax=1.0)
        assert a[0] == b[0] and a[1] == b[1] < len(pairs)


def test_seeded_panda_draws_hold_both_classes():
    """200 draws on the signature rule's default list: at least 10 % free (d > 1e-4) and at least 10 % colliding (d <= 0)"""
    s = S.arm("panda")
    flat, dofs, qpos = s["flat"], s["dofs"], s["qpos"]
    pairs = clearance.default_pairs(flat, dofs)
    q = S.candidates(flat, dofs, 8, 25)
    m32 = clearance._model32(flat)
    d = np.array([clearance.clearance(flat, qpos, dofs, q[e, k], pairs, distmax=S.DISTMAX_ARM, poses=clearance.fk(flat, qpos, dofs, q[e, k], model32=m32))[0]
                  for e in range(8) for k in range(25)])
    free, hit, band = (d > 1e-4).mean(), (d <= 0).mean(), ((d > 0) & (d <= 1e-4)).sum()
    print(f"seeded Panda draws: {free:.1%} free, {hit:.1%} colliding, {band} within 1e-4 m of zero")
    assert free >= 0.10 and hit >= 0.10


def test_refusals_by_name(scene_t):
    flat, qpos = scene_t
    dofs = S.dofs_t(flat, "arm")
    free_dof = int(np.asarray(flat.arrays["jnt_dofadr"]).ravel()[flat.names["joint"].index("fsj")])
    for bad, word in (([], "ndof"), (list(range(17)), "ndof"), ([99], "out of range"), ([dofs[0], dofs[0]], "listed twice"), ([free_dof + 2], "free joint")):
        with pytest.raises(clearance.ClearanceError, match=word):
            clearance.signatures(flat, bad)
    with pytest.raises(clearance.ClearanceError, match="holds 3 positions"):
        clearance.fk(flat, qpos[0], dofs, [0.0, 0.0])
    gn = flat.names["geom"].index
    for bad, word in (([[0, 99]], "out of range"), ([[gn("g_cap"), gn("g_cap")]], "against itself")):
        with pytest.raises(distance.DistanceError, match=word):
            clearance.clearance(flat, qpos[0], dofs, [0.0, 0.0, 0.0], bad)
    only_fingers = S.dofs_of(flat, ("fs1",))      # a finger moves against everything: a list exists; a dof list that moves nothing collidable has none
    assert len(clearance.default_pairs(flat, only_fingers)) > 0
    lone = mjcf.compile_mjcf('<mujoco><worldbody><body><joint name="j" type="hinge"/><geom size="0.1" contype="0" conaffinity="0"/></body></worldbody></mujoco>')
    with pytest.raises(clearance.ClearanceError, match="default pair list is empty"):
        clearance.default_pairs(lone, [0])
