"""Carried objects in the fp64 mirror (robosuite_amd/clearance.py, sweep.py with attach / held / rel) against brute force, on scene T with the sphere `fsb`
attached to the last link and the box `fbb` to the side link (tests/attach_scenes.py).  The kernels are held to the mirror by tests/test_attach.py.

  * attached FK against mjcf.kinematics_np: the free joint's seven qpos entries written to X_carrier(q) o rel, composed HERE from kinematics_np's carrier
    pose with this file's own quaternion algebra; every body agrees to 1e-12.  rel from the state and rel given, every held row.
  * the signature rule against brute force: a pair of the default list is active in an env iff the relative pose of its two bodies changes over 8 random
    candidates (by more than 1e-9); all four held rows.  And the list itself: 44 pairs on this scene, 39 of them active with everything held, 39 with
    nothing held (then exactly the plain default list), five swapped either way.
  * motion bound: the centres of the listed geoms move, per active pair and between neighbours of 129 dense samples, no more than L dt.
  * sweep certificate: against 129 dense samples of the mirror's own attached clearance.
  * refusals, each matched by message: the eight the contract names, in the mirror AND through the C-ABI's host-only entry rsim_config_pairs_attached, whole
    message against whole message.  What is refused below an attached body, and mocap bodies, on scene J (a tool with a jaw), two of them edited copies.
  * a subtree rides along (scene J): against kinematics_np as above; body rates down the subtree.
  * test_condition_for_the_gpu_tests: with attach_scenes' segments, rel given and rel from the state, the mirror decides every GPU-shape segment within
    max_steps / 2, FREE and HIT at t > 0 both among the envs that hold something."""
import numpy as np
import pytest

from robosuite_amd import clearance, distance, mjcf, sweep
from tests import attach_scenes as A
from tests import clearance_scenes as S
from tests import sweep_scenes as W

B, K = 6, 3      # six envs: every held row of attach_scenes.held_rows
ROWS = ((False, False), (True, False), (False, True), (True, True))


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    flat = S.scene_t(tmp_path_factory.mktemp("attach_t"))
    return flat, S.f32(S.scene_t_qpos(flat, B)), clearance._model32(flat), S.dofs_t(flat, "all"), A.attach_t(flat)


def _qmul(a, b):
    w1, x1, y1, z1 = a
    w2, x2, y2, z2 = b
    return np.array([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2, w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2])


def _qrot(q, v):
    return _qmul(_qmul(q, np.concatenate([[0.0], v])), q * [1, -1, -1, -1])[1:]


def _rel_from_state(m32, qpos, att):
    xp, xq = mjcf.kinematics_np(m32, qpos)[:2]
    out = []
    for body, carrier in att:
        conj = xq[carrier] * [1, -1, -1, -1]
        out.append(np.concatenate([_qrot(conj, xp[body] - xp[carrier]), _qmul(conj, xq[body])]))
    return np.asarray(out)


@pytest.mark.parametrize("mode", A.REL_MODES)
def test_attached_fk_against_kinematics_with_the_free_joint_written(scene, mode):
    flat, qpos, m32, dofs, att = scene
    rel = A.rel_of(mode, B)
    q = S.candidates(flat, dofs, B, K)
    jadr, qa = clearance._I(flat, "body_jntadr"), clearance._I(flat, "jnt_qposadr")
    worst = 0.0
    for e in range(B):
        for row in ROWS:
            r = _rel_from_state(m32, qpos[e], att) if rel is None else rel[e]
            for k in range(K):
                qc = clearance.candidate_qpos(flat, qpos[e], dofs, q[e, k])
                cp, cq = mjcf.kinematics_np(m32, qc)[:2]
                for (body, carrier), h, ri in zip(att, row, r):
                    if h:
                        a = qa[jadr[body]]
                        qc[a:a + 3] = cp[carrier] + _qrot(cq[carrier], ri[:3])
                        qc[a + 3:a + 7] = _qmul(cq[carrier], ri[3:] / np.linalg.norm(ri[3:]))
                rp, rq = mjcf.kinematics_np(m32, qc)[:2]
                xp, xq = clearance.fk(flat, qpos[e], dofs, q[e, k], model32=m32, attach=att, held=row, rel=None if rel is None else rel[e])
                worst = max(worst, np.abs(xp - rp).max(), np.abs(xq - rq).max())
                for (body, _), h in zip(att, row):      # held: it went with the carrier; not held: where it was
                    assert (np.linalg.norm(xp[body] - cp[body]) > 1e-3) == bool(h) or mode == "state"
                    if not h:
                        assert np.array_equal(xp[body], cp[body]) and np.array_equal(xq[body], cq[body])
    print(f"attached FK, rel {mode}: worst difference to kinematics_np with the free joint written {worst:.3e}")
    assert worst <= 1e-12


def test_the_default_list_with_attachments(scene):
    flat, qpos, m32, dofs, att = scene
    plain, pairs = clearance.default_pairs(flat, dofs), clearance.default_pairs(flat, dofs, att)
    assert len(pairs) == 44 and len(plain) == 39
    none, every = clearance.active_pairs(flat, dofs, pairs, att, (False, False)), clearance.active_pairs(flat, dofs, pairs, att, (True, True))
    assert np.array_equal(pairs[none], plain)      # nothing held: exactly the plain list, in its order
    assert none.sum() == 39 and every.sum() == 39 and (none & every).sum() == 34 and (none | every).all()
    g = flat.names["geom"].index
    at = lambda a, b: int(np.flatnonzero((pairs == (g(a), g(b))).all(axis=1) | (pairs == (g(b), g(a))).all(axis=1))[0])      # noqa: E731
    assert every[at("floor", "fsph")] and not none[at("floor", "fsph")]      # a held sphere against the floor comes in
    assert none[at("g_f1", "fsph")] and not every[at("g_f1", "fsph")]        # ... and against the finger of the link that holds it drops out
    assert np.array_equal(clearance.default_pairs(flat, dofs, []), plain) and np.array_equal(clearance.signatures(flat, dofs, None), clearance.signatures(flat, dofs))


@pytest.mark.parametrize("row", ROWS)
def test_signature_rule_against_brute_force(scene, row):
    flat, qpos, m32, dofs, att = scene
    pairs = clearance.default_pairs(flat, dofs, att)
    gb = clearance._I(flat, "geom_bodyid")
    rel = A.rel_given(B)
    e = 1
    q = S.candidates(flat, dofs, B, 8)[e]
    poses = [clearance.fk(flat, qpos[e], dofs, q[k], model32=m32, attach=att, held=row, rel=rel[e]) for k in range(8)]

    def relative(xp, xq, a, b):
        conj = xq[a] * [1, -1, -1, -1]
        return np.concatenate([_qrot(conj, xp[b] - xp[a]), _qmul(conj, xq[b])])

    changed = []
    for a, b in pairs:
        r = np.array([relative(xp, xq, gb[a], gb[b]) for xp, xq in poses])
        changed.append(bool(np.abs(r - r[0]).max() > 1e-9))
    assert np.array_equal(np.array(changed), clearance.active_pairs(flat, dofs, pairs, att, row))


@pytest.mark.parametrize("mode", A.REL_MODES)
def test_motion_bound_holds_against_dense_centre_displacements(scene, mode):
    flat, qpos, m32, dofs, att = scene
    pairs = clearance.default_pairs(flat, dofs, att)
    held, rel = A.held_rows(B), A.rel_of(mode, B)
    q0, q1 = A.segments(flat, dofs, B, K, mode)
    gb, gpos = clearance._I(flat, "geom_bodyid"), S.f32(flat.arrays["geom_pos"]).reshape(-1, 3)
    geoms = sorted(set(int(g) for g in pairs.ravel()))
    ratio = {True: 0.0, False: 0.0}
    for e in range(B):
        R = None if rel is None else rel[e]
        on = clearance.active_pairs(flat, dofs, pairs, att, held[e])
        for k in range(K):
            L = sweep.motion_bound(flat, qpos[e], dofs, q0[e, k], q1[e, k], None, attach=att, held=held[e], rel=R)
            c = []
            for t in np.linspace(0.0, 1.0, W.DENSE):
                xp, xq = clearance.fk(flat, qpos[e], dofs, W.at(q0[e, k], q1[e, k], t), model32=m32, attach=att, held=held[e], rel=R)
                c.append({g: xp[gb[g]] + mjcf.quat2mat(xq[gb[g]]) @ gpos[g] for g in geoms})
            d = {g: max(np.linalg.norm(c[i + 1][g] - c[i][g]) for i in range(W.DENSE - 1)) for g in geoms}
            got = max(d[int(a)] + d[int(b)] for (a, b), o in zip(pairs, on) if o)
            assert got <= L / (W.DENSE - 1) + 1e-12, (e, k, got * (W.DENSE - 1), L)
            carried = max(d[g] for g in geoms if gb[g] in [a[0] for a in att])
            ratio[bool(held[e].any())] = max(ratio[bool(held[e].any())], carried * (W.DENSE - 1) / L)
            for (body, _), h in zip(att, held[e]):      # a body that is not held stands still
                assert h or all(d[g] == 0.0 for g in geoms if gb[g] == body)
    print(f"attached motion bound, rel {mode}: the carried geoms' worst dense displacement rate reaches {ratio[True]:.3f} of L")
    assert ratio[True] > 0.05      # (the carried bodies do move at a rate the bound has to cover)


@pytest.mark.parametrize("mode,margin", (("given", 0.0), ("given", 0.01), ("state", 0.0)))
def test_sweep_certificate_against_dense_sampling(scene, mode, margin):
    flat, qpos, m32, dofs, att = scene
    held, rel = A.held_rows(B), A.rel_of(mode, B)
    q0, q1 = A.segments(flat, dofs, B, K, mode)
    seen = set()
    for e in range(B):
        R = None if rel is None else rel[e]
        for k in range(K):
            st, t, dist, tm, pair, ft, steps = sweep.sweep(flat, qpos[e], dofs, q0[e, k], q1[e, k], distmax=S.DISTMAX_T, margin=margin, attach=att, held=held[e], rel=R)
            seen.add(st & 3)
            clear_at = lambda x: clearance.clearance(flat, qpos[e], dofs, W.at(q0[e, k], q1[e, k], x), None, S.DISTMAX_T, attach=att, held=held[e], rel=R,      # noqa: E731
                                                     poses=clearance.fk(flat, qpos[e], dofs, W.at(q0[e, k], q1[e, k], x), model32=m32, attach=att, held=held[e], rel=R))[0]
            ts = np.linspace(0.0, 1.0, W.DENSE)
            ts = ts if (st & 3) == sweep.FREE else ts[ts < t]
            c = [clear_at(x) for x in ts]
            assert not c or min(c) > margin, (e, k, st, t, min(c))
            if (st & 3) == sweep.HIT:
                assert clear_at(t) <= margin + sweep.DEFAULTS["slack"] and tm == t
            if pair >= 0:
                assert abs(dist - clear_at(tm)) <= 1e-12
                assert clearance.active_pairs(flat, dofs, clearance.default_pairs(flat, dofs, att), att, held[e])[pair]
    assert seen >= {sweep.FREE, sweep.HIT}


def test_refusals_by_name(scene):
    flat, qpos, m32, dofs, att = scene
    b = flat.names["body"].index
    fsb, fbb, l2, side, l0 = b("fsb"), b("fbb"), b("l2"), b("side"), b("l0")
    arm = S.dofs_t(flat, "arm")      # the side link's hinge is then held: `side` still moves (it hangs from l0), but l0 alone carries h0
    cases = (
        (dofs, [(fsb, l2)] * 5, "5 attachments outside 0..4"),
        (dofs, [(99, l2)], "body id 99 out of range"),
        (dofs, [(fsb, -1)], "body id -1 out of range"),
        (dofs, [(fsb, l2), (fsb, side)], "body %d is attached twice" % fsb),
        (dofs, [(l2, l0)], "body %d is not a child of the world with exactly one free joint" % l2),
        (dofs, [(l0, l2)], "body %d is not a child of the world with exactly one free joint" % l0),
        (dofs, [(0, l2)], "body 0 is not a child of the world with exactly one free joint"),
        (dofs, [(fsb, 0)], "carrier 0 is not moved by the controlled dofs"),
        (dofs, [(fsb, fbb)], "carrier %d is not moved by the controlled dofs" % fbb),
        (dofs, [(fsb, l2), (fbb, fsb)], "carrier %d is an attached body or below one" % fsb),
    )
    for d, a, word in cases:
        for call in (lambda: clearance.signatures(flat, d, a), lambda: clearance.default_pairs(flat, d, a), lambda: clearance.fk(flat, qpos[0], d, np.zeros(len(d)), attach=a),
                     lambda: sweep.motion_bound(flat, qpos[0], d, np.zeros(len(d)), np.ones(len(d)), attach=a)):
            with pytest.raises(clearance.ClearanceError, match=word):
                call()
    assert arm and clearance.signatures(flat, arm, [(fsb, side)])[fsb] == clearance.signatures(flat, arm)[side] != 0
    with pytest.raises(clearance.ClearanceError, match="held has 1 entries for 2 attachments"):
        clearance.signatures(flat, dofs, att, [True])


def c_pairs_refusal(flat, dofs, att):
    """what rsim_config_pairs_attached (host code only: it takes the model, not a batch) answers for the list: its message, or None if it accepts it"""
    import ctypes as C

    from robosuite_amd import backend

    hm, L = backend.HipModel(flat), backend.lib()
    a = np.ascontiguousarray(np.asarray(att), dtype=np.int32).reshape(-1, 2)
    n = L.rsim_config_pairs_attached(hm.ptr, len(dofs), (C.c_int32 * len(dofs))(*dofs), 0, None, len(a), a.ctypes.data_as(C.POINTER(C.c_int32)))
    return L.rsim_last_error().decode() if n < 0 else None


def refusal_cases_j(flat):
    """((model, dofs, attach, message), ...) on scene J: what is refused BELOW an attached body, and a mocap body.  A free joint or a mocap body below a
    child of the world is something the XML compiler does not produce: those two models are edited copies (attach_scenes.edited), read by host code only."""
    b, j = flat.names["body"].index, flat.names["joint"].index
    dofs, att = A.dofs_j(flat), A.attach_j(flat)
    tool, jaw, tip = b("tool"), b("jaw"), b("tip")
    return (
        (A.edited(flat, jnt_type={j("jh"): mjcf.JNT_FREE}), dofs, att, f"attachment 0: joint {j('jh')} (jh) of body {jaw}, below the attached body {tool}, is a free joint"),
        (A.edited(flat, jnt_type={j("ts"): mjcf.JNT_FREE}), dofs, att, f"attachment 0: joint {j('ts')} (ts) of body {tip}, below the attached body {tool}, is a free joint"),
        (flat, dofs, [(b("target"), b("wrist"))], f"attachment 0: body {b('target')} is a mocap body"),
        (A.edited(flat, body_mocapid={tip: 1}), dofs, att, f"attachment 0: body {tip}, below the attached body {tool}, is a mocap body"),
        (flat, dofs + S.dofs_of(flat, ("jh",)), att, f"attachment 0: joint {j('jh')} (jh) of body {jaw}, below the attached body {tool}, is a controlled joint"),
        (flat, dofs, [(b("puck"), b("wrist")), (tool, b("puck"))], f"attachment 1: carrier {b('puck')} is an attached body or below one"),
        (flat, dofs, [(b("puck"), b("jaw"))], f"attachment 0: carrier {jaw} is not moved by the controlled dofs"),
    )


def test_refusals_below_the_attached_body_and_mocap_bodies():
    """every case in the mirror and through the C-ABI's host-only entry, whole message against whole message"""
    flat = A.scene_j()
    for model, dofs, att, word in refusal_cases_j(flat):
        for call in (lambda: clearance.signatures(model, dofs, att), lambda: clearance.default_pairs(model, dofs, att),
                     lambda: clearance.fk(model, np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel(), dofs, np.zeros(len(dofs)), attach=att),
                     lambda: sweep.body_rates(model, np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel(), dofs, np.zeros(len(dofs)), np.ones(len(dofs)), attach=att)):
            with pytest.raises(clearance.ClearanceError) as e:
                call()
            assert str(e.value) == "clearance: " + word
        assert c_pairs_refusal(model, dofs, att) == "rsim_config_pairs_attached: " + word
    assert c_pairs_refusal(flat, A.dofs_j(flat), A.attach_j(flat)) is None and len(clearance.default_pairs(flat, A.dofs_j(flat), A.attach_j(flat))) == 26


def test_the_c_side_refuses_scene_t_lists_in_the_mirrors_words(scene):
    flat, qpos, m32, dofs, att = scene
    b = flat.names["body"].index
    fsb, fbb, l2, side, l0 = b("fsb"), b("fbb"), b("l2"), b("side"), b("l0")
    for a in ([(fsb, l2)] * 5, [(99, l2)], [(fsb, -1)], [(fsb, l2), (fsb, side)], [(l2, l0)], [(0, l2)], [(fsb, 0)], [(fsb, fbb)], [(fsb, l2), (fbb, fsb)]):
        with pytest.raises(clearance.ClearanceError) as e:
            clearance.signatures(flat, dofs, a)
        assert c_pairs_refusal(flat, dofs, a) == str(e.value).replace("clearance: ", "rsim_config_pairs_attached: ", 1)


def test_a_subtree_rides_along():
    """scene J: the jaw, the tip below it and the guard beside them go with the held tool, their joints at the env's qpos"""
    flat = A.scene_j()
    b = flat.names["body"].index
    dofs, att = A.dofs_j(flat), A.attach_j(flat)
    tool, below = b("tool"), [b("jaw"), b("tip"), b("guard")]
    sig = clearance.signatures(flat, dofs, att)
    assert all(sig[x] == sig[b("wrist")] == 3 for x in [tool] + below) and not clearance.signatures(flat, dofs, att, [False])[[tool] + below].any()
    m32 = clearance._model32(flat)
    a = clearance._I(flat, "jnt_qposadr")[flat.names["joint"].index("tf")]
    for e, qpos in enumerate(S.f32(A.scene_j_qpos(flat, 3))):
        for r in (_rel_from_state(m32, qpos, att), A.rel_given_j(3)[e]):
            for q in S.candidates(flat, dofs, 1, 2)[0]:
                qc = clearance.candidate_qpos(flat, qpos, dofs, q)
                cp, cq = mjcf.kinematics_np(m32, qc)[:2]
                qc[a:a + 3], qc[a + 3:a + 7] = cp[b("wrist")] + _qrot(cq[b("wrist")], r[0, :3]), _qmul(cq[b("wrist")], r[0, 3:] / np.linalg.norm(r[0, 3:]))
                rp, rq = mjcf.kinematics_np(m32, qc)[:2]
                xp, xq = clearance.fk(flat, qpos, dofs, q, model32=m32, attach=att, rel=r)
                assert np.abs(xp - rp).max() <= 1e-12 and np.abs(xq - rq).max() <= 1e-12
                up, uq = clearance.fk(flat, qpos, dofs, q, model32=m32, attach=att, held=[False], rel=r)
                assert all(np.array_equal(up[x], cp[x]) and np.array_equal(uq[x], cq[x]) for x in [tool] + below)      # not held: where it was
    qpos = S.f32(A.scene_j_qpos(flat, 1))[0]
    om, v = sweep.body_rates(flat, qpos, dofs, [-0.7, 0.1], [0.9, 0.4], attach=att)
    assert om[b("tip")] == om[b("jaw")] == om[tool] == om[b("wrist")] > 0 and v[b("tip")] > v[b("jaw")] > v[tool] > v[b("wrist")] >= 0
    om, v = sweep.body_rates(flat, qpos, dofs, [-0.7, 0.1], [0.9, 0.4], attach=att, held=[False])
    assert not om[[tool] + below].any() and not v[[tool] + below].any()


def test_condition_for_the_gpu_tests(scene):
    """With the seeds of attach_scenes, in both rel modes, the mirror decides every segment tests/test_attach.py sweeps within max_steps / 2 samples; among
    the segments of envs that hold something FREE and HIT at t > 0 both occur in every shape; held rows of all four kinds occur.  And for clearance at (3, 5):
    the attached reading differs from the plain one by more than 0.1 mm on most candidates, so the clearance tests cannot pass by accident."""
    flat, _, m32, dofs, att = scene
    SHAPES = A.SHAPES
    worst = 0
    for mode in A.REL_MODES:
        for Bs, Ks in SHAPES:
            qpos, held, rel = S.f32(S.scene_t_qpos(flat, Bs)), A.held_rows(Bs), A.rel_of(mode, Bs)
            q0, q1 = A.segments(flat, dofs, Bs, Ks, mode)
            seen = set()
            for e in range(Bs):
                for k in range(Ks):
                    st, t, _, _, _, _, steps = sweep.sweep(flat, qpos[e], dofs, q0[e, k], q1[e, k], distmax=S.DISTMAX_T, attach=att, held=held[e], rel=None if rel is None else rel[e])
                    assert (st & 3) != sweep.UNDECIDED and not st & distance.CAP, (mode, Bs, Ks, e, k)
                    worst = max(worst, steps)
                    if held[e].any() and ((st & 3) == sweep.FREE or t > 0):
                        seen.add(st & 3)
            assert seen == {sweep.FREE, sweep.HIT}, (mode, Bs, Ks, seen)
            assert Bs < 6 or len({tuple(r) for r in held}) == 4
    print(f"the mirror's worst step count over the attached GPU-shape segments: {worst}")
    assert worst <= sweep.DEFAULTS["max_steps"] // 2
    Bs, Ks = SHAPES[0]
    assert len({tuple(r) for r in A.held_rows(Bs)}) == 3
    qpos, held, q = S.f32(S.scene_t_qpos(flat, Bs)), A.held_rows(Bs), S.candidates(flat, dofs, Bs, Ks)
    for mode in A.REL_MODES:
        rel = A.rel_of(mode, Bs)
        differ = 0
        for e in range(Bs):
            for k in range(Ks):
                a = clearance.clearance(flat, qpos[e], dofs, q[e, k], None, S.DISTMAX_T, attach=att, held=held[e], rel=None if rel is None else rel[e])[0]
                differ += abs(a - clearance.clearance(flat, qpos[e], dofs, q[e, k], None, S.DISTMAX_T)[0]) > 1e-4
        print(f"clearance at {SHAPES[0]}, rel {mode}: the attached reading differs from the plain one on {differ} of {Bs * Ks} candidates")
        assert differ >= Bs * Ks // 3
