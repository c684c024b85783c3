"""Collision-aware IK on the device (csrc/rsim_ik_avoid.hip: rsim_ik_site_avoid, HipBatch.solve_ik_avoid) against fp64: the mirror robosuite_amd/ik_avoid.py and
the step formula fed with the device's own collision-cost gradient.  The reference is never a second device run, except where bits are compared.

  1. ONE UPDATE (max_iters = 1, scene A, B = 3, K = 5, position and pose targets; both tolerances 0, so nothing stops before the update): q_out - clamp(q_init)
     in two tiers -- "formula": against ik_avoid.update fed with the DEVICE's own config_collision_cost gradient at clamp(q_init), which isolates the step
     arithmetic; "mirror": against the mirror end to end, which carries the GJK witness error profiles/grad_parity.txt explains, times avoid_gain.
  2. THE FEATURE (B = 4, K = 6, the cases the mirror is held to): plain solve_ik converges and config_clearance at its answer is negative; solve_ik_avoid reports
     converged and finished with err < pos_tol, and an independent config_clearance(q_out) reads at least d_safe / 2 minus the fp32 distance bound of
     tests/test_clearance.py.
  3. avoid_gain = 0, cost_tol = inf agrees with solve_ik on the well-conditioned chain3 and panda cases of tests/ik_scenes.py (the FK summation order differs).
  4. BITS: a repeat call; check_every 0 against 3; problem (e, k) of a K = 65 call against the same problem of a K = 5 call with the same chunks; cost / nnear /
     noverlap against config_collision_cost(q_out) with the same chunks.
  5. n = RSIM_JNT_MAX: the sixteen-hinge chain, a pose target, an explicit list against one added sphere: the one-update comparison.
  6. A CARRIED BOX on the last link, held in half of the envs: those finish clear of the scene with the box; the others return the no-attachment call's bits.
  7. a pure query; rsim_ik_avoid_tables; every refusal by its text; per-env model parameters.

MEASURED holds the worst figures of one MI355X run (profiles/ik_avoid_parity.txt, tools/ik_avoid_parity.py --device from figures() below); the tests assert four
times that -- the margin is for seeds and boxes not drawn."""
import numpy as np
import pytest
import torch

from robosuite_amd import backend, clearance, ik, ik_avoid, mjcf
from tests import capacity_models
from tests import clearance_scenes as S
from tests import ik_avoid_scenes as A
from tests import ik_scenes
from tests import test_clearance as TC
from tests.util import make_hip

pytestmark = pytest.mark.gpu

# worst |q_out - reference| per entry (rad) of one MI355X run (profiles/ik_avoid_parity.txt); plain_*: |q(solve_ik_avoid, gain 0, cost_tol inf) - q(solve_ik)|.
# The one-update figures are taken at avoid_gain = GAIN_1, whatever the default is: the mirror tier grows with the gain.
GAIN_1 = 100.0
MEASURED = {"A_pos_formula": 1.363e-6, "A_pos_mirror": 7.166e-6, "A_pose_formula": 7.579e-5, "A_pose_mirror": 7.579e-5, "plain_chain3": 5.960e-7, "plain_panda": 5.990e-6,
            "chain16_formula": 8.411e-7, "chain16_mirror": 9.363e-6}
BOUND = {k: 4 * v for k, v in MEASURED.items()}
C16_D_SAFE = 0.08
DIST_BOUND = TC.BOUND["T"]["dist"]
dev = TC.dev
_CACHE = {}


def batch_a(B, K):
    """scene A's batch of B envs at the cases' state (each env's sphere where its cases put it), made once per shape"""
    if (B, K) not in _CACHE:
        a, c = A.scene_a(), A.cases(B, K)
        hm, hb = make_hip(a["flat"], None, B=B)
        hb.set("qpos", c["qpos"].astype(np.float32)); hb.forward()
        _CACHE[B, K] = dict(a, hm=hm, hb=hb, c=c, B=B, K=K)
    return _CACHE[B, K]


def np_(out):
    return tuple(t.cpu().numpy() for t in out)


def limits32(flat, dofs):
    lo, hi, _ = ik_scenes.ranges(flat, dofs)
    return S.f32(lo), S.f32(hi)


def one_update(flat, hb, site, dofs, qpos, pos, quat, q_init, pairs, **opts):
    """(formula, mirror): worst |q_out - reference| per entry over the problems after ONE update; asserted here: one update made by every problem"""
    o = dict(opts, max_iters=1, pos_tol=0.0, rot_tol=0.0)
    B, K = pos.shape[:2]
    lo, hi = limits32(flat, dofs)
    jl = np.asarray(flat.arrays["jnt_limited"]).ravel().astype(bool)[ik_scenes._joints_of(flat, dofs)]
    start = np.where(jl, np.clip(q_init, lo, hi), q_init)
    q, err, it, conv, fin, cost, nnear, nover = np_(hb.solve_ik_avoid(site, dofs, dev(pos), None if quat is None else dev(quat), dev(q_init), pairs=pairs, **o))
    assert (it == 1).all() and not fin.any()
    g = hb.config_collision_cost(dofs, dev(start), pairs=pairs, d_safe=o["d_safe"])[1].cpu().numpy().astype(np.float64)
    formula = mirror = 0.0
    for e in range(B):
        for k in range(K):
            args = (flat, qpos[e], site, dofs, start[e, k], start[e, k], pos[e, k], None if quat is None else quat[e, k], pairs)
            formula = max(formula, np.abs(q[e, k] - ik_avoid.update(*args, g=g[e, k], **o)).max())
            mirror = max(mirror, np.abs(q[e, k] - ik_avoid.update(*args, params=S.params32(flat), **o)).max())
    return float(formula), float(mirror)


def pose_targets(c, a):
    """pose targets for scene A's cases: position and orientation of the site at plain IK's answer"""
    B, K = c["pos"].shape[:2]
    pos, quat = np.zeros((B, K, 3)), np.zeros((B, K, 4))
    qa = np.asarray(a["flat"].arrays["jnt_qposadr"]).ravel()[ik_scenes._joints_of(a["flat"], a["dofs"])]
    for e in range(B):
        for k in range(K):
            qp = c["qpos"][e].copy()
            qp[qa] = c["q_plain"][e, k]
            p, R = ik.fk(a["flat"], qp, a["site"])
            pos[e, k], quat[e, k] = p, mjcf.mat2quat(R)
    return S.f32(pos), S.f32(quat)


def chain16():
    """the sixteen-hinge chain with one added world sphere beside its eighth link at the target configuration, an explicit list of that sphere against every
    third link, and seeded pose cases"""
    if "chain16" not in _CACHE:
        xml = capacity_models.model_xml(16, 0)
        base = mjcf.compile_mjcf(xml)
        site, dofs = base.names["site"].index("tip"), list(range(16))
        q0 = np.asarray(base.arrays["qpos0"], dtype=np.float64).ravel()
        B, K = 2, 5
        one = ik_scenes.cases(base, site, dofs, 1, seed=7300)      # ONE target; the starts stay within 0.1 rad of it, so that link 8 stays beside the sphere
        lo, hi, _ = ik_scenes.ranges(base, dofs)
        rng = np.random.default_rng(7301)
        cs = [dict(pos=np.tile(one["pos"], (K, 1)), quat=np.tile(one["quat"], (K, 1)),
                   q_init=S.f32(np.clip(one["q_true"] + 0.1 * rng.uniform(-1, 1, (K, 16)), lo, hi))) for e in range(B)]
        mid = clearance.fk(base, q0, dofs, one["q_true"][0])[0][8]
        sphere = f'<worldbody><geom name="obst" type="sphere" size="0.05" pos="{mid[0] + 0.03:.4f} {mid[1] + 0.06:.4f} {mid[2] + 0.02:.4f}"/>'
        flat = mjcf.compile_mjcf(xml.replace("<worldbody>", sphere, 1))
        assert int(flat.nbody) == int(base.nbody) and flat.names["site"].index("tip") == site
        gb = np.asarray(flat.arrays["geom_bodyid"]).ravel()
        obst = flat.names["geom"].index("obst")
        pairs = np.array([[obst, g] for g in range(int(flat.ngeom)) if g != obst and gb[g] > 0 and gb[g] % 3 == 2], dtype=np.int32)
        hm, hb = make_hip(flat, None, B=B)
        hb.set("qpos", np.tile(q0, (B, 1)).astype(np.float32)); hb.forward()
        _CACHE["chain16"] = dict(flat=flat, site=site, dofs=dofs, pairs=pairs, hm=hm, hb=hb, qpos=np.tile(q0, (B, 1)),
                                 pos=np.stack([c["pos"] for c in cs]), quat=np.stack([c["quat"] for c in cs]), q_init=np.stack([c["q_init"] for c in cs]))
    return _CACHE["chain16"]


def plain_agreement(name):
    """worst |q(avoid_gain 0, cost_tol inf) - q(solve_ik)| over the well-conditioned cases of an ik_scenes scene; asserted: both converge there"""
    s = ik_scenes.scene(name)
    flat, site, dofs = s["flat"], s["site"], s["dofs"]
    B, n = 3, 8
    hm, hb = make_hip(flat, s["cfg"], B=B)
    qpos = np.tile(np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel(), (B, 1)).astype(np.float32)
    hb.set("qpos", qpos); hb.forward()
    C = [ik_scenes.cases(flat, site, dofs, n, seed=ik_scenes.case_seed(name, e), quat=s["quat"]) for e in range(B)]
    ok = np.stack([ik_scenes.well(flat, qpos[e].astype(np.float64), site, dofs, C[e]) for e in range(B)])
    pos, qi = dev(np.stack([c["pos"] for c in C])), dev(np.stack([c["q_init"] for c in C]))
    quat = dev(np.stack([c["quat"] for c in C])) if s["quat"] else None
    gt = np.asarray(flat.arrays["geom_type"]).ravel()
    gb = np.asarray(flat.arrays["geom_bodyid"]).ravel()
    plane = int(np.flatnonzero(gt == mjcf.GEOM_PLANE)[0])
    moved = clearance.moved_bodies(flat, dofs)
    link = [g for g in range(int(flat.ngeom)) if gb[g] in moved and gt[g] in (mjcf.GEOM_CAPSULE, mjcf.GEOM_SPHERE, mjcf.GEOM_BOX, mjcf.GEOM_CYLINDER)][:3]
    pairs = np.array([[plane, g] for g in link], dtype=np.int32)
    q0, e0, it0, c0 = np_(hb.solve_ik(site, dofs, pos, quat, qi))
    q1, e1, it1, c1, f1, cost, nn, no = np_(hb.solve_ik_avoid(site, dofs, pos, quat, qi, pairs=pairs, avoid_gain=0.0, cost_tol=float("inf"), max_iters=ik.DEFAULTS["max_iters"]))
    assert ok.sum() >= 0.8 * ok.size and c0[ok].all() and c1[ok].all() and (f1 == c1).all()
    assert (np.abs(it1.astype(int) - it0)[ok] <= 1).all()      # (a case may cross the tolerance one update apart)
    return float(np.abs(q1 - q0)[ok].max())


def figures():
    """every MEASURED figure, from one run (tools/ik_avoid_parity.py --device)"""
    out = {}
    s = batch_a(3, 5)
    c = s["c"]
    out["A_pos_formula"], out["A_pos_mirror"] = one_update(s["flat"], s["hb"], s["site"], s["dofs"], c["qpos"], c["pos"], None, c["q_init"], s["pairs"], **dict(A.OPTS, avoid_gain=GAIN_1))
    pp, pq = pose_targets(c, s)
    out["A_pose_formula"], out["A_pose_mirror"] = one_update(s["flat"], s["hb"], s["site"], s["dofs"], c["qpos"], pp, pq, c["q_init"], s["pairs"], **dict(A.OPTS, avoid_gain=GAIN_1))
    h = chain16()
    out["chain16_formula"], out["chain16_mirror"] = one_update(h["flat"], h["hb"], h["site"], h["dofs"], h["qpos"], h["pos"], h["quat"], h["q_init"], h["pairs"],
                                                               d_safe=C16_D_SAFE, avoid_gain=GAIN_1)
    for name in ("chain3", "panda"):
        out[f"plain_{name}"] = plain_agreement(name)
    return out


def check(fig):
    for k, v in fig.items():
        print(f"ik avoid parity: {k} {v:.3e} (bound {BOUND[k]:.1e})")
    for k, v in fig.items():
        assert v <= BOUND[k], (k, v, BOUND[k])


# ---- 1: one update ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("target", ("pos", "pose"))
def test_one_update_scene_a(target):
    s = batch_a(3, 5)
    c = s["c"]
    pos, quat = (c["pos"], None) if target == "pos" else pose_targets(c, s)
    f, m = one_update(s["flat"], s["hb"], s["site"], s["dofs"], c["qpos"], pos, quat, c["q_init"], s["pairs"], **dict(A.OPTS, avoid_gain=GAIN_1))
    check({f"A_{target}_formula": f, f"A_{target}_mirror": m})


# ---- 2: the feature itself ----------------------------------------------------------------------------------------------------------------------------------
def test_grazing_solutions_are_repaired_scene_a():
    s = batch_a(4, 6)
    c, hb, site, dofs, pairs = s["c"], s["hb"], s["site"], s["dofs"], s["pairs"]
    held = A.held(4, 6)
    assert (~held).sum() <= A.CAP * held.size, held
    pos, qi = dev(c["pos"]), dev(c["q_init"])
    q0, e0, it0, c0 = hb.solve_ik(site, dofs, pos, None, qi, max_iters=A.MAX_ITERS)
    d0 = hb.config_clearance(dofs, q0, pairs=pairs)[0].cpu().numpy()
    out = hb.solve_ik_avoid(site, dofs, pos, None, qi, pairs=pairs, **A.OPTS)
    q, err, it, conv, fin, cost, nnear, nover = np_(out)
    d1 = hb.config_clearance(dofs, out[0], pairs=pairs)[0].cpu().numpy()
    print(f"scene A: {int(held.sum())}/{held.size} cases held; plain IK clearance {d0[held].min():.4f} .. {d0[held].max():.4f}; finished {int(fin.sum())}/{fin.size}; "
          f"clearance at q_out of the held cases {d1[held].min():.4f} .. {d1[held].max():.4f}; median iterations {np.median(it[held]):.0f}")
    assert c0.cpu().numpy()[held].all() and (d0[held] < 0).all()      # plain IK reaches the target inside the obstacle
    assert conv[held].all() and fin[held].all() and (err[..., 0][held] < ik.DEFAULTS["pos_tol"]).all()
    assert (d1[held] >= 0.5 * A.D_SAFE - DIST_BOUND).all()
    assert (cost[fin] <= ik_avoid.options(**A.OPTS)["cost_tol"]).all() and (nover[fin] == 0).all()
    lo, hi = limits32(s["flat"], dofs)
    assert np.isfinite(q).all() and (q >= lo).all() and (q <= hi).all()


# ---- 3: agreement with plain IK --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("chain3", "panda"))
def test_without_gain_and_cost_it_is_plain_ik(name):
    check({f"plain_{name}": plain_agreement(name)})


# ---- 4: bit identities ----------------------------------------------------------------------------------------------------------------------------------
def test_bit_identities_scene_a():
    s = batch_a(2, 65)
    hb, site, dofs, pairs = s["hb"], s["site"], s["dofs"], s["pairs"]
    c5 = A.cases(2, 5)
    assert np.array_equal(c5["qpos"], s["c"]["qpos"])      # (env e's sphere depends on (seed, e) only)
    rng = np.random.default_rng(99)
    lo, hi, _ = ik_scenes.ranges(s["flat"], dofs)
    pos = np.repeat(c5["pos"][:, :1], 65, axis=1)
    qi = np.clip(S.f32(c5["q_init"][:, :1] + 0.3 * rng.uniform(-1, 1, (2, 65, len(dofs)))), lo, hi)
    pos[:, :5], qi[:, :5] = c5["pos"], c5["q_init"]
    o = dict(A.OPTS, chunks=3)
    big = hb.solve_ik_avoid(site, dofs, dev(pos), None, dev(qi), pairs=pairs, **o)
    again = hb.solve_ik_avoid(site, dofs, dev(pos), None, dev(qi), pairs=pairs, **o)
    every3 = hb.solve_ik_avoid(site, dofs, dev(pos), None, dev(qi), pairs=pairs, check_every=3, **o)
    small = hb.solve_ik_avoid(site, dofs, dev(pos[:, :5]), None, dev(qi[:, :5]), pairs=pairs, **o)
    for x, y, z, w in zip(big, again, every3, small):
        assert torch.equal(x, y) and torch.equal(x, z) and torch.equal(x[:, :5], w)
    fin = big[4].cpu().numpy()
    assert 0 < fin.sum() < fin.size      # (frozen and running problems side by side)
    cost, _, nnear, nover = hb.config_collision_cost(dofs, big[0], pairs=pairs, d_safe=A.D_SAFE, chunks=3)
    assert torch.equal(cost, big[5]) and torch.equal(nnear, big[6]) and torch.equal(nover, big[7])


# ---- 5: n = RSIM_JNT_MAX ---------------------------------------------------------------------------------------------------------------------------------
def test_one_update_sixteen_hinges():
    h = chain16()
    f, m = one_update(h["flat"], h["hb"], h["site"], h["dofs"], h["qpos"], h["pos"], h["quat"], h["q_init"], h["pairs"], d_safe=C16_D_SAFE, avoid_gain=GAIN_1)
    near = h["hb"].config_collision_cost(h["dofs"], dev(h["q_init"]), pairs=h["pairs"], d_safe=C16_D_SAFE)[2].cpu().numpy()
    assert (near > 0).sum() >= 5 and near.max() == 1      # the sphere is near in half of the problems and more (the avoidance term takes part), one pair each
    check({"chain16_formula": f, "chain16_mirror": m})


# ---- 6: a carried object ----------------------------------------------------------------------------------------------------------------------------------
def test_carried_box_scene_a():
    a = A.scene_a()
    flat, site, dofs = a["flat"], a["site"], a["dofs"]
    B, K = 4, 2
    c = A.cargo_cases(B, K)
    att = A.cargo_attach()
    hm, hb = make_hip(flat, None, B=B)
    hb.set("qpos", c["qpos"].astype(np.float32)); hb.forward()
    held = c["held"]
    pos, qi = dev(c["pos"]), dev(c["q_init"])
    kw = dict(attach=att, held=dev(held, torch.bool), rel=dev(c["rel"]))
    out = hb.solve_ik_avoid(site, dofs, pos, None, qi, **A.OPTS, **kw)
    plain = hb.solve_ik_avoid(site, dofs, pos, None, qi, **A.OPTS)
    q, err, it, conv, fin, cost, nnear, nover = np_(out)
    h = held[:, 0]
    q0 = hb.solve_ik(site, dofs, pos, None, qi, max_iters=A.MAX_ITERS)[0]
    d0 = hb.config_clearance(dofs, q0, **kw)[0].cpu().numpy()
    d1 = hb.config_clearance(dofs, out[0], **kw)[0].cpu().numpy()
    print(f"carried box: plain IK clearance with the box {d0[h].min():.4f} .. {d0[h].max():.4f}; at q_out {d1[h].min():.4f} .. {d1[h].max():.4f}; iterations {it[h].ravel()}")
    assert (d0[h] < 0).all() and conv[h].all() and fin[h].all() and (d1[h] >= 0.5 * A.D_SAFE - DIST_BOUND).all()
    for x, y in zip(out, plain):      # an env that holds nothing: the no-attachment call's bits
        assert torch.equal(x[~torch.as_tensor(h)], y[~torch.as_tensor(h)])
    assert not torch.equal(out[0][torch.as_tensor(h)], plain[0][torch.as_tensor(h)])


# ---- 7: pure query, refusals, per-env parameters ----------------------------------------------------------------------------------------------------------
def test_pure_query_and_tables():
    a, c = A.scene_a(), A.cases(3, 5)
    hm, hb = make_hip(a["flat"], None, B=3)
    hb.set("qpos", c["qpos"].astype(np.float32)); hb.forward()
    assert hb.ik_avoid_tables() == 0
    hb.solve_ik(a["site"], a["dofs"], dev(c["pos"]), None, dev(c["q_init"]))
    hb.config_collision_cost(a["dofs"], dev(c["q_init"]), pairs=a["pairs"])
    assert hb.ik_avoid_tables() == 0
    names = ("qpos", "qvel", "time", "xpos", "xquat")
    before = [hb.get(n).copy() for n in names]
    hb.solve_ik_avoid(a["site"], a["dofs"], dev(c["pos"]), None, dev(c["q_init"]), pairs=a["pairs"], **A.OPTS)
    hb.solve_ik_avoid(a["site"], a["dofs"], dev(c["pos"][:, 0]), None, None, **A.OPTS)      # 2-D, the default list, the env's own qpos as the start
    for n, b in zip(names, before):
        assert np.array_equal(b, hb.get(n)), n
    assert hb.ik_avoid_tables() == 1


def test_refusals_by_their_text():
    a, c = A.scene_a(), A.cases(3, 5)
    flat, site, dofs = a["flat"], a["site"], a["dofs"]
    hm, hb = make_hip(flat, None, B=3)
    hb.set("qpos", c["qpos"].astype(np.float32)); hb.forward()
    pos, qi = dev(c["pos"]), dev(c["q_init"])
    call = lambda **kw: hb.solve_ik_avoid(kw.pop("site", site), kw.pop("dofs", dofs), kw.pop("pos", pos), None, kw.pop("q_init", qi), **kw)      # noqa: E731
    for kw, text in ((dict(avoid_gain=-1.0), "avoid_gain -1.0 is not >= 0"), (dict(cost_tol=-1e-3), "cost_tol -0.001 is not >= 0"), (dict(check_every=-1), "check_every -1 is not >= 0"),
                     (dict(d_safe=0.0), "d_safe 0.0 is not > 0"), (dict(bogus=1), "unknown IK option"), (dict(pairs=[[0, 0]]), "geom 0 against itself"),
                     (dict(site=99), "site 99 out of range"), (dict(attach=[(1, 1)]), "is not a child of the world with exactly one free joint")):
        with pytest.raises(backend.RsimError, match=text):
            call(**kw)
    L = backend.lib()
    import ctypes as C
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    q, err, it, cost = torch.empty((3, 5, 5), device="cuda"), torch.empty((3, 5, 2), device="cuda"), torch.empty((3, 5), dtype=torch.int32, device="cuda"), torch.empty((3, 5), device="cuda")

    def raw(opts, sdofs=dofs):      # the C entry itself: what the Python layer would stop first
        io = backend.IkAvoidOpts(1e-4, 0.5, 1e-4, 1e-3, 0.0, 5, 1, *opts)
        return L.rsim_ik_site_avoid(hb.ptr, site, len(sdofs), (C.c_int32 * len(sdofs))(*sdofs), 5, P(pos), None, P(qi), -1, None, C.byref(io), None, None, P(q), P(err), P(it), P(cost), None, None)

    for opts, text in (((0.04, -1.0, 1e-4, 0), "rsim_ik_site_avoid: avoid_gain -1 is not >= 0"), ((0.04, 30.0, -1.0, 0), "rsim_ik_site_avoid: cost_tol -1 is not >= 0"),
                       ((0.04, 30.0, 1e-4, -2), "rsim_ik_site_avoid: check_every -2 is not >= 0"), ((-0.04, 30.0, 1e-4, 0), "rsim_ik_site_avoid: d_safe -0.04 is not > 0")):
        assert raw(opts) != 0 and text in L.rsim_last_error().decode(), L.rsim_last_error().decode()
    ball = int(np.asarray(flat.arrays["jnt_dofadr"]).ravel()[flat.names["joint"].index("ballj")])
    assert raw((0.04, 30.0, 1e-4, 0), [0, 1, ball]) != 0
    assert f"rsim_ik_site_avoid: controlled dof {ball} is not a hinge or slide joint on the path to site {site}" in L.rsim_last_error().decode()
    assert raw((0.04, 30.0, float("inf"), 0)) == 0      # +inf: never wait for the cost
    # a ball joint on the path
    s = ik_scenes.scene("chain3")
    xml = ik_scenes.CHAIN3_XML.replace('<joint name="s1" type="slide" axis="1 0.3 -0.2" limited="true" range="-0.15 0.25" ref="0.05"/>', '<joint name="s1" type="ball"/>')
    fb = mjcf.compile_mjcf(xml)
    hm2, hb2 = make_hip(fb, None, B=3)
    with pytest.raises(backend.RsimError, match=r"rsim_ik_site_avoid: joint 1 \(s1\) on the path to site 0 is a ball joint"):
        hb2.solve_ik_avoid(fb.names["site"].index("tip"), [0], dev(np.zeros((3, 1, 3))), None, None, pairs=[[0, 1]])
    assert s["site"] == 0
    assert hb.ik_avoid_tables() == 1      # (only the +inf call got as far as a launch)


def test_per_env_params_are_honoured():
    """env 1's arm base is moved 5 cm: with the same targets it needs other joint angles, and reaches them on its own model"""
    a, c = A.scene_a(), A.cases(3, 5)
    flat, site, dofs, pairs = a["flat"], a["site"], a["dofs"], a["pairs"]
    hm, hb = make_hip(flat, None, B=3, per_env=True)
    qpos = np.tile(c["qpos"][0], (3, 1))
    hb.set("qpos", qpos.astype(np.float32)); hb.forward()
    base = flat.names["body"].index("l0")
    bp = hb.param_get("body_pos")
    bp[1, base] += [0.05, 0.0, 0.0]
    hb.param_set("body_pos", bp[1:2], env0=1)
    hb.forward()
    ov = [ik.rounded(flat, {"body_pos": hb.param_get("body_pos")[e]}) for e in range(3)]
    pos, qi = np.tile(c["pos"][:1], (3, 1, 1)), np.tile(c["q_init"][:1], (3, 1, 1))
    q, err, it, conv, fin, cost, nnear, nover = np_(hb.solve_ik_avoid(site, dofs, dev(pos), None, dev(qi), pairs=pairs, **A.OPTS))
    assert np.array_equal(q[0], q[2]) and np.array_equal(it[0], it[2])
    both = conv[0] & conv[1]
    assert both.sum() >= 3 and (np.abs(q[1] - q[0]).max(axis=1)[both] > 1e-3).all()
    for k in np.flatnonzero(both):
        e1 = ik.error(flat, qpos[1], site, dofs, q[1, k].astype(np.float64), pos[1, k], None, ov[1])
        e0 = ik.error(flat, qpos[1], site, dofs, q[1, k].astype(np.float64), pos[1, k], None, ov[0])
        assert e1[0] <= ik.DEFAULTS["pos_tol"] + 1e-5 and e0[0] > 0.04      # right on env 1's model, 5 cm off on env 0's
