"""Carried objects on the device (include/rsim.h rsim_attach: rsim_config_fk_attached, rsim_config_pairs_attached, rsim_config_clearance_attached,
rsim_config_sweep_attached, rsim_config_motion_bound_attached; the kernels k_clear_fk_att, k_clear_dist_att, k_sweep_att) against the fp64 mirror
(robosuite_amd/clearance.py, sweep.py with attach / held / rel) and against the plain queries.

Scene T with the sphere `fsb` on the last link and the box `fbb` on the side link, dofs "all", held[e] = (e % 2 == 0, e % 3 != 0), both rel modes
(tests/attach_scenes.py), at the lane-mapping shapes of tests/test_clearance.py: (3, 5) a partial wavefront over three envs with three held rows, (65, 3)
wavefronts that straddle envs -- lanes of one wave disagree about every skip --, (2, 70) K larger than a wave.

  1. nothing held: config_fk, config_clearance(chunks=1), config_sweep and config_motion_bound with attachments equal the calls without them BIT FOR BIT in
     every output; `pair` is compared as geom ids through the two lists.
  2. FK: unattached bodies to the imported BOUND against the mirror; attached bodies that are not held are the env's pose bit for bit; held ones go through
     two more quaternion products: their error is MEASURED and held at 4 x, the convention of tests/test_clearance.py.
  3. the distance layer at the device's own poses against the mirror over the pairs each env evaluates: the imported BOUND["dist"], no new allowance;
     automatic chunks and chunks=3.
  4. transplant, at (3, 5): a second batch of B K envs with the free bodies' qpos written to the device's attached poses, queried by the PLAIN
     config_clearance over the explicit list of each env's active pairs -- the parent's code path is the reference.  MEASURED, held at 4 x.
  5. sweep: the closest sample is config_clearance(attach=...) at q(t_min) bit for bit; the certificate against 129 dense attached config_clearance
     samples; L in [1 - 1e-5, 1 + 1e-4] of the mirror's; the centres of the listed geoms, attached ones included, move no more than L dt; a repeat call is
     bit-identical.  No segment is UNDECIDED and FREE and HIT both occur, in both rel modes: each has segments of its own (tests/attach_scenes.py SEGMENTS), and
     tests/test_attach_host.py holds the mirror alone to that condition.
  6. Lift / Panda, the shipped asset: the cube attached to the eef body, the hand lowered until the cube is below the table top: HIT, naming (table, cube) --
     a pair the plain default list does not contain; the env with held = 0 in the same call agrees with the plain call.  THE TEST THAT FAILS WITHOUT THE FEATURE.
  7. purity; 8. refusals by message through the C-ABI, each held to the mirror's whole message; 9. the VecEnv layer.
 10. scene J (tests/attach_scenes.py), a tool that carries a SUBTREE -- jaw, tip, guard -- on the wrist, at (5, 3): FK, the distance layer and the sweep as
     above.  Its bounds are the host rehearsal's (tests/test_clearance_core_host.py FK_BOUND and BOUND, reasoned from the number format, not measured): the
     MEASURED figures of this file and of tests/test_clearance.py belong to scene T."""
import numpy as np
import pytest
import torch

from robosuite_amd import backend, clearance, sweep
from tests import attach_scenes as A
from tests import clearance_scenes as S
from tests import sweep_scenes as W
from tests.test_attach_host import c_pairs_refusal, refusal_cases_j
from tests.test_clearance import BOUND, SHAPES, _actions, _lift, _lift_batch, clear_figures, dev
from tests.test_clearance_core_host import BOUND as HOST_DIST_BOUND
from tests.test_clearance_core_host import FK_BOUND as HOST_FK_BOUND
from tests.test_sweep import FREE, HIT, MAX_STEPS, SLACK, UNDECIDED
from tests.util import make_hip

pytestmark = pytest.mark.gpu
assert SHAPES == A.SHAPES

# worst figures of one GPU run (profiles/attach_parity.txt, written by tools/attach_parity.py from the functions below): position (m) and rotation (rad) of
# HELD attached bodies against the mirror, and |dist| of the transplant against the plain query.  The tests assert 4 x.
MEASURED = {"held_pos": 4.503e-7, "held_rot": 3.987e-7, "transplant": 2.235e-8}
HELD_BOUND = {k: 4 * v for k, v in MEASURED.items()}


def tdev(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


@pytest.fixture(scope="module")
def scene_t(tmp_path_factory):
    return S.scene_t(tmp_path_factory.mktemp("attach_t")), {}


def batch_t(scene_t, B, K):
    """the batch of B envs at the seeded state with what both rel modes share; made once per shape"""
    flat, cache = scene_t
    if (B, K) not in cache:
        hm, hb = make_hip(flat, None, B=B)
        hb.set("qpos", S.scene_t_qpos(flat, B).astype(np.float32)); hb.forward()
        dofs, att = S.dofs_t(flat, "all"), A.attach_t(flat)
        pairs = clearance.default_pairs(flat, dofs, att)
        held = A.held_rows(B)
        cache[B, K] = dict(hm=hm, hb=hb, dofs=dofs, att=att, pairs=pairs, held=held, held_dev=tdev(held, torch.bool), q=S.candidates(flat, dofs, B, K),
                           on=np.stack([clearance.active_pairs(flat, dofs, pairs, att, held[e]) for e in range(B)]), seg=A.segments(flat, dofs, B, K), modes={})
    return cache[B, K]


def mode_of(scene_t, B, K, mode):
    """... and per rel mode: the device's attached poses at the candidates and the mirror's pair distances there"""
    flat, _ = scene_t
    c = batch_t(scene_t, B, K)
    if mode not in c["modes"]:
        rel = A.rel_of(mode, B)
        kw = dict(attach=c["att"], held=c["held_dev"], rel=None if rel is None else tdev(rel, torch.float32))
        xp, xq = (t.cpu().numpy() for t in c["hb"].config_fk(c["dofs"], dev(c["q"]), **kw))
        ref = S.pair_reference(flat, xp.astype(np.float64), xq.astype(np.float64), c["pairs"], S.params32(flat))[0]
        c["modes"][mode] = dict(rel=rel, kw=kw, xp=xp, xq=xq, ref=np.where(c["on"][:, None, :], ref, 1e9),      # (a pair the env does not evaluate never attains its minimum)
                                seg=A.segments(flat, c["dofs"], B, K, mode))
    return c, c["modes"][mode]


SHAPE_J = (5, 3)      # a partial wavefront over five envs, every other one holding the tool: neighbouring lanes disagree about every branch
_J = {}


def batch_j(mode):
    """scene J's counterpart of batch_t / mode_of: (flat, c, m)"""
    B, K = SHAPE_J
    if "c" not in _J:
        flat = A.scene_j()
        hm, hb = make_hip(flat, None, B=B)
        hb.set("qpos", A.scene_j_qpos(flat, B).astype(np.float32)); hb.forward()
        dofs, att = A.dofs_j(flat), A.attach_j(flat)
        pairs, held = clearance.default_pairs(flat, dofs, att), A.held_rows_j(B)
        _J["flat"], _J["c"] = flat, dict(hm=hm, hb=hb, dofs=dofs, att=att, pairs=pairs, held=held, held_dev=tdev(held, torch.bool), q=S.candidates(flat, dofs, B, K),
                                         on=np.stack([clearance.active_pairs(flat, dofs, pairs, att, held[e]) for e in range(B)]), seg=A.segments(flat, dofs, B, K), modes={})
    flat, c = _J["flat"], _J["c"]
    if mode not in c["modes"]:
        rel = None if mode == "state" else A.rel_given_j(B)
        kw = dict(attach=c["att"], held=c["held_dev"], rel=None if rel is None else tdev(rel, torch.float32))
        xp, xq = (t.cpu().numpy() for t in c["hb"].config_fk(c["dofs"], dev(c["q"]), **kw))
        ref = S.pair_reference(flat, xp.astype(np.float64), xq.astype(np.float64), c["pairs"], S.params32(flat))[0]
        c["modes"][mode] = dict(rel=rel, kw=kw, xp=xp, xq=xq, ref=np.where(c["on"][:, None, :], ref, 1e9))
    return flat, c, c["modes"][mode]


# ---- the figures (also what tools/attach_parity.py prints) ----------------------------------------------------------------------------------------------
def fk_figures(flat, c, m):
    """config_fk(attach=...) against the mirror: {"fk_pos", "fk_rot"} over the unattached bodies, {"held_pos", "held_rot"} over held attached bodies; what is
    not moved or not held is asserted bitwise the env's pose"""
    hb, B = c["hb"], c["q"].shape[0]
    now_p, now_q = hb.get("xpos"), hb.get("xquat")
    xp, xq = m["xp"], m["xq"]
    assert xp.shape == c["q"].shape[:2] + (int(flat.nbody), 3) and xp.dtype == np.float32
    bodies = [a[0] for a in c["att"]]
    for e in range(B):
        still = clearance.signatures(flat, c["dofs"], c["att"], c["held"][e]) == 0
        assert np.array_equal(xp[e][:, still], np.broadcast_to(now_p[e, still], xp[e][:, still].shape))      # bit for bit the env's pose
        assert np.array_equal(xq[e][:, still], np.broadcast_to(now_q[e, still], xq[e][:, still].shape))
        assert all(still[b] != h for b, h in zip(bodies, c["held"][e]))
    rp, rq = A.mirror_fk(flat, hb.get("qpos").astype(np.float64), c["dofs"], c["q"], c["att"], c["held"], m["rel"], now=(now_p.astype(np.float64), now_q.astype(np.float64)))
    perr, aerr = np.linalg.norm(xp - rp, axis=-1), S.rot_angle(xq, rq)
    rest = np.ones(int(flat.nbody), dtype=bool)
    rest[bodies] = False
    h = np.broadcast_to(c["held"][:, None, :], perr[:, :, bodies].shape)
    moved = np.linalg.norm(xp[:, :, bodies] - now_p[:, None, bodies], axis=-1)
    assert (moved[h] > 1e-4).all() or m["rel"] is None      # a held body went with its carrier
    return {"fk_pos": float(perr[:, :, rest].max()), "fk_rot": float(aerr[:, :, rest].max()), "held_pos": float(perr[:, :, bodies][h].max()),
            "held_rot": float(aerr[:, :, bodies][h].max())}


def transplant_figure(flat, c, m):
    """worst ||dist| - |plain dist|| where the plain config_clearance runs on a second batch of B K envs whose free bodies sit at the device's attached
    poses, over the explicit list of the env's active pairs"""
    B, K = c["q"].shape[:2]
    hm2, hb2 = make_hip(flat, None, B=B * K)
    jadr, qa = clearance._I(flat, "body_jntadr"), clearance._I(flat, "jnt_qposadr")
    qpos = np.repeat(c["hb"].get("qpos"), K, axis=0)
    for body, _ in c["att"]:
        a = qa[jadr[body]]
        qpos[:, a:a + 3], qpos[:, a + 3:a + 7] = m["xp"][:, :, body].reshape(B * K, 3), m["xq"][:, :, body].reshape(B * K, 4)
    hb2.set("qpos", qpos); hb2.forward()
    got = c["hb"].config_clearance(c["dofs"], dev(c["q"]), distmax=S.DISTMAX_T, **m["kw"])[0].cpu().numpy().reshape(B * K)
    q2 = dev(c["q"].reshape(B * K, -1))
    worst = 0.0
    for row in {tuple(r) for r in c["held"]}:
        envs = np.flatnonzero((c["held"] == row).all(axis=1))
        lanes = (envs[:, None] * K + np.arange(K)).ravel()
        listed = c["pairs"][clearance.active_pairs(flat, c["dofs"], c["pairs"], c["att"], row)]
        plain = hb2.config_clearance(c["dofs"], q2, pairs=listed, distmax=S.DISTMAX_T)[0].cpu().numpy()
        worst = max(worst, float(np.abs(np.abs(got[lanes]) - np.abs(plain[lanes])).max()))
    return worst


def sweep_figures(flat, c, m, distmax=S.DISTMAX_T, margin=0.0):
    """one config_sweep(attach=...) call held to every exact property; -> its outputs and the figures"""
    hb, dofs, kw = c["hb"], c["dofs"], m["kw"]
    q0, q1 = m.get("seg", c["seg"])      # (the segments of the rel mode, tests/attach_scenes.py SEGMENTS)
    B, K, nd = q0.shape
    a, b = dev(q0), dev(q1)
    out = hb.config_sweep(dofs, a, b, distmax=distmax, margin=margin, **kw)
    st, t, dist, tmin, pair, ft, steps = out
    assert all(x.shape == (B, K) for x in (st, t, dist, tmin, pair, steps)) and ft.shape == (B, K, 6)
    again = hb.config_sweep(dofs, a, b, distmax=distmax, margin=margin, **kw)
    assert all(torch.equal(x, y) for x, y in zip(out, again))                      # a repeat call: bit-identical
    s = st.cpu().numpy()
    kind = s & 3
    assert not (s & 256).any() and (kind <= 2).all()
    tn, tm, sn, pn = t.cpu().numpy(), tmin.cpu().numpy(), steps.cpu().numpy(), pair.cpu().numpy()
    assert (sn >= 1).all() and (sn <= MAX_STEPS).all() and (tm >= 0).all() and (tm <= tn).all() and (tn <= 1).all()
    assert (tn[kind == FREE] == 1).all() and (tm[kind == HIT] == tn[kind == HIT]).all()
    ee, kk = np.nonzero(pn >= 0)
    assert c["on"][ee, pn[pn >= 0]].all()      # no env reports a pair it does not evaluate
    # sample identity: config_clearance(attach=...) at q(t_min), bit for bit
    ref = hb.config_clearance(dofs, dev(W.at32(q0, q1, tm[..., None])), distmax=distmax, chunks=1, **kw)
    assert torch.equal(dist, ref[0]) and torch.equal(pair, ref[1]) and torch.equal(ft, ref[2])
    # certificate: 129 dense attached samples over [0, t]
    ts = tn.astype(np.float64)[..., None] * np.linspace(0.0, 1.0, W.DENSE)
    qd = W.at32(q0[:, :, None, :], q1[:, :, None, :], ts.astype(np.float32)[..., None]).reshape(B, K * W.DENSE, nd)
    cd = hb.config_clearance(dofs, dev(qd), distmax=distmax, fromto=False, **kw)[0].cpu().numpy().astype(np.float64).reshape(B, K, W.DENSE)
    hit = kind == HIT
    certified = ~(hit & (tn == 0))      # a HIT at the first sample certifies nothing: [0, 0) is empty
    fig = {"shortfall": float(np.maximum(0.0, margin - cd.min(axis=-1))[certified].max()) if certified.any() else 0.0,
           "hit": float(np.maximum(0.0, cd[..., -1][hit] - (margin + SLACK)).max()) if hit.any() else 0.0}
    # the bound against the mirror's, and against the centres' dense displacements at attached config_fk poses
    L = hb.config_motion_bound(dofs, a, b, **kw)
    qpos = hb.get("qpos").astype(np.float64)
    Lref = np.array([[sweep.motion_bound(flat, qpos[e], dofs, q0[e, k], q1[e, k], None, attach=c["att"], held=c["held"][e], rel=None if m["rel"] is None else m["rel"][e])
                      for k in range(K)] for e in range(B)])
    Ln = L.cpu().numpy().astype(np.float64)
    assert ((Lref == 0) == (Ln == 0)).all()
    rel = np.where(Lref > 0, Ln / np.where(Lref > 0, Lref, 1.0) - 1.0, 0.0)
    fig["bound_lo"], fig["bound_hi"] = float(-rel.min()), float(rel.max())
    tu = np.broadcast_to(np.linspace(0.0, 1.0, W.DENSE, dtype=np.float32), (B, K, W.DENSE))
    qu = W.at32(q0[:, :, None, :], q1[:, :, None, :], tu[..., None]).reshape(B, K * W.DENSE, nd)
    xp, xq = (x.double() for x in hb.config_fk(dofs, dev(qu), **kw))
    gb = torch.as_tensor(clearance._I(flat, "geom_bodyid").astype(np.int64), device="cuda")
    lp = torch.as_tensor(S.f32(flat.arrays["geom_pos"]).reshape(-1, 3), device="cuda")[None, None]
    w, v = xq[:, :, gb, :1], xq[:, :, gb, 1:]
    ctr = (xp[:, :, gb] + lp + 2 * torch.cross(v, torch.cross(v, lp.expand_as(v), dim=-1) + w * lp, dim=-1)).reshape(B, K, W.DENSE, -1, 3)
    d = (ctr[:, :, 1:] - ctr[:, :, :-1]).norm(dim=-1)                              # [B, K, n - 1, ngeom]
    pr = torch.as_tensor(np.asarray(c["pairs"], dtype=np.int64), device="cuda")
    both = (d[..., pr[:, 0]] + d[..., pr[:, 1]]) * torch.as_tensor(c["on"], device="cuda")[:, None, None, :]      # the pairs the env evaluates
    fig["centres"] = float((both.amax(dim=(2, 3)) - L.double() / (W.DENSE - 1) - 4 * BOUND["T"]["fk_pos"]).max())
    carried = d[..., torch.isin(gb, torch.as_tensor([x[0] for x in c["att"]], device="cuda"))].amax(dim=(2, 3))   # [B, K]
    fig["carried_share"] = float((carried * (W.DENSE - 1) / L.double().clamp_min(1e-9))[torch.as_tensor(c["held"].any(axis=1), device="cuda")].max())
    print(f"attached sweep ({B}, {K}): free {int((kind == FREE).sum())}, hit {int((kind == HIT).sum())}, undecided {int((kind == UNDECIDED).sum())}; steps mean {sn.mean():.1f} max {sn.max()}")
    return out, fig


def show(what, fig):
    for k, v in fig.items():
        print(f"attach parity {what}: {k} {v:.3e}")


# ---- 1. nothing held is the plain query -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,K", SHAPES)
def test_nothing_held_is_the_plain_query_bit_for_bit(scene_t, B, K):
    flat, _ = scene_t
    c = batch_t(scene_t, B, K)
    hb, dofs, q = c["hb"], c["dofs"], dev(c["q"])
    a, b = dev(c["seg"][0]), dev(c["seg"][1])
    plain_list = hb.config_pairs(dofs)
    assert np.array_equal(hb.config_pairs(dofs, attach=c["att"]), c["pairs"]) and np.array_equal(plain_list, clearance.default_pairs(flat, dofs))
    geoms = lambda pair, lst: np.where(pair.cpu().numpy()[..., None] >= 0, lst[np.maximum(pair.cpu().numpy(), 0)], -1)      # noqa: E731
    for rel in (None, tdev(A.rel_given(B), torch.float32)):
        for held in (torch.zeros(B, dtype=torch.bool, device="cuda"), torch.zeros((B, 2), dtype=torch.uint8, device="cuda")):
            kw = dict(attach=c["att"], held=held, rel=rel)
            assert all(torch.equal(x, y) for x, y in zip(hb.config_fk(dofs, q), hb.config_fk(dofs, q, **kw)))
            p, g = hb.config_clearance(dofs, q, distmax=S.DISTMAX_T, chunks=1), hb.config_clearance(dofs, q, distmax=S.DISTMAX_T, chunks=1, **kw)
            assert torch.equal(p[0], g[0]) and torch.equal(p[2], g[2]) and torch.equal(p[3], g[3]) and np.array_equal(geoms(p[1], plain_list), geoms(g[1], c["pairs"]))
            assert (p[1] >= 0).any() and (p[1] < 0).any()
            p, g = hb.config_sweep(dofs, a, b, distmax=S.DISTMAX_T), hb.config_sweep(dofs, a, b, distmax=S.DISTMAX_T, **kw)
            assert all(torch.equal(x, y) for i, (x, y) in enumerate(zip(p, g)) if i != 4) and np.array_equal(geoms(p[4], plain_list), geoms(g[4], c["pairs"]))
            assert torch.equal(hb.config_motion_bound(dofs, a, b), hb.config_motion_bound(dofs, a, b, **kw))


# ---- 2. FK -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", A.REL_MODES)
@pytest.mark.parametrize("B,K", SHAPES)
def test_attached_fk(scene_t, B, K, mode):
    flat, _ = scene_t
    c, m = mode_of(scene_t, B, K, mode)
    fig = fk_figures(flat, c, m)
    show(f"({B}, {K}) rel {mode}", fig)
    assert fig["fk_pos"] <= BOUND["T"]["fk_pos"] and fig["fk_rot"] <= BOUND["T"]["fk_rot"], fig
    assert fig["held_pos"] <= HELD_BOUND["held_pos"] and fig["held_rot"] <= HELD_BOUND["held_rot"], fig


# ---- 3. the distance layer -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", A.REL_MODES)
@pytest.mark.parametrize("B,K", SHAPES)
def test_attached_clearance_at_the_devices_own_poses(scene_t, B, K, mode):
    flat, _ = scene_t
    c, m = mode_of(scene_t, B, K, mode)
    bound = BOUND["T"]["dist"]
    plain = c["hb"].config_clearance(c["dofs"], dev(c["q"]), distmax=S.DISTMAX_T)[0]
    for chunks in (0, 3):
        out = c["hb"].config_clearance(c["dofs"], dev(c["q"]), distmax=S.DISTMAX_T, chunks=chunks, **m["kw"])
        fig, _ = clear_figures(flat, out, m["xp"].astype(np.float64), m["xq"].astype(np.float64), c["pairs"], S.DISTMAX_T, bound, ref=m["ref"])
        show(f"({B}, {K}) rel {mode} chunks {chunks}", fig)
        assert fig["dist"] <= bound and fig["witness"] <= bound and fig["pick"] <= 2 * bound, fig
        pn = out[1].cpu().numpy()
        ee, kk = np.nonzero(pn >= 0)
        assert c["on"][ee, pn[pn >= 0]].all()      # no env reports a pair it does not evaluate
        assert float((out[0] - plain).abs().max()) > 1e-4      # ... and the carried objects change the answer
    # an explicit list is taken as given: every pair in every env, the held sphere against its own fingers included
    given = c["hb"].config_clearance(c["dofs"], dev(c["q"]), pairs=c["pairs"], distmax=S.DISTMAX_T, **m["kw"])
    full = S.pair_reference(flat, m["xp"].astype(np.float64), m["xq"].astype(np.float64), c["pairs"], S.params32(flat))[0] if (B, K) == SHAPES[0] else None
    if full is not None:
        fig, _ = clear_figures(flat, given, m["xp"].astype(np.float64), m["xq"].astype(np.float64), c["pairs"], S.DISTMAX_T, bound, ref=full)
        assert fig["dist"] <= bound and fig["pick"] <= 2 * bound, fig


# ---- 4. transplant ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", A.REL_MODES)
def test_transplant_against_the_plain_query(scene_t, mode):
    flat, _ = scene_t
    c, m = mode_of(scene_t, *SHAPES[0], mode)
    worst = transplant_figure(flat, c, m)
    show(f"{SHAPES[0]} rel {mode}", {"transplant": worst})
    assert worst <= HELD_BOUND["transplant"]


# ---- 5. sweep --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", A.REL_MODES)
@pytest.mark.parametrize("B,K", SHAPES)
def test_attached_sweep(scene_t, B, K, mode):
    flat, _ = scene_t
    c, m = mode_of(scene_t, B, K, mode)
    out, fig = sweep_figures(flat, c, m)
    show(f"({B}, {K}) rel {mode}", fig)
    bound = BOUND["T"]["dist"]
    assert fig["shortfall"] <= bound and fig["hit"] <= bound, fig
    assert fig["bound_lo"] <= 1e-5 and fig["bound_hi"] <= 1e-4, fig
    assert fig["centres"] <= 0.0 and fig["carried_share"] > 0.05, fig
    kind = out[0].cpu().numpy() & 3
    assert not (kind == UNDECIDED).any() and (kind == FREE).any() and (kind == HIT).any()
    holding = c["held"].any(axis=1)
    assert (kind[holding] == FREE).any() and ((kind[holding] == HIT) & (out[1].cpu().numpy()[holding] > 0)).any()


# ---- 6. Lift / Panda -------------------------------------------------------------------------------------------------------------------------------------
LIFT_DOFS = list(range(1, 7))      # without joint 1: link0 / link1 stand 1.0 mm apart whatever it does, and with it in the list every sweep is a HIT at once
LIFT_LOWER = (0.8, 0.0, 0.7, 0.0, 0.0, 0.0)      # added to the start: the hand comes down to 1 cm below the table top


def test_lift_a_carried_cube_hits_the_table():
    s, hm, hb = _lift_batch(B=3)
    flat = s["flat"]
    gn, bn = flat.names["geom"].index, flat.names["body"].index
    eef = int(np.asarray(flat.arrays["site_bodyid"]).ravel()[int(s["cfg"]["eef_site"])])
    att = [(bn("cube_main"), eef)]
    q0 = np.tile(s["qpos"][1:7], (3, 1)).astype(np.float32)
    q1 = q0 + np.asarray(LIFT_LOWER, dtype=np.float32)
    rel = tdev(np.tile([0, 0, 0, 1, 0, 0, 0], (3, 1, 1)), torch.float32)      # the cube between the fingers, at the grip site
    held = tdev([True, False, True], torch.bool)
    table_cube = {gn("table_collision"), gn("cube_g0")}
    plain_list, att_list = hb.config_pairs(LIFT_DOFS), hb.config_pairs(LIFT_DOFS, attach=att)
    assert not any(set(p) == table_cube for p in plain_list.tolist())      # the plain default list does not contain that pair at all
    assert sum(set(p) == table_cube for p in att_list.tolist()) == 1
    xp, _ = hb.config_fk(LIFT_DOFS, dev(q1), attach=att, held=held, rel=rel)
    top = 0.8      # the table's top face
    assert float(xp[0, bn("cube_main"), 2]) < top and float(xp[2, bn("cube_main"), 2]) < top and float(xp[1, bn("cube_main"), 2]) > top      # carried below it; left on it
    plain = hb.config_sweep(LIFT_DOFS, dev(q0), dev(q1))
    out = hb.config_sweep(LIFT_DOFS, dev(q0), dev(q1), attach=att, held=held, rel=rel)
    st, t, dist, tmin, pair, ft, steps = (x.cpu().numpy() for x in out)
    print(f"Lift, carried cube: status {st.tolist()}, t {t.tolist()}, dist {dist.tolist()}, steps {steps.tolist()}; plain: status {plain[0].tolist()}, t {plain[1].tolist()}")
    for e in (0, 2):
        assert st[e] == HIT and 0 < t[e] < 1 and set(att_list[pair[e]].tolist()) == table_cube
    # the env that holds nothing agrees with the plain call: it runs into the cube where it lies, a pair the holding envs do not evaluate
    for i, (x, y) in enumerate(zip(plain, out)):
        assert torch.equal(x[1], y[1]) or i == 4
    assert plain_list[int(plain[4][1])].tolist() == att_list[pair[1]].tolist() and gn("cube_g0") in att_list[pair[1]].tolist() and t[1] < t[0]


# ---- 7. purity -------------------------------------------------------------------------------------------------------------------------------------------
def _lift_attach(s):
    flat = s["flat"]
    eef = int(np.asarray(flat.arrays["site_bodyid"]).ravel()[int(s["cfg"]["eef_site"])])
    return [(flat.names["body"].index("cube_main"), eef)]


def _ask(hb, s, att, q):
    held = tdev([True, False, True], torch.bool)
    hb.config_fk(s["dofs"], q, attach=att, held=held)
    hb.config_clearance(s["dofs"], q, attach=att, held=held)
    hb.config_sweep(s["dofs"], q[:, :-1], q[:, 1:], attach=att, held=held, max_steps=4)
    hb.config_motion_bound(s["dofs"], q[:, :-1], q[:, 1:], attach=att)


def test_state_is_bitwise_unchanged_and_no_table_is_built_without_attach():
    s, hm, hb = _lift_batch()
    q = dev(S.candidates(s["flat"], s["dofs"], 3, 5))
    names = ("qpos", "qvel", "time", "xpos", "xquat")
    before = [hb.get(n).copy() for n in names]
    assert hb.config_tables() == 0
    hb.config_fk(s["dofs"], q); hb.config_clearance(s["dofs"], q); hb.config_sweep(s["dofs"], q[:, :-1], q[:, 1:], max_steps=4)
    assert hb.config_tables() == 1      # a batch that never passes attach holds the one table of its dof list
    _ask(hb, s, _lift_attach(s), q)
    assert hb.config_tables() == 2
    _ask(hb, s, _lift_attach(s), q)
    assert hb.config_tables() == 2      # a repeat call builds nothing
    for n, a in zip(names, before):
        assert np.array_equal(a, hb.get(n)), n


def test_an_attached_query_between_control_steps_changes_nothing_ten_steps_later():
    got = []
    for ask in (False, True):
        s, hm, hb = _lift_batch()
        q = dev(S.candidates(s["flat"], s["dofs"], 3, 5))
        for t in range(10):
            hb.control_step(_actions(hm, 3, t), 25)
            if ask and t in (0, 4):
                _ask(hb, s, _lift_attach(s), q)
        got.append((hb.get("qpos").copy(), hb.get("qvel").copy()))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_message(scene_t):
    flat, _ = scene_t
    c = batch_t(scene_t, *SHAPES[0])
    hb, dofs, q = c["hb"], c["dofs"], dev(c["q"])
    b = flat.names["body"].index
    fsb, fbb, l2, side, l0 = b("fsb"), b("fbb"), b("l2"), b("side"), b("l0")
    cases = (([(fsb, l2)] * 5, "5 attachments outside 0..4"), ([(99, l2)], "body id 99 out of range"), ([(fsb, l2), (fsb, side)], "is attached twice"),
             ([(l2, l0)], "not a child of the world with exactly one free joint"), ([(0, l2)], "not a child of the world with exactly one free joint"),
             ([(fsb, 0)], "carrier 0 is not moved by the controlled dofs"), ([(fsb, fbb)], f"carrier {fbb} is not moved by the controlled dofs"),
             ([(fsb, l2), (fbb, fsb)], f"carrier {fsb} is an attached body or below one"))
    tables = hb.config_tables()
    five = lambda hb, dofs, q, att: (lambda: hb.config_fk(dofs, q, attach=att), lambda: hb.config_clearance(dofs, q, attach=att),      # noqa: E731
                                     lambda: hb.config_sweep(dofs, q, q, attach=att), lambda: hb.config_motion_bound(dofs, q, q, attach=att),
                                     lambda: hb.config_pairs(dofs, attach=att))

    def same_words(err, model, dofs, att):      # the mirror refuses the same list in the same words: the whole message behind the entry's name
        with pytest.raises(clearance.ClearanceError) as m:
            clearance.signatures(model, dofs, att)
        assert str(err.value).split(": ", 1)[1] == str(m.value).split(": ", 1)[1], (str(err.value), str(m.value))

    for att, word in cases:
        for call in five(hb, dofs, q, att):
            with pytest.raises(backend.RsimError, match=word) as err:
                call()
            same_words(err, flat, dofs, att)
    assert hb.config_tables() == tables      # refused before anything is built or launched
    # scene J: what is refused below an attached body, and mocap bodies.  The compiled model through all five entries of a batch; the two EDITED models (a free
    # joint, a mocap body below the tool -- inconsistent on purpose) are never given a batch: rsim_config_pairs_attached reads the model on the host and runs
    # the same clear_plan
    fj, cj, _ = batch_j("given")
    seen = set()
    for model, dj, att, word in refusal_cases_j(fj):
        seen |= {w for w in ("a free joint", "a mocap body", "a controlled joint") if word.endswith(w)}
        assert c_pairs_refusal(model, dj, att) == "rsim_config_pairs_attached: " + word
        if model is fj:
            qj = torch.zeros((SHAPE_J[0], 2, len(dj)), device="cuda")
            for call in five(cj["hb"], dj, qj, att):
                with pytest.raises(backend.RsimError) as err:
                    call()
                assert str(err.value).split(": ", 1)[1] == word
                same_words(err, model, dj, att)
    assert seen >= {"a free joint", "a mocap body", "a controlled joint"}
    with pytest.raises(backend.RsimError, match="held must be"):
        hb.config_fk(dofs, q, attach=c["att"], held=torch.zeros((3, 3), dtype=torch.bool, device="cuda"))
    with pytest.raises(backend.RsimError, match="held must be"):
        hb.config_fk(dofs, q, attach=c["att"], held=torch.zeros(3, dtype=torch.bool))
    with pytest.raises(backend.RsimError, match="rel must be"):
        hb.config_fk(dofs, q, attach=c["att"], rel=torch.zeros((3, 2, 6), device="cuda"))
    with pytest.raises(backend.RsimError, match="without attach"):
        hb.config_fk(dofs, q, held=c["held_dev"])
    floor_on_cube = [[flat.names["geom"].index("floor"), flat.names["geom"].index("fsph")]]      # fine: the plane stands still ...
    hb.config_sweep(dofs, q, q, pairs=floor_on_cube, attach=c["att"])


# ---- 9. the VecEnv layer ---------------------------------------------------------------------------------------------------------------------------------
def test_vec_env_layer():
    from robosuite_amd.vec_env import VecEnv

    s = _lift()
    flat = s["flat"]
    env = VecEnv("Lift", 3, flat, s["cfg"], horizon=50)
    env.reset()
    batch, att = env.env.batch, _lift_attach(s)
    q = dev(S.candidates(flat, s["dofs"], 3, 4))
    held = tdev([True, False, True], torch.bool)
    ref = batch.config_clearance(s["dofs"], q, attach=att, held=held)
    for named in ([("cube_main", None)], [("cube_main", "gripper0_right_eef")], [(att[0][0], att[0][1])]):      # names, carrier=None = the eef site's body, ids
        assert all(torch.equal(a, b) for a, b in zip(env.config_clearance(q, attach=named, held=held), ref))
    xp, xq = env.config_fk(q, attach=[("cube_main", None)], held=held)
    assert all(torch.equal(a, b) for a, b in zip((xp, xq), batch.config_fk(s["dofs"], q, attach=att, held=held)))
    assert not torch.equal(xp[0, :, att[0][0]], xp[1, :, att[0][0]])
    a = env.config_sweep(q[:, :-1], q[:, 1:], attach=[("cube_main", None)], held=held, max_steps=8)
    assert all(torch.equal(x, y) for x, y in zip(a, batch.config_sweep(s["dofs"], q[:, :-1], q[:, 1:], attach=att, held=held, max_steps=8)))
    free, seg, t, dist, pair = env.path_clearance(q[:, None], attach=[("cube_main", None)], held=held, max_steps=8)
    assert free.shape == (3, 1) and pair.shape == (3, 1)
    plain = env.path_clearance(q[:, None], max_steps=8)
    assert torch.equal(plain[2][1], t[1]) and torch.equal(plain[3][1], dist[1])      # the env that holds nothing: the plain answer
    with pytest.raises(KeyError):
        env.config_clearance(q, attach=[("no_such_body", None)])
    with pytest.raises(ValueError):
        env.config_clearance(q, attach=[("cube_main",)])


# ---- 10. an attached subtree -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", A.REL_MODES)
def test_a_tool_with_its_jaw_rides_on_the_wrist(mode):
    flat, c, m = batch_j(mode)
    B, K = SHAPE_J
    hb, dofs, q = c["hb"], c["dofs"], dev(c["q"])
    b = flat.names["body"].index
    tool, below = b("tool"), [b("jaw"), b("tip"), b("guard")]
    # FK: fk_figures asserts that what an env does not hold -- the tool AND what hangs below it -- is the env's pose bit for bit; "fk_*" covers the subtree
    fig = fk_figures(flat, c, m)
    show(f"scene J {SHAPE_J} rel {mode}", fig)
    assert max(fig.values()) <= HOST_FK_BOUND, fig
    went = np.linalg.norm(m["xp"][:, :, below] - hb.get("xpos")[:, None, below], axis=-1).max(axis=1)      # [B, 3]
    assert (went[c["held"][:, 0]] > 1e-3).all() and not went[~c["held"][:, 0]].any()
    # the distance layer at the device's own poses, automatic chunks and three
    for chunks in (0, 3):
        out = hb.config_clearance(dofs, q, distmax=S.DISTMAX_T, chunks=chunks, **m["kw"])
        fig, _ = clear_figures(flat, out, m["xp"].astype(np.float64), m["xq"].astype(np.float64), c["pairs"], S.DISTMAX_T, HOST_DIST_BOUND, ref=m["ref"])
        show(f"scene J {SHAPE_J} rel {mode} chunks {chunks}", fig)
        assert fig["dist"] <= HOST_DIST_BOUND and fig["witness"] <= HOST_DIST_BOUND and fig["pick"] <= 2 * HOST_DIST_BOUND, fig
        pn = out[1].cpu().numpy()
        assert c["on"][np.nonzero(pn >= 0)[0], pn[pn >= 0]].all()
    # the sweep: sample identity, certificate, L against the mirror's, the centres of the subtree's geoms within L dt, repeat call (all in sweep_figures)
    out, fig = sweep_figures(flat, c, m)
    show(f"scene J {SHAPE_J} rel {mode} sweep", fig)
    assert fig["shortfall"] <= HOST_DIST_BOUND and fig["hit"] <= HOST_DIST_BOUND, fig
    assert fig["bound_lo"] <= 1e-5 and fig["bound_hi"] <= 1e-4, fig
    assert fig["centres"] <= 0.0 and fig["carried_share"] > 0.05, fig
    # nothing held: the plain query bit for bit, subtree and all
    none = dict(attach=c["att"], held=torch.zeros(B, dtype=torch.bool, device="cuda"), rel=m["kw"]["rel"])
    assert all(torch.equal(x, y) for x, y in zip(hb.config_fk(dofs, q), hb.config_fk(dofs, q, **none)))
    p, g = hb.config_clearance(dofs, q, distmax=S.DISTMAX_T, chunks=1), hb.config_clearance(dofs, q, distmax=S.DISTMAX_T, chunks=1, **none)
    assert torch.equal(p[0], g[0]) and torch.equal(p[2], g[2]) and torch.equal(p[3], g[3])
