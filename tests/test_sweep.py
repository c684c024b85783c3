"""Swept clearance on the device (csrc/rsim_sweep.hip: rsim_config_sweep, rsim_config_motion_bound): certified checks of joint-space motions.

The device is never compared step for step with the fp64 mirror (robosuite_amd/sweep.py): the step sequence is sensitive to rounding.  It is held to
properties, with config_clearance and config_fk as the reference (themselves held to the mirror by tests/test_clearance.py), BOUND = BOUND[scene]["dist"] of
that file:

  * sample identity: dist, pair, fromto equal config_clearance (one chunk) at q(t_min), recomputed in fp32 as the kernel interpolates, fmaf(t, q1 - q0, q0)
    (sweep_scenes.at32).  ACHIEVED: BIT FOR BIT, on every scene.
  * certificate: config_clearance at 129 uniform samples over [0, t] of every segment reads > margin - BOUND; for a HIT the value at t is <= margin + slack +
    BOUND.  The sample at t itself is held to the first as well (a conservative step cannot land below margin), except for a HIT at t = 0: the motion is
    certified on [0, t), which is empty there, and a start configuration in collision reads a negative distance.
  * bound: config_motion_bound lies in [L (1 - 1e-5), L (1 + 1e-4)] of the mirror's L, and the centres of the listed geoms at config_fk poses of 129 uniform
    samples move, per pair and between neighbours, no more than L dt (plus the rounding of four fp32 positions, 4 BOUND["fk_pos"]).
  * no segment is UNDECIDED at the default max_steps on scene T with the seeds of sweep_scenes.segments (tests/test_sweep_host.py holds the mirror to
    max_steps / 2 on them); FREE and HIT both occur; steps lies in 1 .. max_steps; a repeat call is bit-identical.
  * the thin wall: HIT on the device while config_clearance at the ten uniform samples reads free by a centimetre.
  * small cases, refusals by message, purity, the VecEnv layer.

Shapes: scene T at the lane-mapping shapes of tests/test_clearance.py -- (3, 5) one partial wavefront over three envs, (65, 3) three full wavefronts that
straddle env boundaries and a partial one, (2, 70) K larger than a wavefront; Panda and baxter_both at (3, 5).

MEASURED: no allowance beyond the imported BOUND was needed; the figures of one run (tools/sweep_parity.py, profiles/sweep_parity.txt) are listed for the record."""
import numpy as np
import pytest
import torch

from robosuite_amd import backend, clearance, sweep
from tests import clearance_scenes as S
from tests import sweep_scenes as W
from tests.test_clearance import BOUND, SHAPES, _actions, _lift, _lift_batch, dev
from tests.util import make_hip

pytestmark = pytest.mark.gpu

# worst figures of one GPU run (profiles/sweep_parity.txt): sample identity |dist - config_clearance(q(t_min))| (m; 0 = bit for bit), certificate shortfall
# max(0, margin - dense minimum) (m), and device L / mirror L - 1.  Nothing below is asserted at 4 x these: the tests hold the imported BOUND and the issue's band.
MEASURED = {
    "T": {"ident": 0.0, "shortfall": 0.0, "bound_rel": 1.839e-7},
    "panda": {"ident": 0.0, "shortfall": 0.0, "bound_rel": 1.171e-7},
    "baxter": {"ident": 0.0, "shortfall": 0.0, "bound_rel": 9.905e-8},
}
SLACK, MAX_STEPS = sweep.DEFAULTS["slack"], sweep.DEFAULTS["max_steps"]
FREE, HIT, UNDECIDED = sweep.FREE, sweep.HIT, sweep.UNDECIDED


# ---- the figures (also what tools/sweep_parity.py prints) ----------------------------------------------------------------------------------------------
def identity_figure(hb, dofs, q0, q1, out, distmax, pairs=None):
    """worst |dist - config_clearance(q(t_min))| and whether dist, pair and fromto are equal bit for bit"""
    st, t, dist, tmin, pair, ft, steps = out
    q = dev(W.at32(q0, q1, tmin.cpu().numpy()[..., None]))
    ref = hb.config_clearance(dofs, q, pairs=pairs, distmax=distmax, chunks=1)
    same = torch.equal(dist, ref[0]) and torch.equal(pair, ref[1]) and torch.equal(ft, ref[2])
    return float((dist - ref[0]).abs().max()), same


def dense_clearance(hb, dofs, q0, q1, t, distmax, n=W.DENSE, pairs=None):
    """config_clearance at n uniform samples over [0, t] of every segment: float64 [B, K, n]"""
    B, K, nd = q0.shape
    ts = t.cpu().numpy().astype(np.float64)[..., None] * np.linspace(0.0, 1.0, n)      # [B, K, n]; the last one is t itself, exactly
    q = W.at32(q0[:, :, None, :], q1[:, :, None, :], ts.astype(np.float32)[..., None]).reshape(B, K * n, nd)
    return hb.config_clearance(dofs, dev(q), pairs=pairs, distmax=distmax, fromto=False)[0].cpu().numpy().astype(np.float64).reshape(B, K, n)


def certificate_figures(hb, dofs, q0, q1, out, distmax, margin, pairs=None):
    """{"shortfall": how far the dense minimum over [0, t] falls below margin, "hit": how far a HIT's value at t lies above margin + slack}"""
    st, t = out[0].cpu().numpy() & 3, out[1]
    c = dense_clearance(hb, dofs, q0, q1, t, distmax, pairs=pairs)
    hit = st == HIT
    held = ~(hit & (t.cpu().numpy() == 0))      # a HIT at the first sample certifies nothing: [0, 0) is empty, and the start may well be in collision
    return {"shortfall": float(np.maximum(0.0, margin - c.min(axis=-1))[held].max()) if held.any() else 0.0, "hit": float(np.maximum(0.0, c[..., -1][hit] - (margin + SLACK)).max()) if hit.any() else 0.0}


def mirror_bounds(flat, qpos, dofs, q0, q1, pairs, overrides=None, params=None):
    B, K = q0.shape[:2]
    pick = lambda x, e: x[e] if isinstance(x, list) else x      # noqa: E731
    return np.array([[sweep.motion_bound(flat, qpos[e], dofs, q0[e, k], q1[e, k], pairs, pick(overrides, e), pick(params, e)) for k in range(K)] for e in range(B)])


def centre_displacement_figure(flat, hb, dofs, q0, q1, pairs, L, allowance, params=None, n=W.DENSE):
    """worst of (displacement of geom1's centre + of geom2's between neighbouring uniform samples, at config_fk poses) - L dt - allowance, over pairs"""
    B, K, nd = q0.shape
    ts = np.broadcast_to(np.linspace(0.0, 1.0, n, dtype=np.float32), (B, K, n))
    q = W.at32(q0[:, :, None, :], q1[:, :, None, :], ts[..., None]).reshape(B, K * n, nd)
    xp, xq = (x.double() for x in hb.config_fk(dofs, dev(q)))
    gb = torch.as_tensor(np.asarray(flat.arrays["geom_bodyid"]).ravel().astype(np.int64), device="cuda")
    gpos = np.asarray(flat.arrays["geom_pos"], dtype=np.float64).reshape(-1, 3) if params is None else None
    gp = torch.as_tensor(gpos if params is None else np.stack([np.asarray(p["geom_pos"]).reshape(-1, 3) for p in params]), device="cuda")
    w, v = xq[:, :, gb, :1], xq[:, :, gb, 1:]                                      # rotate geom_pos by the body's quaternion
    lp = gp[None, None] if params is None else gp[:, None]
    c = xp[:, :, gb] + lp + 2 * torch.cross(v, torch.cross(v, lp.expand_as(v), dim=-1) + w * lp, dim=-1)
    c = c.reshape(B, K, n, -1, 3)
    d = (c[:, :, 1:] - c[:, :, :-1]).norm(dim=-1)                                  # [B, K, n - 1, ngeom]
    pr = torch.as_tensor(np.asarray(pairs, dtype=np.int64), device="cuda")
    worst = (d[..., pr[:, 0]] + d[..., pr[:, 1]]).amax(dim=(2, 3))                 # [B, K]
    return float((worst - L.double() / (n - 1) - allowance).max())


def sweep_checks(scene, flat, hb, dofs, q0, q1, distmax, margin=0.0, overrides=None, params=None, fk_params=None, given=None):
    """one config_sweep call held to every property; -> its outputs and the figures.  given: an explicit pair list (None: the default list)"""
    B, K = q0.shape[:2]
    pairs = clearance.default_pairs(flat, dofs) if given is None else given
    a, b = dev(q0), dev(q1)
    out = hb.config_sweep(dofs, a, b, pairs=given, distmax=distmax, margin=margin)
    st, t, dist, tmin, pair, ft, steps = out
    assert [x.dtype for x in out] == [torch.int32, torch.float32, torch.float32, torch.float32, torch.int32, torch.float32, torch.int32]
    assert all(x.shape == (B, K) for x in (st, t, dist, tmin, pair, steps)) and ft.shape == (B, K, 6)
    again = hb.config_sweep(dofs, a, b, pairs=given, distmax=distmax, margin=margin)
    assert all(torch.equal(x, y) for x, y in zip(out, again))                      # a repeat call: bit-identical
    s = st.cpu().numpy()
    kind = s & 3
    assert not (s & 256).any() and (kind <= 2).all()
    tn, tm, sn = t.cpu().numpy(), tmin.cpu().numpy(), steps.cpu().numpy()
    assert (sn >= 1).all() and (sn <= MAX_STEPS).all() and (tm >= 0).all() and (tm <= tn).all() and (tn <= 1).all()
    assert (tn[kind == FREE] == 1).all() and (tm[kind == HIT] == tn[kind == HIT]).all()      # for a HIT the closest sample is the last one
    none = pair.cpu().numpy() < 0
    assert (dist.cpu().numpy()[none] == np.float32(distmax)).all() and (ft.cpu().numpy()[none] == 0).all() and (kind[none] != HIT).all()
    fig = {}
    fig["ident"], same = identity_figure(hb, dofs, q0, q1, out, distmax, given)
    assert same, "dist / pair / fromto are not config_clearance at q(t_min) bit for bit"
    fig.update(certificate_figures(hb, dofs, q0, q1, out, distmax, margin, given))
    L = hb.config_motion_bound(dofs, a, b, pairs=given)
    assert L.shape == (B, K) and L.dtype == torch.float32
    ref = mirror_bounds(flat, hb.get("qpos").astype(np.float64), dofs, q0, q1, pairs, overrides, params)
    rel = L.cpu().numpy().astype(np.float64) / ref - 1.0
    fig["bound_lo"], fig["bound_hi"] = float(-rel.min()), float(rel.max())
    fig["centres"] = centre_displacement_figure(flat, hb, dofs, q0, q1, pairs, L, 4 * BOUND[scene]["fk_pos"], fk_params)
    for k, v in fig.items():
        print(f"sweep parity scene {scene} ({B}, {K}): {k} {v:.3e}")
    print(f"sweep scene {scene} ({B}, {K}): free {int((kind == FREE).sum())}, hit {int((kind == HIT).sum())}, undecided {int((kind == UNDECIDED).sum())}; "
          f"steps mean {sn.mean():.1f} max {sn.max()}")
    bound = BOUND[scene]["dist"]
    assert fig["shortfall"] <= bound and fig["hit"] <= bound, fig
    assert fig["bound_lo"] <= 1e-5 and fig["bound_hi"] <= 1e-4, fig
    assert fig["centres"] <= 0.0, fig
    return out, fig


# ---- scene T -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_t(tmp_path_factory):
    return S.scene_t(tmp_path_factory.mktemp("sweep_t")), {}


def batch_t(scene_t, B, K, which="all"):
    flat, cache = scene_t
    if (B, K, which) not in cache:
        hm, hb = make_hip(flat, None, B=B)
        hb.set("qpos", S.scene_t_qpos(flat, B).astype(np.float32)); hb.forward()
        dofs = S.dofs_t(flat, which)
        q0, q1 = W.segments(flat, dofs, B, K)
        cache[B, K, which] = dict(hm=hm, hb=hb, dofs=dofs, q0=q0, q1=q1)
    return cache[B, K, which]


@pytest.mark.parametrize("B,K", SHAPES)
def test_sweep_scene_t(scene_t, B, K):
    flat, _ = scene_t
    c = batch_t(scene_t, B, K)
    out, _ = sweep_checks("T", flat, c["hb"], c["dofs"], c["q0"], c["q1"], S.DISTMAX_T)
    kind = out[0].cpu().numpy() & 3
    assert not (kind == UNDECIDED).any() and (kind == FREE).any() and (kind == HIT).any()
    given = c["hb"].config_sweep(c["dofs"], dev(c["q0"]), dev(c["q1"]), pairs=clearance.default_pairs(flat, c["dofs"]), distmax=S.DISTMAX_T)
    assert all(torch.equal(x, y) for x, y in zip(out, given))                      # the default list, given: the same answer
    lean = c["hb"].config_sweep(c["dofs"], dev(c["q0"]), dev(c["q1"]), distmax=S.DISTMAX_T, fromto=False)
    assert lean[5] is None and all(torch.equal(x, y) for x, y in zip(out[:5] + out[6:], lean[:5] + lean[6:]))


def test_margin_and_the_other_dof_list_scene_t(scene_t):
    flat, _ = scene_t
    c = batch_t(scene_t, *SHAPES[0], which="arm")      # the side link is held: bodies with another signature
    out, _ = sweep_checks("T", flat, c["hb"], c["dofs"], c["q0"], c["q1"], S.DISTMAX_T, margin=0.01)
    base = c["hb"].config_sweep(c["dofs"], dev(c["q0"]), dev(c["q1"]), distmax=S.DISTMAX_T)
    assert (out[1] <= base[1]).all()      # a margin can only end a motion earlier


def test_thin_wall_is_hit_where_uniform_samples_read_free():
    flat, dofs, pairs, q0, q1 = W.thin_wall()
    hm, hb = make_hip(flat, None, B=2)
    hb.forward()
    uniform = np.linspace(0.0, 1.0, W.THIN_WALL_SAMPLES + 2, dtype=np.float32)
    q = np.broadcast_to(W.at32(q0[None], q1[None], uniform[:, None])[None], (2, len(uniform), 1))
    d = hb.config_clearance(dofs, dev(q), pairs=pairs)[0]
    assert float(d.min()) >= W.THIN_WALL_FREE_BY      # sampling calls this motion free
    a, b = dev(np.broadcast_to(q0, (2, 1))), dev(np.broadcast_to(q1, (2, 1)))
    st, t, dist, tmin, pair, ft, steps = hb.config_sweep(dofs, a, b, pairs=pairs)      # (2-D ends: K = 1)
    assert st.shape == (2,) and ft.shape == (2, 6)
    print(f"thin wall on the device: status {st.tolist()}, t {t.tolist()}, dist {dist.tolist()}, steps {steps.tolist()}")
    assert (st == HIT).all() and (pair == 0).all() and (dist <= SLACK).all() and (dist >= 0).all()
    assert (t > float(uniform[4])).all() and (t < float(uniform[5])).all()      # between two of the samples that read free
    assert torch.equal(t[0], t[1])


def test_small_cases_scene_t(scene_t):
    flat, _ = scene_t
    c = batch_t(scene_t, *SHAPES[0])
    hb, dofs, a, b = c["hb"], c["dofs"], dev(c["q0"]), dev(c["q1"])
    full = hb.config_sweep(dofs, a, b, distmax=S.DISTMAX_T)
    one = hb.config_sweep(dofs, a, b, distmax=S.DISTMAX_T, max_steps=1)      # one sample: UNDECIDED, or a HIT at once
    first = hb.config_clearance(dofs, a, distmax=S.DISTMAX_T, chunks=1)
    assert (one[6] == 1).all() and (one[1] == 0).all() and (one[3] == 0).all()
    assert torch.equal(one[0] & 3, torch.where(first[0] <= SLACK, HIT, UNDECIDED).int())
    assert torch.equal(one[2], first[0]) and torch.equal(one[4], first[1]) and torch.equal(one[5], first[2])
    assert torch.equal((one[0] & 3) == HIT, full[6] == 1)
    still = hb.config_sweep(dofs, a, a, distmax=S.DISTMAX_T)                   # q0 == q1: one config_clearance call
    assert (hb.config_motion_bound(dofs, a, a) == 0).all() and (still[6] == 1).all()
    assert torch.equal(still[0] & 3, torch.where(first[0] <= SLACK, HIT, FREE).int())
    assert torch.equal(still[1], torch.where(first[0] <= SLACK, 0.0, 1.0)) and (still[3] == 0).all()
    assert torch.equal(still[2], first[0]) and torch.equal(still[4], first[1]) and torch.equal(still[5], first[2])
    two = hb.config_sweep(dofs, a[:, 0], b[:, 0], distmax=S.DISTMAX_T)         # the 2-D convention
    assert all(torch.equal(x, y[:, 0]) for x, y in zip(two, hb.config_sweep(dofs, a[:, :1], b[:, :1], distmax=S.DISTMAX_T)))
    assert torch.equal(hb.config_motion_bound(dofs, a[:, 0], b[:, 0]), hb.config_motion_bound(dofs, a, b)[:, 0])


def test_per_env_parameters_scene_t(tmp_path):
    flat = S.scene_t(tmp_path)
    B, K = 3, 5
    hm, hb = make_hip(flat, None, B=B, per_env=True)
    hb.set("qpos", np.repeat(S.scene_t_qpos(flat, 1), B, axis=0).astype(np.float32)); hb.forward()      # the same state in every env
    dofs = S.dofs_t(flat, "all")
    q0, q1 = (np.repeat(x, B, axis=0) for x in W.segments(flat, dofs, 1, K))                              # ... and the same segments
    before = hb.config_sweep(dofs, dev(q0), dev(q1), distmax=1.0)
    l_before = hb.config_motion_bound(dofs, dev(q0), dev(q1))
    bp, gs = hb.param_get("body_pos"), hb.param_get("geom_size")
    body, g = flat.names["body"].index("l1"), flat.names["geom"].index("g_cyl")
    bp[1, body] += [0.05, -0.03, 0.04]; gs[1, g] = gs[1, g] * [1.6, 1.3, 1.0]      # geom_size alone: geom_rbound stays as it was
    hb.param_set("body_pos", bp[1:2], env0=1); hb.param_set("geom_size", gs[1:2], env0=1)
    hb.forward()
    live = {k: hb.param_get(k) for k in ("body_pos", "geom_size", "geom_pos", "geom_quat")}
    over = [{"body_pos": S.f32(live["body_pos"][e])} for e in range(B)]
    params = [{k: S.f32(live[k][e]) for k in ("geom_size", "geom_pos", "geom_quat")} for e in range(B)]
    after, _ = sweep_checks("T", flat, hb, dofs, q0, q1, 1.0, overrides=over, params=params, fk_params=params)
    l_after = hb.config_motion_bound(dofs, dev(q0), dev(q1))
    for x, y in zip(before, after):
        assert torch.equal(x[0], y[0]) and torch.equal(x[2], y[2])                   # the other envs' answers are unchanged
    assert torch.equal(l_before[0], l_after[0]) and torch.equal(l_before[2], l_after[2])
    assert not torch.equal(before[2][1], after[2][1]) and (l_after[1] > l_before[1]).all()      # a longer arm and a fatter geom: a larger bound


def test_refusals_scene_t(scene_t, tmp_path):
    flat, _ = scene_t
    c = batch_t(scene_t, *SHAPES[0])
    hb, dofs, a, b = c["hb"], c["dofs"], dev(c["q0"]), dev(c["q1"])
    free_dof = int(np.asarray(flat.arrays["jnt_dofadr"]).ravel()[flat.names["joint"].index("fsj")])
    for call in (lambda *x, **k: hb.config_sweep(*x, **k), lambda *x, **k: hb.config_motion_bound(*x, **k)):
        with pytest.raises(backend.RsimError, match="CUDA tensor"):
            call(dofs, a.cpu(), b)                                                  # wrong device
        with pytest.raises(backend.RsimError, match="CUDA tensor"):
            call(dofs, a, b.cpu())
        with pytest.raises(backend.RsimError, match="shape"):
            call(dofs, a[:, :, :3], b[:, :, :3])                                    # wrong shape
        with pytest.raises(backend.RsimError, match="shape"):
            call(dofs, a, b[:, :2])                                                 # the two ends differ
        with pytest.raises(backend.RsimError, match="shape"):
            call(dofs, a[:, :0], b[:, :0])                                          # K = 0
        with pytest.raises(backend.RsimError, match="free joint"):
            call([free_dof] + dofs[1:], a, b)
        with pytest.raises(backend.RsimError, match="listed twice"):
            call([dofs[0]] + dofs[:3], a, b)
        with pytest.raises(backend.RsimError, match="out of range"):
            call([999] + dofs[1:], a, b)
        gn = flat.names["geom"].index
        for bad, word in (([[0, 99]], "out of range"), ([[gn("g_cap"), gn("g_cap")]], "against itself"), (np.zeros((0, 2), dtype=np.int32), "npair < 1")):
            with pytest.raises(backend.RsimError, match=word):
                call(dofs, a, b, pairs=bad)
    for kw, word in ((dict(slack=0.0), "slack"), (dict(slack=-1.0), "slack"), (dict(margin=-1e-3), "margin"), (dict(max_steps=0), "max_steps"),
                     (dict(max_steps=4097), "max_steps"), (dict(distmax=0.011, margin=0.01), "distmax"), (dict(distmax=1e-3), "distmax"), (dict(max_iters=0), "max_iters")):
        with pytest.raises(backend.RsimError, match=word):
            hb.config_sweep(dofs, a, b, **kw)
    # a plane on a moved body
    import os
    from robosuite_amd import mjcf
    from tests import raycast_scenes as R
    R.write_obj(os.path.join(str(tmp_path), "poly.obj"), R.POLY_VERTS)
    flat2 = mjcf.compile_mjcf(S.SCENE_T_XML.replace('<geom name="g_cap"', '<geom name="g_pl" type="plane" size="1 1 0.1"/><geom name="g_cap"'), asset_dir=str(tmp_path))
    hm2, hb2 = make_hip(flat2, None, B=3)
    hb2.forward()
    g = flat2.names["geom"].index
    for call in (hb2.config_sweep, hb2.config_motion_bound):
        with pytest.raises(backend.RsimError, match="plane geom"):
            call(S.dofs_t(flat2, "all"), a, b, pairs=[[g("g_pl"), g("wbox")]])
    assert hb2.config_clearance(S.dofs_t(flat2, "all"), a, pairs=[[g("g_pl"), g("wbox")]])[0].shape == (3, 5)      # (the point query carries it)


# ---- Panda and Baxter ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("panda", "baxter_both"))
def test_arms_default_list(name):
    s = S.arm(name)
    flat, cfg, dofs = s["flat"], s["cfg"], s["dofs"]
    B, K = SHAPES[0]
    hm, hb = make_hip(flat, cfg, B=B)
    hb.set("qpos", np.tile(s["qpos"], (B, 1)).astype(np.float32)); hb.set("qvel", 0); hb.forward()
    q0, q1 = W.segments(flat, dofs, B, K)
    out, _ = sweep_checks("panda" if name == "panda" else "baxter", flat, hb, dofs, q0, q1, S.DISTMAX_ARM)
    assert ((out[0] & 3) == HIT).any()


def test_lift_from_the_home_pose():
    """Most random arm configurations collide, and on the Panda the default list holds link0 / link1, whose geoms stand 1.0 mm apart whatever the arm does:
    every segment above is decided by its first sample.  Here the loop advances: the shipped Lift model, from its start pose (free by 2 cm), towards the seeded
    ends (a fifth of the way), over the default list without parent / child pairs."""
    s, hm, hb = _lift_batch()
    flat, dofs = s["flat"], s["dofs"]
    pairs = W.without_adjacent(flat, clearance.default_pairs(flat, dofs))
    assert 0 < len(pairs) < len(clearance.default_pairs(flat, dofs))
    _, q1 = W.segments(flat, dofs, *SHAPES[0])
    home = np.broadcast_to(hb.get("qpos")[:, None, :7].astype(np.float64), q1.shape).copy()
    q1 = S.f32(home + 0.2 * (q1 - home))      # a fifth of the way: a motion of a size a planner would ask about
    out, _ = sweep_checks("panda", flat, hb, dofs, home, q1, S.DISTMAX_ARM, given=pairs)
    assert (out[6] > 1).all() and (out[1] > 0).all() and ((out[0] & 3) == FREE).any()


# ---- purity and the layers above -----------------------------------------------------------------------------------------------------------------------------
def _lift_segments(s, B=3, K=5):
    return tuple(dev(x) for x in W.segments(s["flat"], s["dofs"], B, K))


def test_state_is_bitwise_unchanged_by_both_calls():
    s, hm, hb = _lift_batch()
    a, b = _lift_segments(s)
    names = ("qpos", "qvel", "time", "xpos", "xquat")
    before = [hb.get(n).copy() for n in names]
    hb.config_sweep(s["dofs"], a, b); hb.config_motion_bound(s["dofs"], a, b)
    for n, x in zip(names, before):
        assert np.array_equal(x, hb.get(n)), n


def test_a_sweep_between_control_steps_changes_nothing_ten_steps_later():
    got = []
    for ask in (False, True):
        s, hm, hb = _lift_batch()
        a, b = _lift_segments(s)
        for t in range(10):
            hb.control_step(_actions(hm, 3, t), 25)
            if ask and t in (0, 4):
                hb.config_sweep(s["dofs"], a, b); hb.config_motion_bound(s["dofs"], a, b)
        got.append((hb.get("qpos").copy(), hb.get("qvel").copy()))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


def test_unmoved_bodies_are_current_behind_a_fused_step():
    s, hm, hb = _lift_batch()
    dofs = [s["dofs"][-1]]      # the last arm joint alone: the links before it are not moved by the motion, and they move in the step
    a, b = dev(np.zeros((3, 2, 1))), dev(np.full((3, 2, 1), 0.5))
    hb.control_step(_actions(hm, 3, 0), 25)      # the derived arrays are stale now: the query brings them up first
    out = hb.config_sweep(dofs, a, b)
    hb.get("xpos")                                  # (a read that refreshes, as the query did)
    assert all(torch.equal(x, y) for x, y in zip(out, hb.config_sweep(dofs, a, b)))
    ident, same = identity_figure(hb, dofs, a.cpu().numpy(), b.cpu().numpy(), out, 1.0)      # ... and its samples are config_clearance's on the refreshed poses
    assert same
    hb.control_step(_actions(hm, 3, 1), 25)
    later = hb.config_sweep(dofs, a, b)
    assert identity_figure(hb, dofs, a.cpu().numpy(), b.cpu().numpy(), later, 1.0)[1]


def test_vec_env_layer():
    from robosuite_amd.vec_env import VecEnv

    s = _lift()
    env = VecEnv("Lift", 3, s["flat"], s["cfg"], horizon=50)
    env.reset()
    a, b = _lift_segments(s)
    out = env.config_sweep(a, b)
    ref = env.env.batch.config_sweep(s["dofs"], a, b)
    assert all(torch.equal(x, y) for x, y in zip(out, ref))
    named = [("gripper0_right_finger1_pad_collision", "cube_g0"), ("table_collision", s["flat"].names["geom"].index("gripper0_right_hand_collision"))]
    st2 = env.config_sweep(a, b, pairs=named, margin=0.005)
    assert st2[0].shape == (3, 5) and int(st2[4].max()) <= 1
    with pytest.raises(ValueError):
        env.config_sweep(a, b, arm=1)
    # a path of three waypoints is its two segments
    mid = 0.5 * (a + b)
    way = torch.stack((a, mid, b), dim=2)      # [3, 5, 3, 7]
    free, seg, t, dist, pair = env.path_clearance(way)
    s1, s2 = env.config_sweep(a, mid, fromto=False), env.config_sweep(mid, b, fromto=False)
    ok1, ok2 = (s1[0] & 3) == FREE, (s2[0] & 3) == FREE
    assert torch.equal(free, ok1 & ok2)
    assert torch.equal(seg, torch.where(~ok1, 0, torch.where(~ok2, 1, -1)))
    first = torch.where(~ok1, 0, 1)                                                   # the segment a path that is not free reports
    closest = torch.where(s2[2] < s1[2], 1, 0)                                        # ... and a free one: its closest segment, the earlier on ties
    which = torch.where(free, closest, first)
    for got, x1, x2 in ((t, s1[1], s2[1]), (dist, s1[2], s2[2]), (pair, s1[4], s2[4])):
        assert torch.equal(got, torch.where(which == 0, x1, x2))
    assert (t[free] == 1).all()
    with pytest.raises(ValueError):
        env.path_clearance(way[:, :, :1])
