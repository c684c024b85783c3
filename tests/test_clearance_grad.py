"""Clearance gradients and the collision cost on the device (csrc/rsim_grad.hip: rsim_config_clearance_grad, rsim_config_collision_cost) against fp64
references: the formula evaluated in fp64 on the device's own outputs, and the host mirror (robosuite_amd/clearance.py clearance_grad / collision_cost) at the
device's own poses.  The reference is never a second device run.

  * unchanged outputs: dist, pair, fromto, status of config_clearance_grad equal config_clearance's bitwise, for chunks 1, 2 and automatic.
  * formula, EVERY candidate: grad against n . (s2 v(p2) - s1 v(p1)) in fp64 from the device's config_fk poses (axis = R_body a, anchor = p_body + R_body
    jnt_pos: every controlled joint of these scenes is its body's only joint), fromto, dist and pair.  Only rounding is left, so candidates closer than a
    millimetre are covered too.  The zero rules (far, overlap, |dist| < 1e-7) are asserted exactly.
  * mirror: grad against the mirror's gradient from ITS OWN witnesses (distance_scenes.REF) and its own joint frames, over the candidates with status 0,
    |dist| >= 1e-3 and the mirror's pair; at most 10 % of those may be dropped for a different pair.
  * cost: cost and grad against the mirror's reduction of the same reference distances; nnear / noverlap equal except where a reference distance lies within
    the distance bound (tests/test_clearance.py BOUND) of d_safe or of 0; chunks 1, 2, the list length and automatic agree within the bound; a repeat call is
    bitwise identical.
  * shapes as tests/test_clearance.py: (3, 5), (65, 3), (2, 70) and 2-D tensors for K = 1.

MEASURED holds the worst figures of one GPU run per scene (profiles/grad_parity.txt, written by tools/grad_parity.py from the functions below); the tests assert
four times that -- the margin is for one box, one run and pose-dependent rounding.  The mirror figure is dominated by the lateral error of the device's witness
points on curved solids at tol = 1e-6, of order sqrt(tol radius) / lever: it is large against the formula figure, and it is what it is (README)."""
import numpy as np
import pytest
import torch

from robosuite_amd import backend, clearance, distance, mjcf
from tests import attach_scenes as A
from tests import clearance_scenes as S
from tests import test_clearance as TC
from tests import test_clearance_grad_host as H
from tests.util import make_hip

pytestmark = pytest.mark.gpu

# worst figures of one GPU run (profiles/grad_parity.txt).  formula / mirror: |grad - reference| per entry (m/rad or m/m); cost: |cost - reference| (m^2);
# cost_grad: per entry of the cost's gradient (m^2/rad).  "chain" is the 16-hinge chain of tests/test_clearance_grad_host.py.
MEASURED = {
    "T": {"formula": 4.152e-7, "mirror": 2.536e-3, "cost": 7.544e-8, "cost_grad": 2.746e-4},
    "panda": {"formula": 6.836e-8, "mirror": 3.870e-4, "cost": 4.913e-8, "cost_grad": 5.608e-5},
    "chain": {"formula": 2.119e-7, "mirror": 2.710e-6, "cost": 7.153e-7, "cost_grad": 2.562e-4},
}
BOUND = {s: {k: 4 * v for k, v in m.items()} for s, m in MEASURED.items()}
DIST_BOUND = {"T": TC.BOUND["T"]["dist"], "panda": TC.BOUND["panda"]["dist"], "chain": TC.BOUND["T"]["dist"]}      # the band about d_safe and 0 for the counts
SHAPES = TC.SHAPES
MIN_DIST = 1e-3      # below it the mirror check leaves a candidate to the formula check (the direction is read from fromto)
D_SAFE = {"T": 0.08, "panda": 0.05, "chain": 0.6}
dev = TC.dev


# ---- the references --------------------------------------------------------------------------------------------------------------------------------------
def frames_from_poses(flat, dofs, xpos, xquat, m32):
    """joint frames from body poses: axis = R_body a, anchor = p_body + R_body jnt_pos -- right where the joint is its body's only one (a hinge turns about its
    own axis through its own anchor, a slide moves along its own axis)"""
    col = clearance._columns(flat, dofs)
    jb, jnum = clearance._I(flat, "jnt_bodyid"), clearance._I(flat, "body_jntnum")
    axis, anchor, slide = np.zeros((len(col), 3)), np.zeros((len(col), 3)), np.zeros(len(col), dtype=bool)
    for j, c in col.items():
        assert jnum[jb[j]] == 1
        R = mjcf.quat2mat(xquat[jb[j]])
        axis[c], anchor[c], slide[c] = R @ m32.jnt_axis[j], xpos[jb[j]] + R @ m32.jnt_pos[j], m32.jnt_type[j] == mjcf.JNT_SLIDE
    return axis, anchor, slide


def make_case(flat, hb, dofs, q, pairs=None, attach=None, held=None, rel=None, overrides=None, params=None):
    """everything the figures need, made once per batch and shape: the device's poses at the candidates, the mirror's per-pair distances there (REF), the
    mirror's joint frames, and each env's signatures.  pairs None: the default list, with the per-env skip rule marked in `active`.  held bool [B, n] / rel
    [B, n, 7] numpy; overrides: a list of one dict per env (FK tables); params: a list of one dict per env (geom tables)."""
    B, K = q.shape[:2]
    att = dict(attach=attach, held=None if held is None else dev(held, torch.bool), rel=None if rel is None else dev(rel)) if attach else {}
    xp, xq = (t.cpu().numpy().astype(np.float64) for t in hb.config_fk(dofs, dev(q), **att))
    plist = clearance.default_pairs(flat, dofs, attach) if pairs is None else np.asarray(pairs, dtype=np.int32)
    par = params if params is not None else S.params32(flat)
    d, ft, st = S.pair_reference(flat, xp, xq, plist, par)
    qpos = hb.get("qpos").astype(np.float64)
    sig, frames = [], {}
    for e in range(B):
        row = None if held is None else held[e]
        sig.append(clearance.signatures(flat, dofs, attach, row) if attach else clearance.signatures(flat, dofs))
        if pairs is None and attach:
            st[e][:, ~clearance.active_pairs(flat, dofs, plist, attach, row)] |= distance.FAR
        m32 = clearance._model32(flat, overrides[e] if overrides else None)
        for k in range(K):
            frames[e, k] = (clearance.joint_frames(flat, qpos[e], dofs, q[e, k], model32=m32), frames_from_poses(flat, dofs, xp[e, k], xq[e, k], m32))
    return dict(flat=flat, hb=hb, dofs=dofs, q=q, pairs=pairs, plist=plist, att=att, xp=xp, xq=xq, d=d, ft=ft, st=st, sig=sig, frames=frames)


def grad_figures(c, out, distmax):
    """device (dist, pair, fromto, status, grad) against the fp64 formula on those very outputs (every candidate) and against the mirror (status 0, |dist| >=
    MIN_DIST, the mirror's pair).  Asserted here: shapes, the zero rules exactly, and that at most 10 % of the mirror check's candidates are dropped."""
    dist, pair, ft, st, grad = (o.cpu().numpy() for o in out)
    flat, gb = c["flat"], clearance._I(c["flat"], "geom_bodyid")
    B, K = c["q"].shape[:2]
    assert grad.shape == (B, K, len(c["dofs"])) and grad.dtype == np.float32
    formula = mirror = 0.0
    eligible = dropped = zeros = 0
    for e in range(B):
        for k in range(K):
            has = pair[e, k] >= 0 and (st[e, k] & (distance.FAR | distance.OVERLAP)) == 0 and abs(dist[e, k]) >= clearance.GRAD_MIN_DIST
            if not has:
                assert not grad[e, k].any(), (e, k)      # far, overlap, the band: exactly zero
                zeros += 1
                continue
            g1, g2 = c["plist"][pair[e, k]]
            f64 = ft[e, k].astype(np.float64)
            want = clearance.pair_grad(c["frames"][e, k][1], c["sig"][e][gb[g1]], c["sig"][e][gb[g2]], f64[:3], f64[3:], float(dist[e, k]))
            formula = max(formula, np.abs(grad[e, k] - want).max())
            if st[e, k] != distance.OK or abs(dist[e, k]) < MIN_DIST:
                continue
            eligible += 1
            r = clearance.reduce_grad(flat, c["plist"], c["d"][e, k], c["ft"][e, k], c["st"][e, k], c["sig"][e], c["frames"][e, k][0], distmax)
            if r[1] != pair[e, k] or r[3] != distance.OK:
                dropped += 1
                continue
            mirror = max(mirror, np.abs(grad[e, k] - r[4]).max())
    assert dropped <= 0.1 * eligible, (dropped, eligible)
    return {"formula": float(formula), "mirror": float(mirror)}, dict(eligible=eligible, dropped=dropped, zeros=zeros)


def cost_figures(c, out, d_safe, dist_bound):
    """device (cost, grad, nnear, noverlap) against the mirror's reduction of the reference distances at the device's poses; the counts are asserted equal
    outside the band of dist_bound about d_safe and 0"""
    cost, grad, nnear, nover = (o.cpu().numpy() for o in out)
    B, K = c["q"].shape[:2]
    assert cost.shape == nnear.shape == nover.shape == (B, K) and grad.shape == (B, K, len(c["dofs"])) and nnear.dtype == np.int32
    fc = fg = 0.0
    several = 0
    for e in range(B):
        for k in range(K):
            d, st = c["d"][e, k], c["st"][e, k]
            r = clearance.reduce_cost(c["flat"], c["plist"], d, c["ft"][e, k], st, c["sig"][e], c["frames"][e, k][0], d_safe)
            live = (st & distance.FAR) == 0
            edge = (live & (np.abs(d - d_safe) <= dist_bound)).any() or (live & (st == distance.OK) & (np.abs(d) <= dist_bound)).any()
            if not edge:
                assert (nnear[e, k], nover[e, k]) == (r[2], r[3]), (e, k, nnear[e, k], nover[e, k], r[2], r[3])
                fc, fg = max(fc, abs(cost[e, k] - r[0])), max(fg, np.abs(grad[e, k] - r[1]).max())
                several += r[2] > 1
    return {"cost": float(fc), "cost_grad": float(fg)}, dict(several=several)


def check(scene, fig):
    for k, v in fig.items():
        print(f"gradient parity scene {scene}: {k} {v:.3e} (bound {BOUND[scene][k]:.1e})")
    for k, v in fig.items():
        assert v <= BOUND[scene][k], (scene, k, v)


# ---- scene T -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_t(tmp_path_factory):
    return S.scene_t(tmp_path_factory.mktemp("grad_t")), {}


def case_t(scene_t, B, K, which="all"):
    flat, cache = scene_t
    if (B, K, which) not in cache:
        hm, hb = make_hip(flat, None, B=B)
        hb.set("qpos", S.scene_t_qpos(flat, B).astype(np.float32)); hb.forward()
        dofs = S.dofs_t(flat, which)
        cache[B, K, which] = dict(make_case(flat, hb, dofs, S.candidates(flat, dofs, B, K)), hm=hm)
    return cache[B, K, which]


def case_panda(B, K, cache={}):
    if (B, K) not in cache:
        s = S.arm("panda")
        hm, hb = make_hip(s["flat"], s["cfg"], B=B)
        hb.set("qpos", np.tile(s["qpos"], (B, 1)).astype(np.float32)); hb.set("qvel", 0); hb.forward()
        cache[B, K] = dict(make_case(s["flat"], hb, s["dofs"], S.candidates(s["flat"], s["dofs"], B, K)), hm=hm)
    return cache[B, K]


def _case(scene_t, scene, B, K):
    return (case_t(scene_t, B, K), S.DISTMAX_T) if scene == "T" else (case_panda(B, K), S.DISTMAX_ARM)


@pytest.mark.parametrize("B,K", SHAPES)
@pytest.mark.parametrize("scene", ("T", "panda"))
def test_outputs_are_config_clearances_bitwise(scene_t, scene, B, K):
    c, distmax = _case(scene_t, scene, B, K)
    hb, q = c["hb"], dev(c["q"])
    for chunks in (1, 2, 0):
        plain = hb.config_clearance(c["dofs"], q, distmax=distmax, chunks=chunks)
        out = hb.config_clearance_grad(c["dofs"], q, distmax=distmax, chunks=chunks)
        assert all(torch.equal(a, b) for a, b in zip(plain, out[:4])), chunks
        assert out[4].dtype == torch.float32 and out[4].shape == (B, K, len(c["dofs"]))


@pytest.mark.parametrize("B,K", SHAPES)
@pytest.mark.parametrize("scene", ("T", "panda"))
def test_gradient(scene_t, scene, B, K):
    c, distmax = _case(scene_t, scene, B, K)
    out = c["hb"].config_clearance_grad(c["dofs"], dev(c["q"]), distmax=distmax)
    fig, n = grad_figures(c, out, distmax)
    print(n)
    check(scene, fig)
    if scene == "T":
        assert n["zeros"] > 0 and n["eligible"] > 0
        st, pair = out[3].cpu().numpy(), out[1].cpu().numpy()
        assert (pair < 0).any() and (st == distance.OVERLAP).any()      # far and overlap: both zero rules are met
    else:
        # the Panda's default list holds link0 / link1 geoms 1.0 mm apart: the minimum of most candidates, under MIN_DIST.  The same check without the pairs
        # that are closer than 2 mm at qpos0, so that the mirror check has candidates
        keep = [i for i, p in enumerate(c["plist"]) if not _static_near(c, i)]
        sub = dict(c, plist=c["plist"][keep], d=c["d"][..., keep], ft=c["ft"][:, :, keep], st=c["st"][..., keep])
        out = c["hb"].config_clearance_grad(c["dofs"], dev(c["q"]), pairs=sub["plist"], distmax=distmax)
        fig, n = grad_figures(sub, out, distmax)
        print(n)
        check(scene, fig)
        assert n["eligible"] > 0


def _static_near(c, i):
    """a listed pair that is closer than 2 mm at every candidate: it would win every minimum"""
    return bool((c["d"][..., i] < 2e-3).all())


@pytest.mark.parametrize("B,K", SHAPES)
@pytest.mark.parametrize("scene", ("T", "panda"))
def test_cost(scene_t, scene, B, K):
    c, _ = _case(scene_t, scene, B, K)
    hb, q, d_safe = c["hb"], dev(c["q"]), D_SAFE[scene]
    base = hb.config_collision_cost(c["dofs"], q, d_safe=d_safe, chunks=1)
    for chunks in (1, 2, len(c["plist"]), 0):
        out = base if chunks == 1 else hb.config_collision_cost(c["dofs"], q, d_safe=d_safe, chunks=chunks)
        fig, n = cost_figures(c, out, d_safe, DIST_BOUND[scene])
        check(scene, fig)
        assert n["several"] > 0
        assert float((out[0] - base[0]).abs().max()) <= BOUND[scene]["cost"] and float((out[1] - base[1]).abs().max()) <= BOUND[scene]["cost_grad"]
        assert torch.equal(out[2], base[2]) and torch.equal(out[3], base[3])
        again = hb.config_collision_cost(c["dofs"], q, d_safe=d_safe, chunks=chunks)      # a repeat call: bit-identical
        assert all(torch.equal(a, b) for a, b in zip(out, again))
    given = hb.config_collision_cost(c["dofs"], q, pairs=c["plist"], d_safe=d_safe, chunks=1)      # the same list, given: the same answer
    assert all(torch.equal(a, b) for a, b in zip(base, given))


def test_two_dimensional_tensors(scene_t):
    c = case_t(scene_t, *SHAPES[0])
    hb, q2 = c["hb"], dev(c["q"][:, 0])
    a, b = hb.config_clearance_grad(c["dofs"], q2, distmax=S.DISTMAX_T), hb.config_clearance_grad(c["dofs"], q2[:, None], distmax=S.DISTMAX_T)
    assert a[4].shape == (3, len(c["dofs"])) and a[2].shape == (3, 6) and all(torch.equal(x, y[:, 0]) for x, y in zip(a, b))
    a, b = hb.config_collision_cost(c["dofs"], q2, d_safe=0.08), hb.config_collision_cost(c["dofs"], q2[:, None], d_safe=0.08)
    assert a[0].shape == (3,) and a[1].shape == (3, len(c["dofs"])) and all(torch.equal(x, y[:, 0]) for x, y in zip(a, b))


def test_refusals(scene_t):
    c = case_t(scene_t, *SHAPES[0])
    hb, q = c["hb"], dev(c["q"])
    for d_safe in (0.0, -0.1):
        with pytest.raises(backend.RsimError, match="d_safe"):
            hb.config_collision_cost(c["dofs"], q, d_safe=d_safe)
    with pytest.raises(backend.RsimError, match="listed twice"):
        hb.config_clearance_grad([c["dofs"][0]] + c["dofs"][:3], q)
    with pytest.raises(backend.RsimError, match="max_iters"):
        hb.config_collision_cost(c["dofs"], q, max_iters=0)


def test_equal_signature_pair_scene_t(scene_t):
    flat, _ = scene_t
    arm = case_t(scene_t, *SHAPES[0], "arm")
    g = flat.names["geom"].index
    pairs = np.array([[g("g_cyl"), g("g_f2")], [g("g_ell"), g("g_f1")]], dtype=np.int32)
    out = arm["hb"].config_clearance_grad(arm["dofs"], dev(arm["q"]), pairs=pairs, distmax=1.0)
    assert (out[3] == distance.OK).any() and float(out[4].abs().max()) <= 4 * 2.0 ** -23      # the two terms are the same fp32 numbers: they cancel to rounding


# ---- attachments ---------------------------------------------------------------------------------------------------------------------------------------
def test_attachments_scene_t(scene_t):
    """half the envs hold, half do not: the envs that hold nothing equal the plain call bitwise, the held ones are checked against the mirror; an explicit list
    with attachments uses the held signature"""
    flat, _ = scene_t
    B, K = 6, 5
    hm, hb = make_hip(flat, None, B=B)
    hb.set("qpos", S.scene_t_qpos(flat, B).astype(np.float32)); hb.forward()
    dofs = S.dofs_t(flat, "all")
    q = S.candidates(flat, dofs, B, K)
    att, rel = A.attach_t(flat), A.rel_given(B)
    held = np.repeat((np.arange(B) % 2 == 0)[:, None], 2, axis=1)
    g = flat.names["geom"].index
    explicit = np.array([[g("fsph"), g("floor")], [g("fbox"), g("wbox")], [g("g_ell"), g("floor")]], dtype=np.int32)
    for pairs, distmax in ((None, S.DISTMAX_T), (explicit, 5.0)):
        c = make_case(flat, hb, dofs, q, pairs=pairs, attach=att, held=held, rel=rel)
        kw = dict(pairs=None if pairs is None else c["plist"], distmax=distmax)
        out = hb.config_clearance_grad(dofs, dev(q), **kw, **c["att"])
        same = hb.config_clearance(dofs, dev(q), **kw, **c["att"])
        assert all(torch.equal(a, b) for a, b in zip(same, out[:4]))
        fig, n = grad_figures(c, out, distmax)
        check("T", fig)
        cost = hb.config_collision_cost(dofs, dev(q), pairs=kw["pairs"], d_safe=0.08, **c["att"])
        check("T", cost_figures(c, cost, 0.08, DIST_BOUND["T"])[0])
        if pairs is None:      # the envs that hold nothing: the plain call on the plain default list, whose pairs are a subset in the same order
            plain = hb.config_clearance_grad(dofs, dev(q), distmax=distmax)
            pc = hb.config_collision_cost(dofs, dev(q), d_safe=0.08)
            for i in (0, 2, 3, 4):
                assert torch.equal(out[i][1::2], plain[i][1::2]), i
            assert all(torch.equal(a[1::2], b[1::2]) for a, b in zip(cost, pc))
        else:                  # a held body against a static geom: the gradient is the carrier's, where the plain call has none
            plain = hb.config_clearance_grad(dofs, dev(q), **kw)
            carried = ((out[1] < 2) & (out[3] == distance.OK))[0::2]      # the envs that hold: a carried body's pair attains the minimum
            assert carried.any() and bool((out[4][0::2][carried].abs().amax(dim=-1) > 0).all())
            free = (plain[1] < 2) & (plain[3] == distance.OK)
            assert float(plain[4][free].abs().max()) == 0 if free.any() else True
            assert all(torch.equal(out[i][1::2], plain[i][1::2]) for i in range(5))


# ---- other cases -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndof", (H.CHAIN_N, 1))
def test_chain_of_sixteen_hinges_and_one_dof(ndof):
    flat = mjcf.compile_mjcf(H.chain_xml())
    B, K = 2, 35      # more than one wavefront
    dofs = S.dofs_of(flat, [f"cj{i}" for i in range(H.CHAIN_N)]) if ndof > 1 else S.dofs_of(flat, ["cj7"])
    hm, hb = make_hip(flat, None, B=B)
    hb.forward()
    c = make_case(flat, hb, dofs, S.candidates(flat, dofs, B, K), pairs=H.chain_pairs(flat))
    out = hb.config_clearance_grad(dofs, dev(c["q"]), pairs=c["plist"], distmax=5.0)
    fig, n = grad_figures(c, out, 5.0)
    check("chain", fig)
    assert n["eligible"] > 0
    for chunks in (1, 3):
        cost = hb.config_collision_cost(dofs, dev(c["q"]), pairs=c["plist"], d_safe=D_SAFE["chain"], chunks=chunks)
        check("chain", cost_figures(c, cost, D_SAFE["chain"], DIST_BOUND["chain"])[0])


def test_per_env_parameters_scene_t(tmp_path):
    flat = S.scene_t(tmp_path)
    B, K = 3, 5
    hm, hb = make_hip(flat, None, B=B, per_env=True)
    hb.set("qpos", np.repeat(S.scene_t_qpos(flat, 1), B, axis=0).astype(np.float32)); hb.forward()
    dofs = S.dofs_t(flat, "all")
    q = np.repeat(S.candidates(flat, dofs, 1, K), B, axis=0)
    before = hb.config_clearance_grad(dofs, dev(q), distmax=1.0)
    bp, ja = hb.param_get("body_pos"), hb.param_get("jnt_axis")
    b, j = flat.names["body"].index("l1"), flat.names["joint"].index("h2")
    bp[1, b] += [0.05, -0.03, 0.04]
    ax = ja[1, j] + [0.3, -0.2, 0.0]
    ja[1, j] = ax / np.linalg.norm(ax)
    hb.param_set("body_pos", bp[1:2], env0=1); hb.param_set("jnt_axis", ja[1:2], env0=1)
    hb.forward()
    live = {k: hb.param_get(k) for k in ("body_pos", "jnt_axis", "geom_size", "geom_pos", "geom_quat")}
    over = [{k: S.f32(live[k][e]) for k in ("body_pos", "jnt_axis")} for e in range(B)]
    params = [{k: S.f32(live[k][e]) for k in ("geom_size", "geom_pos", "geom_quat")} for e in range(B)]
    c = make_case(flat, hb, dofs, q, overrides=over, params=params)
    after = hb.config_clearance_grad(dofs, dev(q), distmax=1.0)
    check("T", grad_figures(c, after, 1.0)[0])
    check("T", cost_figures(c, hb.config_collision_cost(dofs, dev(q), d_safe=0.08), 0.08, DIST_BOUND["T"])[0])
    for a, z in zip(before, after):
        assert torch.equal(a[0], z[0]) and torch.equal(a[2], z[2])      # the other envs' results are unchanged
    assert not torch.equal(before[4][1], after[4][1])


def test_purity_and_tables():
    s, hm, hb = TC._lift_batch()
    q = dev(S.candidates(s["flat"], s["dofs"], 3, 5))
    names = ("qpos", "qvel", "time", "xpos", "xquat")
    before = [hb.get(n).copy() for n in names]
    hb.config_clearance(s["dofs"], q); hb.config_fk(s["dofs"], q)
    assert hb.config_grad_tables() == 0      # a batch that never asked has built no signature table
    hb.config_clearance_grad(s["dofs"], q)
    hb.config_collision_cost(s["dofs"], q)
    assert hb.config_grad_tables() == 1 and hb.config_tables() == 1      # ... one for the dof list, kept; no second body table
    for n, a in zip(names, before):
        assert np.array_equal(a, hb.get(n)), n


def test_collision_cost_is_differentiable():
    from robosuite_amd.vec_env import VecEnv

    s = TC._lift()
    env = VecEnv("Lift", 3, s["flat"], s["cfg"], horizon=50)
    env.reset()
    q = dev(S.candidates(s["flat"], s["dofs"], 3, 5)).requires_grad_(True)
    cost = env.collision_cost(q, 0.05)
    ref = env.config_collision_cost(q.detach(), 0.05)
    assert torch.equal(cost.detach(), ref[0]) and cost.requires_grad
    assert all(torch.equal(x, y) for x, y in zip(ref, env.env.batch.config_collision_cost(s["dofs"], q.detach(), d_safe=0.05)))
    g5 = env.config_clearance_grad(q.detach())
    assert all(torch.equal(x, y) for x, y in zip(g5, env.env.batch.config_clearance_grad(s["dofs"], q.detach())))
    w = torch.arange(1, 16, device="cuda", dtype=torch.float32).reshape(3, 5)
    (cost * w).sum().backward()
    assert torch.equal(q.grad, w[..., None] * ref[1]) and bool(q.grad.abs().sum() > 0)
