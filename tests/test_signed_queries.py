"""Signed distances in config_clearance and config_clearance_grad on the device (csrc/rsim_pen_query.hip k_clear_dist_signed (_att); include/rsim.h
rsim_config_clearance_signed / rsim_config_clearance_grad_signed) against fp64: the mirror robosuite_amd/clearance.py (signed=True) on the device's own
config_fk poses, and the gradient formula on the device's own outputs.  The reference is never a second device run, except where bits are compared.

Candidates: penetration_scenes.arm_cases(3, 70) -- 210, four wavefronts of which one is partial; odd k sunk 2 to 5 mm into the last link, even k uniform in
the joint ranges: lanes that sign an overlap beside lanes that do not.

  * config_clearance(signed=True): dist within BOUND["dist"] of the mirror's smallest signed per-pair value; pair equal unless the mirror's two smallest lie
    within BOUND["dist"] of each other; no status has bit 2; every sunk candidate has dist < 0.
  * the same on the 80 sunk starts of tests/signed_query_scenes.py within BOUND["dist_descend"]: half of them sunk into a box, whose cores overlap, so the
    descent runs (the arm cases are sunk into a capsule, which is exact without descent); their gradient against the formula.
  * identities: a candidate whose unsigned status lacks bit 2 is bit for bit the unsigned call's four outputs for chunks 1, 3 and automatic; chunks 1, 3 and
    the list length agree in dist and pair; a repeat call is bit-identical; config_tables / config_grad_tables read the same before and after.
  * config_clearance_grad(signed=True): the first four outputs are config_clearance(signed=True)'s bits; grad within BOUND["grad"] of clearance.pair_grad in fp64
    on the device's own dist / fromto / poses; on the sunk candidates the unsigned gradient is exactly zero, the signed one is not, and q + eta grad (eta: a
    step of STEP_RAD in the largest entry) raises the mirror's smallest signed distance.
  * attached: the cargo box held by the last link in half of the envs -- the others equal the plain signed call bit for bit, the holders are within bound.
  * VecEnv on the shipped Lift asset; the refusal of a library without the entry, by name.

BOUND = max(4 x MEASURED, floor).  MEASURED: the worst figures of one MI355X run of figures() below (profiles/signed_queries_parity.txt, written by
tools/signed_queries_parity.py).  Floors: 4 x 2^-23 x 1.5 m for a distance (coordinates of this scene stay inside 1.5 m), 4 x 2^-23 x the largest reference
entry for a gradient."""
import numpy as np
import pytest
import torch

from robosuite_amd import backend, clearance, distance
from tests import clearance_scenes as S
from tests import ik_avoid_scenes as IA
from tests import penetration_scenes as Q
from tests import signed_query_scenes as SQ
from tests import test_clearance as TC
from tests import test_clearance_grad as TG
from tests.util import make_hip

pytestmark = pytest.mark.gpu

# worst figures of one MI355X run (profiles/signed_queries_parity.txt): |dist - mirror| (m) over all candidates, over the holders of the attached case and over
# the sunk starts, half of which descend; |grad - formula| per entry (m / rad); "step": tests/test_signed_ik_avoid.py's one-update figure (rad)
MEASURED = {"dist": 8.227e-8, "dist_att": 6.048e-8, "dist_descend": 4.318e-8, "grad": 1.527e-7, "step": 1.709e-6}
ULP4 = 4 * 2.0 ** -23
FLOOR = {"dist": ULP4 * 1.5, "dist_att": ULP4 * 1.5, "dist_descend": ULP4 * 1.5, "step": ULP4 * np.pi}
AB, AK = 3, 70
DISTMAX = 1.0
STEP_RAD = 3e-3
dev = TC.dev


def bound(key, largest=None):
    """max(4 x MEASURED, floor); a gradient's floor is 4 x 2^-23 x the largest reference entry of the run at hand"""
    return max(4 * MEASURED[key], ULP4 * largest if key == "grad" else FLOOR[key])


def np_(out):
    return tuple(t.cpu().numpy() for t in out)


def mirror_pairs(flat, qpos, dofs, q, pairs, xp, xq, **att):
    """the mirror's signed per-pair (dist, fromto, status) of one candidate at the device's poses, far pairs at +inf, and the env's signatures"""
    p, d, ft, st, sig = clearance._pair_distances(flat, qpos, dofs, q, pairs, DISTMAX, Q.REF["tol"], Q.REF["max_iters"], S.params32(flat), None, (xp, xq),
                                                  att.get("attach"), att.get("held"), att.get("rel"), False, True)
    return p, np.where((st & distance.FAR) == 0, d, np.inf), ft, st, sig


def make_arm():
    c = Q.arm_cases(AB, AK)
    flat, dofs, pairs = c["flat"], c["dofs"], c["pairs"]
    hm, hb = make_hip(flat, None, B=AB)
    hb.set("qpos", c["qpos"].astype(np.float32))
    hb.forward()
    q = dev(c["q"])
    plain = hb.config_clearance_grad(dofs, q, pairs=pairs, distmax=DISTMAX, chunks=1)
    tables = (hb.config_tables(), hb.config_grad_tables())
    signed = hb.config_clearance(dofs, q, pairs=pairs, distmax=DISTMAX, chunks=1, signed=True)
    signed_grad = hb.config_clearance_grad(dofs, q, pairs=pairs, distmax=DISTMAX, chunks=1, signed=True)
    assert (hb.config_tables(), hb.config_grad_tables()) == tables                                  # the signed calls build no table of their own
    xp, xq = (o.cpu().numpy().astype(np.float64) for o in hb.config_fk(dofs, q))
    per = [[mirror_pairs(flat, c["qpos"][e], dofs, c["q"][e, k], pairs, xp[e, k], xq[e, k])[1] for k in range(AK)] for e in range(AB)]
    return dict(c=c, hm=hm, hb=hb, q=q, plain=plain, signed=signed, signed_grad=signed_grad, xp=xp, xq=xq, per=np.array(per))


@pytest.fixture(scope="module")
def arm():
    return make_arm()


def dist_figures(per, out):
    """device (dist, pair, fromto, status), as numpy arrays, against the mirror's per-pair values [.., P]: (worst |dist - mirror|, pair == the mirror's, the gap
    between the mirror's two smallest, the mirror's smallest)"""
    dist, pair, ft, st = out
    srt = np.sort(per, axis=-1)
    md, mp, gap = srt[..., 0], np.argmin(per, axis=-1), srt[..., 1] - srt[..., 0]
    return float(np.abs(dist - md).max()), (pair == mp), gap, md


def grad_figures(c, xp, xq, out):
    """device grad against clearance.pair_grad in fp64 on the device's own dist / pair / fromto and config_fk poses: (worst |difference|, largest |reference|)"""
    dist, pair, ft, st, grad = np_(out)
    flat, dofs, pairs = c["flat"], c["dofs"], c["pairs"]
    gb, sig, m32 = clearance._I(flat, "geom_bodyid"), clearance.signatures(flat, dofs), clearance._model32(flat)
    worst = largest = 0.0
    for e in range(dist.shape[0]):
        for k in range(dist.shape[1]):
            if pair[e, k] < 0 or (st[e, k] & (distance.FAR | distance.OVERLAP)) or abs(dist[e, k]) < clearance.GRAD_MIN_DIST:
                assert not grad[e, k].any(), (e, k)
                continue
            g1, g2 = pairs[pair[e, k]]
            f64 = ft[e, k].astype(np.float64)
            want = clearance.pair_grad(TG.frames_from_poses(flat, dofs, xp[e, k], xq[e, k], m32), sig[gb[g1]], sig[gb[g2]], f64[:3], f64[3:], float(dist[e, k]))
            worst, largest = max(worst, np.abs(grad[e, k] - want).max()), max(largest, np.abs(want).max())
    return float(worst), float(largest)


def make_attached():
    """the cargo box held by l4 (ik_avoid_scenes.CARGO_REL) in the first half of B = 4 envs, K = 16 uniform candidates, the default list with the attachment"""
    a = IA.scene_a()
    flat, dofs = a["flat"], a["dofs"]
    B, K = 4, 16
    att = IA.cargo_attach()
    q0 = S.f32(np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel())
    q = Q.arm_cases(AB, AK)["q"][:, ::2].reshape(-1, len(dofs))[:B * K].reshape(B, K, len(dofs))      # the uniform draws of the arm cases
    held, rel = np.arange(B)[:, None] < B // 2, np.tile(IA.CARGO_REL, (B, 1, 1))
    hm, hb = make_hip(flat, None, B=B)
    hb.set("qpos", np.tile(q0, (B, 1)).astype(np.float32))
    hb.forward()
    kw = dict(attach=att, held=dev(held, torch.bool), rel=dev(rel))
    out = hb.config_clearance(dofs, dev(q), distmax=DISTMAX, chunks=1, signed=True, **kw)
    plain = hb.config_clearance(dofs, dev(q), distmax=DISTMAX, chunks=1, signed=True)
    xp, xq = (o.cpu().numpy().astype(np.float64) for o in hb.config_fk(dofs, dev(q), **kw))
    per = np.array([[mirror_pairs(flat, q0, dofs, q[e, k], None, xp[e, k], xq[e, k], attach=att, held=held[e], rel=rel[e])[1] for k in range(K)] for e in range(B)])
    return dict(flat=flat, dofs=dofs, att=att, held=held, hm=hm, hb=hb, out=out, plain=plain, per=per)


def make_starts():
    """the sunk starts of tests/signed_query_scenes.py as candidates: B = 20, K = 4, half of the envs sunk into the box b3 -- box against box, whose cores overlap:
    the lanes that DESCEND (the arm cases above are sunk into a capsule, which is exact without descent)"""
    c = SQ.cases()
    hm, hb = make_hip(c["flat"], None, B=SQ.B)
    hb.set("qpos", c["qpos"].astype(np.float32))
    hb.forward()
    q = dev(c["q_init"])
    signed = hb.config_clearance_grad(c["dofs"], q, pairs=c["pairs"], distmax=DISTMAX, signed=True)
    xp, xq = (o.cpu().numpy().astype(np.float64) for o in hb.config_fk(c["dofs"], q))
    per = np.array([[mirror_pairs(c["flat"], c["qpos"][e], c["dofs"], c["q_init"][e, k], c["pairs"], xp[e, k], xq[e, k])[1] for k in range(SQ.K)] for e in range(SQ.B)])
    return dict(c=c, hm=hm, hb=hb, q=q, signed=signed[:4], grad=signed[4], per=per, xp=xp, xq=xq)


def figures():
    """every MEASURED figure of this file, from one run (tools/signed_queries_parity.py)"""
    a = make_arm()
    fig = {"dist": dist_figures(a["per"], np_(a["signed"]))[0]}
    fig["grad"], fig["grad_largest"] = grad_figures(a["c"], a["xp"], a["xq"], a["signed_grad"])
    t = make_attached()
    h = t["held"][:, 0]
    fig["dist_att"] = dist_figures(t["per"][h], tuple(o[h] for o in np_(t["out"])))[0]
    s = make_starts()
    fig["dist_descend"] = dist_figures(s["per"], np_(s["signed"]))[0]
    return fig


# ---- config_clearance(signed=True) against the mirror ----------------------------------------------------------------------------------------------------
def test_signed_clearance_against_the_mirror(arm):
    worst, same_pair, gap, md = dist_figures(arm["per"], np_(arm["signed"]))
    dist, pair, ft, st = np_(arm["signed"])
    sunk = arm["c"]["sunk"]
    print(f"signed clearance, {AB} x {AK} candidates: worst |dist - mirror| {worst:.3e} (bound {bound('dist'):.1e}); {int((dist < 0).sum())} below zero, {int(sunk.sum())} sunk; "
          f"{int((~same_pair).sum())} with another pair than the mirror, smallest gap among the others {gap[same_pair].min():.2e}")
    assert worst <= bound("dist")
    assert same_pair[gap > bound("dist")].all()
    assert not (st & distance.OVERLAP).any() and (pair >= 0).all()
    assert (dist[sunk] < 0).all() and (md[sunk] <= -Q.ARM_DEPTH[0] + bound("dist")).all()
    n = (ft[..., 3:] - ft[..., :3])[sunk] / dist[sunk][:, None]
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 2e-4      # six fp32 coordinates up to 1 m, 2^-24 each, over a depth of 2e-3 m


def test_identities(arm):
    hb, c, q = arm["hb"], arm["c"], arm["q"]
    dofs, pairs = c["dofs"], c["pairs"]
    kw = dict(pairs=pairs, distmax=DISTMAX)
    for chunks in (1, 3, 0):
        plain = hb.config_clearance(dofs, q, chunks=chunks, **kw)
        signed = hb.config_clearance(dofs, q, chunks=chunks, signed=True, **kw)
        free = (plain[3] & distance.OVERLAP) == 0
        assert int(free.sum()) >= AB * AK // 3 and int((~free).sum()) >= AB * AK // 3
        assert all(torch.equal(x[free], y[free]) for x, y in zip(plain, signed)), chunks
        assert bool((signed[0][~free] < 0).all())      # what the unsigned call reports as 0 with status 2
    one = arm["signed"]
    for chunks in (3, len(pairs)):
        other = hb.config_clearance(dofs, q, chunks=chunks, signed=True, **kw)
        assert torch.equal(one[0], other[0]) and torch.equal(one[1], other[1]), chunks
    again = hb.config_clearance(dofs, q, chunks=1, signed=True, **kw)
    assert all(torch.equal(x, y) for x, y in zip(one, again))
    with pytest.raises(backend.RsimError, match="pen goes with signed=True"):
        hb.config_clearance(dofs, q, pen=dict(pen_iters=8), **kw)
    with pytest.raises(backend.RsimError, match="pen_iters"):
        hb.config_clearance(dofs, q, signed=True, pen=dict(pen_iters=0), **kw)


def test_signed_clearance_where_the_descent_runs():
    s = make_starts()
    c = s["c"]
    worst, same_pair, gap, md = dist_figures(s["per"], np_(s["signed"]))
    dist, pair, ft, st = np_(s["signed"])
    box = np.arange(SQ.B) % 2 == 0      # sunk into b3: box against box
    print(f"signed clearance on the {dist.size} sunk starts: worst |dist - mirror| {worst:.3e} (bound {bound('dist_descend'):.1e}); into the box "
          f"{np.abs(dist - md)[box].max():.3e}, into the capsule {np.abs(dist - md)[~box].max():.3e}; {int((~same_pair).sum())} with another pair than the mirror")
    assert worst <= bound("dist_descend")
    assert same_pair[gap > bound("dist_descend")].all()
    assert (dist < 0).all() and not (st & distance.OVERLAP).any()
    assert (np.abs(s["grad"].cpu().numpy()).max(axis=2) > 0).all()      # every sunk start has a direction out
    worst_g, largest = grad_figures(c, s["xp"], s["xq"], tuple(s["signed"]) + (s["grad"],))
    print(f"   its gradient against the formula: {worst_g:.3e} (bound {bound('grad', largest):.1e})")
    assert worst_g <= bound("grad", largest)


# ---- config_clearance_grad(signed=True) ------------------------------------------------------------------------------------------------------------------
def test_signed_gradient(arm):
    c = arm["c"]
    flat, dofs, pairs, sunk = c["flat"], c["dofs"], c["pairs"], c["sunk"]
    assert all(torch.equal(x, y) for x, y in zip(arm["signed"], arm["signed_grad"][:4]))
    worst, largest = grad_figures(c, arm["xp"], arm["xq"], arm["signed_grad"])
    print(f"signed clearance gradient: worst |grad - formula| {worst:.3e} (bound {bound('grad', largest):.1e}; largest reference entry {largest:.3f})")
    assert worst <= bound("grad", largest)
    pg, sg = arm["plain"][4].cpu().numpy(), arm["signed_grad"][4].cpu().numpy().astype(np.float64)
    assert not pg[sunk].any() and (np.abs(sg[sunk]).max(axis=1) > 0).all()
    params = S.params32(flat)
    raised = []
    for e, k in np.argwhere(sunk)[::3]:
        eta = STEP_RAD / np.abs(sg[e, k]).max()
        before, after = (SQ.smallest(flat, c["qpos"][e], dofs, x, pairs, params)[0] for x in (c["q"][e, k], c["q"][e, k] + eta * sg[e, k]))
        raised.append(after - before)
    print(f"q + eta grad, a step of {STEP_RAD} rad in the largest entry, raises the smallest signed distance of {len(raised)} sunk candidates by {min(raised):.2e} .. {max(raised):.2e} m")
    assert min(raised) > 0


# ---- attachments -----------------------------------------------------------------------------------------------------------------------------------------
def test_attached_case():
    t = make_attached()
    flat, dofs, held = t["flat"], t["dofs"], t["held"][:, 0]
    full, part = clearance.default_pairs(flat, dofs, t["att"]), clearance.default_pairs(flat, dofs)
    index = np.array([int(np.flatnonzero((full == p).all(axis=1))[0]) for p in part])      # where the plain list's pairs sit in the attachment's list
    d, pr, ft, st = np_(t["out"])
    pd, pp, pf, ps = np_(t["plain"])
    free = ~held
    assert np.array_equal(d[free], pd[free]) and np.array_equal(ft[free], pf[free]) and np.array_equal(st[free], ps[free])
    assert np.array_equal(pr[free], np.where(pp[free] >= 0, index[np.maximum(pp[free], 0)], -1))
    worst, same_pair, gap, md = dist_figures(t["per"][held], tuple(o[held] for o in (d, pr, ft, st)))
    print(f"attached, {int(held.sum())} envs holding: worst |dist - mirror| {worst:.3e} (bound {bound('dist_att'):.1e}); {int((d[held] < 0).sum())} of {d[held].size} below zero, "
          f"{int((d[held] != pd[held]).sum())} differ from the call without the attachment")
    assert worst <= bound("dist_att") and same_pair[gap > bound("dist_att")].all()
    assert not (st & distance.OVERLAP).any()
    assert (d[held] != pd[held]).any() and (d[held] < 0).any()      # the box is in the way, and in some candidates in the scene


# ---- VecEnv, refusals ----------------------------------------------------------------------------------------------------------------------------------------
def test_vec_env_and_refusals(monkeypatch):
    from robosuite_amd.vec_env import VecEnv

    s = TC._lift()
    env = VecEnv("Lift", 3, s["flat"], s["cfg"], horizon=50)
    env.reset()
    hb = env.env.batch
    q = dev(S.candidates(s["flat"], s["dofs"], 3, 5))
    env.config_clearance_grad(q)
    tables = (hb.config_tables(), hb.config_grad_tables())
    out = env.config_clearance(q, signed=True)
    assert all(torch.equal(x, y) for x, y in zip(out, hb.config_clearance(s["dofs"], q, signed=True)))
    outg = env.config_clearance_grad(q, signed=True, pen=dict(pen_iters=32))
    assert all(torch.equal(x, y) for x, y in zip(outg, hb.config_clearance_grad(s["dofs"], q, signed=True, pen=dict(pen_iters=32))))
    assert (hb.config_tables(), hb.config_grad_tables()) == tables
    assert not bool((out[3] & distance.OVERLAP).any())
    for entry, call in (("rsim_config_clearance_signed", lambda: env.config_clearance(q, signed=True)),
                        ("rsim_config_clearance_grad_signed", lambda: env.config_clearance_grad(q, signed=True)),
                        ("rsim_ik_site_avoid_signed", lambda: env.solve_ik_avoid(dev(np.zeros((3, 3))), signed=True))):
        with monkeypatch.context() as m:      # a library from before these entries
            m.setattr(backend, "hasattr", lambda o, name, entry=entry: name != entry and hasattr(o, name), raising=False)
            with pytest.raises(backend.RsimError, match=f"the loaded library has no {entry}"):
                call()
