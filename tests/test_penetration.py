"""The signed distance of overlapping convex pairs on the device (csrc/rsim_pen.hip: rsim_geom_distance_signed, rsim_config_collision_cost_signed) against the
fp64 host mirror (robosuite_amd/penetration.py) on the poses read back from the device, geometry rounded to fp32.  The reference is never a second device run.

Scenes P and P2 (tests/penetration_scenes.py: two casts of eight free bodies), B = 70 envs -- one full wavefront and a partial one, lanes that descend beside lanes that do not -- all 28 pairs.
  * a pair whose unsigned status lacks the overlap bit: dist, fromto and status of signed=True equal the unsigned call's bit for bit;
  * dist on EVERY pair outside the band within BOUND["dist"] of the mirror (the signed distance is continuous through touching, so nothing else is left out);
    an overlapping pair outside the band has status 0, dist < 0 and no cap bit;
  * the certificate on every overlapping pair, band or not, from the device's own witnesses and n = (p2 - p1) / dist -- the gradient formula's direction --
    in fp64: | -dist - delta(n) |, h_A(n) - n . p1 and h_B(-n) + n . p2, each within BOUND["cert"] outside the band and BOUND["cert_band"] inside it, where
    depths below 1e-4 m leave n little to be read from.  (|p2 - p1 - dist n| is zero by this n.)
  * a pair inside the band (penetration_scenes.in_band, the mirror alone; at most 10 % of the overlapping pairs): depth >= multistart_depth - BOUND["dist"] only.
BOUND is four times what one GPU run measured (profiles/penetration_parity.txt, written by tools/penetration_parity.py from the functions below), floored at
4 x 2^-23 x the coordinate scale, 1.5 m: tests/test_distance.py's rule and its reason -- one box, one run, pose-dependent rounding.  The certificate figure is
dominated by n read from fp32 world coordinates: ulp(1.5 m) / |dist| of angle times the shapes' size (README, "the direction is read from fromto").

The signed collision cost on the five-hinge arm of tests/ik_avoid_scenes.py with its cargo box sunk 2 .. 5 mm into the last link (penetration_scenes.arm_cases),
B = 3, K = 70: against the fp64 formula (clearance.reduce_cost) on the device's own per-pair dist / fromto -- read from a second batch of B K envs posed at the
candidates and queried with geom_distance(signed=True) -- and joint frames from the device's config_fk poses; bounds as above, floored at 4 x 2^-23 x d_safe^2
(cost) and x d_safe (gradient)."""
import numpy as np
import pytest
import torch

from robosuite_amd import backend, clearance
from robosuite_amd import distance as D
from robosuite_amd import penetration as P
from tests import distance_scenes as S
from tests import penetration_scenes as Q
from tests.util import make_hip

pytestmark = pytest.mark.gpu

B = 70
SCALE = 1.5                                    # metres: the largest coordinate of scene P
FLOOR = 4 * 2.0 ** -23 * SCALE
# worst figures of one GPU run over both scenes (profiles/penetration_parity.txt): |dist - mirror| outside the band, the certificate's worst residual, and for the arm
# |cost - formula| (m^2) and per entry of its gradient (m^2 / rad)
MEASURED = {"dist": 1.176e-4, "cert": 2.571e-5, "cert_band": 2.545e-8, "cost": 2.829e-8, "cost_grad": 2.245e-7}
BOUND = {"dist": max(4 * MEASURED["dist"], FLOOR), "cert": max(4 * MEASURED["cert"], FLOOR), "cert_band": max(4 * MEASURED["cert_band"], FLOOR),
         "cost": max(4 * MEASURED["cost"], 4 * 2.0 ** -23 * Q.ARM_D_SAFE ** 2), "cost_grad": max(4 * MEASURED["cost_grad"], 4 * 2.0 ** -23 * Q.ARM_D_SAFE)}
WORST = {}


def dev(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32, device="cuda")


# ---- scene P ---------------------------------------------------------------------------------------------------------------------------------------------
def make_scene(tmpdir, cast="P"):
    """the batch of B envs at scene P's (P2's) seeded poses, both calls' results and the mirror's reference (also what tools/penetration_parity.py measures on)"""
    flat = Q.scene_p(tmpdir, cast)
    pairs = Q.all_pairs(flat)
    hm, hb = make_hip(flat, None, B=B)
    hb.set("qpos", Q.scene_p_qpos(flat, B, Q.SEEDS[cast]).astype(np.float32))
    hb.forward()
    xp, xq = hb.get("xpos").astype(np.float64), hb.get("xquat").astype(np.float64)
    plain = hb.geom_distance(pairs, distmax=Q.DISTMAX)
    signed = hb.geom_distance(pairs, distmax=Q.DISTMAX, signed=True, steps=True)
    return dict(flat=flat, pairs=pairs, hm=hm, hb=hb, plain=plain, signed=signed, ref=Q.reference(flat, xp, xq, pairs, Q.DISTMAX))


@pytest.fixture(scope="module", params=("P", "P2"))
def scene(request, tmp_path_factory):
    return make_scene(tmp_path_factory.mktemp("pen"), request.param)


def figures(s):
    """-> (dict of worst figures, dict of counts); asserts what is exact"""
    ref = s["ref"]
    ud, uf, ust = (o.cpu().numpy() for o in s["plain"])
    d, f, st, steps = (o.cpu().numpy() for o in s["signed"])
    same = (ust & D.OVERLAP) == 0
    assert np.array_equal(d[same], ud[same]) and np.array_equal(f[same], uf[same]) and np.array_equal(st[same], ust[same]) and (steps[same] == 0).all()
    over, band = (ref["plain"] & D.OVERLAP) != 0, ref["band"]
    assert same.any() and (~same).any() and (steps > 0).any() and ((steps[:64] > 0).any(axis=0) & (steps[:64] == 0).any(axis=0)).any()      # side by side
    assert band[over].mean() <= Q.BAND_SHARE, (int(band.sum()), int(over.sum()))
    assert not (st & D.OVERLAP).any()
    held = over & ~band
    assert (st[held] == D.OK).all() and (d[held] < 0).all(), np.argwhere(held & ((st != 0) | (d >= 0)))[:8]
    err = np.abs(d.astype(np.float64) - ref["dist"])
    worst_cert, worst_band, worst_ms = 0.0, 0.0, 0.0
    recs = ref["recs"]
    npair = len(s["pairs"])
    for e, k in np.argwhere(over & (d < 0)):
        g1, g2 = recs[e * npair + k]
        res = Q.certificate(g1, g2, float(d[e, k]), f[e, k].astype(np.float64))
        if band[e, k]:
            worst_band = max(worst_band, max(abs(r) for r in res[:3]))
            worst_ms = max(worst_ms, P.multistart_depth(g1, g2)[0] + float(d[e, k]))      # how far the depth is BELOW the global reference
        else:
            worst_cert = max(worst_cert, max(abs(r) for r in res[:3]))
    desc = steps[steps > 0]
    return ({"dist": float(err[~band].max()), "cert": worst_cert, "cert_band": worst_band, "below_multistart": worst_ms},
            {"pairs": int(d.size), "overlap": int(over.sum()), "band": int(band.sum()), "descend": int(desc.size), "steps_mean": float(desc.mean()),
             "steps_worst": int(desc.max()), "cap": int(((st & (D.CAP | P.PEN_CAP)) != 0).sum()), "mirror_steps_mean": float(ref["steps"][ref["steps"] > 0].mean())})


def test_scene_p_against_the_mirror(scene):
    fig, n = figures(scene)
    WORST.update({k: max(v, WORST.get(k, 0.0)) for k, v in fig.items()})
    print(f"penetration parity: {n}; worst |dist - mirror| {fig['dist']:.3e} (bound {BOUND['dist']:.1e}), certificate {fig['cert']:.3e} (bound {BOUND['cert']:.1e}), in the band {fig['cert_band']:.3e} (bound {BOUND['cert_band']:.1e}), "
          f"depth below the multistart minimum in the band {fig['below_multistart']:.3e}")
    assert n["cap"] == 0
    assert fig["dist"] <= BOUND["dist"] and fig["cert"] <= BOUND["cert"] and fig["cert_band"] <= BOUND["cert_band"] and fig["below_multistart"] <= BOUND["dist"]


def test_repeat_call_and_options(scene):
    hb, pairs = scene["hb"], scene["pairs"]
    again = hb.geom_distance(pairs, distmax=Q.DISTMAX, signed=True, steps=True)
    assert all(torch.equal(a, b) for a, b in zip(scene["signed"], again))                        # bit-identical
    three = hb.geom_distance(pairs, distmax=Q.DISTMAX, signed=True)
    assert len(three) == 3 and all(torch.equal(a, b) for a, b in zip(three, again[:3]))
    d_only = hb.geom_distance(pairs, distmax=Q.DISTMAX, signed=True, fromto=False)
    assert d_only[1] is None and torch.equal(d_only[0], again[0]) and torch.equal(d_only[2], again[2])
    for bad in ({"pen_iters": 0}, {"pen_iters": P.PEN_ITERS_LIMIT + 1}, {"offset": 0.0}, {"pen_tol": -1.0}, {"rho": 1.0}):
        with pytest.raises(backend.RsimError, match="penetration option"):
            hb.geom_distance(pairs, signed=True, pen=bad)
    with pytest.raises(backend.RsimError, match="signed=True"):
        hb.geom_distance(pairs, pen={"offset": 1e-3})


def test_one_projection_sets_the_cap_bit_and_stays_a_directional_depth(scene):
    hb, pairs, ref = scene["hb"], scene["pairs"], scene["ref"]
    d, f, st, steps = (o.cpu().numpy() for o in hb.geom_distance(pairs, distmax=Q.DISTMAX, signed=True, pen={"pen_iters": 1}, steps=True))
    capped = (st & P.PEN_CAP) != 0
    assert capped.any() and (steps[capped] == 1).all() and (steps <= 1).all()
    full = scene["signed"][0].cpu().numpy()
    assert (d[capped] <= full[capped] + BOUND["dist"]).all()                                     # an upper bound of the depth the full descent reaches
    npair = len(pairs)
    worst = 0.0
    for e, k in np.argwhere(capped):
        g1, g2 = ref["recs"][e * npair + k]
        worst = max(worst, Q.certificate(g1, g2, float(d[e, k]), f[e, k].astype(np.float64))[0])
    print(f"pen_iters = 1: {capped.sum()} pairs capped, worst | -dist - delta(n) | {worst:.3e} (bound {BOUND['cert']:.1e})")
    assert worst <= BOUND["cert"]


def test_body_distance_signed_is_the_minimum_over_its_pairs():
    from robosuite_amd.vec_env import VecEnv
    from tests import raycast_scenes as R

    flat, cfg = R.lift()
    env = VecEnv("Lift", 3, flat, cfg, horizon=50)
    env.reset()
    env.step(torch.zeros((3, env.action_dim), device="cuda"))
    dm, fm, k, pairs = env.body_distance(S.L_ROBOT, S.L_SCENE, distmax=S.DISTMAX_L, signed=True)
    full = env.env.batch.geom_distance(pairs, distmax=S.DISTMAX_L, signed=True)
    assert torch.equal(dm, full[0].min(dim=1).values) and torch.equal(fm, full[1][torch.arange(3), k])
    named = env.geom_distance([("table_collision", "cube_g0")], distmax=S.DISTMAX_L, signed=True)
    ids = np.array([[flat.names["geom"].index("table_collision"), flat.names["geom"].index("cube_g0")]], dtype=np.int32)
    assert all(torch.equal(a, b) for a, b in zip(named, env.env.batch.geom_distance(ids, distmax=S.DISTMAX_L, signed=True)))
    assert not (full[2] & D.OVERLAP).any()


# ---- the signed collision cost on the five-hinge arm ------------------------------------------------------------------------------------------------------
AB, AK = 3, 70


def make_arm():
    from tests import test_clearance_grad as TG

    c = Q.arm_cases(AB, AK)
    flat, dofs, pairs = c["flat"], c["dofs"], c["pairs"]
    hm, hb = make_hip(flat, None, B=AB)
    hb.set("qpos", c["qpos"].astype(np.float32))
    hb.forward()
    q = dev(c["q"])
    plain = hb.config_collision_cost(dofs, q, pairs=pairs, d_safe=Q.ARM_D_SAFE, chunks=1)
    tables = (hb.config_tables(), hb.config_grad_tables())
    signed = hb.config_collision_cost(dofs, q, pairs=pairs, d_safe=Q.ARM_D_SAFE, chunks=1, signed=True)
    assert (hb.config_tables(), hb.config_grad_tables()) == tables                              # the signed call builds no table of its own
    # the device's own per-pair results: a batch of B K envs posed at the candidates
    qadr = [int(np.asarray(flat.arrays["jnt_qposadr"]).ravel()[list(np.asarray(flat.arrays["jnt_dofadr"]).ravel()).index(dof)]) for dof in dofs]
    wide = np.repeat(c["qpos"], AK, axis=0)
    wide[:, qadr] = c["q"].reshape(AB * AK, -1)
    hm2, hb2 = make_hip(flat, None, B=AB * AK)
    hb2.set("qpos", wide.astype(np.float32))
    hb2.forward()
    per_pair = tuple(o.cpu().numpy().astype(np.float64) if o.dtype != torch.int32 else o.cpu().numpy() for o in hb2.geom_distance(pairs, distmax=Q.ARM_D_SAFE, signed=True))
    xp, xq = (o.cpu().numpy().astype(np.float64) for o in hb.config_fk(dofs, q))
    m32, sig = clearance._model32(flat), clearance.signatures(flat, dofs, None, None)
    formula = [clearance.reduce_cost(flat, pairs, per_pair[0][i], per_pair[1][i], per_pair[2][i], sig,
                                     TG.frames_from_poses(flat, dofs, xp[i // AK, i % AK], xq[i // AK, i % AK], m32), Q.ARM_D_SAFE, signed=True) for i in range(AB * AK)]
    return dict(c=c, hb=hb, q=q, plain=plain, signed=signed, formula=formula, per_pair=per_pair)


@pytest.fixture(scope="module")
def arm():
    return make_arm()


def arm_figures(a):
    cost, grad, nnear, nover = (o.cpu().numpy().reshape((AB * AK,) + tuple(o.shape[2:])) for o in a["signed"])
    rc, rg = np.array([f[0] for f in a["formula"]]), np.array([f[1] for f in a["formula"]])
    rn, ro = np.array([f[2] for f in a["formula"]]), np.array([f[3] for f in a["formula"]])
    d, near = a["per_pair"][0], (a["per_pair"][2] & D.FAR) == 0
    edge = (near & ((np.abs(d - Q.ARM_D_SAFE) <= BOUND["dist"]) | (np.abs(d) <= BOUND["dist"]))).any(axis=1)      # a pair at d_safe or at 0: the counts may differ
    assert np.array_equal(nnear[~edge], rn[~edge]) and np.array_equal(nover[~edge], ro[~edge])
    return {"cost": float(np.abs(cost - rc).max()), "cost_grad": float(np.abs(grad - rg).max())}, {"edge": int(edge.sum()), "largest_grad": float(np.abs(rg).max())}


def test_signed_cost_against_the_formula_on_the_devices_own_distances(arm):
    fig, n = arm_figures(arm)
    WORST.update(fig)
    print(f"signed collision cost, {AB} x {AK} candidates: worst |cost - formula| {fig['cost']:.3e} (bound {BOUND['cost']:.1e}), gradient entry {fig['cost_grad']:.3e} "
          f"(bound {BOUND['cost_grad']:.1e}); {n}")
    assert fig["cost"] <= BOUND["cost"] and fig["cost_grad"] <= BOUND["cost_grad"]


def test_candidates_without_an_overlap_are_bit_for_bit_the_unsigned_call(arm):
    hb, c, q = arm["hb"], arm["c"], arm["q"]
    for d_safe, plain, signed in ((Q.ARM_D_SAFE, arm["plain"], arm["signed"]),) + tuple(
            (ds, hb.config_collision_cost(c["dofs"], q, pairs=c["pairs"], d_safe=ds, chunks=ch), hb.config_collision_cost(c["dofs"], q, pairs=c["pairs"], d_safe=ds, chunks=ch, signed=True))
            for ds, ch in ((0.04, 1), (0.04, 3), (0.04, 0))):
        free = (plain[3] == 0) & (signed[3] == 0)                                                # no pair with dist < 0, by either count
        assert int(free.sum()) >= AB * AK // 3 and (d_safe < 0.02 or bool((plain[2][free] > 0).any()))      # at 0.04 free candidates have near pairs
        assert all(torch.equal(x[free], y[free]) for x, y in zip(plain, signed))
        assert bool((signed[3] >= plain[3]).all())
    again = hb.config_collision_cost(c["dofs"], q, pairs=c["pairs"], d_safe=Q.ARM_D_SAFE, chunks=1, signed=True)
    assert all(torch.equal(x, y) for x, y in zip(arm["signed"], again))                          # a repeat call: bit-identical
    chunked = hb.config_collision_cost(c["dofs"], q, pairs=c["pairs"], d_safe=Q.ARM_D_SAFE, chunks=len(c["pairs"]), signed=True)
    assert torch.equal(chunked[2], again[2]) and torch.equal(chunked[3], again[3])
    # one pair per chunk: the same terms added in another order, a few ulp of the largest sum (a candidate through the floor costs 3e-2, far above the sunk ones)
    ulps = 4 * 2.0 ** -23
    assert float((chunked[0] - again[0]).abs().max()) <= ulps * float(again[0].max()) and float((chunked[1] - again[1]).abs().max()) <= ulps * float(again[1].abs().max())


def test_the_signed_gradient_leads_out_of_an_overlap(arm):
    c = arm["c"]
    flat, dofs, pairs = c["flat"], c["dofs"], c["pairs"]
    pc, pg, pn, po = (o.cpu().numpy() for o in arm["plain"])
    sc, sg, sn, so = (o.cpu().numpy() for o in arm["signed"])
    only = c["sunk"] & (pn == po) & (pn > 0)                                                     # every near pair overlaps: the unsigned cost is flat
    assert int(only.sum()) >= 30, int(only.sum())
    assert not pg[only].any() and np.allclose(pc[only], 0.5 * Q.ARM_D_SAFE ** 2 * pn[only], rtol=1e-6, atol=0)      # the constant 1/2 d_safe^2 per pair
    assert (np.abs(sg[only]).max(axis=1) > 0).all() and (sc[only] > pc[only]).all()
    params = S.params32(flat)
    eta = 1.0                                                                                     # |grad| ~ 5e-3 m^2 / rad: a step of some 5e-3 rad
    raised = []
    for e, k in np.argwhere(only)[::3]:
        def dmin(q):
            return clearance._pair_distances(flat, c["qpos"][e], dofs, q, pairs, 1.0, Q.REF["tol"], Q.REF["max_iters"], params, None, None, None, None, None, False, True)[1].min()
        raised.append(dmin(c["q"][e, k] - eta * sg[e, k].astype(np.float64)) - dmin(c["q"][e, k]))
    print(f"{only.sum()} overlap-only candidates; q - {eta} grad raises the smallest signed distance of {len(raised)} checked by {min(raised):.2e} .. {max(raised):.2e} m")
    assert min(raised) > 0


def test_collision_cost_signed_is_differentiable():
    from robosuite_amd.vec_env import VecEnv
    from tests import clearance_scenes as C
    from tests import test_clearance as TC

    s = TC._lift()
    env = VecEnv("Lift", 3, s["flat"], s["cfg"], horizon=50)
    env.reset()
    q = dev(C.candidates(s["flat"], s["dofs"], 3, 5)).requires_grad_(True)
    hb = env.env.batch
    env.config_collision_cost(q.detach(), 0.05)
    tables = (hb.config_tables(), hb.config_grad_tables())
    ref = env.config_collision_cost(q.detach(), 0.05, signed=True)
    assert (hb.config_tables(), hb.config_grad_tables()) == tables
    assert all(torch.equal(x, y) for x, y in zip(ref, hb.config_collision_cost(s["dofs"], q.detach(), d_safe=0.05, signed=True)))
    env.collision_cost(q, 0.05, signed=True).sum().backward()
    assert torch.equal(q.grad, ref[1]) and bool(q.grad.abs().sum() > 0)
