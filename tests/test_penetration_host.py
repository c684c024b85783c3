"""The fp64 mirror of the signed overlap distance (robosuite_amd/penetration.py) against closed forms, and against its own certificate on the random scene of
tests/penetration_scenes.py.  CPU only; the figures of a run are printed before they are asserted.

Closed forms: to 1e-9 m in depth and 1e-9 in every component of the normal, with the descent iterated to pen_tol = 1e-12.

Certificate of an overlap the mirror reports as (dist, p1, p2) with normal n, at the query's defaults (pen_tol 1e-7, offset 4e-3) on distance_scenes.REF:
  * | -dist - delta(n) | <= 1e-12 for a pair that descended: dist IS -delta(n), evaluated with the support functions; for a sphere or capsule whose core is
    apart from the other shape dist and both witnesses are GJK's, and every residual is within the reference's tol = 1e-10;
  * 0 <= h_A(n) - n . p1 <= GAP and -GAP <= h_B(-n) + n . p2 <= 0: the projection's witnesses lie within its gap tolerance pen_tol * offset = 4e-10 m of their
    supporting planes (GJK ends with h_C(n) - n . c <= gap, and both terms of that sum are >= 0); asserted with GAP = 1e-9;
  * | p2 - p1 - dist n | <= 1e-12 (by construction);
  * geom2 moved by (depth + 1e-6) n is disjoint from geom1 on distance.pair;
  * depth >= multistart_depth - 1e-6 (descents from all 162 icosphere directions; run on the first MS_ENVS envs, a third of a second per pair);
  * delta never rises along the iterates;
  * a pair distance.pair does not send to status 2 comes back exactly as distance.pair returns it;
  * at most 10 % of the overlapping pairs are in the band (penetration_scenes.in_band).

The signed collision cost's gradient against central differences of the signed cost itself, on the sunk candidates of penetration_scenes.arm_cases (a capsule in
a box: one face of the Minkowski difference, smooth in q while the face stays): h = 1e-5 rad, descent iterated to pen_tol = 1e-12.  Bound 1e-5 per entry: the
mirror showed 7.5e-11 at gradients up to 7e-3; the margin is for the truncation error h^2 |c'''| / 6 at other draws, as in tests/test_clearance_grad_host.py,
whose cost bound this is."""
import numpy as np
import pytest

from robosuite_amd import clearance
from robosuite_amd import distance as D
from robosuite_amd import penetration as P
from tests import distance_scenes as S
from tests import penetration_scenes as Q

B = 24
MS_ENVS = 2
GAP = 1e-9
H = 1e-5
COST_BOUND = 1e-5


def test_closed_forms():
    for name, a, b, depth, n in Q.closed_forms():
        info = {}
        d, ft, st = P.pair_signed(a, b, 1.0, 1e-12, 1000, pen_tol=1e-12, pen_iters=64, info=info)
        res = Q.certificate(a, b, d, ft, info["normal"])
        print(f"{name}: depth error {d + depth:.2e}, normal error {np.abs(np.array(info['normal']) - n).max():.2e}, {info['steps']} projections, residuals {res}")
        assert D.pair(a, b, 1.0, 1e-12, 1000)[2] == D.OVERLAP and st == D.OK
        assert abs(d + depth) <= 1e-9 and np.abs(np.array(info["normal"]) - n).max() <= 1e-9, name
        assert max(abs(r) for r in res) <= 1e-9, (name, res)
        assert abs(P.support_width(a, b, n) - depth) <= 1e-12
        assert abs(P.multistart_depth(a, b, keep=12)[0] - depth) <= 1e-9, name      # no direction of the screen finds less


def test_options_are_refused_by_name():
    assert P.options() == P.DEFAULTS and P.options({"offset": 1e-3})["offset"] == 1e-3
    for bad in ({"pen_iters": 0}, {"pen_iters": P.PEN_ITERS_LIMIT + 1}, {"offset": 0.0}, {"pen_tol": -1.0}, {"rho": 1.0}):
        with pytest.raises(P.PenetrationError):
            P.options(bad)


SEEN = {}


@pytest.fixture(scope="module", params=("P", "P2"))
def scene(request, tmp_path_factory):
    flat = Q.scene_p(tmp_path_factory.mktemp("pen_host"), request.param)
    q = Q.scene_p_qpos(flat, B, Q.SEEDS[request.param])
    poses = [S.body_poses(flat, q[e]) for e in range(B)]
    xp, xq = S.f32(np.stack([p[0] for p in poses])), S.f32(np.stack([p[1] for p in poses]))
    pairs = Q.all_pairs(flat)
    return flat, pairs, Q.reference(flat, xp, xq, pairs, Q.DISTMAX)


def test_every_type_combination_overlaps_somewhere(scene):
    flat, pairs, ref = scene
    over = (ref["plain"] & D.OVERLAP) != 0
    gt = np.asarray(flat.arrays["geom_type"]).ravel()
    seen = {tuple(sorted((int(gt[a]), int(gt[b])))) for (a, b), o in zip(pairs, over.any(axis=0)) if o}
    hard, rnd = (4, 5, 6, 7), (2, 3)
    cast = {tuple(sorted((int(gt[a]), int(gt[b])))) for a, b in pairs}                         # what this cast of eight can pose
    want = ({tuple(sorted((a, b))) for a in hard for b in hard} | {tuple(sorted((a, b))) for a in rnd for b in hard})
    SEEN[len(SEEN)] = seen
    print(f"{over.sum()} overlapping pairs of {over.size}; type combinations seen: {len(seen)} of the {len(want & cast)} this cast can pose")
    assert seen == want & cast, (want & cast) - seen
    if len(SEEN) == 2:                                                                           # the two casts together: every combination that goes to status 2
        assert SEEN[0] | SEEN[1] == want, want - (SEEN[0] | SEEN[1])
    assert not (ref["status"] & (D.OVERLAP | D.CAP | P.PEN_CAP)).any()
    assert (ref["dist"][over] < 0).all()


def test_the_band_is_small(scene):
    flat, pairs, ref = scene
    over = (ref["plain"] & D.OVERLAP) != 0
    print(f"band: {ref['band'].sum()} of {over.sum()} overlapping pairs; projections mean {ref['steps'][over].mean():.2f} worst {ref['steps'].max()}")
    assert ref["band"][over].mean() <= Q.BAND_SHARE


def test_certificate_on_the_random_scene(scene):
    flat, pairs, ref = scene
    dist, ft, nrm, plain = (ref[k].reshape((-1,) + ref[k].shape[2:]) for k in ("dist", "fromto", "normal", "plain"))
    worst = np.zeros(4)
    n_over = 0
    for i, (a, b) in enumerate(ref["recs"]):
        if not plain[i] & D.OVERLAP:
            assert (dist[i], tuple(ft[i]), int(ref["status"].ravel()[i])) == D.pair(a, b, Q.DISTMAX, **Q.REF)      # untouched, exactly
            continue
        n_over += 1
        res = Q.certificate(a, b, dist[i], ft[i], nrm[i])
        worst = np.maximum(worst, np.abs(res))
        if ref["steps"].ravel()[i] > 0:
            assert res[0] <= 1e-12 and -1e-12 <= res[1] <= GAP and -GAP <= res[2] <= 1e-12 and res[3] <= 1e-12, (i, res)
        else:                                              # the cores are apart: GJK's own witnesses and upper bound, each within its tol
            assert max(abs(r) for r in res) <= Q.REF["tol"], (i, res)
        assert Q.separates(a, b, dist[i], nrm[i]), i
        info = {}
        P.pair_signed(a, b, Q.DISTMAX, **Q.REF, info=info)
        assert all(y <= x for x, y in zip(info["trace"], info["trace"][1:])), (i, info["trace"])
    print(f"{n_over} overlapping pairs: worst residuals |-dist - delta| {worst[0]:.2e}, h_A - n.p1 {worst[1]:.2e}, h_B + n.p2 {worst[2]:.2e}, "
          f"|p2 - p1 - dist n| {worst[3]:.2e}")


def test_depth_is_never_below_the_multistart_minimum(scene):
    flat, pairs, ref = scene
    npair = len(pairs)
    local = n = 0
    for i in range(MS_ENVS * npair):
        if not ref["plain"].ravel()[i] & D.OVERLAP:
            continue
        depth, ms = -ref["dist"].ravel()[i], P.multistart_depth(*ref["recs"][i])[0]
        n += 1
        local += depth > ms + 1e-5
        assert depth >= ms - 1e-6, (i, depth, ms)
    print(f"{n} pairs against the multistart minimum: {local} at a larger, local minimum")
    assert n >= 10


def test_signed_cost_gradient_against_central_differences():
    c = Q.arm_cases(3, 70)
    flat, dofs, pairs = c["flat"], c["dofs"], c["pairs"]
    kw = dict(pairs=pairs, d_safe=Q.ARM_D_SAFE, params=S.params32(flat), check_options=False, **S.REF, signed=True, pen={"pen_tol": 1e-12, "pen_iters": 64})
    worst = gmax = 0.0
    compared = 0
    for e in range(3):
        for k in range(1, 70, 6):
            assert c["sunk"][e, k]
            q = c["q"][e, k]
            cost, g, nnear, nover = clearance.collision_cost(flat, c["qpos"][e], dofs, q, **kw)
            plain = clearance.collision_cost(flat, c["qpos"][e], dofs, q, **dict(kw, signed=False, pen=None))
            assert nover >= 1 and cost > 0.5 * Q.ARM_D_SAFE ** 2 and np.abs(g).max() > 0
            if plain[2] == plain[3]:                       # every near pair overlaps: the unsigned cost is flat here
                assert not plain[1].any()
            fd, same = np.zeros(len(dofs)), True
            for col in range(len(dofs)):
                qp, qm = q.copy(), q.copy()
                qp[col] += H
                qm[col] -= H
                cp, cm = (clearance.collision_cost(flat, c["qpos"][e], dofs, x, **kw) for x in (qp, qm))
                same = same and cp[2:] == (nnear, nover) and cm[2:] == (nnear, nover)
                fd[col] = (cp[0] - cm[0]) / (2 * H)
            if not same:
                continue
            compared += 1
            worst, gmax = max(worst, np.abs(g - fd).max()), max(gmax, np.abs(g).max())
    print(f"signed cost: {compared} candidates compared, worst |analytic - FD| {worst:.2e} (bound {COST_BOUND:.0e}), largest gradient entry {gmax:.2e}")
    assert compared >= 20 and worst <= COST_BOUND
