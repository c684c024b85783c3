"""The fp64 mirror of the clearance gradient and the collision cost (robosuite_amd/clearance.py clearance_grad / collision_cost) against central differences
of the mirror's own distance, iterated with distance_scenes.REF (fp64, bounds agreeing to 1e-10 m): h = 1e-5, scene T, both dof lists, the default pair list,
clearance_scenes' seeded draws at (B, K) = (5, 13).  CPU only.

Bounds (set by the issue this file came with).  Gradient: 1e-4 per entry over the candidates with status 0 whose +-h stencil keeps the same pair (seen: 1.1e-5
/ 1.4e-5; the margin is for the truncation error h^2 |d'''| / 6 at other draws); at least 20 compared per dof list, at most 10 % of the defined ones left out
for a pair switch.  Cost: d_safe = 0.08, 1e-5 per entry (seen 7.7e-7 / 1.4e-6); only candidates whose noverlap changes inside the stencil are left out; at
least 20 compared, at least 10 of them with nnear > 1.  The figures of this run are printed before they are asserted."""
import numpy as np
import pytest

from robosuite_amd import clearance, distance, mjcf
from tests import attach_scenes as A
from tests import clearance_scenes as S
from tests import distance_scenes as D

H = 1e-5
B, K = 5, 13
D_SAFE = 0.08
GRAD_BOUND, COST_BOUND = 1e-4, 1e-5
REF = dict(check_options=False, **D.REF)


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    flat = S.scene_t(tmp_path_factory.mktemp("grad_host"))
    return dict(flat=flat, qpos=S.f32(S.scene_t_qpos(flat, B)), m32=clearance._model32(flat), params=S.params32(flat))


def _stencil(q, c):
    qp, qm = q.copy(), q.copy()
    qp[c] += H
    qm[c] -= H
    return qp, qm


@pytest.mark.parametrize("which", ("arm", "all"))
def test_gradient_against_central_differences(scene, which):
    flat, qpos = scene["flat"], scene["qpos"]
    dofs = S.dofs_t(flat, which)
    pairs = clearance.default_pairs(flat, dofs)
    q = S.candidates(flat, dofs, B, K)
    kw = dict(pairs=pairs, distmax=S.DISTMAX_T, params=scene["params"], **REF)
    defined = far = overlap = compared = switched = 0
    worst = 0.0
    for e in range(B):
        for k in range(K):
            d, pr, _, st, g = clearance.clearance_grad(flat, qpos[e], dofs, q[e, k], **kw)
            far += pr < 0
            overlap += pr >= 0 and st == distance.OVERLAP
            if pr < 0 or st != distance.OK:
                assert not g.any()      # the zero rules
                continue
            defined += 1
            fd, same = np.zeros(len(dofs)), True
            for c in range(len(dofs)):
                (dp, pp, _, sp), (dm, pm, _, sm) = (clearance.clearance_grad(flat, qpos[e], dofs, x, **kw)[:4] for x in _stencil(q[e, k], c))
                same = same and pp == pr and pm == pr and sp == distance.OK and sm == distance.OK
                fd[c] = (dp - dm) / (2 * H)
            if not same:
                switched += 1
                continue
            compared += 1
            worst = max(worst, np.abs(g - fd).max())
    print(f"dofs {which}: {defined} defined, {far} far, {overlap} overlap; {compared} compared, {switched} switched pair in the stencil; "
          f"worst |analytic - FD| {worst:.2e} (bound {GRAD_BOUND:.0e})")
    assert compared >= 20 and switched <= 0.1 * defined
    assert worst <= GRAD_BOUND


@pytest.mark.parametrize("which", ("arm", "all"))
def test_cost_against_central_differences(scene, which):
    flat, qpos = scene["flat"], scene["qpos"]
    dofs = S.dofs_t(flat, which)
    pairs = clearance.default_pairs(flat, dofs)
    q = S.candidates(flat, dofs, B, K)
    kw = dict(pairs=pairs, d_safe=D_SAFE, params=scene["params"], **REF)
    compared = several = excluded = 0
    worst = gmax = 0.0
    for e in range(B):
        for k in range(K):
            cost, g, nnear, nover = clearance.collision_cost(flat, qpos[e], dofs, q[e, k], **kw)
            if nnear == 0:
                assert cost == 0 and not g.any()
            fd, same = np.zeros(len(dofs)), True
            for c in range(len(dofs)):
                (cp, _, _, op), (cm, _, _, om) = (clearance.collision_cost(flat, qpos[e], dofs, x, **kw) for x in _stencil(q[e, k], c))
                same = same and op == nover and om == nover
                fd[c] = (cp - cm) / (2 * H)
            if not same:
                excluded += 1
                continue
            compared += 1
            several += nnear > 1
            worst, gmax = max(worst, np.abs(g - fd).max()), max(gmax, np.abs(g).max())
    print(f"dofs {which}, d_safe {D_SAFE}, {len(pairs)} pairs: {compared} compared, {several} with several near pairs, {excluded} excluded; "
          f"worst |analytic - FD| {worst:.2e} (bound {COST_BOUND:.0e}); gradient entries up to {gmax:.1e}")
    assert compared >= 20 and several >= 10
    assert worst <= COST_BOUND


def test_zero_rules(scene):
    """far: nothing closer than distmax; overlap: status 2; band: |dist| < GRAD_MIN_DIST -- each gives an all-zero gradient"""
    flat, qpos = scene["flat"], scene["qpos"]
    dofs = S.dofs_t(flat, "arm")
    q = S.candidates(flat, dofs, B, K)
    seen = set()
    for e in range(B):
        for k in range(K):
            d, pr, ft, st, g = clearance.clearance_grad(flat, qpos[e], dofs, q[e, k], distmax=S.DISTMAX_T, params=scene["params"])
            kind = "far" if pr < 0 else "overlap" if st & distance.OVERLAP else "defined"
            seen.add(kind)
            if kind == "far":
                assert d == S.DISTMAX_T and not ft.any() and not g.any()
            elif kind == "overlap":
                assert d == 0 and not g.any()
                cost, cg, nnear, nover = clearance.collision_cost(flat, qpos[e], dofs, q[e, k], pairs=clearance.default_pairs(flat, dofs)[pr:pr + 1], d_safe=D_SAFE,
                                                                  params=scene["params"])
                assert (cost, nnear, nover) == (0.5 * D_SAFE ** 2, 1, 1) and not cg.any()      # an overlapping pair: 1/2 d_safe^2, counted, no gradient
            else:
                assert g.any()
    assert seen == {"far", "overlap", "defined"}
    # the band: two spheres whose surfaces are 5e-8 m apart have a direction in fp64, and still no gradient
    assert not clearance._has_dir(5e-8, distance.OK) and not clearance._has_dir(-5e-8, distance.OK) and clearance._has_dir(-2e-7, distance.OK)
    fr = (np.array([[0.0, 0, 1]]), np.zeros((1, 3)), np.array([False]))
    assert clearance.pair_grad(fr, 0, 1, [1.0, 0, 0], [1.0, 0.5, 0], 0.5)[0] == pytest.approx(1.0)      # a hinge about z at the origin moves p2 by (-0.5, 1, 0): away from p1
    with pytest.raises(clearance.ClearanceError, match="d_safe"):
        clearance.collision_cost(flat, qpos[0], dofs, q[0, 0], d_safe=0.0)


def test_equal_signature_pair_gives_zero(scene):
    """an explicit list may hold a pair whose two bodies share a signature (two geoms of l2's subtree, finger against l2's cylinder): the terms cancel"""
    flat, qpos = scene["flat"], scene["qpos"]
    dofs = S.dofs_t(flat, "arm")
    g = flat.names["geom"].index
    pairs = np.array([[g("g_cyl"), g("g_f2")], [g("g_ell"), g("g_f1")]], dtype=np.int32)
    sig, gb = clearance.signatures(flat, dofs), clearance._I(flat, "geom_bodyid")
    assert all(sig[gb[a]] == sig[gb[b]] != 0 for a, b in pairs)
    q = S.candidates(flat, dofs, B, K)
    n = 0
    for e in range(B):
        for k in range(0, K, 4):
            d, pr, _, st, grad = clearance.clearance_grad(flat, qpos[e], dofs, q[e, k], pairs=pairs, distmax=1.0, params=scene["params"])
            assert pr >= 0
            n += st == distance.OK
            assert np.abs(grad).max() <= 1e-12
            assert np.abs(clearance.collision_cost(flat, qpos[e], dofs, q[e, k], pairs=pairs, d_safe=1.0, params=scene["params"])[1]).max() <= 1e-12
    assert n > 0


def test_attachment_uses_the_carriers_signature(scene):
    """scene T with the free sphere on l2 and the free box on the side link: a held body's gradient is the carrier's; an env that holds nothing is the plain one"""
    flat, qpos = scene["flat"], scene["qpos"]
    dofs = S.dofs_t(flat, "all")
    att, rel = A.attach_t(flat), A.rel_given(B)
    g = flat.names["geom"].index
    pairs = np.array([[g("fsph"), g("floor")], [g("fbox"), g("wbox")]], dtype=np.int32)      # each carried body against a static geom: explicit
    q = S.candidates(flat, dofs, B, K)
    for e in range(B):
        for k in (0, 5):
            kw = dict(pairs=pairs, distmax=5.0, params=scene["params"])
            plain = clearance.clearance_grad(flat, qpos[e], dofs, q[e, k], **kw)
            none = clearance.clearance_grad(flat, qpos[e], dofs, q[e, k], attach=att, held=[False, False], rel=rel[e], **kw)
            assert plain[:2] == none[:2] and np.array_equal(plain[4], none[4]) and not plain[4].any()      # free bodies against static geoms: no dof moves them
            both = clearance.clearance_grad(flat, qpos[e], dofs, q[e, k], attach=att, held=[True, True], rel=rel[e], **kw)
            if both[3] != distance.OK:
                continue
            carrier = att[both[1]][1]
            sig = clearance.signatures(flat, dofs)
            assert clearance.signatures(flat, dofs, att, [True, True])[att[both[1]][0]] == sig[carrier] != 0
            assert both[4].any() and not both[4][[c for c in range(len(dofs)) if not (sig[carrier] >> c) & 1]].any()
            # ... and it is the derivative: central differences with the grasp fixed
            for c in range(len(dofs)):
                dp, dm = (clearance.clearance(flat, qpos[e], dofs, x, pairs[both[1]:both[1] + 1], 5.0, params=scene["params"], attach=att, held=[True, True], rel=rel[e],
                                              tol=1e-10)[0] for x in _stencil(q[e, k], c))
                assert abs((dp - dm) / (2 * H) - both[4][c]) <= GRAD_BOUND, (e, k, c)


CHAIN_N = 16      # RSIM_JNT_MAX


def chain_xml(n=CHAIN_N):
    """a chain of n hinges with alternating axes, a capsule on every link, over a floor and beside a box"""
    body = ""
    for i in reversed(range(n)):
        axis = ("0 1 0.2", "0.3 0 1", "1 0.1 0")[i % 3]
        body = (f'<body name="c{i}" pos="{0.0 if i == 0 else 0.11} 0 {0.5 if i == 0 else 0.01}"><joint name="cj{i}" type="hinge" axis="{axis}" pos="0.01 0 0" '
                f'limited="true" range="-0.5 0.5"/><geom name="cg{i}" type="capsule" size="0.02 0.04" pos="0.055 0 0" euler="0 1.5708 0"/>{body}</body>')
    return f"""<mujoco><compiler angle="radian"/><worldbody><geom name="floor" type="plane" size="3 3 0.1"/>
      <geom name="post" type="box" size="0.05 0.05 0.4" pos="0.9 0.15 0.4"/>{body}</worldbody></mujoco>"""


def chain_pairs(flat, n=CHAIN_N):
    g = flat.names["geom"].index
    return np.array([[g(f"cg{i}"), g(s)] for i in range(n) for s in ("floor", "post")], dtype=np.int32)


@pytest.mark.parametrize("ndof", (CHAIN_N, 1))
def test_chain_of_sixteen_hinges_and_one_dof(ndof):
    flat = mjcf.compile_mjcf(chain_xml())
    dofs = S.dofs_of(flat, [f"cj{i}" for i in range(CHAIN_N)])[:ndof] if ndof > 1 else S.dofs_of(flat, ["cj7"])
    pairs = chain_pairs(flat)
    qpos = S.f32(np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel())
    q = S.candidates(flat, dofs, 1, 6)[0]
    compared, worst = 0, 0.0
    for k in range(len(q)):
        d, pr, _, st, g = clearance.clearance_grad(flat, qpos, dofs, q[k], pairs=pairs, distmax=5.0, **REF)
        assert g.shape == (ndof,)
        if st != distance.OK:
            continue
        fd = np.zeros(ndof)
        same = True
        for c in range(ndof):
            (dp, pp, _, sp), (dm, pm, _, sm) = (clearance.clearance_grad(flat, qpos, dofs, x, pairs=pairs, distmax=5.0, **REF)[:4] for x in _stencil(q[k], c))
            same = same and pp == pr == pm and sp == sm == distance.OK
            fd[c] = (dp - dm) / (2 * H)
        if same:
            compared += 1
            worst = max(worst, np.abs(g - fd).max())
        cost, cg, nnear, _ = clearance.collision_cost(flat, qpos, dofs, q[k], pairs=pairs, d_safe=0.6, **REF)
        assert nnear >= 1 and cg.shape == (ndof,)
    print(f"{ndof}-dof chain: {compared} compared, worst |analytic - FD| {worst:.2e}")
    assert compared >= 3 and worst <= GRAD_BOUND
