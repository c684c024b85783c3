"""The fp64 mirror of collision-aware IK (robosuite_amd/ik_avoid.py), alone on the CPU: what the device tests (tests/test_ik_avoid.py) hold the kernels to.

  * with avoid_gain = 0 and cost_tol = inf the mirror IS ik.solve: every output equal, exactly;
  * the finish rule: a finished problem has converged, cost <= cost_tol, no overlapping pair, and clearance.clearance(q) >= d_safe / 2 over the list;
  * a finished problem is frozen: more iterations return the same q after the same number of updates, and a solve started at it makes no update;
  * scene A: plain IK's answers stand inside the sphere, and at most 40 % of the cases are left out of what the device is held to;
  * the refusals, by their words."""
import numpy as np
import pytest

from robosuite_amd import clearance, ik, ik_avoid
from tests import ik_avoid_scenes as A
from tests import ik_scenes

B, K = 4, 6


@pytest.fixture(scope="module")
def solved():
    c = A.cases(B, K)
    return c, [[A.solve_case(c, e, k) for k in range(K)] for e in range(B)]


@pytest.mark.parametrize("name", ("chain3", "sceneA"))
def test_without_gain_and_cost_the_mirror_is_plain_ik(name):
    if name == "sceneA":
        a, c = A.scene_a(), A.cases(B, K)
        flat, site, dofs, pairs = a["flat"], a["site"], a["dofs"], a["pairs"]
        probs = [(c["qpos"][e], c["pos"][e, k], c["q_init"][e, k]) for e in range(2) for k in range(3)]
    else:
        s = ik_scenes.scene(name)
        flat, site, dofs = s["flat"], s["site"], s["dofs"]
        pairs = np.array([[0, 1], [0, 3]], dtype=np.int32)      # the floor against two links: the model's own collision list is empty
        cs = ik_scenes.cases(flat, site, dofs, 6, seed=11, quat=False)
        probs = [(np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel(), cs["pos"][i], cs["q_init"][i]) for i in range(6)]
    for posture in (0.0, 0.1):
        for qpos, pos, qi in probs:
            want = ik.solve(flat, qpos, site, dofs, pos, None, qi, max_iters=30, posture_gain=posture)
            got = ik_avoid.solve(flat, qpos, site, dofs, pos, None, qi, pairs, avoid_gain=0.0, cost_tol=np.inf, max_iters=30, posture_gain=posture)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2] and got[3] == want[3] == got[4]


def test_the_finish_rule_proves_half_of_d_safe(solved):
    c, r = solved
    a = A.scene_a()
    tol = ik_avoid.options(**A.OPTS)["cost_tol"]
    assert tol == 0.5 * (0.5 * A.D_SAFE) ** 2
    nfin = 0
    for e in range(B):
        for k in range(K):
            q, err, it, conv, fin, cost, nnear, nover = r[e][k]
            assert fin == (conv and cost <= tol)
            if fin:
                nfin += 1
                assert err[0] < ik.DEFAULTS["pos_tol"] and nover == 0 and it <= A.MAX_ITERS
                assert clearance.clearance(a["flat"], c["qpos"][e], a["dofs"], q, a["pairs"])[0] >= 0.5 * A.D_SAFE
            else:
                assert it == A.MAX_ITERS
    assert nfin >= 12


def test_a_finished_problem_is_frozen(solved):
    c, r = solved
    seen = 0
    for e in range(B):
        for k in range(K):
            if not r[e][k][4] or seen >= 6:
                continue
            seen += 1
            more = A.solve_case(c, e, k, max_iters=A.MAX_ITERS + 20)
            assert np.array_equal(more[0], r[e][k][0]) and more[2:] == r[e][k][2:]
            again = A.solve_case(dict(c, q_init=np.tile(r[e][k][0], (B, K, 1))), e, k)
            assert again[2] == 0 and again[4] and np.array_equal(again[0], r[e][k][0])
    assert seen == 6


def test_scene_a_cases_and_the_cap():
    c = A.cases(B, K)
    d = A.plain_clearance(c)
    print(f"scene A, the mirror alone: plain IK's clearance {d.min():.4f} .. {d.max():.4f}; {len(A.scene_a()['pairs'])} pairs")
    assert (d <= -A.HIT_MIN).all()      # every plain answer stands inside the sphere
    held = A.held(B, K)
    print(f"scene A: {int((~held).sum())} of {held.size} cases left out")
    assert (~held).sum() <= A.CAP * held.size


def test_refusals():
    a, c = A.scene_a(), A.cases(B, K)
    flat, site, dofs = a["flat"], a["site"], a["dofs"]
    call = lambda dofs=dofs, **o: ik_avoid.solve(flat, c["qpos"][0], site, dofs, c["pos"][0, 0], None, c["q_init"][0, 0], a["pairs"], **o)      # noqa: E731
    for o, text in ((dict(avoid_gain=-1.0), "avoid_gain -1.0 is not >= 0"), (dict(cost_tol=-1.0), "cost_tol -1.0 is not >= 0"), (dict(check_every=-1), "check_every -1 is not >= 0"),
                    (dict(d_safe=0.0), "d_safe 0.0 is not > 0"), (dict(max_dq=0.0), "IK options out of range")):
        with pytest.raises(ValueError, match=text):
            call(**o)
    with pytest.raises(TypeError, match="unknown IK option"):
        call(bogus=1)
    ball = int(np.asarray(flat.arrays["jnt_dofadr"]).ravel()[flat.names["joint"].index("ballj")])
    with pytest.raises(ValueError, match=f"controlled dof {ball} is not a hinge or slide joint on the path to site {site}"):
        ik_avoid.solve(flat, c["qpos"][0], site, [0, 1, ball], c["pos"][0, 0], None, None, a["pairs"])
    assert ik_avoid.options(cost_tol=np.inf)["cost_tol"] == np.inf and ik_avoid.DEFAULTS["avoid_gain"] == ik_avoid.AVOID_GAIN
