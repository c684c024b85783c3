"""The fp64 mirrors of the signed queries -- clearance.clearance / clearance_grad and ik_avoid.solve / update / held_to with signed=True -- on the CPU.

  * signed=False is what a call without the argument returns, bit for bit, on clearance_scenes' scene T and on scene A;
  * on penetration_scenes.arm_cases(3, 70): a sunk candidate reports its deepest pair, dist in [-5e-3, -2e-3] m, no OVERLAP bit, pair = the argmin of the signed
    per-pair values; a candidate with no overlap equals the unsigned result exactly; the signed gradient is within 1.2e-5 of central differences (h = 1e-5) of
    the signed distance -- the figure tests/test_clearance_grad_host.py saw for the unsigned mirror -- on the sunk candidates whose two smallest pairs lie
    further apart than the stencil can move them: a pair's distance is 1-Lipschitz in the witness motion, a joint step h moves a point of this 1 m arm by at
    most h x 1 m, so two pairs GAP = 1e-4 m apart (ten times 2 h x 1 m) keep their order inside the stencil;
  * on the sunk starts of tests/signed_query_scenes.py the mirror finishes all but CAP of the cases, and where the unsigned cost has nnear == noverlap > 0 the
    unsigned solver does not move and does not finish -- the gap the signed call closes."""
import numpy as np
import pytest

from robosuite_amd import clearance, distance, ik_avoid
from tests import clearance_scenes as S
from tests import ik_avoid_scenes as IA
from tests import penetration_scenes as Q
from tests import signed_query_scenes as SQ

H, GAP, FD_BOUND = 1e-5, 1e-4, 1.2e-5
B, K = 3, 70


def same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.fixture(scope="module")
def arm():
    c = Q.arm_cases(B, K)
    return dict(c, params=S.params32(c["flat"]))


def test_unsigned_results_are_unchanged_scene_t(tmp_path):
    flat = S.scene_t(tmp_path)
    qpos, dofs = S.f32(S.scene_t_qpos(flat, 2)), S.dofs_t(flat, "arm")
    q = S.candidates(flat, dofs, 2, 5)
    kw = dict(distmax=S.DISTMAX_T, params=S.params32(flat))
    for e in range(2):
        for k in range(5):
            assert same(clearance.clearance(flat, qpos[e], dofs, q[e, k], **kw), clearance.clearance(flat, qpos[e], dofs, q[e, k], signed=False, pen=None, **kw))
            assert same(clearance.clearance_grad(flat, qpos[e], dofs, q[e, k], **kw), clearance.clearance_grad(flat, qpos[e], dofs, q[e, k], signed=False, pen=None, **kw))


def test_unsigned_results_are_unchanged_scene_a():
    a, c = IA.scene_a(), IA.cases(2, 2)
    for e in range(2):
        for k in range(2):
            args = (a["flat"], c["qpos"][e], a["site"], a["dofs"], c["pos"][e, k], None, c["q_init"][e, k], a["pairs"])
            assert same(ik_avoid.solve(*args, **IA.OPTS), ik_avoid.solve(*args, signed=False, pen=None, **IA.OPTS))
            q = c["q_init"][e, k]
            assert same(clearance.clearance(a["flat"], c["qpos"][e], a["dofs"], q, a["pairs"]), clearance.clearance(a["flat"], c["qpos"][e], a["dofs"], q, a["pairs"], signed=False))
            assert same(clearance.clearance_grad(a["flat"], c["qpos"][e], a["dofs"], q, a["pairs"]),
                        clearance.clearance_grad(a["flat"], c["qpos"][e], a["dofs"], q, a["pairs"], signed=False))


def test_sunk_candidates_report_their_deepest_pair(arm):
    flat, dofs, pairs = arm["flat"], arm["dofs"], arm["pairs"]
    two = 0
    for e in range(B):
        for k in np.flatnonzero(arm["sunk"][e]):
            d, pr, ft, st = clearance.clearance(flat, arm["qpos"][e], dofs, arm["q"][e, k], pairs, params=arm["params"], signed=True, **Q.REF)
            per = SQ.smallest(flat, arm["qpos"][e], dofs, arm["q"][e, k], pairs, arm["params"])[1]
            assert -5e-3 <= d <= -2e-3 and not st & distance.OVERLAP, (e, k, d, st)
            assert pr == int(np.argmin(per)) and d == per[pr], (e, k, pr)
            n = (ft[3:] - ft[:3]) / d
            assert abs(np.linalg.norm(n) - 1) <= 1e-9      # the witnesses carry the direction the gradient reads
            two += (per < 0).sum() > 1
    print(f"{arm['sunk'].sum()} sunk candidates, {two} with more than one pair below zero")


def test_a_candidate_without_overlap_is_the_unsigned_result(arm):
    flat, dofs, pairs = arm["flat"], arm["dofs"], arm["pairs"]
    for e in range(B):
        for k in np.flatnonzero(~arm["sunk"][e])[:12]:
            kw = dict(pairs=pairs, params=arm["params"])
            u = clearance.clearance_grad(flat, arm["qpos"][e], dofs, arm["q"][e, k], **kw)
            assert not u[3] & distance.OVERLAP
            assert same(u, clearance.clearance_grad(flat, arm["qpos"][e], dofs, arm["q"][e, k], signed=True, **kw))
            assert same(u[:4], clearance.clearance(flat, arm["qpos"][e], dofs, arm["q"][e, k], signed=True, **kw))


def test_signed_gradient_against_central_differences(arm):
    flat, dofs, pairs = arm["flat"], arm["dofs"], arm["pairs"]
    kw = dict(pairs=pairs, params=arm["params"], signed=True, check_options=False, **Q.REF)
    worst, compared, close = 0.0, 0, 0
    for e in range(B):
        for k in np.flatnonzero(arm["sunk"][e]):
            q = arm["q"][e, k]
            per = np.sort(SQ.smallest(flat, arm["qpos"][e], dofs, q, pairs, arm["params"])[1])
            if per[1] - per[0] <= GAP:
                close += 1
                continue
            d, pr, _, st, g = clearance.clearance_grad(flat, arm["qpos"][e], dofs, q, **kw)
            assert d < 0 and g.any()
            fd = np.zeros(len(dofs))
            for c in range(len(dofs)):
                qp, qm = q.copy(), q.copy()
                qp[c] += H
                qm[c] -= H
                rp, rm = (clearance.clearance_grad(flat, arm["qpos"][e], dofs, x, **kw) for x in (qp, qm))
                assert rp[1] == pr and rm[1] == pr
                fd[c] = (rp[0] - rm[0]) / (2 * H)
            compared += 1
            worst = max(worst, np.abs(g - fd).max())
    print(f"signed gradient: {compared} compared, {close} left out (two smallest pairs within {GAP:.0e} m); worst |analytic - FD| {worst:.2e} (bound {FD_BOUND:.1e})")
    assert compared >= 50
    assert worst <= FD_BOUND


def test_sunk_starts_held_share_and_the_unsigned_solver_stands_still():
    c = SQ.cases()
    held, stuck = SQ.held(c), SQ.stuck(c)
    print(f"sunk starts: {held.sum()} of {held.size} held ({held[0::2].sum()} of {held[0::2].size} into b3, {held[1::2].sum()} of {held[1::2].size} into c2); "
          f"{stuck.sum()} starts with unsigned nnear == noverlap > 0; {(c['nneg'] > 1).sum()} with two pairs below zero")
    assert (~held).sum() <= SQ.CAP * held.size
    assert stuck.sum() >= held.size // 2      # the recipe produces the situation it is meant to
    for e, k in zip(*np.nonzero(stuck)):
        q, _, it, _, fin = SQ.solve_case(c, e, k, signed=False)[:5]
        assert not fin and it == SQ.MAX_ITERS and np.abs(q - c["q_init"][e, k]).max() <= 1e-6, (e, k)
    moved = [np.abs(SQ.solve_case(c, e, k)[0] - c["q_init"][e, k]).max() for e, k in zip(*np.nonzero(stuck & held))]
    assert min(moved) > 1e-4      # ... and the signed solver leaves every one of them
