"""The kernel's narrow phase (csrc/rsim_step.hip: plane-box, plane-convex, box-box manifold, MPR) held to fp64 geometry at constructed depths: the samples of
tests/test_contact_certificates_host.py -- 36 pair classes x {1 mm deep, 0.1 mm deep, 0.1 mm apart} x 8 seeded draws -- as ONE batch of 864 envs and one forward().
The reference is the fp64 geometry of tests/contact_scenes.py (certificates C1 - C7 there) on the device's own xpos / xquat with the model's geometry rounded to
fp32 as the device holds it; never the oracle.  Contacts are read through the RSIM_CONTACT records (HipBatch.get("contact") / contacts()).

Allowances: four times the worst residual ONE GPU run measured per certificate (MEASURED; profiles/contact_certificates.txt -- the margin is for one box, one run
and pose-dependent rounding), not below FLOOR = 4 x 2^-23 x 1.5 m, the rounding of coordinates up to 1.5 m (the plane rows sit 1.2 m below the origin).  As on the
oracle the depth of a curved MPR pair is one-sided against the exact one (C5lo / C5hi tight, C5da / C5db wide: contact_scenes docstring)."""
import numpy as np
import pytest

from tests import contact_scenes as CS
from tests import distance_scenes as S
from tests.util import make_hip

pytestmark = pytest.mark.gpu

# worst residual per certificate of one GPU run on these samples (metres; <= 0: slack)
MEASURED = {"C3": 4.212e-5, "C4": 8.093e-8, "C4hi": 5.390e-9, "C4n": 0.0, "C5da": 4.269e-4, "C5db": 3.056e-5, "C5lo": -1.132e-7, "C5hi": 8.098e-8, "C5n": 5.353e-8,
            "C5p": 1.138e-7, "C6": -8.081e-6}
FLOOR = 4 * 2.0 ** -23 * 1.5
EPS = CS.tolerances(MEASURED, FLOOR)


def device_contacts(hb):
    """(contacts per env as HipBatch.contacts() returns them, overflow counters), from one read of the RSIM_CONTACT records"""
    ncon, rec, ovf = hb.get("ncon"), hb.get("contact"), hb.get("overflow")
    out = []
    for e in range(len(ncon)):
        out.append([dict(dist=float(r[0]), pos=r[1:4].astype(np.float64), frame=r[4:13].astype(np.float64).reshape(3, 3), geom1=int(r[13]), geom2=int(r[14]))
                    for r in rec[e][:int(ncon[e])]])
    return out, [int(x) for x in ovf], rec, ncon


def run(flat, Q):
    hm, hb = make_hip(flat, None, B=len(Q))
    hb.set("qpos", Q.astype(np.float32)); hb.set("qvel", 0.0); hb.set("ctrl", 0.0); hb.set("qacc_warmstart", 0.0)
    hb.forward()
    return hm, hb


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    flat = CS.scene(tmp_path_factory.mktemp("contact_certificates"))
    smp = CS.samples()
    Q = CS.batch_qpos(flat, smp)
    hm, hb = run(flat, Q)
    xp, xq = hb.get("xpos").astype(np.float64), hb.get("xquat").astype(np.float64)
    cons, ovf, rec, ncon = device_contacts(hb)
    return flat, smp, Q, hm, hb, xp, xq, cons, ovf, rec.copy(), ncon.copy()


def test_every_pair_class_at_constructed_depths_on_the_kernel(sweep):
    flat, smp, Q, hm, hb, xp, xq, cons, ovf, rec, ncon = sweep
    assert len(smp) == 864
    records = CS.evaluate(flat, smp, xp, xq, cons, ovf, S.params32(flat))
    print(CS.table(flat, records, "kernel (fp32), B = 864"))
    CS.check(records, EPS, "kernel")
    assert {r["kind"] for r in records if r["res"]} == {"plane", "plane-box", "box-box", "round", "general"}
    for e in (0, 200, 863):                                      # the same records through contacts()
        one = hb.contacts(e)
        assert len(one) == len(cons[e]) and all(a["dist"] == b["dist"] and np.array_equal(a["pos"], b["pos"]) for a, b in zip(one, cons[e]))


def test_a_second_forward_returns_the_same_contacts(sweep):
    """C7: the warm-start records are filled by the first forward(); the second one reports the same contact set, and C1 - C6 hold on it"""
    flat, smp, Q, hm, hb, xp, xq, cons, ovf, rec, ncon = sweep
    hb.forward()
    cons2, ovf2, rec2, ncon2 = device_contacts(hb)
    assert np.array_equal(ncon2, ncon)
    for a, b in zip(cons, cons2):
        assert [(k["geom1"], k["geom2"]) for k in a] == [(k["geom1"], k["geom2"]) for k in b]
    same = sum(np.array_equal(rec[e][:ncon[e], :15], rec2[e][:ncon[e], :15]) for e in range(len(smp)))
    print(f"second forward(): {same} of {len(smp)} envs bitwise the same contact geometry")
    records = CS.evaluate(flat, smp, hb.get("xpos").astype(np.float64), hb.get("xquat").astype(np.float64), cons2, ovf2, S.params32(flat))
    CS.check(records, EPS, "kernel, second forward()")


def test_one_partial_wavefront_gives_the_same_contacts_bitwise(sweep):
    flat, smp, Q, hm, hb, xp, xq, cons, ovf, rec, ncon = sweep
    first = [e for e in range(len(smp)) if CS.CASES[smp[e][2]] > 0][:3]          # the first three deep samples
    hm3, hb3 = run(flat, Q[first])
    cons3, ovf3, rec3, ncon3 = device_contacts(hb3)
    assert ovf3 == [0, 0, 0]
    for k, e in enumerate(first):
        assert ncon3[k] == ncon[e] >= 1
        assert np.array_equal(rec3[k][:ncon[e], :15], rec[e][:ncon[e], :15]), (k, e)       # dist, pos, frame, geom1, geom2


def test_sphere_against_each_face_of_a_tetrahedron(tmp_path):
    """the kernel's twin of the host test: the hull whose bounding-box centre lies outside it (MPR's interior point is `sm.gcen`, from geom_rcenter)"""
    flat = CS.tet_scene(tmp_path)
    cases = CS.tet_cases(flat)
    hm, hb = run(flat, np.stack([q for q, n, gap in cases]))
    cons, ovf, rec, ncon = device_contacts(hb)
    assert ovf == [0] * len(cases)
    for (q, n, gap), c in zip(cases, cons):
        CS.check_tet(c, n, gap, FLOOR, (tuple(np.round(n, 3)), gap))
