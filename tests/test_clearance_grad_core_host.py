"""Host rehearsal of the clearance gradient / collision cost kernels' fp32 core (robosuite_amd/csrc/rsim_grad_core.h on rsim_clear_core.h: the joint walk, the
gradient of a result and the cost loop k_clear_joints / k_clear_grad / k_clear_cost run per candidate) under AddressSanitizer + UndefinedBehaviorSanitizer:
tests/san/grad_core_driver.cpp is built with g++ and run as a subprocess on scene T's tables and seeded candidates at (5, 13), plain and with attachments,
and on the 16-hinge chain.  Pass = the sanitizers report nothing, every candidate returns, and the program's fp32 gradients and costs agree with fp64.

Bounds, by reasoning, not from a run.
  * FORMULA: grad against n . (s2 v(p2) - s1 v(p1)) in fp64 from the program's own poses, fromto, dist and pair -- every candidate.  What differs is fp32
    rounding of the joint frames (the pose chain's allowance of tests/test_clearance_core_host.py, 2e-5 m and rad, times |n| = 1 and a lever of at most L) and
    of the products: FORMULA_BOUND = 2e-5 (1 + L).
  * MIRROR: against the mirror's gradient at ITS OWN witnesses (distance_scenes.REF) at the program's poses, for status 0, |dist| >= 1e-3 and the same pair.
    The iteration stops when its bounds on the distance agree to tol; on a surface of curvature radius r a witness may then sit sqrt(2 tol r) beside the
    true one, which turns the normal by sqrt(2 tol / r): MIRROR_BOUND = sqrt(2 tol / R_MIN) L + sqrt(2 tol R_MAX) + FORMULA_BOUND, R_MIN / R_MAX the
    smallest / largest curvature radius of a curved geom of the scene (flat faces turn no normal).
  * COST: a near pair's term 1/2 (d_safe - d)^2 is off by at most d_safe |dd|, |dd| <= tol + 2e-5 (that file's distance bound), its gradient by
    |dd| L + d_safe MIRROR_BOUND; times the number of near pairs of the candidate.  Counts are compared outside the distance bound of d_safe and 0.
Nothing sanitized is loaded into Python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from robosuite_amd import clearance, distance, mjcf
from tests import attach_scenes as A
from tests import clearance_scenes as S
from tests import test_clearance_grad_host as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "san", "grad_core_driver.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
TOL, MAX_ITERS = distance.DEFAULTS["tol"], distance.DEFAULTS["max_iters"]
DIST_BOUND = TOL + 2e-5
MIN_DIST = 1e-3
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
# lever L (m): the reach of the scene from its first joint; R_MIN / R_MAX (m): curvature radii of its curved geoms (scene T: the 0.015 sphere and the ellipsoid's
# 0.03^2 / 0.06 up to the 0.07 sphere and the ellipsoid's 0.06^2 / 0.03; the chain: capsules of radius 0.02)
SCENES = {"T": dict(L=1.2, r_min=0.015, r_max=0.12), "chain": dict(L=16 * 0.12, r_min=0.02, r_max=0.02)}


def bounds(scene):
    s = SCENES[scene]
    formula = 2e-5 * (1 + s["L"])
    mirror = np.sqrt(2 * TOL / s["r_min"]) * s["L"] + np.sqrt(2 * TOL * s["r_max"]) + formula
    return formula, mirror, s["L"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("grad_san") / "grad_core_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", DRIVER, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def pack(flat, dofs, qpos, xp0, xq0, q, pairs, distmax, d_safe, attach=None, held=None, rel=None, skip=False):
    """clearance_scenes.pack_scene, the attached table in place of the plain one, and the driver's tail"""
    blob = S.pack_scene(flat, dofs, qpos, xp0, xq0, q, pairs, distmax, TOL, MAX_ITERS)
    B, nb = q.shape[0], int(flat.nbody)
    col, jt = clearance._columns(flat, dofs), clearance._I(flat, "jnt_type")
    slide = sum(1 << c for j, c in col.items() if jt[j] == mjcf.JNT_SLIDE)
    sig = clearance.signatures(flat, dofs)
    bsig, batt, natt = (sig | (sig << 16)).astype(np.int32), np.full(nb, -1, dtype=np.int32), 0
    if attach:
        plain_tab, plain_slot = S.body_table(flat, dofs)
        tab, slot, bsig, batt = A.attach_table(flat, dofs, attach)
        head = struct.calcsize("<10i2fi3i")
        fields = list(struct.unpack("<10i2fi3i", blob[:head]))
        fields[6], fields[7] = len(tab), int((slot >= 0).sum())
        old = plain_tab.astype("<i4").tobytes() + plain_slot.astype("<i4").tobytes()
        assert blob[head:head + len(old)] == old
        blob = struct.pack("<10i2fi3i", *fields) + tab.astype("<i4").tobytes() + slot.astype("<i4").tobytes() + blob[head + len(old):]
        natt = len(attach)
    tail = [struct.pack("<3i", natt, int(rel is not None), int(skip)), bsig.astype("<i4").tobytes(), batt.astype("<i4").tobytes()]
    if natt:
        tail.append(np.asarray(held, dtype=np.uint8).reshape(B, natt).tobytes())
    if rel is not None:
        tail.append(np.asarray(rel, dtype="<f4").reshape(B, natt, 7).tobytes())
    tail.append(struct.pack("<fi", d_safe, slide))
    return blob + b"".join(tail)


def run(exe, tmp, blob, B, K, nbody, n):
    fin, fout = os.path.join(str(tmp), "scene.bin"), os.path.join(str(tmp), "out.bin")
    with open(fin, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-300:], r.stderr[-4000:])       # no sanitizer finding, no crash, every candidate returned
    with open(fout, "rb") as f:
        raw = f.read()
    N = B * K
    f = np.frombuffer(raw, dtype="<f4", count=N * nbody * 7)
    xp, xq = f[:N * nbody * 3].reshape(B, K, nbody, 3).astype(np.float64), f[N * nbody * 3:].reshape(B, K, nbody, 4).astype(np.float64)
    dt = np.dtype([("f", "<f4", 7), ("i", "<i4", 2), ("g", "<f4", n), ("c", "<f4"), ("cg", "<f4", n), ("n", "<i4", 2)])
    rec = np.frombuffer(raw, dtype=dt, count=N, offset=N * nbody * 7 * 4).reshape(B, K)
    assert len(raw) == N * nbody * 7 * 4 + N * dt.itemsize
    return xp, xq, rec


def compare(scene, flat, dofs, qpos, q, pairs, distmax, d_safe, xp, xq, rec, sigs, active=None):
    formula_b, mirror_b, L = bounds(scene)
    B, K = q.shape[:2]
    gb = clearance._I(flat, "geom_bodyid")
    d, ft, st = S.pair_reference(flat, xp, xq, pairs, S.params32(flat))
    m32 = clearance._model32(flat)
    worst = dict(formula=0.0, mirror=0.0, cost=0.0, cost_grad=0.0)
    n_mirror = n_drop = n_cost = 0
    for e in range(B):
        if active is not None:
            st[e][:, ~active[e]] |= distance.FAR
        for k in range(K):
            r = rec[e, k]
            dist, f6, pair, status, grad = float(r["f"][0]), r["f"][1:].astype(np.float64), int(r["i"][0]), int(r["i"][1]), np.atleast_1d(r["g"]).astype(np.float64)
            fr = clearance.joint_frames(flat, qpos[e], dofs, q[e, k], model32=m32)
            if pair < 0 or status & (distance.FAR | distance.OVERLAP) or abs(dist) < clearance.GRAD_MIN_DIST:
                assert not grad.any()
            else:
                g1, g2 = pairs[pair]
                want = clearance.pair_grad(fr, sigs[e][gb[g1]], sigs[e][gb[g2]], f6[:3], f6[3:], dist)
                worst["formula"] = max(worst["formula"], np.abs(grad - want).max())
                if status == distance.OK and abs(dist) >= MIN_DIST:
                    ref = clearance.reduce_grad(flat, pairs, d[e, k], ft[e, k], st[e, k], sigs[e], fr, distmax)
                    if ref[1] == pair and ref[3] == distance.OK:
                        n_mirror += 1
                        worst["mirror"] = max(worst["mirror"], np.abs(grad - ref[4]).max())
                    else:
                        n_drop += 1
            c = clearance.reduce_cost(flat, pairs, d[e, k], ft[e, k], st[e, k], sigs[e], fr, d_safe)
            live = (st[e, k] & distance.FAR) == 0
            if (live & (np.abs(d[e, k] - d_safe) <= DIST_BOUND)).any() or (live & (st[e, k] == distance.OK) & (np.abs(d[e, k]) <= DIST_BOUND)).any():
                continue
            assert (int(r["n"][0]), int(r["n"][1])) == (c[2], c[3]), (e, k)
            n_cost += c[2] > 0
            m = max(c[2], 1)
            ec, eg = abs(float(r["c"]) - c[0]) / m, np.abs(np.atleast_1d(r["cg"]) - c[1]).max() / m
            worst["cost"], worst["cost_grad"] = max(worst["cost"], ec), max(worst["cost_grad"], eg)
    bound = dict(formula=formula_b, mirror=mirror_b, cost=d_safe * DIST_BOUND, cost_grad=DIST_BOUND * L + d_safe * mirror_b)
    for k_, v in worst.items():
        print(f"fp32 core on the host, scene {scene}: {k_} {v:.3e} (bound {bound[k_]:.1e}; cost figures per near pair); mirror check {n_mirror}, dropped {n_drop}")
    assert n_drop <= 0.1 * (n_mirror + n_drop) and n_mirror > 0 and n_cost > 0
    for k_, v in worst.items():
        assert v <= bound[k_], (k_, v)


def poses(flat, qpos):
    m32 = clearance._model32(flat)
    now = [mjcf.kinematics_np(m32, qpos[e])[:2] for e in range(len(qpos))]
    return S.f32(np.stack([p[0] for p in now])), S.f32(np.stack([p[1] for p in now]))


@pytest.mark.parametrize("which", ("arm", "all"))
def test_scene_t_under_sanitizers(exe, tmp_path, which):
    flat = S.scene_t(tmp_path)
    B, K, nb = 5, 13, int(flat.nbody)
    dofs = S.dofs_t(flat, which)
    pairs = clearance.default_pairs(flat, dofs)
    qpos = S.f32(S.scene_t_qpos(flat, B))
    xp0, xq0 = poses(flat, qpos)
    q = S.candidates(flat, dofs, B, K)
    xp, xq, rec = run(exe, tmp_path, pack(flat, dofs, qpos, xp0, xq0, q, pairs, S.DISTMAX_T, 0.08), B, K, nb, len(dofs))
    compare("T", flat, dofs, qpos, q, pairs, S.DISTMAX_T, 0.08, xp, xq, rec, [clearance.signatures(flat, dofs)] * B)


def test_scene_t_attached_under_sanitizers(exe, tmp_path):
    flat = S.scene_t(tmp_path)
    B, K, nb = 5, 13, int(flat.nbody)
    dofs = S.dofs_t(flat, "all")
    att, held, rel = A.attach_t(flat), A.held_rows(B), A.rel_given(B)
    pairs = clearance.default_pairs(flat, dofs, att)
    qpos = S.f32(S.scene_t_qpos(flat, B))
    xp0, xq0 = poses(flat, qpos)
    q = S.candidates(flat, dofs, B, K)
    blob = pack(flat, dofs, qpos, xp0, xq0, q, pairs, S.DISTMAX_T, 0.08, attach=att, held=held, rel=rel, skip=True)
    xp, xq, rec = run(exe, tmp_path, blob, B, K, nb, len(dofs))
    rp, rq = A.mirror_fk(flat, qpos, dofs, q, att, held, rel, now=(xp0, xq0))
    assert np.linalg.norm(xp - rp, axis=-1).max() <= 2e-5      # the attached walk (the pose chain's allowance)
    sigs = [clearance.signatures(flat, dofs, att, held[e]) for e in range(B)]
    active = [clearance.active_pairs(flat, dofs, pairs, att, held[e]) for e in range(B)]
    compare("T", flat, dofs, qpos, q, pairs, S.DISTMAX_T, 0.08, xp, xq, rec, sigs, active)


@pytest.mark.parametrize("ndof", (H.CHAIN_N, 1))
def test_chain_under_sanitizers(exe, tmp_path, ndof):
    flat = mjcf.compile_mjcf(H.chain_xml())
    B, K, nb = 2, 9, int(flat.nbody)
    dofs = S.dofs_of(flat, [f"cj{i}" for i in range(H.CHAIN_N)]) if ndof > 1 else S.dofs_of(flat, ["cj7"])
    pairs = H.chain_pairs(flat)
    qpos = S.f32(np.tile(np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel(), (B, 1)))
    xp0, xq0 = poses(flat, qpos)
    q = S.candidates(flat, dofs, B, K)
    xp, xq, rec = run(exe, tmp_path, pack(flat, dofs, qpos, xp0, xq0, q, pairs, 5.0, 0.6), B, K, nb, ndof)
    compare("chain", flat, dofs, qpos, q, pairs, 5.0, 0.6, xp, xq, rec, [clearance.signatures(flat, dofs)] * B)
