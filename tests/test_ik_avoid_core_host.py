"""Host rehearsal of the collision-aware IK kernels' fp32 core (robosuite_amd/csrc/rsim_ik_avoid_core.h on rsim_grad_core.h: what k_ika_init / k_ika_cost /
k_ika_step run per problem) under AddressSanitizer + UndefinedBehaviorSanitizer: tests/san/ik_avoid_core_driver.cpp is built with g++ and run as a subprocess on
scene A (B = 3, K = 5, two pair chunks) for three updates.  Pass = the sanitizers report nothing, every problem returns, and every iterate agrees with fp64.

Each update is held apart from the ones before it: the mirror's update formula (ik_avoid.update) is fed the PROGRAM's own iterate q_i and compared with the
program's q_i+1, so no error is carried along.  Bounds, by reasoning, not from a run:
  * ERR: |err_pos| at q_i against ik.Problem.error: the pose chain's allowance of tests/test_clearance_core_host.py, 2e-5 m, once for the site body and once more
    for the site offset and the subtraction: 4e-5.
  * COST: a near pair's term is off by at most W |dd|, |dd| <= tol + 2e-5 (that file's distance bound), W = d_safe + DEPTH the largest d_safe - d of the scene
    (DEPTH = 0.1: sphere radius + capsule radius); times the near pairs of the problem.  Compared where no pair stands within |dd| of d_safe or of 0.
  * STEP: the projector I - J^T A^-1 J has norm <= 1 and the max_dq scaling is <= 1, so the secondary term's error is at most avoid_gain times the gradient's:
    per near pair |dd| L + W (sqrt(2 tol / R_MIN) L + sqrt(2 tol R_MAX) + 2e-5 (1 + L)) (tests/test_clearance_grad_core_host.py's MIRROR bound: witness error on
    curved solids); the primary term J^T A^-1 e carries the error of e, 4e-5, times |J^T A^-1| <= 1 / (2 sqrt(damping)) = 50, and as much again for the fp32
    factorisation of a matrix of condition <= |J|^2 / damping: 4e-3.
Nothing sanitized is loaded into Python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from robosuite_amd import clearance, distance, ik, ik_avoid, mjcf
from tests import clearance_scenes as S
from tests import ik_avoid_scenes as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "san", "ik_avoid_core_driver.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
TOL, MAX_ITERS = distance.DEFAULTS["tol"], distance.DEFAULTS["max_iters"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
DD, L, DEPTH, R_MIN, R_MAX = TOL + 2e-5, 1.0, 0.1, 0.03, 0.07
ERR_BOUND = 4e-5
UPDATES, CHUNKS = 3, 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ika_san") / "ik_avoid_core_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", DRIVER, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def pack(flat, site, dofs, qpos, xp0, xq0, q_init, pairs, pos, o):
    blob = S.pack_scene(flat, dofs, qpos, xp0, xq0, q_init, pairs, o["d_safe"], TOL, MAX_ITERS)
    nft = S.float_offsets(flat)["_len"]
    _, slot = S.body_table(flat, dofs)
    I = lambda k: np.asarray(flat.arrays[k]).ravel().astype(int)      # noqa: E731
    _, jid = ik.chain(flat, site, dofs)
    rng = np.asarray(flat.arrays["jnt_range"], dtype=np.float64).reshape(-1, 2)
    extra = np.concatenate([rng[jid].ravel(), np.asarray(flat.arrays["site_pos"], dtype=np.float64).reshape(-1, 3)[site],
                            np.asarray(flat.arrays["site_quat"], dtype=np.float64).reshape(-1, 4)[site]]).astype("<f4")
    n = len(dofs)
    head = np.array([[nft + 2 * c, I("jnt_limited")[jid[c]], I("jnt_qposadr")[jid[c]], I("jnt_type")[jid[c]]] for c in range(n)], dtype="<i4")
    sig = clearance.signatures(flat, dofs)
    body = I("site_bodyid")[site]
    slide = sum(1 << c for c in range(n) if I("jnt_type")[jid[c]] == mjcf.JNT_SLIDE)
    tail = [struct.pack("<i", len(extra)), extra.tobytes(),
            struct.pack("<10i", int(slot[body]), nft + 2 * n, nft + 2 * n + 3, int(sig[body]), slide, 3, o["max_iters"], int(o["clamp_range"]), o["max_iters"] + 1, CHUNKS),
            head.tobytes(), (sig | (sig << 16)).astype("<i4").tobytes(),
            struct.pack("<8f", o["damping"], o["max_dq"], o["pos_tol"], o["rot_tol"], o["posture_gain"], o["avoid_gain"], o["cost_tol"], o["d_safe"]),
            np.asarray(pos, dtype="<f4").tobytes()]
    return blob + b"".join(tail)


def test_scene_a_chain_under_sanitizers(exe, tmp_path):
    a = A.scene_a()
    flat, site, dofs, pairs = a["flat"], a["site"], a["dofs"], a["pairs"]
    B, K, n = 3, 5, len(dofs)
    c = A.cases(B, K)
    o = ik_avoid.options(**dict(A.OPTS, max_iters=UPDATES))
    m32 = clearance._model32(flat)
    now = [mjcf.kinematics_np(m32, c["qpos"][e])[:2] for e in range(B)]
    xp0, xq0 = S.f32(np.stack([p[0] for p in now])), S.f32(np.stack([p[1] for p in now]))
    fin, fout = os.path.join(str(tmp_path), "scene.bin"), os.path.join(str(tmp_path), "out.bin")
    with open(fin, "wb") as f:
        f.write(pack(flat, site, dofs, c["qpos"], xp0, xq0, c["q_init"], pairs, c["pos"], o))
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-300:], r.stderr[-4000:])       # no sanitizer finding, no crash, every problem returned
    raw = np.fromfile(fout, dtype="<f4").astype(np.float64)
    N = B * K
    assert len(raw) == N * n + (UPDATES + 1) * (N * 8 + N * n)
    qs, recs, at = [raw[:N * n].reshape(B, K, n)], [], N * n
    for _ in range(UPDATES + 1):
        recs.append(raw[at:at + N * 8].reshape(B, K, 8)); at += N * 8
        qs.append(raw[at:at + N * n].reshape(B, K, n)); at += N * n
    lo, hi, _ = A.ik_scenes.ranges(flat, dofs)
    assert np.array_equal(qs[0], np.clip(c["q_init"], lo, hi))
    grad_pair = DD * L + (o["d_safe"] + DEPTH) * (np.sqrt(2 * TOL / R_MIN) * L + np.sqrt(2 * TOL * R_MAX) + 2e-5 * (1 + L))
    worst = dict(err=0.0, cost=0.0, step=0.0)
    n_cost = n_step = 0
    P = [ik.Problem(flat, c["qpos"][e], site, dofs) for e in range(B)]
    for e in range(B):
        for k in range(K):
            stopped = False
            for i in range(UPDATES + 1):
                q_i, rec = qs[i][e, k], recs[i][e, k]
                if stopped:
                    assert np.array_equal(qs[i + 1][e, k], q_i)      # frozen
                    continue
                err, _ = P[e].error(q_i, c["pos"][e, k], None)
                worst["err"] = max(worst["err"], abs(rec[0] - np.linalg.norm(err[:3])))
                xp = clearance.fk(flat, c["qpos"][e], dofs, q_i, model32=m32)
                d, ft, st = distance.geom_distance(flat, xp[0], xp[1], pairs, o["d_safe"], TOL, MAX_ITERS, S.params32(flat))
                ref = clearance.collision_cost(flat, c["qpos"][e], dofs, q_i, pairs, o["d_safe"], params=S.params32(flat), poses=xp)
                live = (st & distance.FAR) == 0
                edge = (live & (np.abs(d - o["d_safe"]) <= DD)).any() or (live & (st == distance.OK) & (np.abs(d) <= DD)).any()
                near = max(ref[2], 1)
                if not edge:
                    assert (int(rec[3]), int(rec[4])) == (ref[2], ref[3])
                    worst["cost"] = max(worst["cost"], abs(rec[2] - ref[0]) / near)
                    n_cost += ref[2] > 0
                assert int(rec[5]) == i
                stopped = bool(rec[7]) or i >= UPDATES
                if stopped:
                    assert np.array_equal(qs[i + 1][e, k], q_i)
                    continue
                if edge or ref[3]:      # (an overlapping pair gives no push in either; its neighbourhood is one-sided)
                    continue
                want = ik_avoid.update(flat, c["qpos"][e], site, dofs, q_i, qs[0][e, k], c["pos"][e, k], None, pairs, params=S.params32(flat), **o)
                worst["step"] = max(worst["step"], np.abs(qs[i + 1][e, k] - want).max() / (4e-3 + o["avoid_gain"] * near * grad_pair))
                n_step += 1
    print(f"fp32 IK-avoid core on the host, scene A: |err| {worst['err']:.3e} (bound {ERR_BOUND:.0e}); cost per near pair {worst['cost']:.3e} "
          f"(bound {(o['d_safe'] + DEPTH) * DD:.1e}); update / its bound {worst['step']:.3f} (4e-3 + gain x near pairs x {grad_pair:.2e}); compared {n_cost} costs, {n_step} updates")
    assert n_cost > 0 and n_step >= N
    assert worst["err"] <= ERR_BOUND and worst["cost"] <= (o["d_safe"] + DEPTH) * DD and worst["step"] <= 1.0
