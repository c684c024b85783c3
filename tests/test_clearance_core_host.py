"""Host rehearsal of the configuration clearance kernels' fp32 core (robosuite_amd/csrc/rsim_clear_core.h on rsim_dist_core.h: the FK walk and the pair loop
k_clear_fk / k_clear_dist run per candidate) under AddressSanitizer + UndefinedBehaviorSanitizer: tests/san/clear_core_driver.cpp is built with g++ and run
as a subprocess on scene T's tables and seeded candidates.  Pass = the sanitizers report nothing, every candidate returns, and the program's fp32 poses and
minima agree with the fp64 mirror (robosuite_amd/clearance.py).

Bounds, by reasoning, not from a run.  FK: a pose of this scene is composed over at most four bodies (three joints), each step a handful of fp32 products of
numbers up to 1.5 m (2^-24 relative each) and one sine / cosine pair from a polynomial good to ~1e-7: some 50 roundings of 1e-7 m, held to 2e-5 m and 2e-5 rad --
the allowance tests/test_distance_core_host.py makes for the pose chain of its scenes.  Distance: the minimum is compared with the mirror's at THE PROGRAM'S OWN
poses, so only the distance layer's error is left: that test's bound, tol + 2e-5 m.  Nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from robosuite_amd import clearance, distance
from tests import clearance_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "san", "clear_core_driver.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
TOL, MAX_ITERS = distance.DEFAULTS["tol"], distance.DEFAULTS["max_iters"]
FK_BOUND = 2e-5
BOUND = TOL + 2e-5
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("clear_san") / "clear_core_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", DRIVER, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run(exe, tmp, blob, B, K, nbody):
    fin, fout = os.path.join(str(tmp), "scene.bin"), os.path.join(str(tmp), "out.bin")
    with open(fin, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-300:], r.stderr[-4000:])       # no sanitizer finding, no crash, every candidate returned
    with open(fout, "rb") as f:
        return S.unpack_scene(f.read(), B, K, nbody)


@pytest.mark.parametrize("which,pairs_from", (("arm", "default"), ("all", "default"), ("all", "every")))
def test_scene_t_under_sanitizers(exe, tmp_path, which, pairs_from):
    from tests import distance_scenes as D

    flat = S.scene_t(tmp_path)
    B, K, nb = 5, 13, int(flat.nbody)
    dofs = S.dofs_t(flat, which)
    pairs = clearance.default_pairs(flat, dofs) if pairs_from == "default" else D.all_pairs(flat)      # "every": static pairs and same-signature pairs too
    qpos = S.f32(S.scene_t_qpos(flat, B))
    now = [mjcf_poses(flat, qpos[e]) for e in range(B)]
    xp0, xq0 = S.f32(np.stack([p[0] for p in now])), S.f32(np.stack([p[1] for p in now]))
    q = S.candidates(flat, dofs, B, K)
    xp, xq, dist, pair, ft, st = run(exe, tmp_path, S.pack_scene(flat, dofs, qpos, xp0, xq0, q, pairs, S.DISTMAX_T, TOL, MAX_ITERS), B, K, nb)

    # FK: every body against the mirror; a body the dofs do not move is the env's pose, bit for bit
    rp, rq = S.fk_reference(flat, qpos, dofs, q)
    moved = clearance.signatures(flat, dofs) != 0
    assert np.array_equal(xp[:, :, ~moved], np.broadcast_to(xp0[:, None, ~moved], xp[:, :, ~moved].shape))
    assert np.array_equal(xq[:, :, ~moved], np.broadcast_to(xq0[:, None, ~moved], xq[:, :, ~moved].shape))
    perr, aerr = np.linalg.norm(xp - rp, axis=-1).max(), S.rot_angle(xq, rq).max()
    print(f"fp32 FK on the host, dofs {which}: worst position error {perr:.3e} m, worst rotation error {aerr:.3e} rad (bound {FK_BOUND:.0e})")
    assert perr <= FK_BOUND and aerr <= FK_BOUND

    # the minimum, at the program's own poses
    d_ref, _, _ = S.pair_reference(flat, xp, xq, pairs, S.params32(flat))
    m_ref = d_ref.min(axis=-1)
    far = m_ref >= S.DISTMAX_T
    err = np.abs(dist - np.where(far, S.DISTMAX_T, m_ref))
    print(f"fp32 minimum on the host, {len(pairs)} pairs: worst |d - min_ref| {err.max():.3e} (bound {BOUND:.1e}); {int((pair < 0).sum())} of {pair.size} far")
    assert not (st & distance.CAP).any()
    assert err.max() <= BOUND
    edge = np.abs(m_ref - S.DISTMAX_T) <= 2 * BOUND
    assert ((pair < 0) == far)[~edge].all() and (pair >= 0).any()
    assert (pair < 0).any() or pairs_from == "every"      # (the full list holds static pairs that touch: nothing is far there)
    none = pair < 0
    assert (dist[none] == np.float32(S.DISTMAX_T)).all() and (ft[none] == 0).all() and (st[none] == distance.FAR).all()
    e_, k_ = np.nonzero(~none)
    assert (pair[~none] < len(pairs)).all()
    assert (d_ref[e_, k_, pair[~none]] <= m_ref[~none] + 2 * BOUND).all()      # the chosen pair attains the minimum (a near-tie may go either way)
    for e, k in zip(e_, k_):
        if st[e, k] in (distance.OK, distance.OVERLAP):
            G = distance.world_geoms(flat, xp[e, k], xq[e, k], pairs[pair[e, k]], S.params32(flat))
            g1, g2 = G[int(pairs[pair[e, k]][0])], G[int(pairs[pair[e, k]][1])]
            assert max(D.outside_by(g1, ft[e, k, :3]), D.outside_by(g2, ft[e, k, 3:])) <= BOUND, (e, k)
            assert abs(np.linalg.norm(ft[e, k, 3:] - ft[e, k, :3]) - abs(dist[e, k])) <= BOUND, (e, k)


def mjcf_poses(flat, qpos):
    from robosuite_amd import mjcf

    return mjcf.kinematics_np(clearance._model32(flat), qpos)[:2]
