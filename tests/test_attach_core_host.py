"""Host rehearsal of the carried-object paths of the fp32 cores (robosuite_amd/csrc/rsim_clear_core.h and rsim_sweep_core.h with ATT = true: the walk of the
attached subtrees, the per-lane pair skip, the motion bound of a held body, the advancement loop -- what k_clear_fk_att, k_clear_dist_att and k_sweep_att run
per lane) under AddressSanitizer + UndefinedBehaviorSanitizer: tests/san/attach_core_driver.cpp is built with g++ exactly as the two other drivers are and run
as a program on scene T with fsb on l2 and fbb on side, and on scene J, where the attached tool carries a subtree -- a jaw on a hinge, a tip below it on a
slide, a guard beside them: the table's CL_BODY elements with o3 = attachment + 1 (tests/attach_scenes.py).  Pass = the sanitizers report nothing, every segment returns, and the outputs
agree with the fp64 mirror (robosuite_amd/clearance.py, sweep.py with attach / held / rel).

Bounds: those of tests/test_clearance_core_host.py and tests/test_sweep_core_host.py, by their reasoning.  A held body adds two quaternion products and one
rotation to a chain of some fifty roundings: FK_BOUND = 2e-5 m / rad has room for them.  The minimum is compared at THE PROGRAM'S OWN poses over the pairs
the env evaluates: tol + 2e-5 m.  The sweep's certificate is held against the mirror's own attached clearance at the same t to the same bound, L to a
relative 1e-5.  A body that is not held is the env's pose bit for bit.  Nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from robosuite_amd import clearance, distance, sweep
from tests import attach_scenes as A
from tests import clearance_scenes as S
from tests import sweep_scenes as W
from tests.test_clearance_core_host import BOUND, ENV, FK_BOUND, MAX_ITERS, TOL, mjcf_poses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "san", "attach_core_driver.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("attach_san") / "attach_core_san")
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
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-300:], r.stderr[-4000:])       # no sanitizer finding, no crash, every segment within max_steps
    print(r.stdout.strip())
    with open(fout, "rb") as f:
        return A.unpack_attach(f.read(), B, K, nbody)


def _scene(name, tmp_path, mode, B):
    """-> (flat, dofs, attach, held [B, n], rel [B, n, 7] or None, qpos [B, nq], how many different held rows there are)"""
    if name == "T":      # fsb on l2, fbb on side: two single bodies, all four held rows
        flat = S.scene_t(tmp_path)
        return flat, S.dofs_t(flat, "all"), A.attach_t(flat), A.held_rows(B), A.rel_of(mode, B), S.f32(S.scene_t_qpos(flat, B)), 4
    flat = A.scene_j()   # the tool with its jaw, tip and guard on the wrist: an attached SUBTREE, held in every other env
    return flat, A.dofs_j(flat), A.attach_j(flat), A.held_rows_j(B), None if mode == "state" else A.rel_given_j(B), S.f32(A.scene_j_qpos(flat, B)), 2


@pytest.mark.parametrize("mode", A.REL_MODES)
@pytest.mark.parametrize("name", ("T", "J"))
def test_attached_scenes_under_sanitizers(exe, tmp_path, name, mode):
    B, K = 6, 4
    flat, dofs, att, held, rel, qpos, rows = _scene(name, tmp_path, mode, B)
    nb = int(flat.nbody)
    assert len({tuple(r) for r in held}) == rows
    pairs = clearance.default_pairs(flat, dofs, att)
    now = [mjcf_poses(flat, qpos[e]) for e in range(B)]
    xp0, xq0 = S.f32(np.stack([p[0] for p in now])), S.f32(np.stack([p[1] for p in now]))
    q0, q1 = W.segments(flat, dofs, B, K)
    margin, slack, max_steps = 0.0, sweep.DEFAULTS["slack"], 256
    blob = A.pack_attach(flat, dofs, att, held, rel, qpos, xp0, xq0, q0, q1, pairs, S.DISTMAX_T, TOL, MAX_ITERS, margin, slack, max_steps)
    xp, xq, cl, sw = run(exe, tmp_path, blob, B, K, nb)

    # FK at q0: every body against the mirror; what is not moved, and what is not held, is the env's pose bit for bit
    rp, rq = A.mirror_fk(flat, qpos, dofs, q0, att, held, rel, now=(xp0, xq0))
    for e in range(B):
        still = clearance.signatures(flat, dofs, att, held[e]) == 0
        assert np.array_equal(xp[e][:, still], np.broadcast_to(xp0[e, still], xp[e][:, still].shape))
        assert np.array_equal(xq[e][:, still], np.broadcast_to(xq0[e, still], xq[e][:, still].shape))
    perr, aerr = np.linalg.norm(xp - rp, axis=-1).max(), S.rot_angle(xq, rq).max()
    print(f"fp32 attached FK on the host, scene {name}, rel {mode}: worst position error {perr:.3e} m, worst rotation error {aerr:.3e} rad (bound {FK_BOUND:.0e})")
    assert perr <= FK_BOUND and aerr <= FK_BOUND
    moved = np.linalg.norm(xp[:, :, [a[0] for a in att]] - xp0[:, None, [a[0] for a in att]], axis=-1).max(axis=1)      # [B, natt]
    assert (moved[held] > 1e-3).all()      # ... and a held body did go with its carrier
    below = [c for body, _ in att for c in clearance.subtree(flat, body)[1:]]
    assert (name == "J") == bool(below)
    if below:      # ... and so did what hangs below it, joints at the env's qpos (within the bound above); where it is not held it is the env's pose (above)
        went = np.linalg.norm(xp[:, :, below] - xp0[:, None, below], axis=-1).max(axis=1)      # [B, len(below)]
        assert (went[held[:, 0]] > 1e-3).all() and not went[~held[:, 0]].any()

    # the minimum at q0, at the program's own poses, over the pairs each env evaluates
    d_ref = S.pair_reference(flat, xp, xq, pairs, S.params32(flat))[0]
    on = np.stack([clearance.active_pairs(flat, dofs, pairs, att, held[e]) for e in range(B)])
    assert len({tuple(r) for r in on}) == rows
    m_ref = np.where(on[:, None, :], d_ref, np.inf).min(axis=-1)
    far = m_ref >= S.DISTMAX_T
    err = np.abs(cl["dist"] - np.where(far, S.DISTMAX_T, m_ref))
    print(f"fp32 attached minimum on the host, scene {name}, rel {mode}: worst |d - min_ref| {err.max():.3e} (bound {BOUND:.1e}); {int((cl['pair'] < 0).sum())} of {cl['pair'].size} far")
    assert not (cl["status"] & distance.CAP).any() and err.max() <= BOUND
    edge = np.abs(m_ref - S.DISTMAX_T) <= 2 * BOUND
    none = cl["pair"] < 0
    assert (none == far)[~edge].all() and (~none).any()
    e_, k_ = np.nonzero(~none)
    assert on[e_, cl["pair"][~none]].all()      # no env reports a pair it does not evaluate
    assert (d_ref[e_, k_, cl["pair"][~none]] <= m_ref[~none] + 2 * BOUND).all()

    # the sweep: L against the mirror, the certificate against the mirror's own attached clearance
    m32 = clearance._model32(flat)
    R = lambda e: None if rel is None else rel[e]      # noqa: E731

    def clear_at(e, k, t):
        q = W.at(q0[e, k], q1[e, k], t)
        poses = clearance.fk(flat, qpos[e], dofs, q, model32=m32, attach=att, held=held[e], rel=R(e), now=(xp0[e], xq0[e]))
        return clearance.clearance(flat, qpos[e], dofs, q, None, S.DISTMAX_T, poses=poses, attach=att, held=held[e])[0]

    st = sw["status"]
    assert not (st & distance.CAP).any() and ((st & 3) <= 2).all() and (sw["steps"] >= 1).all() and (sw["steps"] <= max_steps).all()
    worst_l = worst_c = 0.0
    for e in range(B):
        for k in range(K):
            L = sweep.motion_bound(flat, qpos[e], dofs, q0[e, k], q1[e, k], None, attach=att, held=held[e], rel=R(e))
            worst_l = max(worst_l, abs(sw["L"][e, k] - L) / L if L else abs(sw["L"][e, k]))
            t, tm, s = sw["t"][e, k], sw["t_min"][e, k], int(st[e, k]) & 3
            assert 0.0 <= tm <= t <= 1.0
            ts = np.linspace(0.0, 1.0, W.DENSE)
            ts = ts if s == sweep.FREE else ts[ts < t]
            c = np.array([clear_at(e, k, x) for x in ts[::4]])      # (every fourth of the dense samples: the mirror's attached clearance is slow)
            assert len(c) == 0 or c.min() > margin - BOUND, (e, k, s, t, c.min())
            if s == sweep.HIT:
                assert clear_at(e, k, t) <= margin + slack + BOUND, (e, k, t)
            if sw["pair"][e, k] >= 0:
                worst_c = max(worst_c, abs(sw["dist"][e, k] - clear_at(e, k, tm)))
    print(f"fp32 attached sweep on the host, scene {name}, rel {mode}: worst |L - L_ref| / L_ref {worst_l:.3e} (bound 1e-5), worst |dist - c(t_min)| {worst_c:.3e} (bound {BOUND:.1e})")
    assert worst_l <= 1e-5 and worst_c <= BOUND


def test_an_explicit_list_is_not_skipped_in(exe, tmp_path):
    """skip = 0 (what an explicit pair list sets): every pair in every env, the held cube against its own fingers included"""
    flat = S.scene_t(tmp_path)
    B, K, nb = 4, 2, int(flat.nbody)
    dofs, att = S.dofs_t(flat, "all"), A.attach_t(flat)
    held, rel = A.held_rows(B), A.rel_given(B)
    pairs = clearance.default_pairs(flat, dofs, att)
    qpos = S.f32(S.scene_t_qpos(flat, B))
    now = [mjcf_poses(flat, qpos[e]) for e in range(B)]
    xp0, xq0 = S.f32(np.stack([p[0] for p in now])), S.f32(np.stack([p[1] for p in now]))
    q0, q1 = W.segments(flat, dofs, B, K)
    blob = A.pack_attach(flat, dofs, att, held, rel, qpos, xp0, xq0, q0, q1, pairs, 1.0, TOL, MAX_ITERS, 0.0, 1e-3, 8, skip=False)
    xp, xq, cl, sw = run(exe, tmp_path, blob, B, K, nb)
    m_ref = S.pair_reference(flat, xp, xq, pairs, S.params32(flat))[0].min(axis=-1)
    assert np.abs(cl["dist"] - np.minimum(m_ref, 1.0)).max() <= BOUND
