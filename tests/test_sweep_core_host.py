"""Host rehearsal of the swept clearance kernel's fp32 core (robosuite_amd/csrc/rsim_sweep_core.h on rsim_clear_core.h and rsim_dist_core.h: the motion-bound
walk and the advancement loop k_sweep runs per segment) under AddressSanitizer + UndefinedBehaviorSanitizer: tests/san/sweep_core_driver.cpp is built with g++
and run as a subprocess on scene T's tables and seeded segments.  Pass = the sanitizers report nothing, every segment returns within max_steps (the program
checks that itself), and the certificate properties of tests/test_sweep_host.py hold against the fp64 mirror (robosuite_amd/sweep.py, clearance.py).

The program's step sequence is not compared with the mirror's: it is sensitive to rounding.  Bounds, by reasoning, not from a run.  The program's sample is
the fp32 minimum at fp32 poses of an fp32 q(t); the mirror evaluates the clearance at the same t in fp64: tests/test_clearance_core_host.py's bound for
the distance layer, tol + 2e-5 m, is held here for the two layers together (that file measures the FK layer of this scene some fifty roundings of 1e-7 m deep;
q(t) adds one rounding of a joint value, 1e-7 rad on an arm of a metre).  The bound L: the same sum of a few dozen terms in fp32 and in fp64, both inflated
by 1 + 2^-16: held to a relative 1e-5 either way.  Nothing sanitized is loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from robosuite_amd import clearance, distance, sweep
from tests import clearance_scenes as S
from tests import sweep_scenes as W
from tests.test_clearance_core_host import mjcf_poses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "san", "sweep_core_driver.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
TOL, MAX_ITERS = distance.DEFAULTS["tol"], distance.DEFAULTS["max_iters"]
BOUND = TOL + 2e-5
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sweep_san") / "sweep_core_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", DRIVER, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run(exe, tmp, blob, B, K):
    fin, fout = os.path.join(str(tmp), "scene.bin"), os.path.join(str(tmp), "out.bin")
    with open(fin, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-300:], r.stderr[-4000:])       # no sanitizer finding, no crash, every segment within max_steps
    print(r.stdout.strip())
    with open(fout, "rb") as f:
        return W.unpack_sweep(f.read(), B, K)


@pytest.mark.parametrize("which,margin,max_steps", (("arm", 0.0, 256), ("all", 0.01, 256), ("all", 0.0, 3)))
def test_scene_t_under_sanitizers(exe, tmp_path, which, margin, max_steps):
    flat = S.scene_t(tmp_path)
    B, K = 3, 8
    dofs = S.dofs_t(flat, which)
    pairs = clearance.default_pairs(flat, dofs)
    qpos = S.f32(S.scene_t_qpos(flat, B))
    now = [mjcf_poses(flat, qpos[e]) for e in range(B)]
    xp0, xq0 = S.f32(np.stack([p[0] for p in now])), S.f32(np.stack([p[1] for p in now]))
    q0, q1 = W.segments(flat, dofs, B, K)
    if max_steps == 256:
        q1[:, 0] = q0[:, 0]      # no motion: L == 0, one sample decides
    slack = sweep.DEFAULTS["slack"]
    out = run(exe, tmp_path, W.pack_sweep(flat, dofs, qpos, xp0, xq0, q0, q1, pairs, S.DISTMAX_T, TOL, MAX_ITERS, margin, slack, max_steps), B, K)

    m32 = clearance._model32(flat)
    clear_at = lambda e, k, t: clearance.clearance(flat, qpos[e], dofs, W.at(q0[e, k], q1[e, k], t), pairs, S.DISTMAX_T,      # noqa: E731
                                                   poses=clearance.fk(flat, qpos[e], dofs, W.at(q0[e, k], q1[e, k], t), model32=m32))[0]
    st = out["status"]
    assert not (st & distance.CAP).any() and ((st & 3) <= 2).all() and (out["steps"] >= 1).all() and (out["steps"] <= max_steps).all()
    worst_l = worst_c = 0.0
    for e in range(B):
        for k in range(K):
            L = sweep.motion_bound(flat, qpos[e], dofs, q0[e, k], q1[e, k], pairs)
            worst_l = max(worst_l, abs(out["L"][e, k] - L) / L if L else abs(out["L"][e, k]))
            t, tm, s = out["t"][e, k], out["t_min"][e, k], int(st[e, k])
            assert 0.0 <= tm <= t <= 1.0
            if L == 0.0:
                assert out["steps"][e, k] == 1 and s in (sweep.FREE, sweep.HIT)
            ts = np.linspace(0.0, 1.0, W.DENSE)
            ts = ts if s == sweep.FREE else ts[ts < t]
            c = np.array([clear_at(e, k, x) for x in ts])
            assert len(c) == 0 or c.min() > margin - BOUND, (e, k, s, t, c.min())      # certified on [0, t)
            if s == sweep.FREE:
                assert t == 1.0
            elif s == sweep.HIT:
                assert clear_at(e, k, t) <= margin + slack + BOUND, (e, k, t)
            else:
                assert out["steps"][e, k] == max_steps and t < 1.0
            if out["pair"][e, k] >= 0:      # the closest sample is the mirror's clearance at t_min
                worst_c = max(worst_c, abs(out["dist"][e, k] - clear_at(e, k, tm)))
            else:
                assert out["dist"][e, k] == np.float32(S.DISTMAX_T) and (out["fromto"][e, k] == 0).all()
    print(f"fp32 sweep on the host, dofs {which}: worst |L - L_ref| / L_ref {worst_l:.3e} (bound 1e-5), worst |dist - c(t_min)| {worst_c:.3e} (bound {BOUND:.1e})")
    assert worst_l <= 1e-5 and worst_c <= BOUND
    seen = set(int(s) & 3 for s in st.ravel())
    assert seen >= ({sweep.FREE, sweep.HIT} if max_steps == 256 else {sweep.UNDECIDED})
