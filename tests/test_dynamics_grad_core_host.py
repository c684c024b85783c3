"""Host rehearsal of the fp32 core of the dynamics derivatives (robosuite_amd/csrc/rsim_dyn_grad_core.h on the untouched rsim_dyn_core.h: the tangent walk
k_dyn_rne_grad / k_dyn_rne_jvp run per candidate, behind the FK, joint and Newton-Euler walks) under AddressSanitizer + UndefinedBehaviorSanitizer:
tests/san/dyn_grad_core_driver.cpp, a stand-alone program with its own main, is built with g++ exactly as tests/test_dynamics_core_host.py builds its driver
and run as a subprocess on scene D's tables and seeded draws at (5, 13).  Pass = the sanitizers report nothing, every candidate returns, and the program's fp32
dtau_dq, dtau_dqd and JVP agree with the fp64 statement by the definition of a derivative (robosuite_amd/dynamics.py) at the fp32-rounded inputs.

The bound, by reasoning, not from a run: dynamics_grad_scenes.tangent_rounding_bound(bodies on the longest path, 2^-24) relative to the per-scene scales
max |dtau_dq_ref| and max |dtau_dqd_ref| -- scene D, four bodies: (50 * 4 + 56) * 4 * 2^-24 = 6.1e-5.  tests/test_dynamics_grad.py holds the device, which
runs the same source, to the same bound.  Nothing sanitized is loaded into Python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from robosuite_amd import clearance, mjcf
from tests import clearance_scenes as S
from tests import dynamics_grad_scenes as G
from tests import dynamics_scenes as D
from tests.test_dynamics_core_host import ENV, float_table, poses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "san", "dyn_grad_core_driver.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dyn_grad_san") / "dyn_grad_core_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", DRIVER, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def pack(flat, dofs, qpos, xp0, xq0, q, rest):
    """rest: (qd, qdd, dq, dqd, dqdd), each [B, K, n] or None"""
    tab, slot = S.body_table(flat, dofs)
    ft, off = float_table(flat)
    B, K, n = q.shape
    col, jt = clearance._columns(flat, dofs), clearance._I(flat, "jnt_type")
    slide = sum(1 << c for j, c in col.items() if jt[j] == mjcf.JNT_SLIDE)
    cols = np.zeros((n, 2), dtype="<i4")
    for e, el in enumerate(tab):
        if el[0] != 0 and el[4] >= 0:
            cols[el[4]] = (dofs[el[4]], e)
    head = struct.pack("<21i", B, K, n, int(flat.nbody), int(flat.nq), len(tab), int((slot >= 0).sum()), *[int(x is not None) for x in rest], slide,
                       off["body_mass"], off["body_inertia"], off["body_ipos"], off["body_iquat"], off["dof_armature"], off["dof_damping"], off["_opt"], len(ft))
    parts = [head, tab.astype("<i4").tobytes(), slot.astype("<i4").tobytes(), cols.tobytes(), ft.tobytes(), np.asarray(qpos, dtype="<f4").tobytes(),
             np.asarray(xp0, dtype="<f4").tobytes(), np.asarray(xq0, dtype="<f4").tobytes(), np.asarray(q, dtype="<f4").tobytes()]
    parts += [np.asarray(x, dtype="<f4").tobytes() for x in rest if x is not None]
    return b"".join(parts)


def run(exe, tmp, blob, B, K, n):
    fin, fout = os.path.join(str(tmp), "scene.bin"), os.path.join(str(tmp), "out.bin")
    with open(fin, "wb") as f:
        f.write(blob)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300, env=ENV)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-300:], r.stderr[-4000:])       # no sanitizer finding, no crash
    assert f"candidates: {B * K} of {B * K}" in r.stdout                                          # every candidate returned
    raw = np.fromfile(fout, dtype="<f4")
    N = B * K
    assert raw.size == N * (2 * n + 4 * n * n)
    tau, gq, gv, ngq, ngv, jvp = np.split(raw, np.cumsum([N * n] + [N * n * n] * 4))
    sq = (B, K, n, n)
    return dict(tau=tau.reshape(B, K, n), dtau_dq=gq.reshape(sq), dtau_dqd=gv.reshape(sq), neg_dq=ngq.reshape(sq), neg_dqd=ngv.reshape(sq), jvp=jvp.reshape(B, K, n))


def rehearse(exe, tmp, which, rates=(True, True), B=5, K=13, dirs=(True, True, True)):
    """the program's results and the statement's for scene D -> (got, ref, bound)"""
    flat = D.scene_d()
    dofs = D.dofs_d(flat, which)
    qpos = S.f32(D.scene_d_qpos(flat, B))
    xp0, xq0 = poses(flat, qpos)
    q, qd, qdd = D.draws(flat, dofs, B, K)
    qd, qdd = qd if rates[0] else None, qdd if rates[1] else None
    d = tuple(x if on else None for x, on in zip(G.directions(B, K, len(dofs)), dirs))
    got = run(exe, tmp, pack(flat, dofs, qpos, xp0, xq0, q, (qd, qdd) + d), B, K, len(dofs))
    ref = G.reference(flat, qpos, dofs, q, qd, qdd)
    ref["jvp"] = G.reference_jvp(flat, qpos, dofs, q, qd, qdd, *d)
    ref["jvp_scale"] = G.jvp_scale(ref, D.reference(flat, qpos, dofs, q, want=("M",))["M"], len(dofs))
    return got, ref, G.tangent_rounding_bound(D.depth(flat, dofs), D.EPS32)


def held(what, got, ref, bound):
    for k, v in G.errors(got, ref).items():
        print(f"fp32 tangent core on the host, {what}: {k} {v:.3e} (bound {bound:.1e})")
        assert v <= bound, (what, k, v)
    assert np.array_equal(got["neg_dq"], -got["dtau_dq"]) and np.array_equal(got["neg_dqd"], -got["dtau_dqd"])      # the negate flag: the same bits, signed


@pytest.mark.parametrize("which", ("arm", "all"))
def test_scene_d_under_sanitizers(exe, tmp_path, which):
    got, ref, bound = rehearse(exe, tmp_path, which)
    held(f"scene D {which}", got, ref, bound)
    assert np.abs(ref["dtau_dq"]).max() > 5 and np.abs(ref["dtau_dqd"]).max() > 2
    tau = D.reference(D.scene_d(), S.f32(D.scene_d_qpos(D.scene_d(), 5)), D.dofs_d(D.scene_d(), which), *D.draws(D.scene_d(), D.dofs_d(D.scene_d(), which), 5, 13),
                      want=("tau",))["tau"]
    assert np.abs(got["tau"] - tau).max() <= D.rounding_bound(4, D.EPS32) * np.abs(tau).max()      # the primal walk in front is rsim_dyn_core.h's


@pytest.mark.parametrize("rates", ((False, False), (True, False), (False, True)))
def test_absent_rates_are_zeros_under_sanitizers(exe, tmp_path, rates):
    got, ref, bound = rehearse(exe, tmp_path, "all", rates, B=2, K=3)
    held(f"scene D all, qd {rates[0]}, qdd {rates[1]}", got, ref, bound)


@pytest.mark.parametrize("dirs", ((True, False, False), (False, True, False), (False, False, True)))
def test_absent_directions_are_zeros_under_sanitizers(exe, tmp_path, dirs):
    got, ref, bound = rehearse(exe, tmp_path, "all", B=2, K=3, dirs=dirs)
    assert np.abs(ref["jvp"]).max() > 0.5
    assert G.errors(dict(jvp=got["jvp"]), ref)["jvp"] <= bound
