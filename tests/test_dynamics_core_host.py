"""Host rehearsal of the dynamics query kernels' fp32 core (robosuite_amd/csrc/rsim_dyn_core.h on rsim_grad_core.h on rsim_clear_core.h: the two walks and the
Jacobian columns k_dyn_rne / k_dyn_crb / k_dyn_jac run per candidate, behind the FK and joint walks) under AddressSanitizer + UndefinedBehaviorSanitizer:
tests/san/dyn_core_driver.cpp is built with g++ and run as a subprocess on scene D's tables and seeded draws at (5, 13).  Pass = the sanitizers report nothing,
every candidate returns, and the program's fp32 tau, M and J agree with the fp64 statement (robosuite_amd/dynamics.py) at the fp32-rounded inputs.

The bound, by reasoning, not from a run: dynamics_scenes.rounding_bound(bodies on the longest path, 2^-24) relative to the per-scene scales max |tau_ref|,
max |M_ref| and 1 for J -- scene D, four bodies: (31 * 4 + 39) * 8 * 2^-24 = 7.8e-5.  tests/test_dynamics.py holds the device, which runs the same source, to
the same bound.  M must be symmetric bit for bit.  Nothing sanitized is loaded into Python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from robosuite_amd import clearance, dynamics, mjcf
from tests import clearance_scenes as S
from tests import dynamics_scenes as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "san", "dyn_core_driver.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
_EXTRA = ("body_mass", "body_inertia", "body_ipos", "body_iquat", "dof_armature", "dof_damping", "_opt", "site_pos")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dyn_san") / "dyn_core_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", DRIVER, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def float_table(flat):
    """clearance_scenes.float_table with the tables the dynamics read behind it -> (float32 table, {field: offset}); "_opt" is laid out as the device's option
    block: timestep, gravity xyz"""
    off = dict(S.float_offsets(flat))
    parts, at = [S.float_table(flat)], off["_len"]
    for k in _EXTRA:
        a = np.concatenate([[float(flat.timestep)], np.asarray(flat.gravity, dtype=np.float64).ravel()]) if k == "_opt" else np.asarray(flat.arrays[k], dtype=np.float64).ravel()
        off[k] = at
        at += a.size
        parts.append(a.astype("<f4"))
    return np.concatenate(parts), off


def pack(flat, dofs, qpos, xp0, xq0, q, qd, qdd, site):
    tab, slot = S.body_table(flat, dofs)
    ft, off = float_table(flat)
    B, K, n = q.shape
    col, jt = clearance._columns(flat, dofs), clearance._I(flat, "jnt_type")
    slide = sum(1 << c for j, c in col.items() if jt[j] == mjcf.JNT_SLIDE)
    cols = np.zeros((n, 2), dtype="<i4")
    for e, el in enumerate(tab):
        if el[0] != 0 and el[4] >= 0:
            cols[el[4]] = (dofs[el[4]], e)
    body = int(clearance._I(flat, "site_bodyid")[site])
    head = struct.pack("<20i", B, K, n, int(flat.nbody), int(flat.nq), len(tab), int((slot >= 0).sum()), int(qd is not None), int(qdd is not None), body,
                       off["site_pos"] + 3 * site, slide, off["body_mass"], off["body_inertia"], off["body_ipos"], off["body_iquat"], off["dof_armature"],
                       off["dof_damping"], off["_opt"], len(ft))
    parts = [head, tab.astype("<i4").tobytes(), slot.astype("<i4").tobytes(), clearance.signatures(flat, dofs).astype("<i4").tobytes(), cols.tobytes(), ft.tobytes(),
             np.asarray(qpos, dtype="<f4").tobytes(), np.asarray(xp0, dtype="<f4").tobytes(), np.asarray(xq0, dtype="<f4").tobytes(), np.asarray(q, dtype="<f4").tobytes()]
    parts += [np.asarray(x, dtype="<f4").tobytes() for x in (qd, qdd) if x is not None]
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
    assert raw.size == N * (n + n * n + 6 * n)
    cut = np.cumsum([N * n, N * n * n, N * 3 * n])
    tau, M, jp, jr = np.split(raw, cut)
    return dict(tau=tau.reshape(B, K, n), M=M.reshape(B, K, n, n), jacp=jp.reshape(B, K, 3, n), jacr=jr.reshape(B, K, 3, n))


def poses(flat, qpos):
    m32 = dynamics.model32(flat)
    now = [mjcf.kinematics_np(m32, qpos[e])[:2] for e in range(len(qpos))]
    return S.f32(np.stack([p[0] for p in now])), S.f32(np.stack([p[1] for p in now]))


def rehearse(exe, tmp, which, site_name, rates=(True, True), B=5, K=13):
    """the program's results and the statement's for scene D -> (got, ref, bound)"""
    flat = D.scene_d()
    dofs = D.dofs_d(flat, which)
    site = flat.names["site"].index(site_name)
    qpos = S.f32(D.scene_d_qpos(flat, B))
    xp0, xq0 = poses(flat, qpos)
    q, qd, qdd = D.draws(flat, dofs, B, K)
    qd, qdd = qd if rates[0] else None, qdd if rates[1] else None
    got = run(exe, tmp, pack(flat, dofs, qpos, xp0, xq0, q, qd, qdd, site), B, K, len(dofs))
    return got, D.reference(flat, qpos, dofs, q, qd, qdd, site), D.rounding_bound(D.depth(flat, dofs), D.EPS32)


@pytest.mark.parametrize("which,site", (("arm", "tip"), ("all", "f1_s"), ("arm", "side_s")))
def test_scene_d_under_sanitizers(exe, tmp_path, which, site):
    got, ref, bound = rehearse(exe, tmp_path, which, site)
    for k, v in D.errors(got, ref).items():
        print(f"fp32 core on the host, scene D {which}, site {site}: {k} {v:.3e} (bound {bound:.1e})")
        assert v <= bound, (k, v)
    assert np.array_equal(got["M"], np.swapaxes(got["M"], -1, -2))      # both triangles from one product
    assert np.abs(ref["tau"]).max() > 5 and np.abs(ref["jacp"]).max() > 0.1


@pytest.mark.parametrize("rates", ((False, False), (True, False), (False, True)))
def test_absent_rates_are_zeros_under_sanitizers(exe, tmp_path, rates):
    got, ref, bound = rehearse(exe, tmp_path, "all", "tip", rates, B=2, K=3)
    assert D.errors(got, ref)["tau"] <= bound
