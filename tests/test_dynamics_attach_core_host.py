"""Host rehearsal of the fp32 core of the dynamics kernels with carried payloads (robosuite_amd/csrc/rsim_dyn_att_core.h on rsim_dyn_core.h: FK with
attachments, the joint walk, the attached RNE and CRB walks and the Jacobian, as k_clear_fk_att / k_clear_joints / k_dyn_rne_att / k_dyn_crb_att /
k_dyn_jac_att run them per candidate) under AddressSanitizer + UndefinedBehaviorSanitizer: tests/san/dyn_att_driver.cpp, a stand-alone program, is built with
g++ and run as a subprocess on the scenes of tests/dynamics_attach_scenes.py.  Pass = the sanitizers report nothing, every candidate returns, the program's
fp32 tau, M and J agree with the fp64 statement (robosuite_amd/dynamics.py with attach / held / rel) at the fp32-rounded tables, and M is symmetric bit for
bit.

The bound, by reasoning, not from a run: dynamics_scenes.rounding_bound(bodies on the longest path INCLUDING THE ATTACHED CHAIN, 2^-24) relative to the
per-scene scales -- scene P, l0 - l1 - l2 - load, as long as the finger chain: four bodies, (31 * 4 + 39) * 8 * 2^-24 = 7.8e-5; scene J, the arm's two and the
tool's three (tool - jaw - tip): 9.3e-5.  tests/test_dynamics_attach.py holds
the device, which runs the same source, to the same bound.  Nothing sanitized is loaded into Python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from robosuite_amd import clearance, mjcf
from tests import attach_scenes as A
from tests import clearance_scenes as S
from tests import dynamics_attach_scenes as P
from tests import dynamics_scenes as D
from tests.test_dynamics_core_host import ENV, float_table, poses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "san", "dyn_att_driver.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("dyn_att_san") / "dyn_att_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", DRIVER, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "asan" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("libasan / libubsan not installed")
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def pack(flat, dofs, attach, held, rel, qpos, xp0, xq0, q, qd, qdd, site):
    tab, slot, bsig, batt = A.attach_table(flat, dofs, attach)
    ft, off = float_table(flat)
    B, K, n = q.shape
    col, jt = clearance._columns(flat, dofs), clearance._I(flat, "jnt_type")
    slide = sum(1 << c for j, c in col.items() if jt[j] == mjcf.JNT_SLIDE)
    cols = np.zeros((n, 2), dtype="<i4")
    for e, el in enumerate(tab):
        if el[0] not in (0, 4) and el[4] >= 0:
            cols[el[4]] = (dofs[el[4]], e)
    body = 0 if site is None else int(clearance._I(flat, "site_bodyid")[site])
    head = struct.pack("<23i", B, K, n, int(flat.nbody), int(flat.nq), len(tab), int((slot >= 0).sum()), int(qd is not None), int(qdd is not None), body,
                       0 if site is None else off["site_pos"] + 3 * site, slide, off["body_mass"], off["body_inertia"], off["body_ipos"], off["body_iquat"],
                       off["dof_armature"], off["dof_damping"], off["_opt"], len(ft), len(attach), int(rel is not None), int(batt[body]))
    parts = [head, tab.astype("<i4").tobytes(), slot.astype("<i4").tobytes(), bsig.astype("<i4").tobytes(), cols.tobytes(), ft.tobytes(),
             np.asarray(qpos, dtype="<f4").tobytes(), np.asarray(xp0, dtype="<f4").tobytes(), np.asarray(xq0, dtype="<f4").tobytes(), np.asarray(q, dtype="<f4").tobytes()]
    parts += [np.asarray(x, dtype="<f4").tobytes() for x in (qd, qdd) if x is not None]
    parts.append(np.asarray(held, dtype=np.uint8).reshape(B, len(attach)).tobytes())
    if rel is not None:
        parts.append(np.asarray(rel, dtype="<f4").reshape(B, len(attach), 7).tobytes())
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
    tau, M, jp, jr = np.split(raw, np.cumsum([N * n, N * n * n, N * 3 * n]))
    return dict(tau=tau.reshape(B, K, n), M=M.reshape(B, K, n, n), jacp=jp.reshape(B, K, 3, n), jacr=jr.reshape(B, K, 3, n))


def rehearse_p(exe, tmp, mode, site_name, B=6, K=5, held=None):
    """the program's results and the statement's for scene P -> (got, ref, bound, held)"""
    flat = P.scene_p()
    dofs, attach = P.dofs_p(flat), P.attach_p(flat)
    held, rel = P.held_rows(B) if held is None else held, P.rel_of(mode, B)
    site = flat.names["site"].index(site_name)
    qpos = S.f32(P.scene_p_qpos(flat, B))
    xp0, xq0 = poses(flat, qpos)
    q, qd, qdd = D.draws(flat, dofs, B, K)
    got = run(exe, tmp, pack(flat, dofs, attach, held, rel, qpos, xp0, xq0, q, qd, qdd, site), B, K, len(dofs))
    ref = P.reference(flat, qpos, dofs, q, attach, held, rel, qd, qdd, site, now=(xp0, xq0))
    return got, ref, D.rounding_bound(P.depth_att(flat, dofs, attach), D.EPS32), held


def rehearse_j(exe, tmp, mode, B=4, K=5):
    flat = A.scene_j()
    dofs, attach, held = A.dofs_j(flat), A.attach_j(flat), A.held_rows_j(B)
    rel = None if mode == "state" else A.rel_given_j(B)
    qpos = S.f32(A.scene_j_qpos(flat, B))
    xp0, xq0 = poses(flat, qpos)
    q, qd, qdd = D.draws(flat, dofs, B, K)
    got = run(exe, tmp, pack(flat, dofs, attach, held, rel, qpos, xp0, xq0, q, qd, qdd, None), B, K, len(dofs))
    ref = P.reference(flat, qpos, dofs, q, attach, held, rel, qd, qdd, None, now=(xp0, xq0), want=("tau", "M"))
    return {k: got[k] for k in ("tau", "M")}, ref, D.rounding_bound(P.depth_att(flat, dofs, attach), D.EPS32)


@pytest.mark.parametrize("mode", P.REL_MODES)
@pytest.mark.parametrize("site", ("load_tip", "tip"))
def test_scene_p_under_sanitizers(exe, tmp_path, mode, site):
    got, ref, bound, held = rehearse_p(exe, tmp_path, mode, site)
    for k, v in D.errors(got, ref).items():
        print(f"fp32 attached core on the host, scene P {mode}, site {site}: {k} {v:.3e} (bound {bound:.1e})")
        assert v <= bound, (k, v)
    assert np.array_equal(got["M"], np.swapaxes(got["M"], -1, -2))      # both triangles from one product
    if site == "load_tip":
        assert not got["jacp"][~held[:, 0]].any() and not got["jacr"][~held[:, 0]].any() and got["jacp"][held[:, 0]].any()      # not held: zeros


@pytest.mark.parametrize("mode", A.REL_MODES)
def test_scene_j_subtree_under_sanitizers(exe, tmp_path, mode):
    got, ref, bound = rehearse_j(exe, tmp_path, mode)
    for k, v in D.errors(got, ref).items():
        print(f"fp32 attached core on the host, scene J {mode}: {k} {v:.3e} (bound {bound:.1e})")
        assert v <= bound, (k, v)
    assert np.array_equal(got["M"], np.swapaxes(got["M"], -1, -2))


def test_nothing_held_is_the_plain_core_bit_for_bit(exe, tmp_path):
    """the attached walks with every held row false against tests/san/dyn_core_driver.cpp's plain walks on the same scene: the same bits"""
    from tests import test_dynamics_core_host as H

    B, K = 3, 4
    got, _, _, _ = rehearse_p(exe, tmp_path, "given", "tip", B, K, held=np.zeros((B, 2), dtype=bool))
    plain_exe = str(tmp_path / "dyn_core_san")
    r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", H.DRIVER, "-o", plain_exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    flat = P.scene_p()
    dofs = P.dofs_p(flat)
    qpos = S.f32(P.scene_p_qpos(flat, B))
    xp0, xq0 = poses(flat, qpos)
    q, qd, qdd = D.draws(flat, dofs, B, K)
    plain = H.run(plain_exe, tmp_path, H.pack(flat, dofs, qpos, xp0, xq0, q, qd, qdd, flat.names["site"].index("tip")), B, K, len(dofs))
    assert all(np.array_equal(got[k], plain[k]) for k in plain)
