"""External forces (mjData.qfrc_applied / xfrc_applied) without a GPU: the C-ABI declares and exports the new field and entry, the Python field table
follows the enum, body names resolve with a loud error, and the numpy xfrc -> qfrc map the GPU parity tests drive the oracle with matches closed forms."""
import os
import re

import numpy as np
import pytest

from robosuite_amd import mjcf
from tests.util import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "rsim.h")).read()


def xfrc_to_qfrc(od, xfrc):
    """mj_xfrcAccumulate on the oracle: the generalised force of wrenches xfrc [nbody, 6] (force, torque; world frame, at each body's COM, xipos),
    from rso_jac_body (the Jacobian of the body ORIGIN, xpos): Jp^T f + Jr^T (torque + (xipos - xpos) x f).  Needs the kinematics of the current
    state (forward or step1)."""
    xfrc = np.asarray(xfrc, dtype=np.float64).reshape(-1, 6)
    xpos, xipos = np.asarray(od.xpos).reshape(-1, 3), np.asarray(od.xipos).reshape(-1, 3)
    q = np.zeros(od.nv)
    for b in np.nonzero(np.any(xfrc != 0, axis=1))[0]:
        jp, jr = od.jac("body", int(b))
        f, t = xfrc[b, :3], xfrc[b, 3:]
        q += jp.T @ f + jr.T @ (t + np.cross(xipos[b] - xpos[b], f))
    return q


def _enum_fields():
    body = HEADER[HEADER.index("enum rsim_field {"):]
    body = body[:body.index("};")]
    return re.findall(r"^\s*(RSIM_[A-Z_]+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S), flags=re.M)


def test_header_appends_xfrc_applied_and_declares_the_switch():
    names = _enum_fields()
    assert names[-1] == "RSIM_FIELD_COUNT" and names[-2] == "RSIM_XFRC_APPLIED"       # appended: no existing enum value moves
    assert names.index("RSIM_QFRC_APPLIED") == 34 and names.index("RSIM_POLISH") == 35
    assert re.search(r"int rsim_set_applied_forces\(rsim_batch\* b, int enable\);", HEADER)


def test_python_field_table_follows_the_enum():
    from robosuite_amd import backend
    names = [n for n in _enum_fields() if n != "RSIM_FIELD_COUNT"]
    assert [("RSIM_" + f).upper() for f in backend.FIELDS] == names
    assert backend.FIELD_ID["xfrc_applied"] == names.index("RSIM_XFRC_APPLIED")


def test_library_exports_the_switch():
    from robosuite_amd import backend
    lib = os.path.join(ROOT, "robosuite_amd", "librsim_hip.so")
    if not os.path.exists(lib):
        pytest.skip("library not built")
    assert hasattr(backend.lib(), "rsim_set_applied_forces")


def test_body_wrench_names_resolve_or_raise():
    from robosuite_amd.vec_env import body_wrench_id
    flat = mjcf.load_model(os.path.join(ROOT, "robosuite_amd", "assets", "lift_panda.rsim"))
    assert body_wrench_id(flat, "cube_main") == flat.nbody - 1
    assert body_wrench_id(flat, "robot0_link3") == flat.name2id("body", "robot0_link3") > 0
    with pytest.raises(KeyError):
        body_wrench_id(flat, "no_such_body")


def test_shim_exposes_xfrc_applied_per_body():
    from robosuite_amd import shim
    assert "xfrc_applied" in shim._DATA_FIELDS and shim._DATA_SHAPES["xfrc_applied"] == 6


def _arm2_box():
    from oracle.oracle import OracleData, OracleModel
    flat = mjcf.compile_mjcf(open(os.path.join(GOLD, "arm2_box.xml")).read())
    om = OracleModel(mjcf.to_blob(flat))
    od = OracleData(om)
    rng = np.random.default_rng(3)
    od.qpos[:3] = [0.4, -0.3, 0.05]
    fq = int(flat.arrays["jnt_qposadr"][flat.name2id("joint", "box_free")])
    qb = rng.normal(size=4)
    od.qpos[fq:fq + 3] = [0.2, 0.3, 0.4]
    od.qpos[fq + 3:fq + 7] = qb / np.linalg.norm(qb)
    od.forward()
    return flat, od, rng


def test_xfrc_of_the_free_box_is_force_and_body_frame_torque():
    """A free joint's dofs: translation in the world frame, rotation in the body frame -- so a wrench at the COM maps to (f, R^T torque)."""
    flat, od, rng = _arm2_box()
    b = flat.name2id("body", "box")
    da = int(flat.arrays["jnt_dofadr"][flat.name2id("joint", "box_free")])
    w = np.zeros((flat.nbody, 6))
    w[b] = rng.normal(size=6)
    q = xfrc_to_qfrc(od, w)
    R = np.asarray(od.xmat).reshape(-1, 3, 3)[b]
    np.testing.assert_allclose(q[da:da + 3], w[b, :3], atol=1e-12)
    np.testing.assert_allclose(q[da + 3:da + 6], R.T @ w[b, 3:], atol=1e-12)
    assert np.abs(np.delete(q, np.arange(da, da + 6))).max() == 0.0


def test_xfrc_on_a_link_gives_the_hinge_its_axis_moment():
    """Hinge j1 carries every link: the wrench on link3 (a slide body with an offset, rotated COM) gives j1 axis . (torque + (xipos - anchor) x f)."""
    flat, od, rng = _arm2_box()
    b = flat.name2id("body", "link3")
    j = flat.name2id("joint", "j1")
    w = np.zeros((flat.nbody, 6))
    w[b] = rng.normal(size=6)
    q = xfrc_to_qfrc(od, w)
    xmat, xpos = np.asarray(od.xmat).reshape(-1, 3, 3), np.asarray(od.xpos).reshape(-1, 3)
    l1 = flat.name2id("body", "link1")
    ax, anc = xmat[l1] @ flat.arrays["jnt_axis"][j], xpos[l1] + xmat[l1] @ flat.arrays["jnt_pos"][j]
    xip = np.asarray(od.xipos).reshape(-1, 3)[b]
    want = ax @ (w[b, 3:] + np.cross(xip - anc, w[b, :3]))
    np.testing.assert_allclose(q[int(flat.arrays["jnt_dofadr"][j])], want, rtol=1e-10, atol=1e-12)
    # the slide j3 (on link3 itself) takes the force along its axis only
    j3 = flat.name2id("joint", "j3")
    np.testing.assert_allclose(q[int(flat.arrays["jnt_dofadr"][j3])], (xmat[b] @ flat.arrays["jnt_axis"][j3]) @ w[b, :3], rtol=1e-10, atol=1e-12)
