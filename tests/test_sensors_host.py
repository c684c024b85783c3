"""Sensors beyond force / torque, the parts that need no GPU: both MJCF compilers agree on the new sensor tables, models without such a sensor compile to the
blob they always compiled to, the library reports what reads zero, and the fp64 host mirror (robosuite_amd/sensors.py) -- the reference of the GPU tests in
tests/test_sensors.py -- is held to closed forms of rigid-body kinematics and to central differences of its own position-stage outputs.

MuJoCo semantics [3P, docs "XML reference: sensor"]."""
import hashlib
import os
import warnings

import numpy as np
import pytest

from robosuite_amd import backend, mjcf, sensors
from tests import sensors_scenes as S
from tests.test_mjcf_cpp import compare

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
G = 9.81
# sha256 of the blobs rsim_mjcf_to_blob compiled from tests/golden/{arm2_box,coupled_fingers}.xml on the commit BEFORE the sensor tables existed
PARENT_SHA = {"arm2_box": "5ace50c3456625b204faa47895f82a870dc351788ada2895f0299096e07774d9",
              "coupled_fingers": "312839d982162bad1ffe22a25f999386773fba13f78cfbf50a43790411ca2b62"}


def _slices(flat):
    adr = np.concatenate([[0], np.cumsum(np.asarray(flat.arrays["sensor_dim"]).ravel())]).astype(int)
    return {n: slice(adr[i], adr[i + 1]) for i, n in enumerate(flat.names["sensor"])}


# ---- compilers, status, blobs --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ("ARM_XML", "FINGERS_XML", "MIXED_XML", "ONLY_ZERO_XML", "ARM_FT_ONLY"))
def test_compilers_agree(scene):
    ref, new, _ = compare(getattr(S, scene))       # every int32 array bit-equal, same entry table: codes, ids, dims, kinds, reasons, shapes
    extra = [k for k in ref.arrays if k in ("sensor_objtype", "sensor_reason", "sensor_shape")]
    assert extra == ([] if scene == "ARM_FT_ONLY" else ["sensor_objtype", "sensor_reason", "sensor_shape"])
    for m in (ref, new):
        assert len(m.arrays["sensor_type"]) == len(m.arrays["sensor_objid"]) == len(m.arrays["sensor_dim"]) == int(m.nsensor)


def test_codes_dims_and_objects_of_every_carried_type():
    flat = mjcf.compile_mjcf(S.ARM_XML)
    fing = mjcf.compile_mjcf(S.FINGERS_XML)
    seen = {}
    for m in (flat, fing):
        for n, t, d, o, k, r in zip(m.names["sensor"], m.sensor_type, m.sensor_dim, m.sensor_objid, m.arrays.get("sensor_objtype"), m.arrays.get("sensor_reason")):
            assert r == 0 and o >= 0, n
            seen.setdefault(mjcf.SENSOR_TYPE_NAMES[int(t)], set()).add(int(d))
    assert set(seen) == set(mjcf.SENSOR_TYPES)       # force, torque and the thirteen further types
    want = {"force": 3, "torque": 3, "jointpos": 1, "tendonpos": 1, "framepos": 3, "framequat": 4, "jointvel": 1, "tendonvel": 1, "velocimeter": 3, "gyro": 3,
            "framelinvel": 3, "frameangvel": 3, "accelerometer": 3, "touch": 1, "actuatorfrc": 1}
    assert {k: v for k, v in seen.items()} == {k: {v} for k, v in want.items()}
    sid = {n: i for i, n in enumerate(flat.names["sensor"])}
    assert flat.sensor_type[sid["s_force"]] == 0 and flat.sensor_type[sid["s_torque"]] == 1                  # the frozen oracle reads these two codes
    assert flat.sensor_objid[sid["s_force"]] == flat.names["site"].index("eef")
    assert flat.sensor_objid[sid["s_fp_body"]] == flat.names["body"].index("link3") and flat.sensor_objtype[sid["s_fp_body"]] == mjcf.SENSOR_OBJ_BODY
    assert flat.sensor_objtype[sid["s_fp_xbody"]] == mjcf.SENSOR_OBJ_XBODY and flat.sensor_objtype[sid["s_fp_site"]] == mjcf.SENSOR_OBJ_SITE
    assert flat.sensor_objid[sid["s_af"]] == flat.names["actuator"].index("p3") and flat.sensor_shape[sid["s_touch"]] == mjcf.GEOM_BOX


def test_status_names_exactly_the_sensors_that_read_zero():
    hm = backend.HipModel.from_xml_string(S.MIXED_XML)
    status = hm.sensor_status()
    assert {n: r for n, _, carried, r in status if not carried} == S.NOT_CARRIED
    assert [n for n, _, carried, _ in status if carried] == ["ok_pos", "ok_touch", "ok_force"]
    assert hm.int("nsensor_zero") == len(S.NOT_CARRIED) and hm.int("nsensor") == 11
    assert [t for _, t, _, _ in status][:3] == ["other", "jointpos", "framepos"]
    z = backend.HipModel.from_xml_string(S.ONLY_ZERO_XML)
    assert z.int("nsensor_zero") == z.int("nsensor") == 3
    ft = backend.HipModel.from_xml_string(S.ARM_FT_ONLY)
    assert ft.int("nsensor_zero") == 0 and all(c for _, _, c, _ in ft.sensor_status())


def test_sensor_slice_matches_the_cumulative_dims():
    for xml in (S.ARM_XML, S.MIXED_XML):
        hm = backend.HipModel.from_xml_string(xml)
        sl = _slices(hm.flat)
        for n, _, carried, _ in hm.sensor_status():
            adr, dim, c = hm.sensor_slice(n)
            assert (adr, adr + dim) == (sl[n].start, sl[n].stop) and c == carried
        assert hm.int("nsensordata") == max(s.stop for s in sl.values())
    with pytest.raises(KeyError):
        hm.sensor_slice("no_such_sensor")
    import ctypes as C
    assert backend.lib().rsim_sensor_slice(hm.ptr, 99, None, None, None) != 0 and b"out of range" in backend.lib().rsim_last_error()
    a = C.c_int()
    assert backend.lib().rsim_sensor_slice(hm.ptr, 1, C.byref(a), None, None) == 0 and a.value == 1


@pytest.mark.parametrize("name", sorted(PARENT_SHA))
def test_models_without_new_sensors_keep_their_blob(name):
    xml = open(os.path.join(GOLD, name + ".xml")).read()
    assert hashlib.sha256(backend.compile_mjcf_blob(xml)).hexdigest() == PARENT_SHA[name]
    assert not [k for k in mjcf.compile_mjcf(xml).arrays if k in ("sensor_objtype", "sensor_reason", "sensor_shape")]


def test_force_torque_only_model_has_the_old_entry_table():
    flat = mjcf.compile_mjcf(S.ARM_FT_ONLY)
    plain = mjcf.compile_mjcf(S.ARM_PLAIN)
    assert list(flat.arrays) == list(plain.arrays)
    assert list(flat.sensor_type) == [0, 1] and list(flat.sensor_objid) == [flat.names["site"].index("eef")] * 2


@pytest.mark.parametrize("rsim", ("lift_panda.rsim", "pickplace_iiwa.rsim"))
def test_shipped_blobs_still_load(rsim):
    path = os.path.join(os.path.dirname(backend.__file__), "assets", rsim)
    hm = backend.HipModel(open(path, "rb").read())
    assert hm.int("nsensor_zero") == 0
    assert all(c and t in ("force", "torque") for _, t, c, _ in hm.sensor_status())


def test_blob_with_a_bad_object_id_is_not_trusted():
    flat = mjcf.compile_mjcf(S.ARM_XML)
    sid = flat.names["sensor"].index("s_jp")
    flat.arrays["sensor_objid"][sid] = 1000
    hm = backend.HipModel(flat)
    assert hm.int("nsensor_zero") == 1 and hm.sensor_slice("s_jp")[2] is False


def test_blob_with_an_actuator_on_a_free_joint_is_not_trusted():
    """actuatorfrc reads one coordinate and one rate of the transmission joint: a hand-edited blob whose actuator sits on a free joint reads zero instead"""
    flat = mjcf.compile_mjcf(S.ARM_XML)
    act = int(flat.arrays["sensor_objid"][flat.names["sensor"].index("s_af")])
    flat.arrays["actuator_trnid"][act] = flat.names["joint"].index("box_free")
    hm = backend.HipModel(flat)
    assert hm.int("nsensor_zero") == 1 and hm.sensor_slice("s_af")[2] is False and hm.sensor_slice("s_af1")[2] is True


def test_shim_warns_once_about_sensors_that_read_zero(monkeypatch):
    from robosuite_amd import hip_shim_backend as hs

    class _NoBatch:
        def __init__(self, *a, **k):
            pass

    monkeypatch.setattr(hs, "HipBatch", _NoBatch)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        be = hs.HipShimBackend(mjcf.compile_mjcf(S.MIXED_XML))
    assert len(w) == 1 and all(f"'{n}' ({r})" in str(w[0].message) for n, r in S.NOT_CARRIED.items()) and "ok_pos" not in str(w[0].message)
    sl = _slices(be.flat)
    pulled = set(int(i) for i in be._posvel)      # step1 pulls the position- and velocity-stage entries, never an acceleration-stage one
    assert sl["ok_pos"].start in pulled and not pulled & set(range(sl["ok_touch"].start, sl["ok_touch"].stop)) | pulled & set(range(sl["ok_force"].start, sl["ok_force"].stop))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        hs.HipShimBackend(mjcf.compile_mjcf(S.ARM_FT_ONLY))
        hs.HipShimBackend(mjcf.compile_mjcf(S.ARM_XML))
    assert not w


# ---- the mirror against closed forms (fp64, 1e-10 relative) -------------------------------------------------------------------------------------------
def _close(got, want, rel=1e-10):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.abs(got - want).max() <= rel * max(1.0, np.abs(want).max()), (got, want)


def test_mirror_pendulum_closed_forms():
    L, th, om, al = 0.37, 0.83, -1.7, 2.9
    flat = mjcf.compile_mjcf(f"""<mujoco><compiler angle="radian"/><worldbody><body name="p" pos="0.2 -0.1 1"><joint name="h" type="hinge" axis="0 1 0"/>
        <geom type="sphere" size="0.02" pos="0 0 -{L}" mass="0.5"/><site name="tip" pos="0 0 -{L}"/></body></worldbody>
        <sensor><gyro name="gy" site="tip"/><velocimeter name="ve" site="tip"/><accelerometer name="ac" site="tip"/><framepos name="fp" objtype="site" objname="tip"/>
        <framequat name="fq" objtype="site" objname="tip"/><jointpos name="jp" joint="h"/><jointvel name="jv" joint="h"/><framelinvel name="lv" objtype="site" objname="tip"/>
        <frameangvel name="av" objtype="xbody" objname="p"/></sensor></mujoco>""")
    sl = _slices(flat)
    sd = sensors.sensor_values(flat, [th], [om], [al], [])
    s, c = np.sin(th), np.cos(th)
    _close(sd[sl["gy"]], [0, om, 0])
    _close(sd[sl["ve"]], [-L * om, 0, 0])
    _close(sd[sl["ac"]], [-L * al - G * s, 0, L * om * om + G * c])          # tangential + centripetal - g, in the site frame
    _close(sd[sl["fp"]], [0.2 - L * s, -0.1, 1 - L * c])
    _close(sd[sl["fq"]], [np.cos(th / 2), 0, np.sin(th / 2), 0])
    _close(sd[sl["jp"]], [th]); _close(sd[sl["jv"]], [om])
    _close(sd[sl["lv"]], [-L * om * c, 0, L * om * s])
    _close(sd[sl["av"]], [0, om, 0])
    rest = sensors.sensor_values(flat, [0.0], [0.0], [0.0], [])
    _close(rest[sl["ac"]], [0, 0, G])                                        # at rest: +|g| along world z


def test_mirror_spinning_free_body_in_free_fall():
    flat = mjcf.compile_mjcf("""<mujoco><worldbody><body name="b" pos="0 0 1"><freejoint/><geom type="box" size="0.1 0.2 0.3"/>
        <site name="s" pos="0.11 -0.07 0.05"/></body></worldbody><sensor><accelerometer name="ac" site="s"/><gyro name="gy" site="s"/>
        <velocimeter name="ve" site="s"/><framelinvel name="lv" objtype="xbody" objname="b"/></sensor></mujoco>""")
    sl = _slices(flat)
    q = np.array([0.7, -0.4, 0.2, 0.3])
    q /= np.linalg.norm(q)
    R = mjcf.quat2mat(q)
    r, w, v = np.array([0.11, -0.07, 0.05]), np.array([0, 0, 4.2]), np.array([0.3, -0.5, 0.9])     # spin about the body's z axis (principal: a box)
    sd = sensors.sensor_values(flat, np.concatenate([[0.1, 0.2, 1.3], q]), np.concatenate([v, w]), [0, 0, -G, 0, 0, 0], [])
    _close(sd[sl["ac"]], np.cross(w, np.cross(w, r)))
    _close(sd[sl["gy"]], w)
    _close(sd[sl["ve"]], R.T @ v + np.cross(w, r))
    _close(sd[sl["lv"]], v)


def test_mirror_tendons_and_actuator_force():
    flat = mjcf.compile_mjcf(S.FINGERS_XML)
    sl = _slices(flat)
    qpos, qvel = np.array([0.3, -0.2, 0.45]), np.array([1.1, 0.7, -0.9])
    sd = sensors.sensor_values(flat, qpos, qvel, np.zeros(3), [0.4, 0.0])
    _close(sd[sl["t_pos"]], [0.3 + 1.5 * -0.2]); _close(sd[sl["t_vel"]], [1.1 + 1.5 * 0.7])
    _close(sd[sl["t2_pos"]], [2 * 0.45]); _close(sd[sl["t2_vel"]], [2 * -0.9])
    _close(sd[sl["a1_frc"]], [20 * 0.4 - 20 * 0.3])
    arm = mjcf.compile_mjcf(S.ARM_XML)
    sl = _slices(arm)
    q = np.asarray(arm.qpos0, dtype=np.float64).ravel().copy()
    q[2] = 0.02
    _close(sensors.sensor_values(arm, q, np.zeros(arm.nv), np.zeros(arm.nv), [3.0, 0, 0.05])[sl["s_af"]], [200 * 0.05 - 200 * 0.02])     # inside forcerange
    q[2] = -0.2
    sd = sensors.sensor_values(arm, q, np.zeros(arm.nv), np.zeros(arm.nv), [30.0, 0, 0.5])
    _close(sd[sl["s_af"]], [30.0])                     # ctrl clipped to 0.1: 200 * 0.1 + 200 * 0.2 = 60, beyond forcerange 30
    _close(sd[sl["s_af1"]], [20.0])                    # motor: ctrl clipped to its range, no forcerange


# ---- the mirror against central differences of its own position stage ------------------------------------------------------------------------------------
def test_mirror_velocity_and_acceleration_are_derivatives_of_position():
    flat = mjcf.compile_mjcf(S.ARM_XML)
    sl = _slices(flat)
    rng = np.random.default_rng(5)
    q0 = np.asarray(flat.qpos0, dtype=np.float64).ravel().copy()
    q0[:3] = [0.7, -0.5, 0.04]
    v0, a0 = np.zeros(flat.nv), np.zeros(flat.nv)
    v0[:3], a0[:3] = rng.uniform(-2, 2, 3), rng.uniform(-5, 5, 3)
    h = 1e-4

    def at(t):
        q, v = q0.copy(), v0 + a0 * t
        q[:3] += v0[:3] * t + 0.5 * a0[:3] * t * t
        return sensors.sensor_values(flat, q, v, a0, np.zeros(flat.nu))

    s0, sp, sm = at(0.0), at(h), at(-h)
    dpos = (sp[sl["s_fp_site"]] - sm[sl["s_fp_site"]]) / (2 * h)
    assert np.abs(dpos - s0[sl["s_flv"]]).max() <= 1e-6 * np.abs(s0[sl["s_flv"]]).max()
    dvel = (sp[sl["s_flv"]] - sm[sl["s_flv"]]) / (2 * h)
    R = mjcf.quat2mat(s0[sl["s_fq_site"]])
    want = R.T @ (dvel - np.array([0, 0, -G]))
    assert np.abs(want - s0[sl["s_acc"]]).max() <= 1e-6 * np.abs(s0[sl["s_acc"]]).max()
    _close(s0[sl["s_vel"]], R.T @ s0[sl["s_flv"]])


# ---- touch geometry -----------------------------------------------------------------------------------------------------------------------------
def test_mirror_touch_geometry():
    flat = mjcf.compile_mjcf("""<mujoco><worldbody><geom name="floor" type="plane" size="1 1 .1"/>
        <body name="a" pos="0 0 0.5"><freejoint/><geom name="ga" type="box" size=".1 .1 .1"/>
          <site name="sb" type="box" size="0.1 0.1 0.02" pos="0 0 -0.1"/><site name="ss" type="sphere" size="0.05" pos="0 0 -0.1"/></body>
        <body name="o" pos="1 0 0.5"><freejoint/><geom name="go" type="sphere" size=".1"/></body></worldbody>
        <sensor><touch name="tb" site="sb"/><touch name="ts" site="ss"/></sensor></mujoco>""")
    sl = _slices(flat)
    floor, ga, go = (flat.names["geom"].index(n) for n in ("floor", "ga", "go"))
    up = np.array([[0, 0, 1.0], [1, 0, 0], [0, 1, 0]])
    down = np.array([[0, 0, -1.0], [1, 0, 0], [0, -1, 0]])
    con = lambda pos, g1, g2, fn, frame=up, efc=0: dict(pos=np.array(pos, dtype=float), frame=frame, geom1=g1, geom2=g2, efc_address=efc, normal_force=fn, dim=3)
    contacts = [con([0.05, 0, 0.39], floor, ga, 2.0),            # inside the box zone; outside the sphere and its ray (towards the body's own surface: -z) leaves
                con([0, 0, 0.5], floor, ga, 3.0),                # above both zones, the ray -z passes through both
                con([0, 0, 0.3], floor, ga, 5.0),                # below both, the ray leaves
                con([0, 0, 0.4], floor, go, 7.0),                # inside, but a contact of another body
                con([0, 0, 0.4], floor, ga, 11.0, efc=-1),       # inside, but inactive
                con([0, 0, 0.45], ga, go, 13.0, frame=down)]     # the body's geom is geom1: the ray follows the normal (-z) through both
    sd = sensors.sensor_values(flat, flat.qpos0, np.zeros(flat.nv), np.zeros(flat.nv), [], contacts)
    assert sd[sl["tb"]] == 2.0 + 3.0 + 13.0 and sd[sl["ts"]] == 3.0 + 13.0
    assert not sensors.sensor_values(flat, flat.qpos0, np.zeros(flat.nv), np.zeros(flat.nv), [], []).any()
