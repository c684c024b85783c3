"""Scenes shared by tests/test_sensors_host.py (CPU) and tests/test_sensors.py (GPU): the golden test models plus <sensor> blocks."""
import os

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _read(name):
    return open(os.path.join(GOLD, name)).read()


# arm2_box.xml + a touch pad under the box (a box site that encloses the floor contacts) + every carried type, dims interleaved (1, 1, 4, 3, ...)
ARM_SENSORS = """<sensor>
    <jointpos name="s_jp" joint="j2"/>
    <touch name="s_touch" site="box_pad"/>
    <framequat name="s_fq_site" objtype="site" objname="eef"/>
    <force name="s_force" site="eef"/>
    <jointvel name="s_jv" joint="j3"/>
    <framepos name="s_fp_site" objtype="site" objname="eef"/>
    <torque name="s_torque" site="eef"/>
    <gyro name="s_gyro" site="eef"/>
    <actuatorfrc name="s_af" actuator="p3"/>
    <velocimeter name="s_vel" site="eef"/>
    <framepos name="s_fp_xbody" objtype="xbody" objname="link3"/>
    <framepos name="s_fp_body" objtype="body" objname="link3"/>
    <framequat name="s_fq_body" objtype="body" objname="link3"/>
    <framequat name="s_fq_xbody" objtype="xbody" objname="box"/>
    <framelinvel name="s_flv" objtype="site" objname="eef"/>
    <frameangvel name="s_fav" objtype="body" objname="link2"/>
    <framelinvel name="s_flv_box" objtype="body" objname="box"/>
    <frameangvel name="s_fav_box" objtype="xbody" objname="box"/>
    <accelerometer name="s_acc" site="eef"/>
    <actuatorfrc name="s_af1" actuator="m1"/>
    <accelerometer name="s_acc_box" site="box_pad"/>
    <gyro name="s_gyro_box" site="box_site"/>
    <velocimeter name="s_vel_box" site="box_pad"/>
    <touch name="s_touch_far" site="box_site"/>
  </sensor>"""
ARM_PAD = '<site name="box_pad" type="box" size="0.07 0.05 0.01" pos="0 0 -0.05" euler="0 0 0.3"/>'
ARM_PLAIN = _read("arm2_box.xml")
ARM_FT_ONLY = ARM_PLAIN.replace("</mujoco>", '<sensor><force name="s_force" site="eef"/><torque name="s_torque" site="eef"/></sensor></mujoco>')
ARM_FT_PAD = ARM_FT_ONLY.replace('<site name="box_site"', ARM_PAD + '\n      <site name="box_site"')      # the same bodies, geoms and sites as ARM_XML, force / torque only
ARM_XML = ARM_PLAIN.replace('<site name="box_site"', ARM_PAD + '\n      <site name="box_site"').replace("</mujoco>", ARM_SENSORS + "\n</mujoco>")
assert ARM_PAD in ARM_XML and ARM_SENSORS in ARM_XML

FINGERS_SENSORS = """<sensor>
    <tendonpos name="t_pos" tendon="cpl"/>
    <jointvel name="j_vel" joint="f1b_j"/>
    <tendonvel name="t_vel" tendon="cpl"/>
    <framequat name="tip_quat" objtype="xbody" objname="f1b"/>
    <tendonpos name="t2_pos" tendon="lim_only"/>
    <tendonvel name="t2_vel" tendon="lim_only"/>
    <actuatorfrc name="a1_frc" actuator="a1"/>
    <jointpos name="j_pos" joint="free_j"/>
    <frameangvel name="tip_w" objtype="body" objname="f1b"/>
  </sensor>"""
FINGERS_PLAIN = _read("coupled_fingers.xml")
FINGERS_XML = FINGERS_PLAIN.replace("</mujoco>", FINGERS_SENSORS + "\n</mujoco>")

# one of each case that is NOT carried (compiles, reads zero, is reported) beside two carried ones
NOT_CARRIED = {"mag": "sensor type not carried", "ref": "reftype / refname not carried", "geomframe": "objtype not carried (site, xbody, body only)",
               "captouch": "touch site shape not carried (sphere, ellipsoid, box only)", "freepos": "joint is not a hinge or slide", "cut": "non-zero cutoff not carried",
               "ballpos": "joint is not a hinge or slide", "nowhere": "object not found"}
MIXED_XML = """<mujoco><worldbody><geom name="floor" type="plane" size="1 1 0.1"/>
    <body name="a" pos="0 0 0.5"><joint name="h" type="hinge" axis="0 1 0"/><geom name="ga" type="sphere" size="0.05"/>
      <site name="pad" type="capsule" size="0.01 0.02"/><site name="ell" type="ellipsoid" size="0.01 0.02 0.03"/></body>
    <body name="f" pos="0.5 0 0.5"><freejoint name="ff"/><geom name="gf" type="box" size="0.05 0.05 0.05"/></body>
    <body name="bl" pos="1 0 0.5"><joint name="bj" type="ball"/><geom name="gb" type="sphere" size="0.05"/></body></worldbody>
  <sensor>
    <magnetometer name="mag" site="ell"/>
    <jointpos name="ok_pos" joint="h"/>
    <framepos name="ref" objtype="site" objname="ell" reftype="body" refname="f"/>
    <framepos name="geomframe" objtype="geom" objname="ga"/>
    <touch name="captouch" site="pad"/>
    <touch name="ok_touch" site="ell"/>
    <jointpos name="freepos" joint="ff"/>
    <jointvel name="cut" joint="h" cutoff="2.5"/>
    <jointpos name="ballpos" joint="bj"/>
    <gyro name="nowhere" site="no_such_site"/>
    <force name="ok_force" site="ell"/>
  </sensor></mujoco>"""
ONLY_ZERO_XML = """<mujoco><worldbody><body name="a" pos="0 0 0.5"><joint name="h" type="hinge" axis="0 1 0"/><geom type="sphere" size="0.05"/><site name="s"/></body></worldbody>
  <sensor><magnetometer name="m0" site="s"/><jointvel name="m1" joint="h" cutoff="1"/><framepos name="m2" objtype="geom" objname="x"/></sensor></mujoco>"""


def add_sensors(flat, new):
    """A copy of a compiled model (one loaded from a blob has no MJCF to edit) with sensors appended: new = [(name, type, objtype, objid, dim)]."""
    import numpy as np

    from robosuite_amd import mjcf

    m = flat.copy()
    n0 = int(m.nsensor)
    old_t = [int(t) for t in np.asarray(m.arrays["sensor_type"]).ravel()]
    cat = lambda key, old, add: m.set(key, np.concatenate([np.asarray(old, dtype=np.int32).ravel(), np.asarray(add, dtype=np.int32)]), np.int32)
    kinds = m.arrays.get("sensor_objtype", [mjcf.SENSOR_OBJ_SITE if t >= 0 else mjcf.SENSOR_OBJ_NONE for t in old_t])
    reasons = m.arrays.get("sensor_reason", [0 if t >= 0 else 1 for t in old_t])
    shapes = m.arrays.get("sensor_shape", [-1] * n0)
    cat("sensor_dim", m.arrays["sensor_dim"], [s[4] for s in new])
    cat("sensor_objid", m.arrays["sensor_objid"], [s[3] for s in new])
    cat("sensor_type", m.arrays["sensor_type"], [mjcf.SENSOR_TYPES[s[1]] for s in new])
    cat("sensor_objtype", kinds, [s[2] for s in new])
    cat("sensor_reason", reasons, [0] * len(new))
    cat("sensor_shape", shapes, [-1] * len(new))
    m.set("nsensor", n0 + len(new), np.int32)
    m.names["sensor"] = list(m.names["sensor"]) + [s[0] for s in new]
    return m
