"""rsim_model_compile / rsim_mjcf_to_blob (include/rsim.h; robosuite_amd/csrc/rsim_mjcf.cpp) -- the MJCF compiler INSIDE the C-ABI library -- held to the
Python compiler robosuite_amd/mjcf.py, its checker.  Reference entry both replace: mujoco.MjModel.from_xml_string (utils/binding_utils.py:1077-1080,
models/base.py:125-147), called with the one MJCF string robosuite assembles per reset (environments/base.py:262-269).

Bar (round-4 review: "blob from C++ bit-equal to mjcf.to_blob"), stated per field class:
  * same entry table: names, order, dtypes, counts;
  * bit-equal: every int32 array, every name table, every float64 array that comes straight out of the XML (sizes, solver parameters, ranges, gains, masses,
    ...), and the hull vertices of every mesh whose hull has no exactly-degenerate points;
  * to the last bit or two (4e-16 of the field's largest entry): frames and axes that are COMPUTED from the XML -- quaternions from euler / axisangle / xyaxes /
    zaxis / fromto, normalised joint axes, fromto centres: numpy's norm (BLAS ddot with fused multiply-adds) and its vectorised sin / cos / arctan2 round the
    last bit differently from libm;
  * to rounding (1e-12 relative asserted, 1.3e-15 measured): what goes through a third-party routine in the Python compiler -- inertia frames (numpy.linalg.eigh),
    inverse weights (numpy.linalg.inv), mesh volume integrals (numpy.linalg.det), bounding radii;
  * body_iquat through the inertia TENSOR it encodes: an eigenvector's sign is a convention LAPACK does not fix, so the two frames may differ by axis flips;
  * mesh hulls (scipy / qhull there, a quickhull here) as CONVEX BODIES: every vertex of either hull within 1e-12 m of the other hull, vertex counts within
    1 % -- qhull and the quickhull keep different members of exactly coplanar / collinear point groups (measured on the IIWA links: 8 of 816 vertices swapped
    for points 1e-17 m off the same facets).
"""
import os
import struct

import numpy as np
import pytest

from robosuite_amd import backend, mjcf

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
HULL = {"nmeshvert", "mesh_vertadr", "mesh_vertnum", "mesh_vert"}
COMPUTED = {"body_quat", "geom_quat", "geom_pos", "geom_size", "site_quat", "jnt_axis", "qpos0", "qpos_spring"}
ROUNDED = {"body_ipos", "body_mass", "body_inertia", "geom_rbound", "geom_rcenter", "body_subtreemass", "body_invweight0", "dof_invweight0", "dof_M0",
           "tendon_length0", "tendon_invweight0", "tendon_lengthspring"}


def _inertia_tensors(m):
    out = []
    for b in range(int(m.nbody)):
        R = mjcf.quat2mat(np.asarray(m.body_iquat).reshape(-1, 4)[b])
        out.append(R @ np.diag(np.asarray(m.body_inertia).reshape(-1, 3)[b]) @ R.T)
    return np.array(out)


def _hull_distance(a, b):
    """largest distance by which a vertex of point set `a` lies outside the convex hull of `b`"""
    from scipy.spatial import ConvexHull

    eq = ConvexHull(b).equations
    return float((a @ eq[:, :3].T + eq[:, 3]).max())


def compare(xml, asset_dir=None):
    ref = mjcf.compile_mjcf(xml, asset_dir)
    blob = backend.compile_mjcf_blob(xml, asset_dir)
    new = mjcf.from_blob(blob)
    assert list(ref.arrays) == list(new.arrays)
    assert ref.names == new.names
    report = {"bit_equal_blob": mjcf.to_blob(ref) == blob, "rounded": {}, "hull_swaps": 0}
    hull_same = all(np.array_equal(np.ravel(ref.arrays[k]), np.ravel(new.arrays[k])) for k in HULL)
    for k, a in ref.arrays.items():
        b = new.arrays[k]
        assert a.dtype == b.dtype and (a.size == b.size or k in HULL), k
        if k in HULL or k == "body_iquat":
            continue
        a, b = np.ravel(a), np.ravel(b)
        if k in ROUNDED or (k in ("geom_rbound", "geom_rcenter") and not hull_same):
            if not np.array_equal(a, b):
                e = float(np.abs(a - b).max() / max(1e-300, np.abs(a).max()))
                report["rounded"][k] = e
                assert e < 1e-12, (k, e)
        elif k in COMPUTED and not np.array_equal(a, b):
            e = float(np.abs(a - b).max() / max(1e-300, np.abs(a).max()))
            report["last_bit"] = max(report.get("last_bit", 0.0), e)
            assert e <= 4e-16, (k, e)
        else:
            assert np.array_equal(a, b), (k, a[a != b][:4], b[a != b][:4])
    It, Jt = _inertia_tensors(ref), _inertia_tensors(new)
    assert np.abs(It - Jt).max() <= 1e-12 * max(1e-300, np.abs(It).max())
    if not hull_same:
        assert int(ref.nmesh) == int(new.nmesh)
        for i in range(int(ref.nmesh)):
            a = np.asarray(ref.mesh_vert).reshape(-1, 3)[ref.mesh_vertadr[i]: ref.mesh_vertadr[i] + ref.mesh_vertnum[i]]
            b = np.asarray(new.mesh_vert).reshape(-1, 3)[new.mesh_vertadr[i]: new.mesh_vertadr[i] + new.mesh_vertnum[i]]
            if a.shape == b.shape and np.array_equal(a, b):
                continue
            assert abs(len(a) - len(b)) <= max(1, 0.01 * len(a)), (i, len(a), len(b))
            assert _hull_distance(a, b) < 1e-12 and _hull_distance(b, a) < 1e-12, i
            report["hull_swaps"] += len({tuple(x) for x in a} ^ {tuple(x) for x in b})
    return ref, new, report


# ---- hand-written MJCF: every construct the compiler knows -----------------------------------------------------------------------------------------
CORPUS = {
    "arm2_box": open(os.path.join(GOLD, "arm2_box.xml")).read(),
    "coupled_fingers": open(os.path.join(GOLD, "coupled_fingers.xml")).read(),
    "defaults_nested": """<mujoco><default><geom friction="0.7 0.01 0.001" density="300"/><joint damping="0.3"/><default class="soft"><geom solref="0.05 1" friction="0.2 0.01 0.001"/>
        <default class="softer"><geom solimp="0.8 0.9 0.002 0.4 3"/></default></default><motor ctrlrange="-2 2"/></default>
        <worldbody><body name="a" childclass="soft"><joint name="ja" type="hinge" axis="0 1 0" range="-90 45" armature="0.1" frictionloss="0.2"/>
        <geom name="g1" type="box" size="0.1 0.2 0.3"/><geom name="g2" class="softer" type="sphere" size="0.05" pos="0.3 0 0"/>
        <body name="b"><joint name="jb" type="slide" axis="1 1 0" range="-0.1 0.2" ref="0.05" springref="0.02" stiffness="3"/><geom name="g3" type="capsule" fromto="0 0 0 0.2 0.1 0.3" size="0.02"/></body></body>
        <body name="c" pos="1 0 0"><joint name="jc" type="ball" pos="0 0 0.1"/><geom name="g4" class="main" type="ellipsoid" size="0.1 0.05 0.07"/></body></worldbody>
        <actuator><motor name="ma" joint="ja" gear="2"/><position name="pb" joint="jb" kp="40" kv="3" ctrlrange="-1 1" forcerange="-5 5"/><velocity name="va" joint="ja" kv="7"/>
        <general name="ga" joint="jb" gainprm="3 0 0" biasprm="0.1 -3 -0.2" biastype="affine" ctrllimited="false"/></actuator></mujoco>""",
    "orientations_degree": """<mujoco><compiler eulerseq="zYx"/><worldbody><body name="q" quat="2 0 0 1"><geom type="sphere" size="0.1"/><joint type="free"/></body>
        <body name="e" pos="1 0 0" euler="30 -40 50"><freejoint name="fe"/><geom type="box" size="0.1 0.1 0.1" euler="10 20 30"/></body>
        <body name="aa" pos="2 0 0" axisangle="1 2 3 75"><freejoint/><geom type="cylinder" size="0.05 0.1" zaxis="1 1 0"/></body>
        <body name="xy" pos="3 0 0" xyaxes="1 1 0 -1 2 0.3"><freejoint/><geom type="capsule" size="0.05 0.1" xyaxes="0 1 0 0 0 1"/><site name="s" pos="0.1 0 0" euler="5 6 7" size="0.01 0.02"/></body>
        <body name="z" pos="4 0 0" zaxis="0 0 -1"><freejoint/><geom type="sphere" size="0.05" mass="0.3"/></body></worldbody></mujoco>""",
    "orientations_radian": """<mujoco><compiler angle="radian" eulerseq="XYZ" autolimits="true"/><option timestep="0.001" gravity="0 0 -3.7" wind="1 0 0" density="1.2" viscosity="0.0002" impratio="3"
        cone="elliptic" iterations="50" tolerance="1e-10" solver="PGS"/><worldbody><body name="e" euler="0.3 -0.4 0.5"><joint name="h" type="hinge" range="-1.2 0.7" limited="true" margin="0.01"
        solreflimit="0.03 0.9" solimplimit="0.8 0.9 0.01 0.3 1" solreffriction="0.04 0.8" solimpfriction="0.7 0.8 0.02 0.2 3"/><geom type="box" size="0.1 0.2 0.3" group="2" contype="2" conaffinity="3" condim="4" priority="1"
        solmix="2" margin="0.002" gap="0.001" rgba="1 0 0 0.5"/></body></worldbody></mujoco>""",
    "inertial_forms": """<mujoco><compiler inertiagrouprange="1 2" boundmass="0.01" boundinertia="0.0001"/><worldbody>
        <body name="full"><freejoint/><inertial pos="0.01 0.02 0.03" mass="1.5" fullinertia="0.02 0.03 0.04 0.001 -0.002 0.003" euler="10 20 30"/><geom type="sphere" size="0.1"/></body>
        <body name="diag" pos="1 0 0"><freejoint/><inertial pos="0 0 0.1" quat="0.9 0.1 0.2 0.3" mass="0.7" diaginertia="0.01 0.02 0.03"/><geom type="sphere" size="0.1"/></body>
        <body name="multi" pos="2 0 0"><freejoint/><geom type="box" size="0.1 0.05 0.02" pos="0.1 0 0" group="1" density="400"/><geom type="sphere" size="0.04" pos="-0.1 0.05 0" group="2" mass="0.2"/>
           <geom type="cylinder" size="0.03 0.08" pos="0 0 0.1" euler="90 0 0" group="0"/></body>
        <body name="tiny" pos="3 0 0"><freejoint/><geom type="sphere" size="0.001" group="1"/></body>
        <body name="mocap" pos="0 0 2" mocap="true"><geom type="box" size="0.01 0.01 0.01" contype="0" conaffinity="0"/></body></worldbody></mujoco>""",
    "pairs_sensors_tendons": """<mujoco><worldbody><geom name="floor" type="plane" size="0 0 1"/><geom name="floor2" type="plane" size="0 0 1" pos="0 0 -1"/>
        <body name="p"><joint name="j0" type="hinge" axis="0 0 1"/><geom name="gp" type="box" size="0.1 0.1 0.1"/><site name="ft" pos="0 0 0.1"/>
          <body name="c1" pos="0.2 0 0"><joint name="j1" type="slide" axis="1 0 0" range="0 0.04"/><geom name="gc1" type="box" size="0.02 0.02 0.02"/>
             <body name="gc" pos="0.1 0 0"><geom name="ggc" type="sphere" size="0.02"/></body></body>
          <body name="c2" pos="-0.2 0 0"><joint name="j2" type="slide" axis="-1 0 0" range="0 0.04"/><geom name="gc2" type="box" size="0.02 0.02 0.02"/></body></body>
        <body name="free" pos="0 0 1"><freejoint name="ff"/><geom name="gf" type="sphere" size="0.05"/></body><camera name="cam"/><light name="sun"/></worldbody>
        <contact><exclude body1="p" body2="free"/></contact>
        <tendon><fixed name="t0" range="-0.01 0.01" stiffness="2" damping="0.1" frictionloss="0.3" margin="0.001"><joint joint="j1" coef="1"/><joint joint="j2" coef="-1"/></fixed>
                <fixed name="t1" springlength="0.01 0.02" limited="false"><joint joint="j1" coef="0.5"/></fixed></tendon>
        <equality><tendon name="e0" tendon1="t0" polycoef="0.001 1 0 0 0" solref="0.01 1"/><tendon name="off" tendon1="t1" active="false"/></equality>
        <sensor><force name="f" site="ft"/><torque name="tq" site="ft"/><touch name="tc" site="ft"/></sensor>
        <actuator><position name="a1" joint="j1" kp="100"/></actuator></mujoco>""",
}


@pytest.mark.parametrize("name", sorted(CORPUS))
def test_cpp_compiler_matches_the_python_checker_on_hand_written_mjcf(name):
    ref, new, rep = compare(CORPUS[name])
    print(name, rep)
    assert max(rep["rounded"].values(), default=0.0) < 1e-12


def _write_meshes(d):
    """a skewed box as binary STL, ASCII STL, OBJ (quads) and legacy MSH; a 200-gon prism (coplanar caps, collinear-free rim) as binary STL"""
    rng = np.random.default_rng(3)
    A = np.eye(3) + 0.2 * rng.standard_normal((3, 3))
    v = np.array([[x, y, z] for x in (-0.1, 0.1) for y in (-0.05, 0.07) for z in (-0.02, 0.04)]) @ A.T
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = [t for q in quads for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    v32 = v.astype(np.float32)

    def stl(path, verts, faces):
        with open(path, "wb") as f:
            f.write(b"\0" * 80 + struct.pack("<I", len(faces)))
            for t in faces:
                f.write(struct.pack("<12fH", 0, 0, 0, *np.asarray(verts[list(t)], dtype=np.float32).ravel(), 0))

    stl(d / "box_bin.stl", v32, tris)
    with open(d / "box_ascii.stl", "w") as f:
        f.write("solid b\n")
        for t in tris:
            f.write("facet normal 0 0 0\nouter loop\n" + "".join(f"vertex {v32[i][0]!r} {v32[i][1]!r} {v32[i][2]!r}\n".replace("np.float32(", "").replace(")", "") for i in t) + "endloop\nendfacet\n")
        f.write("endsolid b\n")
    with open(d / "box.obj", "w") as f:
        f.write("# box\n" + "".join(f"v {p[0]:.9g} {p[1]:.9g} {p[2]:.9g}\n" for p in v32) + "".join("f " + " ".join(f"{i + 1}/1/1" for i in q) + "\n" for q in quads))
    with open(d / "box.msh", "wb") as f:
        f.write(struct.pack("<4i", len(v32), 0, 0, len(tris)) + v32.tobytes() + np.asarray(tris, dtype="<i4").tobytes())
    n = 200
    ang = 2 * np.pi * np.arange(n) / n
    ring = np.stack([0.05 * np.cos(ang), 0.05 * np.sin(ang)], 1)
    pv = np.concatenate([np.c_[ring, np.full(n, -0.03)], np.c_[ring, np.full(n, 0.03)], [[0, 0, -0.03], [0, 0, 0.03]]]).astype(np.float32)
    pf = [(i, (i + 1) % n, n + i) for i in range(n)] + [((i + 1) % n, n + (i + 1) % n, n + i) for i in range(n)] + [(2 * n, (i + 1) % n, i) for i in range(n)] + [(2 * n + 1, n + i, n + (i + 1) % n) for i in range(n)]
    stl(d / "prism.stl", pv, pf)


def test_cpp_compiler_reads_stl_obj_msh_and_builds_the_same_hulls(tmp_path):
    _write_meshes(tmp_path)
    xml = f"""<mujoco><compiler meshdir="{tmp_path}" angle="radian"/><asset><mesh name="a" file="box_bin.stl"/><mesh file="box_ascii.stl" scale="1 2 0.5"/><mesh name="o" file="box.obj"/>
        <mesh name="m" file="box.msh" scale="-1 1 1"/><mesh name="pr" file="prism.stl"/><mesh name="unused" file="does_not_exist.stl"/></asset><worldbody>
        <body name="b1"><freejoint/><geom type="mesh" mesh="a" density="800"/></body><body name="b2" pos="1 0 0"><freejoint/><geom type="mesh" mesh="box_ascii" mass="0.4"/></body>
        <body name="b3" pos="2 0 0"><freejoint/><geom type="mesh" mesh="o" euler="0.1 0.2 0.3"/><geom type="mesh" mesh="pr" pos="0 0 0.2"/></body>
        <body name="b4" pos="3 0 0"><freejoint/><geom type="mesh" mesh="m"/><geom type="mesh" mesh="unused" contype="0" conaffinity="0" group="7"/></body></worldbody></mujoco>"""
    ref, new, rep = compare(xml)
    print(rep)
    assert int(new.nmesh) == 5 and [int(x) for x in new.mesh_vertnum] == [8, 8, 8, 400, 8]      # in order of first use; the prism loses its two cap centres and nothing else
    assert new.names["mesh"] == ["a", "box_ascii", "o", "m", "pr", "unused"]
    # relative file names resolve against asset_dir, then meshdir
    rel = xml.replace(f'meshdir="{tmp_path}"', 'meshdir="sub"')
    os.makedirs(tmp_path / "root" / "sub")
    for f in ("box_bin.stl", "box_ascii.stl", "box.obj", "box.msh", "prism.stl"):
        os.replace(tmp_path / f, tmp_path / "root" / "sub" / f)
    compare(rel, str(tmp_path / "root"))


def test_cpp_compiler_moves_a_mesh_centre_that_is_outside_its_hull_as_the_python_checker_does(tmp_path):
    """geom_rcenter is MPR's interior point.  The bounding-box centre of a tetrahedron with three faces in the coordinate planes lies outside it: both compilers
    take the mean of the hull vertices there, and geom_rbound about it; the polyhedron beside it keeps its box centre."""
    from tests import contact_scenes as CS

    CS.write_meshes(tmp_path)
    ref, new, rep = compare(CS.XML, str(tmp_path))
    print(rep)
    for m in (ref, new):
        rc, rb = np.asarray(m.geom_rcenter).reshape(-1, 3), np.asarray(m.geom_rbound).ravel()
        for name, moved in (("tet", True), ("poly", False)):
            g = m.names["geom"].index(name)
            did = int(np.asarray(m.geom_dataid).ravel()[g])
            V = np.asarray(m.mesh_vert).reshape(-1, 3)[m.mesh_vertadr[did]: m.mesh_vertadr[did] + m.mesh_vertnum[did]]
            box = 0.5 * (V.min(axis=0) + V.max(axis=0))
            want = V.mean(axis=0) if moved else box
            assert (mjcf.hull_inside_by(V, box) < mjcf.RCENTER_INSIDE * np.linalg.norm(V - box, axis=1).max()) == moved
            assert np.abs(rc[g] - want).max() <= 1e-15 and abs(rb[g] - np.linalg.norm(V - want, axis=1).max()) <= 1e-15, (name, rc[g], want)
            assert mjcf.hull_inside_by(V, rc[g]) >= mjcf.RCENTER_INSIDE * rb[g]


BAD = {
    "not xml": "<mujoco><worldbody></mujoco>",
    "root": "<notmujoco/>",
    "integrator": "<mujoco><option integrator='RK4'/></mujoco>",
    "nested free joint": "<mujoco><worldbody><body><joint type='free'/><body><joint type='free'/></body></body></worldbody></mujoco>",
    "unknown mesh": "<mujoco><worldbody><body><geom type='mesh' mesh='nope'/></body></worldbody></mujoco>",
    "missing mesh file": "<mujoco><asset><mesh name='m' file='/nonexistent/m.stl'/></asset><worldbody><body><geom type='mesh' mesh='m'/></body></worldbody></mujoco>",
    "hfield": "<mujoco><worldbody><geom type='hfield'/></worldbody></mujoco>",
    "spatial tendon": "<mujoco><worldbody><body><joint name='j'/><geom size='0.1'/></body></worldbody><tendon><spatial/></tendon></mujoco>",
    "actuator without joint": "<mujoco><worldbody><body><joint name='j'/><geom size='0.1'/></body></worldbody><actuator><motor name='m' joint='k'/></actuator></mujoco>",
    "weld equality": "<mujoco><worldbody><body name='a'><geom size='0.1'/></body></worldbody><equality><weld body1='a'/></equality></mujoco>",
    "contact pair": "<mujoco><worldbody><geom name='a' size='0.1'/></worldbody><contact><pair geom1='a' geom2='a'/></contact></mujoco>",
    "number count": "<mujoco><worldbody><body pos='1 2 3 4'><geom size='0.1'/></body></worldbody></mujoco>",
    "mocap with joint": "<mujoco><worldbody><body mocap='true'><joint/><geom size='0.1'/></body></worldbody></mujoco>",
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_malformed_or_unsupported_mjcf_fails_in_both_compilers_with_a_reason(what):
    """MuJoCo raises on compile errors [3P]; mjcf.compile_mjcf raises MJCFError; rsim_mjcf_to_blob / rsim_model_compile return non-zero with the reason in rsim_last_error()."""
    with pytest.raises((mjcf.MJCFError, KeyError)):
        mjcf.compile_mjcf(BAD[what])
    with pytest.raises(backend.RsimError) as e:
        backend.compile_mjcf_blob(BAD[what])
    assert "MJCF compile error" in str(e.value) and len(str(e.value)) > 25
    with pytest.raises(backend.RsimError):
        backend.HipModel.from_xml_string(BAD[what])


def test_rsim_model_compile_gives_the_model_the_blob_path_gives():
    """rsim_model_compile(xml) == rsim_model_create(mjcf.to_blob(compile_mjcf(xml))) as far as the C-ABI's own queries can tell: sizes, kernel configuration, names."""
    xml = CORPUS["pairs_sensors_tendons"]
    a = backend.HipModel.from_xml_string(xml)
    b = backend.HipModel(mjcf.compile_mjcf(xml))
    for k in ("nq", "nv", "nu", "nbody", "njnt", "ngeom", "nsite", "npair", "ntendon", "neq", "nsensor", "nmesh"):
        assert a.int(k) == b.int(k) >= 0, k
    assert a.name2id("joint", "j2") == b.name2id("joint", "j2") == 2 and a.name2id("tendon", "t1") == 1 and a.name2id("body", "nope") == -1
    assert a.id2name("geom", 0) == "floor" and a.id2name("sensor", 2) == "tc" and a.id2name("actuator", 0) == "a1"
    L = backend.lib()
    import ctypes as C
    la, lb = (C.c_int * 10)(), (C.c_int * 10)()
    assert L.rsim_model_config(a.ptr, C.byref(la)) == L.rsim_model_config(b.ptr, C.byref(lb)) and list(la) == list(lb)
    assert a.flat.names == b.flat.names


REF_ENVS = {"lift_panda": ("Lift", "Panda"), "stack_panda": ("Stack", "Panda"), "peg_baxter": ("TwoArmPegInHole", "Baxter"), "pickplace_iiwa": ("PickPlace", "IIWA")}
_DUMP = r"""
import sys
sys.path.insert(0, %r); sys.path.insert(0, "/root/reference")
from robosuite_amd import shim
from oracle.shim_backend import OracleBackend
shim.install(OracleBackend)
import robosuite as suite
for name, (env, robot) in %r.items():
    e = suite.make(env, robots=robot, has_renderer=False, has_offscreen_renderer=False, use_camera_obs=False)
    e.reset()
    open(sys.argv[1] + "/" + name + ".xml", "w").write(e.sim.model.get_xml())
from robosuite.models.grippers import GripperTester, Robotiq140Gripper
t = GripperTester(gripper=Robotiq140Gripper(), pos="0 0 0.3", quat="0 0 1 0", gripper_low_pos=0.02, gripper_high_pos=0.1, box_size=[0.025] * 3, render=False)
open(sys.argv[1] + "/gripper_tester_robotiq140.xml", "w").write(t.world.get_xml())
"""


@pytest.mark.skipif(not os.path.isdir("/root/reference/robosuite"), reason="reference checkout not present (GPU box): the MJCF strings come from the live reference envs")
def test_cpp_compiler_on_the_mjcf_the_reference_assembles_for_the_baseline_configurations(tmp_path):
    """The four BASELINE models (Lift / Stack with the Panda, TwoArmPegInHole with Baxter, PickPlace with IIWA + Robotiq140: 10 - 17 meshes, tendons, equalities)
    and the GripperTester world, as strings from the unmodified reference (env.sim.model.get_xml() / MujocoWorldBase.get_xml()): compiled by both compilers and
    compared as the module docstring says; the shipped assets (robosuite_amd/assets/*.rsim) are what the Python compiler made of the same strings."""
    import subprocess
    import sys
    import time

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _DUMP % (root, REF_ENVS), str(tmp_path)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in list(REF_ENVS) + ["gripper_tester_robotiq140"]:
        xml = open(tmp_path / f"{name}.xml").read()
        t0 = time.perf_counter(); backend.compile_mjcf_blob(xml); t_cpp = time.perf_counter() - t0
        t0 = time.perf_counter(); ref, new, rep = compare(xml); t_both = time.perf_counter() - t0
        print(f"{name}: nbody {int(ref.nbody)} nv {int(ref.nv)} nmesh {int(ref.nmesh)} hull vertices {int(ref.nmeshvert)} / {int(new.nmeshvert)}; C++ compile {1e3 * t_cpp:.0f} ms, "
              f"Python + C++ + comparison {t_both:.2f} s; {rep}")
        assert rep["hull_swaps"] <= 0.02 * int(ref.nmeshvert) + 4
        if name in REF_ENVS:
            # ... and the model the package ships for this configuration has these sizes
            stem = {"peg_baxter": "peg_baxter_joint_velocity"}.get(name, name)
            from robosuite_amd import factory
            flat, _ = factory.load_shipped(stem)
            assert (int(flat.nq), int(flat.nv), int(flat.nbody), int(flat.ngeom), int(flat.npair)) == (int(new.nq), int(new.nv), int(new.nbody), int(new.ngeom), int(new.npair))
