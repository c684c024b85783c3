"""MJCF compiler (host logic, CPU).  Reference entry it replaces: mujoco.MjModel.from_xml_string
(robosuite/utils/binding_utils.py:1079)."""
import os

import numpy as np
import pytest

from robosuite_amd import mjcf
from tests.util import GOLD, TAGS, load_golden

XML = open(os.path.join(GOLD, "arm2_box.xml")).read()


def test_sizes_and_ids():
    m = mjcf.compile_mjcf(XML)
    assert (m.nq, m.nv, m.nu, m.nbody, m.njnt) == (3 + 7 + 7, 3 + 6 + 6, 3, 7, 5)
    assert m.names["body"] == ["world", "base", "link1", "link2", "link3", "box", "cyl"]
    assert m.names["joint"] == ["j1", "j2", "j3", "box_free", "cyl_free"]
    assert list(m.jnt_type) == [3, 3, 2, 0, 0]
    assert list(m.jnt_qposadr) == [0, 1, 2, 3, 10] and list(m.jnt_dofadr) == [0, 1, 2, 3, 9]
    assert list(m.body_parentid) == [0, 0, 1, 2, 3, 0, 0]
    assert list(m.body_rootid) == [0, 1, 1, 1, 1, 5, 6]
    assert list(m.body_weldid) == [0, 0, 2, 3, 4, 5, 6]
    assert list(m.dof_parentid[:3]) == [-1, 0, 1] and m.dof_parentid[3] == -1 and m.dof_parentid[4] == 3


def test_inertia_from_geoms_and_explicit():
    m = mjcf.compile_mjcf(XML)
    b = m.name2id("body", "box")
    mass = 500 * 8 * 0.05 * 0.04 * 0.05
    assert m.body_mass[b] == pytest.approx(mass)
    assert m.body_inertia[b] == pytest.approx(mass / 3 * np.array([0.04**2 + 0.05**2, 0.05**2 + 0.05**2, 0.05**2 + 0.04**2]))
    l3 = m.name2id("body", "link3")
    assert m.body_mass[l3] == pytest.approx(0.2)  # explicit <inertial> wins over the geom
    assert m.body_iquat[l3] == pytest.approx(np.array([0.9, 0.1, 0.2, 0.3]) / np.linalg.norm([0.9, 0.1, 0.2, 0.3]))
    c = m.name2id("body", "cyl")
    assert m.body_mass[c] == pytest.approx(700 * np.pi * 0.04**2 * 0.12)
    # free-joint qpos0 is the body frame
    assert m.qpos0[3:6] == pytest.approx([0.2, 0.3, 0.051])
    assert m.body_subtreemass[1] == pytest.approx(m.body_mass[1:5].sum())


def test_autolimits_defaults_and_actuators():
    m = mjcf.compile_mjcf(XML)
    assert list(m.jnt_limited) == [1, 1, 1, 0, 0]
    assert m.jnt_range[2] == pytest.approx([0, 0.1])
    assert m.geom_friction[m.name2id("geom", "l1")] == pytest.approx([1, 0.005, 0.0001])
    assert m.geom_solref[0] == pytest.approx([0.02, 1.0]) and m.geom_solimp[0] == pytest.approx([0.9, 0.95, 0.001, 0.5, 2])
    assert m.actuator_biastype.tolist() == [0, 0, 1]
    assert m.actuator_biasprm[2] == pytest.approx([0, -200, 0]) and m.actuator_gainprm[2][0] == 200
    assert m.actuator_forcelimited.tolist() == [0, 0, 1] and m.actuator_ctrllimited.tolist() == [1, 1, 1]
    # capsule fromto -> centre + half length along x
    g = m.name2id("geom", "l1")
    assert m.geom_pos[g] == pytest.approx([0.15, 0, 0]) and m.geom_size[g][:2] == pytest.approx([0.03, 0.15])
    R = mjcf.quat2mat(m.geom_quat[g])
    assert R[:, 2] == pytest.approx([1, 0, 0], abs=1e-12)


def test_collision_pair_filters():
    m = mjcf.compile_mjcf(XML)
    gn = m.names["geom"]
    pairs = {(gn[a], gn[b]) for a, b in zip(m.pair_geom1, m.pair_geom2)}
    assert ("l1", "l2") not in pairs and ("l2", "l1") not in pairs  # parent-child filter
    assert ("l2", "tip") not in pairs and ("tip", "l2") not in pairs
    assert ("floor", "l1") in pairs  # parent is welded to the world: NOT filtered
    assert ("tip", "l1") in pairs or ("l1", "tip") in pairs  # grandparent pairs collide
    assert ("floor", "box_g") in pairs and ("cyl_g", "box_g") in pairs
    # type ordering: geom1 type <= geom2 type
    assert all(m.geom_type[a] <= m.geom_type[b] for a, b in zip(m.pair_geom1, m.pair_geom2))


def test_inverse_weights_match_mass_matrix():
    m = mjcf.compile_mjcf(XML)
    M, _ = mjcf.mass_matrix_np(m, m.qpos0)
    assert np.allclose(M, M.T) and np.linalg.eigvalsh(M).min() > 0
    Minv = np.linalg.inv(M)
    assert m.dof_invweight0[0] == pytest.approx(Minv[0, 0])
    assert m.dof_invweight0[3] == pytest.approx(np.mean(np.diag(Minv)[3:6]))
    b = m.name2id("body", "box")
    assert m.body_invweight0[b, 0] == pytest.approx(1.0 / m.body_mass[b])
    assert m.body_invweight0[0].tolist() == [0, 0] and m.body_invweight0[1].tolist() == [0, 0]


def test_blob_roundtrip(tmp_path):
    m = mjcf.compile_mjcf(XML)
    m2 = mjcf.from_blob(mjcf.to_blob(m))
    assert all(np.array_equal(m.arrays[k].ravel(), m2.arrays[k].ravel()) for k in m.arrays)
    p = str(tmp_path / "m.rsim")
    mjcf.save_model(m, p)
    m3 = mjcf.load_model(p)
    assert m3.names == m.names and m3.nq == m.nq


def test_errors():
    with pytest.raises(mjcf.MJCFError):
        mjcf.compile_mjcf("<mujoco><worldbody><body><joint type='free'/><body><joint type='free'/></body></body></worldbody></mujoco>")
    with pytest.raises(mjcf.MJCFError):
        mjcf.compile_mjcf("<notmujoco/>")
    with pytest.raises(mjcf.MJCFError):
        mjcf.compile_mjcf("<mujoco><option integrator='RK4'/></mujoco>")
    with pytest.raises(mjcf.MJCFError):
        mjcf.from_blob(b"garbage-blob-----")


def test_mesh_hull_props():
    # unit cube as a triangle soup -> hull volume / inertia
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=float)
    hv, hf = mjcf.convex_hull(np.vstack([v, [[0.5, 0.5, 0.5]]]))
    assert len(hv) == 8
    vol, com, I = mjcf.mesh_volume_props(hv, hf)
    assert vol == pytest.approx(1.0) and com == pytest.approx([0.5, 0.5, 0.5]) and np.diag(I) == pytest.approx([1 / 6] * 3)


@pytest.mark.parametrize("tag", TAGS)
def test_golden_model_matches_survey_sizes(tag):
    """Lift/Panda sizes measured from the reference's own model layer (SURVEY.md section 8 preface)."""
    g, cfg, m = load_golden(tag)
    assert (m.nbody, m.njnt, m.nq, m.nv, m.nu, m.ngeom, m.nsite) == (26, 10, 16, 15, 9, 90, 9)
    assert np.allclose(m.dof_armature[:7], [5, 2.5, 5 / 3, 1.25, 1.0, 5 / 6, 5 / 7])
    assert np.allclose(m.dof_damping[:9], [0.1] * 5 + [0.01] * 2 + [100, 100])
    assert np.allclose(m.dof_frictionloss[:9], [0.1] * 7 + [1, 1])
    assert m.names["joint"][-1] == "cube_joint0" and m.jnt_type[-1] == 0
    assert np.allclose(m.geom_size[m.name2id("geom", "cube_g0")], g["cube_size"])


def test_recompile_reference_xml_is_deterministic():
    g, cfg, m = load_golden("seed0_gentle")
    # the golden blob carries no XML; recompile through the generator's path is covered by tools/gen_golden.py.
    assert m.npair > 100 and m.nmeshvert > 1000


def _write_stl(path, verts, faces):
    import struct
    with open(path, "wb") as f:
        f.write(b"\0" * 80 + struct.pack("<I", len(faces)))
        for fc in faces:
            a, b, c = verts[fc[0]], verts[fc[1]], verts[fc[2]]
            n = np.cross(b - a, c - a)
            f.write(struct.pack("<12fH", *(n / max(1e-30, np.linalg.norm(n))), *a, *b, *c, 0))


def _tessellated(kind):
    """(verts, faces, closed-form volume, COM, principal inertia about the COM at unit density) of an off-centre, tessellated primitive."""
    from scipy.spatial import ConvexHull
    c = np.array([0.03, -0.02, 0.05])
    if kind == "box":
        h = np.array([0.04, 0.025, 0.07])
        v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=float) * h
        vol = 8 * h.prod()
        I = vol / 3.0 * np.array([h[1] ** 2 + h[2] ** 2, h[0] ** 2 + h[2] ** 2, h[0] ** 2 + h[1] ** 2])
    elif kind == "cylinder":
        r, hh, n = 0.03, 0.06, 720
        a = 2 * np.pi * np.arange(n) / n
        ring = np.stack([r * np.cos(a), r * np.sin(a)], 1)
        v = np.vstack([np.c_[ring, np.full(n, -hh)], np.c_[ring, np.full(n, hh)]])
        area = 0.5 * n * r * r * np.sin(2 * np.pi / n)                               # the inscribed n-gon, exactly
        vol = area * 2 * hh
        j = r * r * (2 + np.cos(2 * np.pi / n)) / 6.0                               # second polar moment of the n-gon per unit area: J / A
        I = vol * np.array([j / 2 + hh * hh / 3, j / 2 + hh * hh / 3, j])
    else:
        r = 0.045
        # icosphere by hull of many points on the sphere: compared with the sphere's closed form at the tessellation's accuracy
        g = np.random.default_rng(0).standard_normal((4000, 3))
        v = r * g / np.linalg.norm(g, axis=1, keepdims=True)
        vol = 4.0 / 3.0 * np.pi * r ** 3
        I = np.full(3, 0.4 * vol * r * r)
    hull = ConvexHull(v)
    faces = hull.simplices.copy()
    cc = v.mean(0)
    for k, fc in enumerate(faces):
        if np.dot(np.cross(v[fc[1]] - v[fc[0]], v[fc[2]] - v[fc[0]]), v[fc[0]] - cc) < 0:
            faces[k] = fc[::-1]
    return v + c, faces, vol, c, I


@pytest.mark.parametrize("kind,tol", (("box", 1e-6), ("cylinder", 1e-6), ("sphere", 1e-2)))
def test_mesh_bodies_compile_to_closed_form_mass_properties(kind, tol, tmp_path):
    """The mesh path every Panda / IIWA / Robotiq link and every PickPlace object takes (STL file -> vertices -> convex hull -> volume, centre of
    mass, inertia -> body_mass / body_ipos / body_inertia / invweight0 of the compiled model), on tessellated primitives whose answers are known in
    closed form: a box and a 720-gon prism exactly (the prism against the polygon's own area and second moment), a 4000-point sphere to the
    accuracy of its tessellation.  Before round 3 this path was checked on a unit cube only."""
    v, f, vol, com, I = _tessellated(kind)
    _write_stl(tmp_path / "shape.stl", v.astype(np.float32).astype(np.float64), f)
    density = 730.0
    xml = f"""<mujoco><compiler meshdir="{tmp_path}"/><asset><mesh name="m" file="shape.stl"/></asset><worldbody>
      <body name="b" pos="0.1 0.2 0.3"><joint type="free"/><geom name="g" type="mesh" mesh="m" density="{density}"/></body></worldbody></mujoco>"""
    m = mjcf.compile_mjcf(xml)
    b = m.name2id("body", "b")
    assert m.body_mass[b] == pytest.approx(density * vol, rel=max(tol, 2e-6))
    # MuJoCo re-centres a mesh on its centre of mass and aligns it with its principal axes; however the compiler expresses that, the body's inertial
    # frame must sit at the shape's centre of mass (body frame) with the principal moments of the closed form
    assert np.abs(m.body_ipos[b] - com).max() < max(tol, 2e-6) * 0.1
    assert np.sort(m.body_inertia[b]) == pytest.approx(np.sort(density * I), rel=max(tol, 5e-6))
    # free body: translational inverse weight 1 / m, rotational = mean of 1 / I
    assert m.body_invweight0[b][0] == pytest.approx(1.0 / (density * vol), rel=max(tol, 2e-6))
    assert m.body_invweight0[b][1] == pytest.approx(np.mean(1.0 / (density * I)), rel=max(tol, 5e-6))
    # the hull the narrow phase scans: its vertices span the shape (support along +-x, +-y, +-z in the geom frame equals the extents about the COM)
    g = m.name2id("geom", "g")
    adr, num = int(m.mesh_vertadr[m.geom_dataid[g]]), int(m.mesh_vertnum[m.geom_dataid[g]])
    hv = np.asarray(m.mesh_vert).reshape(-1, 3)[adr:adr + num]
    R = mjcf.quat2mat(m.geom_quat[g])
    world = m.geom_pos[g] + hv @ R.T                       # hull vertices in the body frame
    assert np.abs(world.max(0) - v.max(0)).max() < 2e-6 + tol * 0.05 and np.abs(world.min(0) - v.min(0)).max() < 2e-6 + tol * 0.05


# ---- documented MJCF semantics as closed forms (XML reference: geom / inertial / compiler / default; nothing here comes from a simulator) ---------------
def _one_body(geoms, extra="", compiler='<compiler angle="radian"/>'):
    xml = f"""<mujoco>{compiler}{extra}<worldbody><body name="b" pos="0.1 0.2 0.3"><freejoint name="f"/>{geoms}</body></worldbody></mujoco>"""
    m = mjcf.compile_mjcf(xml)
    return m, m.name2id("body", "b")


def test_primitive_geoms_have_closed_form_mass_and_inertia():
    """density x volume and the textbook inertia tensors of sphere, capsule (cylinder + two hemispherical caps), cylinder, ellipsoid, box."""
    rho = 800.0
    r, h = 0.03, 0.07                                           # MJCF sizes: radius, HALF length
    m, b = _one_body(f'<geom type="sphere" size="{r}" density="{rho}"/>')
    ms = rho * 4 / 3 * np.pi * r**3
    assert m.body_mass[b] == pytest.approx(ms, rel=1e-12) and m.body_inertia[b] == pytest.approx([0.4 * ms * r * r] * 3, rel=1e-12)
    m, b = _one_body(f'<geom type="cylinder" size="{r} {h}" density="{rho}"/>')
    mc = rho * np.pi * r * r * 2 * h
    assert m.body_mass[b] == pytest.approx(mc, rel=1e-12)
    assert np.sort(m.body_inertia[b]) == pytest.approx(np.sort([mc * (3 * r * r + (2 * h)**2) / 12] * 2 + [0.5 * mc * r * r]), rel=1e-12)
    m, b = _one_body(f'<geom type="capsule" size="{r} {h}" density="{rho}"/>')
    mcyl, mhemi = rho * np.pi * r * r * 2 * h, rho * 2 / 3 * np.pi * r**3
    Izz = 0.5 * mcyl * r * r + 2 * 0.4 * mhemi * r * r
    # a hemisphere about its own COM (3r/8 from the flat face): (2/5 - 9/64) m r^2 transversal; then the parallel axis to the capsule's centre
    Ixx = mcyl * (3 * r * r + (2 * h)**2) / 12 + 2 * (mhemi * (0.4 - 9 / 64) * r * r + mhemi * (h + 3 * r / 8)**2)
    assert m.body_mass[b] == pytest.approx(mcyl + 2 * mhemi, rel=1e-12)
    assert np.sort(m.body_inertia[b]) == pytest.approx(np.sort([Ixx, Ixx, Izz]), rel=1e-10)
    a, bb, c = 0.02, 0.03, 0.05
    m, b = _one_body(f'<geom type="ellipsoid" size="{a} {bb} {c}" density="{rho}"/>')
    me = rho * 4 / 3 * np.pi * a * bb * c
    assert m.body_mass[b] == pytest.approx(me, rel=1e-12)
    assert m.body_inertia[b] == pytest.approx(me / 5 * np.array([bb * bb + c * c, a * a + c * c, a * a + bb * bb]), rel=1e-12)
    m, b = _one_body(f'<geom type="box" size="{a} {bb} {c}" mass="0.7"/>')          # explicit mass overrides the density
    assert m.body_mass[b] == pytest.approx(0.7) and m.body_inertia[b] == pytest.approx(0.7 / 3 * np.array([bb * bb + c * c, a * a + c * c, a * a + bb * bb]), rel=1e-12)


def test_composite_body_inertia_follows_the_parallel_axis_theorem():
    """Two offset, rotated geoms in one body: mass, centre of mass and the PRINCIPAL inertia (body_ipos / body_iquat / body_inertia) against a direct
    numpy evaluation of sum_i R_i I_i R_i^T + m_i (|d|^2 1 - d d^T)."""
    m, b = _one_body('<geom name="g1" type="box" size="0.02 0.03 0.05" pos="0.04 0 0.01" euler="0.3 -0.2 0.5" density="500"/>'
                     '<geom name="g2" type="sphere" size="0.025" pos="-0.03 0.05 0" density="1500"/>')
    m1 = 500 * 8 * 0.02 * 0.03 * 0.05
    I1 = m1 / 3 * np.diag([0.03**2 + 0.05**2, 0.02**2 + 0.05**2, 0.02**2 + 0.03**2])
    R1 = mjcf.quat2mat(m.geom_quat[m.name2id("geom", "g1")])
    m2 = 1500 * 4 / 3 * np.pi * 0.025**3
    I2 = 0.4 * m2 * 0.025**2 * np.eye(3)
    p1, p2 = np.array([0.04, 0, 0.01]), np.array([-0.03, 0.05, 0])
    com = (m1 * p1 + m2 * p2) / (m1 + m2)
    I = np.zeros((3, 3))
    for mi, Ii, Ri, pi in ((m1, I1, R1, p1), (m2, I2, np.eye(3), p2)):
        d = pi - com
        I += Ri @ Ii @ Ri.T + mi * (d @ d * np.eye(3) - np.outer(d, d))
    assert m.body_mass[b] == pytest.approx(m1 + m2, rel=1e-12) and m.body_ipos[b] == pytest.approx(com, abs=1e-14)
    Rq = mjcf.quat2mat(m.body_iquat[b])
    assert Rq @ np.diag(m.body_inertia[b]) @ Rq.T == pytest.approx(I, abs=1e-12)
    assert np.all(np.diff(m.body_inertia[b]) <= 1e-15)                      # MuJoCo orders the principal moments descending
    # euler="0.3 -0.2 0.5" with the default sequence xyz (intrinsic rotations about x, then the new y, then the new z), radians by the compiler line
    Rx = lambda t: np.array([[1, 0, 0], [0, np.cos(t), -np.sin(t)], [0, np.sin(t), np.cos(t)]])   # noqa: E731
    Ry = lambda t: np.array([[np.cos(t), 0, np.sin(t)], [0, 1, 0], [-np.sin(t), 0, np.cos(t)]])   # noqa: E731
    Rz = lambda t: np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])   # noqa: E731
    assert R1 == pytest.approx(Rx(0.3) @ Ry(-0.2) @ Rz(0.5), abs=1e-12)


def test_orientation_specifiers_and_angle_units():
    """quat / euler (degrees unless the compiler says radian) / axisangle / xyaxes / zaxis / fromto name the same rotations."""
    deg = '<compiler angle="degree"/>'
    m, b = _one_body('<geom name="a" type="box" size="0.01 0.02 0.03" euler="0 0 90"/>'
                     '<geom name="b" type="box" size="0.01 0.02 0.03" axisangle="0 0 1 90"/>'
                     '<geom name="c" type="box" size="0.01 0.02 0.03" xyaxes="0 1 0 -1 0 0"/>'
                     '<geom name="d" type="box" size="0.01 0.02 0.03" quat="0.7071067811865476 0 0 0.7071067811865476"/>'
                     '<geom name="e" type="capsule" size="0.01" fromto="0 0 0 0 0.2 0"/>'
                     '<geom name="f" type="cylinder" size="0.01 0.1" zaxis="0 1 0"/>', compiler=deg)
    Rz90 = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])
    for n in "abcd":
        assert mjcf.quat2mat(m.geom_quat[m.name2id("geom", n)]) == pytest.approx(Rz90, abs=1e-12), n
    for n in "ef":
        assert mjcf.quat2mat(m.geom_quat[m.name2id("geom", n)])[:, 2] == pytest.approx([0, 1, 0], abs=1e-12), n
    e = m.name2id("geom", "e")
    assert m.geom_pos[e] == pytest.approx([0, 0.1, 0]) and m.geom_size[e][:2] == pytest.approx([0.01, 0.1])
    m2, _ = _one_body('<geom name="a" type="box" size="0.01 0.02 0.03" euler="0 0 1.5707963267948966"/>')      # radian compiler (helper default)
    assert mjcf.quat2mat(m2.geom_quat[m2.name2id("geom", "a")]) == pytest.approx(Rz90, abs=1e-12)


def test_default_classes_nest_and_childclass_applies_to_the_subtree():
    xml = """<mujoco><default><geom friction="0.7 0.01 0.001" density="300"/><default class="soft"><geom solref="0.05 1" friction="0.2 0.01 0.001"/>
             <default class="softer"><geom solimp="0.5 0.6 0.01"/></default></default></default>
             <worldbody><body name="a" childclass="soft"><freejoint/><geom name="g0" type="sphere" size="0.01"/>
               <body name="b"><joint type="hinge" axis="0 0 1"/><geom name="g1" type="sphere" size="0.01" pos="0.1 0 0"/>
                 <geom name="g2" class="softer" type="sphere" size="0.01" pos="0.2 0 0"/><geom name="g3" type="sphere" size="0.01" pos="0.3 0 0" friction="0.9 0.01 0.001"/></body></body>
               <body name="c"><freejoint/><geom name="g4" type="sphere" size="0.01"/></body></worldbody></mujoco>"""
    m = mjcf.compile_mjcf(xml)
    g = lambda n: m.name2id("geom", n)   # noqa: E731
    assert m.geom_friction[g("g0")][0] == pytest.approx(0.2) and m.geom_solref[g("g0")] == pytest.approx([0.05, 1])      # childclass on the body
    assert m.geom_friction[g("g1")][0] == pytest.approx(0.2)                                                              # ... and on its descendants
    assert m.geom_solimp[g("g2")][:3] == pytest.approx([0.5, 0.6, 0.01]) and m.geom_solref[g("g2")] == pytest.approx([0.05, 1])   # nested class inherits its parent
    assert m.geom_friction[g("g3")][0] == pytest.approx(0.9)                                                              # an explicit attribute wins
    assert m.geom_friction[g("g4")][0] == pytest.approx(0.7) and m.geom_solref[g("g4")] == pytest.approx([0.02, 1])     # outside: the top-level default
    assert m.body_mass[m.name2id("body", "c")] == pytest.approx(300 * 4 / 3 * np.pi * 0.01**3)                           # density from the top-level default


def test_joint_units_and_bounding_radii():
    """compiler angle="degree" (the MJCF default) converts hinge ranges / ref to radians and leaves slide joints in metres; geom_rbound is the radius
    of the smallest sphere about the geom's centre that contains it (what the broadphase tests first)."""
    xml = """<mujoco><worldbody><body name="a"><joint name="h" type="hinge" axis="0 1 0" range="-90 45" armature="0.1" damping="0.5" frictionloss="0.2"/>
             <geom name="s" type="sphere" size="0.03"/>
             <body name="b" pos="0.1 0 0"><joint name="p" type="slide" axis="1 0 0" range="-0.05 0.2"/>
               <geom name="c" type="capsule" size="0.02 0.05"/><geom name="y" type="cylinder" size="0.02 0.05" pos="0 0.1 0"/>
               <geom name="x" type="box" size="0.01 0.02 0.03" pos="0 0.2 0"/><geom name="e" type="ellipsoid" size="0.01 0.04 0.02" pos="0 0.3 0"/></body></body></worldbody></mujoco>"""
    m = mjcf.compile_mjcf(xml)
    h, p = m.name2id("joint", "h"), m.name2id("joint", "p")
    assert m.jnt_range[h] == pytest.approx(np.radians([-90, 45])) and m.jnt_range[p] == pytest.approx([-0.05, 0.2])
    assert list(m.jnt_limited) == [1, 1]                                         # autolimits: a range makes the joint limited
    d = int(m.jnt_dofadr[h])
    assert (m.dof_armature[d], m.dof_damping[d], m.dof_frictionloss[d]) == pytest.approx((0.1, 0.5, 0.2))
    rb = {n: float(m.geom_rbound[m.name2id("geom", n)]) for n in "scyxe"}
    assert rb["s"] == pytest.approx(0.03) and rb["c"] == pytest.approx(0.07) and rb["y"] == pytest.approx(np.hypot(0.02, 0.05))
    assert rb["x"] == pytest.approx(np.linalg.norm([0.01, 0.02, 0.03])) and rb["e"] == pytest.approx(0.04)
