"""Known answers for model terms that no fixture or generated model moves: MJCF builders and fp64 closed forms of MuJoCo's DOCUMENTED model (Computation:
"Inertia model" of the fluid forces, soft-constraint resting violations inside a margin, the contact-parameter mixing rules, frictionless contacts, the
affine actuator).  Shared by tests/test_known_answers_host.py (the fp64 oracle, CPU) and tests/test_hip_known_answers.py (the fused kernel, GPU).  Nothing
here imports the oracle, the kernel or the model compiler: the builders write MJCF text from the Python constants below, and the closed forms are
evaluated from those same constants, so a reference never passes through a compiled array, `cdof` or `cvel` of either implementation.
"""
import numpy as np

H, G0 = 0.002, 9.81
SOLREF, SOLIMP = (0.02, 1.0), (0.9, 0.95, 0.001, 0.5, 2)

# ---- rotations (fp64; quaternions w x y z, the MJCF order) ----------------------------------------------------------------------------------------------


def rot_axis(axis, angle):
    """Rodrigues' rotation matrix."""
    a = np.asarray(axis, dtype=np.float64); a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def rot_euler(e):
    """MJCF `euler` with the default eulerseq "xyz": intrinsic rotations about x, then the new y, then the new z."""
    return rot_axis((1, 0, 0), e[0]) @ rot_axis((0, 1, 0), e[1]) @ rot_axis((0, 0, 1), e[2])


def rot_quat(q):
    w, x, y, z = np.asarray(q, dtype=np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def _s(v):
    return " ".join(repr(float(x)) for x in np.ravel(v))


# ---- 1. fluid forces: the inertia-box model ------------------------------------------------------------------------------------------------------------
RHO, MU, WIND = 1000.0, 0.5, (0.3, -0.2, 0.1)
BOX_HALF, BOX_MASS = (0.06, 0.04, 0.02), 0.27                    # 12 x 8 x 4 cm, 0.27 kg
GEOM_POS, GEOM_EULER = (0.03, 0.01, -0.02), (0.3, 0.2, 0.1)      # the geom inside its body: ipos != 0, iquat not the identity


def box_inertia(half, mass):
    a, b, c = half
    return mass / 3.0 * np.array([b * b + c * c, a * a + c * c, a * a + b * b])


def fluid_wrench(inertia, mass, Ri, v_com, w, rho, mu, wind):
    """Force and torque (world frame, at the body COM) of the documented inertia model.  `Ri`: inertial frame in the world; `v_com`, `w`: world-frame
    COM velocity and angular velocity.  b_i = sqrt(6 (I_j + I_k - I_i) / m), d = mean(b), v = COM velocity minus wind, both in the inertial frame:
      f_i = -3 pi d mu v_i - 1/2 rho b_j b_k |v_i| v_i        t_i = -pi d^3 mu w_i - rho b_i (b_j^4 + b_k^4) |w_i| w_i / 64"""
    I = np.asarray(inertia, dtype=np.float64)
    b = np.sqrt(6.0 * (I.sum() - 2.0 * I) / mass)
    d = b.mean()
    v = Ri.T @ (np.asarray(v_com, dtype=np.float64) - np.asarray(wind, dtype=np.float64))
    wl = Ri.T @ np.asarray(w, dtype=np.float64)
    f, t = np.zeros(3), np.zeros(3)
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        f[i] = -3 * np.pi * d * mu * v[i] - 0.5 * rho * b[j] * b[k] * abs(v[i]) * v[i]
        t[i] = -np.pi * d ** 3 * mu * wl[i] - rho * b[i] * (b[j] ** 4 + b[k] ** 4) * abs(wl[i]) * wl[i] / 64.0
    return Ri @ f, Ri @ t


def free_box_xml(rho=RHO, mu=MU, wind=WIND):
    return f"""<mujoco><compiler angle="radian"/><option timestep="{H}" gravity="0 0 -{G0}" density="{rho}" viscosity="{mu}" wind="{_s(wind)}"/><worldbody>
      <body name="box" pos="0 0 1"><freejoint/><geom type="box" size="{_s(BOX_HALF)}" mass="{BOX_MASS}" pos="{_s(GEOM_POS)}" euler="{_s(GEOM_EULER)}"
        contype="0" conaffinity="0"/></body></worldbody></mujoco>"""


def free_box_states(n=8, seed=11, rest=False):
    """Seeded poses and 6-velocities (about 1 m/s and 3 rad/s): qpos [n, 7], qvel [n, 6] (linear in the world, angular in the body frame)."""
    rng = np.random.default_rng(seed)
    quat = rng.standard_normal((n, 4)); quat /= np.linalg.norm(quat, axis=1, keepdims=True)
    qpos = np.concatenate([rng.uniform(-0.5, 0.5, (n, 3)) + (0, 0, 1.0), quat], axis=1)
    qvel = np.concatenate([rng.uniform(-1, 1, (n, 3)), rng.uniform(-3, 3, (n, 3))], axis=1)
    return qpos, (np.zeros_like(qvel) if rest else qvel)


def free_box_reference(qpos, qvel, rho=RHO, mu=MU, wind=WIND):
    """(qfrc_passive, qacc) of the free box in one state.  A free joint's linear dofs move the body ORIGIN (world frame), its angular dofs are in the body
    frame.  The wrench acts at the COM c = p + R ipos: the linear generalised force is F, the angular one R^T (T + (c - p) x F).  Accelerations: Newton at
    the COM (a_c = g + F / m), Euler about it (I alpha = T - w x I w), shifted to the origin: a_o = a_c - alpha x r - w x (w x r), r = c - p."""
    p, Rb = np.asarray(qpos[:3], dtype=np.float64), rot_quat(qpos[3:7])
    Ri = Rb @ rot_euler(GEOM_EULER)
    r = Rb @ np.asarray(GEOM_POS)
    w = Rb @ np.asarray(qvel[3:6], dtype=np.float64)
    v_com = np.asarray(qvel[:3], dtype=np.float64) + np.cross(w, r)
    I = box_inertia(BOX_HALF, BOX_MASS)
    F, T = fluid_wrench(I, BOX_MASS, Ri, v_com, w, rho, mu, wind)
    qfrc = np.concatenate([F, Rb.T @ (T + np.cross(r, F))])
    Iw = Ri @ np.diag(I) @ Ri.T
    alpha = np.linalg.solve(Iw, T - np.cross(w, Iw @ w))
    a_c = np.array([0, 0, -G0]) + F / BOX_MASS
    a_o = a_c - np.cross(alpha, r) - np.cross(w, np.cross(w, r))
    return qfrc, np.concatenate([a_o, Rb.T @ alpha])


def free_box_mass_matrix(qpos):
    """Mass matrix of the free box in its joint's coordinates (origin velocity in the world, angular velocity in the body frame): J^T diag(m, I_world) J with
    v_com = v_o - [r]x R w_b and w = R w_b."""
    Rb = rot_quat(qpos[3:7])
    Ri = Rb @ rot_euler(GEOM_EULER)
    r = Rb @ np.asarray(GEOM_POS)
    rx = np.array([[0, -r[2], r[1]], [r[2], 0, -r[0]], [-r[1], r[0], 0]])
    J = np.block([[np.eye(3), -rx @ Rb], [np.zeros((3, 3)), Rb]])
    D = np.zeros((6, 6)); D[:3, :3] = BOX_MASS * np.eye(3); D[3:, 3:] = Ri @ np.diag(box_inertia(BOX_HALF, BOX_MASS)) @ Ri.T
    return J.T @ D @ J


def per_env_media(n=4):
    """Density, viscosity and wind of each env of the per-env case."""
    return [(RHO * (0.4 + 0.5 * e), MU * (1.6 - 0.4 * e), (0.3 - 0.25 * e, -0.2 + 0.1 * e, 0.1 + 0.2 * e)) for e in range(n)]


# hinge - hinge - slide chain on a fixed base: body pos / euler in the parent, joint type / axis / anchor in the body, geom pos / euler / half sizes / mass
CHAIN = (
    dict(pos=(0.0, 0.0, 0.0), euler=(0.1, -0.2, 0.3), jtype="hinge", axis=(0.2, 1.0, 0.3), jpos=(0.01, -0.02, 0.015),
         gpos=(0.08, 0.01, -0.02), geuler=(0.3, 0.2, 0.1), half=(0.06, 0.04, 0.02), mass=0.27),
    dict(pos=(0.16, 0.02, 0.01), euler=(-0.3, 0.25, 0.15), jtype="hinge", axis=(1.0, -0.4, 0.5), jpos=(-0.015, 0.01, 0.02),
         gpos=(0.05, -0.03, 0.02), geuler=(-0.2, 0.4, 0.25), half=(0.05, 0.03, 0.025), mass=0.21),
    dict(pos=(0.11, -0.02, 0.03), euler=(0.2, 0.3, -0.25), jtype="slide", axis=(0.3, 0.2, 1.0), jpos=(0.02, 0.01, -0.01),
         gpos=(0.02, 0.03, 0.06), geuler=(0.15, -0.35, 0.3), half=(0.03, 0.045, 0.05), mass=0.19),
)


def chain_xml(rho=RHO, mu=MU, wind=WIND):
    out, depth = [f"""<mujoco><compiler angle="radian"/><option timestep="{H}" gravity="0 0 -{G0}" density="{rho}" viscosity="{mu}" wind="{_s(wind)}"/><worldbody>
      <body name="base" pos="0 0 1">"""], 1
    for i, L in enumerate(CHAIN):
        out.append(f"""<body name="l{i}" pos="{_s(L['pos'])}" euler="{_s(L['euler'])}"><joint name="j{i}" type="{L['jtype']}" axis="{_s(L['axis'])}" pos="{_s(L['jpos'])}"/>
          <geom type="box" size="{_s(L['half'])}" mass="{L['mass']}" pos="{_s(L['gpos'])}" euler="{_s(L['geuler'])}" contype="0" conaffinity="0"/>""")
        depth += 1
    return "".join(out) + "</body>" * depth + "</worldbody></mujoco>"


def chain_states(n=8, seed=12):
    rng = np.random.default_rng(seed)
    q = np.concatenate([rng.uniform(-1.5, 1.5, (n, 2)), rng.uniform(-0.1, 0.1, (n, 1))], axis=1)
    qd = np.concatenate([rng.uniform(-3, 3, (n, 2)), rng.uniform(-1, 1, (n, 1))], axis=1)
    return q, qd


def chain_fk(q):
    """fp64 forward kinematics written from the MJCF semantics: [(COM, inertial-frame rotation)] per link.  A body's frame is its parent's times (pos, euler);
    a hinge turns it about `axis` through the anchor `jpos` (both in the body frame), a slide moves it along `axis`."""
    p, R, out = np.array([0.0, 0.0, 1.0]), np.eye(3), []
    for L, qi in zip(CHAIN, q):
        p, R = p + R @ np.asarray(L["pos"]), R @ rot_euler(L["euler"])
        ax = np.asarray(L["axis"], dtype=np.float64); ax = ax / np.linalg.norm(ax)
        if L["jtype"] == "hinge":
            anchor = p + R @ np.asarray(L["jpos"])
            R = R @ rot_axis(ax, qi)
            p = anchor - R @ np.asarray(L["jpos"])
        else:
            p = p + R @ ax * qi
        out.append((p + R @ np.asarray(L["gpos"]), R @ rot_euler(L["geuler"])))
    return out


_STENCIL = ((1, 4.0 / 5), (2, -1.0 / 5), (3, 4.0 / 105), (4, -1.0 / 280))     # eighth-order central difference


def _ddir(q, dq, step=4e-3):
    """d/ds of chain_fk(q + s dq) at s = 0 by central differences: per link (COM velocity, angular velocity from dR/ds R^T).  Eighth-order stencil: the
    truncation error is of order (step |dq|)^8 / 630 and the rounding 1e-16 / step, both far below the 1e-12 the oracle twin is held to."""
    q, dq = np.asarray(q, dtype=np.float64), np.asarray(dq, dtype=np.float64)
    base = chain_fk(q)
    dc, dR = [np.zeros(3) for _ in base], [np.zeros((3, 3)) for _ in base]
    for k, c in _STENCIL:
        for sgn in (1.0, -1.0):
            for b, (com, Ri) in enumerate(chain_fk(q + sgn * k * step * dq)):
                dc[b] += sgn * c * com / step; dR[b] += sgn * c * Ri / step
    out = []
    for b, (com, Ri) in enumerate(base):
        W = dR[b] @ Ri.T
        out.append((dc[b], 0.5 * np.array([W[2, 1] - W[1, 2], W[0, 2] - W[2, 0], W[1, 0] - W[0, 1]])))
    return out


def chain_reference(q, qd, rho=RHO, mu=MU, wind=WIND):
    """qfrc_passive of the chain in one state: the fluid wrench of every link at its COM velocity (derivative of the FK along qd), projected on each joint by
    the virtual work of that link's COM displacement and rotation per unit q_i (derivative of the FK along e_i)."""
    fk, vel = chain_fk(q), _ddir(q, qd)
    wrench = [fluid_wrench(box_inertia(L["half"], L["mass"]), L["mass"], Ri, v, w, rho, mu, wind) for L, (com, Ri), (v, w) in zip(CHAIN, fk, vel)]
    out = np.zeros(len(CHAIN))
    for i in range(len(CHAIN)):
        for (F, T), (dc, dw) in zip(wrench, _ddir(q, np.eye(len(CHAIN))[i])):
            out[i] += F @ dc + T @ dw
    return out


# ---- 2. margin and gap / 3. mixing / 4. condim: a 5 cm ball on a plane ------------------------------------------------------------------------------------
BALL_R = 0.05
BALL_MASS = 1000 * 4 / 3 * np.pi * BALL_R ** 3


def resting_depth(a0, solref, solimp, h=H):
    """Resting violation r of one soft constraint that carries the acceleration a0: r = a0 (1 - d(r)) / (k d(r)^2), by fixed-point iteration on the documented
    impedance d(r) and spring k (tests/test_oracle.py: both written from the documentation's text, no simulator involved)."""
    from tests.test_oracle import _documented_impedance, _documented_spring
    k = _documented_spring(solref, solimp[1], h)
    r = a0 / k
    for _ in range(200):
        d = _documented_impedance(solimp, r)
        r = a0 * (1 - d) / (k * d * d)
    return r


def ball_plane_xml(plane="", ball="", option='cone="elliptic"', gravity=(0, 0, -G0)):
    """The ball of the resting-depth tests, touching the plane (dist = 0) at qpos0; `plane` / `ball`: further geom attributes."""
    return f"""<mujoco><option timestep="{H}" gravity="{_s(gravity)}" {option}/><worldbody><geom name="floor" type="plane" size="5 5 0.1" {plane}/>
      <body name="ball" pos="0 0 {BALL_R}"><freejoint/><geom name="ball" type="sphere" size="{BALL_R}" density="1000" {ball}/></body></worldbody></mujoco>"""


def sol_attrs(solref=SOLREF, solimp=SOLIMP):
    return f'solref="{_s(solref)}" solimp="{_s(solimp)}"'


MARGIN, GAP = 0.002, 0.0005
STATE_SEPARATIONS = (0.0021, 0.00175, 0.001, -0.0001)     # outside the margin; inside it but above margin - gap; rows active; penetrating
BOX_HALF_B = 0.04


def box_over_plane_xml(d, margin=MARGIN, gap=GAP):
    mg = f'margin="{margin}" gap="{gap}"'
    return f"""<mujoco><option timestep="{H}" cone="elliptic"/><worldbody><geom name="floor" type="plane" size="1 1 0.1" {mg}/>
      <body name="box" pos="0 0 {BOX_HALF_B + d!r}"><freejoint/><geom name="box" type="box" size="{BOX_HALF_B} {BOX_HALF_B} {BOX_HALF_B}" density="500" {mg}/></body></worldbody></mujoco>"""


def box_over_box_xml(d, margin=MARGIN, gap=GAP):
    """Face to face: a 8 cm cube, turned by 0.2 rad about z, over the top face (z = 0.1) of a fixed 20 x 20 x 10 cm box; no floor."""
    mg = f'margin="{margin}" gap="{gap}"'
    return f"""<mujoco><compiler angle="radian"/><option timestep="{H}" cone="elliptic"/><worldbody><geom name="slab" type="box" size="0.1 0.1 0.05" pos="0 0 0.05" {mg}/>
      <body name="box" pos="0.01 -0.02 {0.1 + BOX_HALF_B + d!r}" euler="0 0 0.2"><freejoint/><geom name="box" type="box" size="{BOX_HALF_B} {BOX_HALF_B} {BOX_HALF_B}" density="500" {mg}/></body>
      </worldbody></mujoco>"""


LIMIT_HI, LIMIT_MARGIN, LIMIT_TORQUE = 0.3, 0.05, 0.4
PENDULUM_INERTIA = 0.5 * 0.2 ** 2 + 0.4 * 0.5 * 0.02 ** 2       # a 2 cm ball of 0.5 kg at 0.2 m from the hinge


def limit_pendulum_xml(margin=LIMIT_MARGIN, solref=SOLREF, solimp=SOLIMP):
    """The limit pendulum of the resting-depth tests (hinge about y, range +-0.3 rad, a motor of gear 1) with a margin on the joint limit."""
    return f"""<mujoco><compiler angle="radian"/><option timestep="{H}" gravity="0 0 0"/><worldbody><body name="p"><joint name="h" type="hinge" axis="0 1 0" range="-{LIMIT_HI} {LIMIT_HI}"
      margin="{margin}" solreflimit="{_s(solref)}" solimplimit="{_s(solimp)}"/><geom type="sphere" size="0.02" pos="0.2 0 0" mass="0.5" contype="0" conaffinity="0"/></body></worldbody>
      <actuator><motor joint="h" gear="1"/></actuator></mujoco>"""


TENDON_COEF = 2.0


def tendon_limit_xml(margin=LIMIT_MARGIN, solref=SOLREF, solimp=SOLIMP):
    """The same pendulum, unlimited, under a fixed tendon of length 2 q limited to +-0.3 with a margin (the `lim_only` tendon of tests/golden/coupled_fingers.xml)."""
    return f"""<mujoco><compiler angle="radian"/><option timestep="{H}" gravity="0 0 0"/><worldbody><body name="p"><joint name="h" type="hinge" axis="0 1 0"/>
      <geom type="sphere" size="0.02" pos="0.2 0 0" mass="0.5" contype="0" conaffinity="0"/></body></worldbody>
      <tendon><fixed name="t" limited="true" range="-{LIMIT_HI} {LIMIT_HI}" margin="{margin}" solreflimit="{_s(solref)}" solimplimit="{_s(solimp)}"><joint joint="h" coef="{TENDON_COEF}"/></fixed></tendon>
      <actuator><motor joint="h" gear="1"/></actuator></mujoco>"""


# 3. mixing: the two geoms' parameters and the rows (solmix 1, solmix 2, priority 1, priority 2); geom 1 is the plane
MIX_SOL = (((0.02, 1.0), (0.9, 0.95, 0.001, 0.5, 2)), ((0.005, 0.6), (0.8, 0.9, 0.002, 0.4, 3)))
MIX_ROWS = ((1, 1, 0, 0), (3, 1, 0, 0), (0, 1, 0, 0), (0, 0, 0, 0), (1, 1, 1, 0), (1, 1, 0, 2))


def mix_xml(row):
    w1, w2, p1, p2 = row
    return ball_plane_xml(f'{sol_attrs(*MIX_SOL[0])} solmix="{w1}" priority="{p1}"', f'{sol_attrs(*MIX_SOL[1])} solmix="{w2}" priority="{p2}"')


def documented_mix(row):
    """(solref, solimp) of the contact by the documented rules: the higher priority's parameters; at equal priority the average weighted with
    w1 / (w1 + w2), where a weight below 1e-15 counts as zero (weight 0 or 1) and two such weights give 1 / 2."""
    w1, w2, p1, p2 = row
    if p1 != p2:
        return MIX_SOL[0 if p1 > p2 else 1]
    tiny = 1e-15
    mix = w1 / (w1 + w2) if (w1 >= tiny and w2 >= tiny) else 0.5 if (w1 < tiny and w2 < tiny) else (0.0 if w1 < tiny else 1.0)
    (r1, i1), (r2, i2) = MIX_SOL
    return tuple(mix * np.array(r1) + (1 - mix) * np.array(r2)), tuple(mix * np.array(i1) + (1 - mix) * np.array(i2))


# friction: (plane friction, box friction, plane priority, box priority) -> |f_t| / f_n of every slipping corner contact
FRICTION_ROWS = (((0.2, 0.5, 0, 0), 0.5), ((0.2, 0.5, 1, 0), 0.2), ((0.6, 0.3, 0, 1), 0.3))
FLAT_BOX_MASS = 400 * 0.2 * 0.2 * 0.02


def friction_xml(row):
    """The flat box of the Coulomb-threshold test (elliptic cone, impratio 20, four corner contacts) with different sliding friction on the two geoms."""
    f1, f2, p1, p2 = row
    return f"""<mujoco><option timestep="{H}" cone="elliptic" impratio="20"/><worldbody><geom type="plane" size="5 5 0.1" friction="{f1} 0.005 0.0001" priority="{p1}"/>
      <body pos="0 0 0.01"><freejoint/><geom type="box" size="0.1 0.1 0.01" density="400" friction="{f2} 0.005 0.0001" priority="{p2}"/></body></worldbody></mujoco>"""


# 4. condim 1: gravity tilted by THETA about y; (plane condim, ball condim, plane priority) -> contact dim = rows
THETA = 0.3
CONDIM_ROWS = (((1, 1, 0), 1), ((1, 3, 0), 3), ((1, 3, 1), 1))


def condim_xml(row):
    c1, c2, p1 = row
    return ball_plane_xml(f'{sol_attrs()} condim="{c1}" priority="{p1}"', f'{sol_attrs()} condim="{c2}"', gravity=(G0 * np.sin(THETA), 0, -G0 * np.cos(THETA)))


# ---- substeps after which the fp64 oracle has settled to |v| < 1e-6 (tests/test_known_answers_host.py asserts it at exactly these counts): measured first
# counts 113 / 109 (ball in the margin, gap 0 / 0.5 mm), 181 (limit pendulum from 0.2 rad), 172 (tendon twin from 0.1 rad), 18 .. 90 (the six mixing rows),
# 132 (flat box), 91 (normal velocity of the ball under tilted gravity).  At that moment the position is still some 1e-8 m and the force 2e-6 away from rest;
# some 60 substeps more bring them inside the 1e-9 m / 1e-6 the oracle twin is held to, and the counts are those, rounded up
SETTLE = {"margin_ball": 180, "limit_pendulum": 250, "limit_tendon": 250, "mix": 150, "friction": 200, "condim": 150}


# ---- 5. actuators ---------------------------------------------------------------------------------------------------------------------------------------
ACT_Q = (0.2, 0.1, 0.1, 0.01, 0.15, -0.12)
ACT_QVEL = (0.0, 0.0, 0.0, 0.0, 0.7, -0.9)
ACT_CTRL = (5.0, 0.3, 0.3, 0.5, 0.4, 0.25)
ACT_INERTIA, ACT_MASS = 1.5 / 3 * (0.1 ** 2 + 0.02 ** 2), 1.5


def actuator_xml():
    """One joint per actuator (the four of the earlier test, then <velocity> and an affine <general> with gear 2), no gravity."""
    body = '<body pos="0 {y} 0"><joint name="{n}" type="{t}" axis="{a}"/><geom type="box" size="0.1 0.02 0.02" mass="1.5" contype="0" conaffinity="0"/></body>'
    joints = (("a", "hinge", "0 0 1"), ("b", "hinge", "0 0 1"), ("c", "hinge", "0 0 1"), ("d", "slide", "1 0 0"), ("e", "hinge", "0 0 1"), ("f", "hinge", "0 0 1"))
    return (f'<mujoco><compiler angle="radian"/><option timestep="{H}" gravity="0 0 0"/><worldbody>' + "".join(body.format(y=i, n=n, t=t, a=a) for i, (n, t, a) in enumerate(joints))
            + """</worldbody><actuator><motor joint="a" gear="3" ctrllimited="true" ctrlrange="-1 1"/><position joint="b" kp="20"/>
              <position joint="c" kp="200" forcelimited="true" forcerange="-1 1"/><position joint="d" kp="50" ctrllimited="true" ctrlrange="0 0.04"/>
              <velocity joint="e" kv="4"/><general joint="f" gainprm="3" biastype="affine" biasprm="0.2 -5 -0.3" gear="2"/></actuator></mujoco>""")


def actuator_forces():
    """Generalised forces at (ACT_Q, ACT_QVEL, ACT_CTRL) as documented (XML reference: actuator/motor, position, velocity, general; Computation: actuation
    model): force = gain x clamp(ctrl) + bias . [1, length, velocity], clamped to forcerange, times the gear on the joint.  Length and velocity are the
    ACTUATOR's: for a joint transmission the documentation defines them as gear x q and gear x qvel, so the affine actuator with gear 2 gives
    gear (3 ctrl + 0.2 - 5 length - 0.3 velocity) = gear (3 ctrl + 0.2 - 5 (gear q) - 0.3 (gear qvel)): 5.38 N m at this state.  (With the bias taken on
    the bare joint coordinates, gear (3 ctrl + 0.2 - 5 q - 0.3 qvel), it would be 3.64 N m: the gear-2 case is there to tell the two apart.)"""
    q, v, u = ACT_Q, ACT_QVEL, ACT_CTRL
    gear = 2.0
    return np.array([3.0 * 1.0,                          # motor: ctrl clamped to 1, gear 3
                     20.0 * (u[1] - q[1]),               # position servo: kp (ctrl - q)
                     1.0,                                # 200 x 0.2 = 40 N m clamped to the force range
                     50.0 * (0.04 - q[3]),               # ctrl clamped to 0.04
                     4.0 * (u[4] - v[4]),                # velocity servo: kv (ctrl - qvel)
                     gear * (3.0 * u[5] + 0.2 - 5.0 * (gear * q[5]) - 0.3 * (gear * v[5]))])
