"""Generated models that sit on the dof and body capacity edges of the compiled kernel configurations; shared by tests/test_capacity_edges_host.py
(CPU) and tests/test_capacity_edges.py (GPU).  MJCF strings for mjcf.compile_mjcf, parametrised by counts, deterministic, no fixture files.

rsim_batch_create picks the smallest configuration that holds a model (config_holds in csrc/rsim_api.cpp): nbody x nv of 32 x 16, 32 x 32, 64 x 16,
64 x 48, 64 x 64 (configurations 0 - 4); njnt <= 16 for 0 - 2 and <= 32 for 3 / 4; articulated trees <= 4 for 0 - 2 and <= 8 for 3 / 4; nq <= nv + 8;
nu <= 16.  The ingredients below set nv, nq, nbody and the tree count independently of each other within those limits:

  chain        fixed base, `n_hinge` hinges (axes x / y / z in turn, every fifth limited to +-0.4 rad) and `n_ball` ball joints, at the tip or in mid-chain; 6 cm capsule links
               that collide with nothing, damping 0.05, armature 0.01; a site on the base and one on the tip; motors (ctrlrange +-2) on the first 16 hinges at most
  welds        `n_weld` jointless bodies between the links (nbody without nv)
  free bodies  `n_free` boxes / spheres in turn, 0.5 mm deep in the floor on a 0.25 m grid: one articulated tree, six dofs, seven qpos entries, one
               to four contacts each
  chain_last   free joints before the chain (its dense mass-matrix block holds the top dof indices and straddles the last tile boundary) or after
               it (the contact rows touch the top dofs)
"""
AXES = ("1 0 0", "0 1 0", "0 0 1")
_WELD = '<body name="w{k}" pos="0.01 0 0"><geom type="sphere" size="0.01" density="800" contype="0" conaffinity="0"/>'


def chain_xml(n_hinge, n_ball=0, n_weld=0, ball_after=None):
    """`ball_after`: the ball joints follow that many hinges (default: all of them, i.e. the balls end the chain)."""
    ch, depth, w = ['<body name="base" pos="0 0 1.2"><site name="base_site"/>'], 1, n_weld
    first = n_hinge if ball_after is None else ball_after
    for i in range(n_hinge + n_ball):
        if w > 0 and i % 2 == 1:
            ch.append(_WELD.format(k=w)); depth += 1; w -= 1
        if first <= i < first + n_ball:
            j = f'<joint name="b{i - first}" type="ball" damping="0.05" armature="0.01"/>'
        else:
            h = i if i < first else i - n_ball
            lim = ' limited="true" range="-0.4 0.4"' if h % 5 == 4 else ""
            j = f'<joint name="h{h}" type="hinge" axis="{AXES[h % 3]}" damping="0.05" armature="0.01"{lim}/>'
        ch.append(f'<body name="l{i}" pos="0.06 0 {0.02 * ((i % 3) - 1)}">{j}'
                  '<geom type="capsule" size="0.015" fromto="0 0 0 0.06 0 0" density="800" contype="0" conaffinity="0"/>')
        depth += 1
    while w > 0:
        ch.append(_WELD.format(k=w)); depth += 1; w -= 1
    ch.append('<site name="tip"/>' + "</body>" * depth)
    return "".join(ch)


def _wrap(chain, free, n_motor, chain_last):
    return ('<mujoco><compiler angle="radian"/><option timestep="0.002" cone="elliptic"/><worldbody><geom name="floor" type="plane" size="3 3 0.1"/>'
            + (free + chain if chain_last else chain + free) + "</worldbody><actuator>"
            + "".join(f'<motor name="m{i}" joint="h{i}" gear="1" ctrllimited="true" ctrlrange="-2 2"/>' for i in range(n_motor)) + "</actuator></mujoco>")


def model_xml(n_hinge, n_free, n_ball=0, n_weld=0, chain_last=True, ball_after=None):
    fr = []
    for i in range(n_free):
        x, y = 0.25 * (i % 4) - 0.4, 0.25 * (i // 4) - 0.6
        g, z = ('type="box" size="0.04 0.03 0.05"', 0.0495) if i % 2 == 0 else ('type="sphere" size="0.04"', 0.0395)
        fr.append(f'<body name="f{i}" pos="{x} {y} {z}"><freejoint/><geom name="fg{i}" {g} density="500"/></body>')
    return _wrap(chain_xml(n_hinge, n_ball, n_weld, ball_after), "".join(fr), min(n_hinge, 16), chain_last)


def overflow_xml(n_hinge=22):
    """Seven boxes in a pile, every contact 1 mm deep: four of half-size 0.05 in the floor (16 contacts), two of 0.05 x 0.045 x 0.05 across pairs of them
    (2 x 2 x 4) and one across those two (2 x 4): 40 contacts / 120 rows, above the 32 contacts of the largest configuration.  Chain last."""
    b = [(f"{sx * 0.06} {sy * 0.06} 0.049", "0.05 0.05 0.05") for sx in (-1, 1) for sy in (-1, 1)]
    b += [(f"0 {sy * 0.06} 0.148", "0.05 0.045 0.05") for sy in (-1, 1)]
    b += [("0 0 0.247", "0.05 0.05 0.05")]
    fr = "".join(f'<body name="f{i}" pos="{p}"><freejoint/><geom name="fg{i}" type="box" size="{s}" density="500"/></body>' for i, (p, s) in enumerate(b))
    return _wrap(chain_xml(n_hinge), fr, min(n_hinge, 16), True)


# name: (configuration, dict(model_xml arguments), nv, nq, njnt, nbody or None)
COMPOSITIONS = {
    "cfg0_top":        (0, dict(n_hinge=10, n_free=1), 16, 17, 11, None),
    "cfg0_top_nb32":   (0, dict(n_hinge=10, n_free=1, n_weld=19), 16, 17, 11, 32),
    "cfg2_nb33":       (2, dict(n_hinge=10, n_free=1, n_weld=20), 16, 17, 11, 33),
    "cfg2_nb64":       (2, dict(n_hinge=10, n_free=1, n_weld=51), 16, 17, 11, 64),
    "cfg1_bottom":     (1, dict(n_hinge=11, n_free=1), 17, 18, 12, None),
    "cfg1_nv31":       (1, dict(n_hinge=13, n_free=3), 31, 34, 16, None),
    "cfg1_top":        (1, dict(n_hinge=11, n_free=3, n_ball=1), 32, 36, 15, None),
    "cfg1_top_nb32":   (1, dict(n_hinge=11, n_free=3, n_ball=1, n_weld=15), 32, 36, 15, 32),
    "cfg3_bottom":     (3, dict(n_hinge=15, n_free=3), 33, 36, 18, None),
    "cfg3_nv47":       (3, dict(n_hinge=23, n_free=4), 47, 51, 27, None),
    "cfg3_top":        (3, dict(n_hinge=24, n_free=4), 48, 52, 28, None),
    "cfg3_top_nb64":   (3, dict(n_hinge=24, n_free=4, n_weld=34), 48, 52, 28, 64),
    "cfg4_bottom":     (4, dict(n_hinge=7, n_free=7), 49, 56, 14, None),
    "cfg4_nv63":       (4, dict(n_hinge=21, n_free=7), 63, 70, 28, None),
    "cfg4_top":        (4, dict(n_hinge=22, n_free=7), 64, 71, 29, None),
    "cfg4_top_nb64":   (4, dict(n_hinge=22, n_free=7, n_weld=33), 64, 71, 29, 64),
    # beside the issue's rows: the body edge of configuration 1 without a ball joint
    "cfg1_nv31_nb32":  (1, dict(n_hinge=13, n_free=3, n_weld=14), 31, 34, 16, 32),
    # the qpos edge of the build that carries ball joints: nq = nv + 8 = 40, six ball joints in mid-chain (a hinge, the balls, a hinge: every ball has descendants)
    "cfg1_nq40":       (1, dict(n_hinge=2, n_free=2, n_ball=6, ball_after=1), 32, 40, 10, None),
}
# the top dof edge of every configuration, where both orders are run
TOP_EDGES = ("cfg0_top", "cfg1_nv31", "cfg1_top", "cfg3_top", "cfg4_top")
# contacts / constraint rows of the fp64 oracle at the three states the GPU tests compare (start, 25 and 50 substeps on; (chain last, chain first)): what
# the contact rows of those cases rest on -- at nv 48 chain first 10 contacts / 30 rows, at nv 64 19 / 57 after settling (rows beyond three per contact: joint limits)
TOP_COUNTS = {
    "cfg0_top":  ([(4, 13), (4, 13), (4, 12)], [(4, 13), (2, 7), (4, 12)]),
    "cfg1_nv31": ([(9, 28), (7, 22), (9, 27)], [(9, 28), (9, 28), (9, 27)]),
    "cfg1_top":  ([(9, 28), (9, 28), (9, 27)], [(9, 28), (7, 22), (9, 27)]),
    "cfg3_top":  ([(10, 31), (5, 16), (8, 24)], [(10, 31), (8, 25), (10, 30)]),
    "cfg4_top":  ([(19, 58), (16, 49), (19, 57)], [(19, 58), (16, 49), (19, 57)]),
}
# beyond the largest configuration by one: dof, body, tree; nq 73 at nv 64 (a ball joint carries four qpos entries on three dofs: eight trees give nq - nv = 8
# at most without, so on the 64 x 64 build, which carries no ball joints, the nq limit cannot be reached and this model meets the ball-joint refusal first);
# nq41: one qpos entry beyond nv + 8 on the 32 x 32 build, which does carry them (nine ball joints + five hinges, nv 32, one tree, every other count within its limits)
REFUSED = {
    "nv65":    dict(n_hinge=23, n_free=7),
    "nbody65": dict(n_hinge=22, n_free=7, n_weld=34),
    "trees9":  dict(n_hinge=10, n_free=8),
    "nq73":    dict(n_hinge=16, n_free=7, n_ball=2),
    "nq41":    dict(n_hinge=5, n_free=0, n_ball=9, ball_after=2),
}


def build(name, chain_last=True):
    """(configuration, compiled model) of a COMPOSITIONS row."""
    from robosuite_amd import mjcf
    cfg, kw, *_ = COMPOSITIONS[name]
    return cfg, mjcf.compile_mjcf(model_xml(chain_last=chain_last, **kw))


def start_state(flat, seed, amp=0.5, sigma=0.2):
    """qpos0 with the chain's hinge angles drawn in +-amp rad (beyond the +-0.4 of the limited ones), ball joints turned by up to amp rad and qvel ~ N(0, sigma)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    q = np.array(flat.qpos0, dtype=np.float64)
    for j in range(len(flat.jnt_type)):
        if int(flat.jnt_type[j]) == 3:
            q[int(flat.jnt_qposadr[j])] = rng.uniform(-amp, amp)
        elif int(flat.jnt_type[j]) == 1:       # ball: a rotation of up to amp rad about a seeded axis
            ax, ang, a = rng.standard_normal(3), rng.uniform(-amp, amp), int(flat.jnt_qposadr[j])
            q[a], q[a + 1:a + 4] = np.cos(ang / 2), np.sin(ang / 2) * ax / np.linalg.norm(ax)
    return q, sigma * rng.standard_normal(flat.nv)
