"""States a library build steps to from fixed inputs, for the bit-for-bit comparison of the default build with -DRSIM_MPR_PRETEST_ALWAYS
(tests/test_mpr_touch_record.py): a visit of a convex pair whose warm-start record says the pair touched at its previous visit skips the primitive pretest
and starts MPR's cold run at once (rsim_step.hip Sim::convex_convex); the other build runs the pretest in front of every cold run.

Usage (GPU box):  RSIM_LIB=/path/to/librsim_hip_<name>.so python tools/mpr_touch_states.py <case> <out.npz>

  press   8 envs.  A convex mesh hull of 42 vertices on a hinge (about the vertical) on a sled (slide joint towards the axis of a fixed upright cylinder) flies
          into the cylinder's side, is stopped by the contact and pulled off again by a spring (a fixed tendon over the slide joint): contact made within the first few substeps,
          broken between substeps 20 and 30 (CPU oracle: contact from substep 3 or 4 to substep 26 - 28, depending on the env).  40 substeps, dumped every ten.  The envs
          differ in the hull's angle about the vertical (another facet, edge or vertex meets the cylinder) and in the approach speed.
  (the cases lift, stack_over and crowd of tools/cand_desc_states.py are run through this file as well, so that one tool serves the test)"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.cand_desc_states import OUT, run as cand_desc_run  # noqa: E402

R_CYL, R_HULL, GAP0 = 0.04, 0.03, 0.001


def hull_vertices():
    """An icosahedron with its edge midpoints pushed out to the sphere (42 vertices), squeezed to an ellipsoid-like body so that no two facets are alike."""
    t = (1 + 5 ** 0.5) / 2
    v = np.array([(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)], dtype=float)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    d = np.linalg.norm(v[:, None] - v[None], axis=2)
    edge = d[d > 0].min()
    mid = [(v[i] + v[j]) / 2 for i in range(12) for j in range(i + 1, 12) if d[i, j] < 1.01 * edge]
    m = np.array(mid); m /= np.linalg.norm(m, axis=1, keepdims=True)
    v = np.vstack([v, m]) * R_HULL
    assert len(v) == 42
    return (v * np.array([1.0, 0.85, 0.7])).astype(np.float32).astype(np.float64)


def press_xml(meshdir):
    v = hull_vertices()
    with open(os.path.join(meshdir, "hull42.obj"), "w") as f:
        f.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v) + "f 1 2 3\n")       # the compiler takes the convex hull of the vertices
    return ('<mujoco><compiler angle="radian" meshdir="%s"/><option timestep="0.002" gravity="0 0 0"/><asset><mesh name="hull42" file="hull42.obj"/></asset><worldbody>'
            '<geom name="post" type="cylinder" size="%g 0.1" pos="0 0 0.5"/>'
            '<body name="sled" pos="0 0 0.5"><joint name="in" type="slide" axis="1 0 0"/><geom type="sphere" size="0.005" contype="0" conaffinity="0"/>'
            '<body name="h"><joint name="turn" type="hinge" axis="0 0 1"/><geom name="hull" type="mesh" mesh="hull42"/></body></body></worldbody>'
            '<tendon><fixed name="pull" stiffness="20" springlength="%g"><joint joint="in" coef="1"/></fixed></tendon></mujoco>'       # (the kernel has tendon springs, no joint springs)
            % (meshdir, R_CYL, R_CYL + R_HULL + 0.008))


def press_inputs(B):
    q0, v0 = np.zeros((B, 2)), np.zeros((B, 2))
    q0[:, 1] = 0.37 * np.arange(B)                       # the hull's angle about the vertical: its extent along x differs from env to env ...
    v = hull_vertices()
    for e in range(B):
        c, s = np.cos(q0[e, 1]), np.sin(q0[e, 1])
        q0[e, 0] = R_CYL + GAP0 - (c * v[:, 0] - s * v[:, 1]).min()    # ... so every env starts 1 mm off the cylinder
    v0[:, 0] = -0.3 - 0.02 * np.arange(B)
    v0[:, 1] = 0.5
    return q0, v0


def run(case):
    if case != "press":
        return cand_desc_run(case)
    from robosuite_amd import mjcf
    from tests.util import make_hip

    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        flat = mjcf.compile_mjcf(press_xml(tmp))
    B = 8
    hm, hb = make_hip(flat, None, B=B)
    q0, v0 = press_inputs(B)
    hb.set("qpos", q0); hb.set("qvel", v0); hb.set("qacc_warmstart", 0); hb.set("ctrl", 0)
    hb.forward()
    for s in range(40):
        hb.step()
        if s % 10 == 9:
            for k in OUT:
                res[f"{k}_{s // 10}"] = hb.get(k)
    return res


if __name__ == "__main__":
    r = run(sys.argv[1])
    np.savez(sys.argv[2], **r)
    print(f"{os.environ.get('RSIM_LIB', 'default library')}: {sys.argv[1]}: {len(r)} arrays -> {sys.argv[2]}")
