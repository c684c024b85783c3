"""States a library build steps to from fixed inputs, for a bit-for-bit comparison of two builds of the narrow phase (tests/test_candidate_descriptors.py:
the default build, whose candidate descriptors are fetched one per lane, against -DRSIM_NO_CAND_PREFETCH, which fetches them candidate by candidate).

Usage (GPU box):  RSIM_LIB=/path/to/librsim_hip_<name>.so python tools/cand_desc_states.py <case> <out.npz>

  stack_over   tests/golden/stack_over_capacity.npz: 16 Stack envs whose control step outgrows the native body (both bodies of the kernel run), 3 control steps
  stack_mixed  the same states with mixed contact parameters: two priority classes, zero and unequal solmix weights, direct (negative) solref on some geoms --
               every branch of the pair-parameter rules, 2 control steps
  lift         8 envs from the recorded Lift / Panda trajectory (tests/golden/lift_panda_seed1_full), 6 control steps
  crowd        two free clusters of six convex geoms next to ten static ones, within each other's margins: about a hundred geom pairs pass the broadphase in every
               substep while few touch: more candidates than the wavefront has lanes, so candidates 64.. take the per-candidate path in both builds; 4 envs, 40 substeps"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = ("qpos", "qvel", "qacc_warmstart", "ctrl", "cstate", "contact", "efc_force", "ncon", "nefc", "niter", "cap_need", "overflow", "diverged")


def mix_contact_parameters(flat):
    """Per-geom contact parameters that send the geom pairs of a model through every branch of the mixing rules."""
    a = flat.arrays
    ng = len(a["geom_priority"])
    g = np.arange(ng)
    a["geom_priority"][:] = g % 2                                         # pairs of unequal priority take one side's parameters ...
    a["geom_solmix"][:] = np.where(g % 3 == 0, 0.0, 1.0 + 0.5 * (g % 4))  # ... equal priority: weights s1 / (s1 + s2), 0.5 (both zero), 0 or 1 (one zero)
    sr = a["geom_solref"].reshape(ng, 2)
    sr[g % 5 == 4] = (-4000.0, -120.0)                                    # direct stiffness / damping: the pair takes the element-wise minimum
    a["geom_friction"].reshape(ng, 3)[:, 0] *= 1.0 + 0.1 * (g % 3)
    a["geom_solimp"].reshape(ng, 5)[:, 0] = 0.9 - 0.02 * (g % 4)


def crowd_xml():
    """The clusters sit a little more than one diameter apart and every geom has a margin of more than that gap: every pair of cluster A with cluster B and with
    the static cluster passes the broadphase (6 x 6 + 6 x 10 = 96 candidates), and the narrow phase finds that few of them touch."""
    r = 0.05
    shapes = ('type="sphere" size="%g"' % r, 'type="ellipsoid" size="%g %g %g"' % (r, 0.9 * r, 0.8 * r), 'type="capsule" size="%g %g"' % (0.7 * r, 0.3 * r),
              'type="cylinder" size="%g %g"' % (0.9 * r, 0.9 * r), 'type="box" size="%g %g %g"' % (0.8 * r, 0.8 * r, 0.8 * r))
    geoms = lambda n, k0: "".join('<geom %s pos="%g %g %g"/>' % (shapes[(k0 + i) % len(shapes)], 0.0015 * i, 0.001 * i, -0.001 * i) for i in range(n))
    return ('<mujoco><option timestep="0.002"/><default><geom margin="0.06" gap="0.06"/></default><worldbody>'
            '<body name="s" pos="%g %g %g">%s</body>' % (1.5 * r, -1.5 * r, 0.5 - 0.3 * r, geoms(10, 0))
            + '<body name="a" pos="0 0 0.5"><freejoint/>%s</body>' % "".join('<geom type="sphere" size="%g" pos="%g %g %g"/>' % (r, 0.002 * i, -0.001 * i, 0.001 * i) for i in range(6))
            + '<body name="b" pos="%g %g %g"><freejoint/>%s</body>' % (1.35 * r, 1.35 * r, 0.5 + 1.35 * r, geoms(6, 1))
            + '</worldbody></mujoco>')


def run(case):
    import torch

    from robosuite_amd import mjcf
    from tests.util import load_golden, make_hip

    res = {}
    if case in ("stack_over", "stack_mixed"):
        adir = os.path.join(ROOT, "robosuite_amd", "assets")
        flat, cfg = mjcf.load_model(os.path.join(adir, "stack_panda.rsim")), json.load(open(os.path.join(adir, "stack_panda.cfg.json")))
        if case == "stack_mixed":
            mix_contact_parameters(flat)
        z = np.load(os.path.join(ROOT, "tests", "golden", "stack_over_capacity.npz"))
        n, n_sub = len(z["envs"]), int(z["n_sub"])
        hm, hb = make_hip(flat, cfg, B=n)
        for k in ("qpos", "qvel", "qacc_warmstart", "ctrl", "cstate"):
            hb.set(k, z[k])
        t0 = hb.tier_stats()
        for s in range(3 if case == "stack_over" else 2):
            hb.control_step(torch.tensor(z["actions"][:, s], dtype=torch.float32, device="cuda"), n_sub)
            for k in OUT:
                res[f"{k}_{s}"] = hb.get(k)
        t1 = hb.tier_stats()
        res["tier_steps"] = np.array([t1[0] - t0[0], t1[1] - t0[1]], dtype=np.int64)
    elif case == "lift":
        g, cfg, flat = load_golden("seed1_full")
        nq, B = flat.nq, 8
        hm, hb = make_hip(flat, cfg, B=B)
        s0 = g["states"][np.linspace(0, len(g["states"]) - 8, B).astype(int)]
        hb.set("qpos", s0[:, 1:1 + nq]); hb.set("qvel", s0[:, 1 + nq:]); hb.set("qacc_warmstart", 0); hb.set("ctrl", 0)
        hb.forward()
        hb.ctrl_reset()
        for s in range(6):
            hb.control_step(torch.tensor(np.repeat(g["actions"][s][None], B, 0), dtype=torch.float32, device="cuda"), 25)
            for k in OUT:
                res[f"{k}_{s}"] = hb.get(k)
    elif case == "crowd":
        flat = mjcf.compile_mjcf(crowd_xml())
        B = 4
        hm, hb = make_hip(flat, None, B=B)
        q0 = np.repeat(np.asarray(flat.qpos0, dtype=np.float64)[None], B, 0)
        q0[:, 7:10] += 0.002 * np.arange(B)[:, None]        # cluster b a little further out from env to env
        hb.set("qpos", q0); hb.set("qvel", 0); hb.set("qacc_warmstart", 0); hb.set("ctrl", 0)
        hb.forward()
        hb.profile(True)
        for s in range(40):
            hb.step()
            if s % 10 == 9:
                for k in OUT:
                    res[f"{k}_{s // 10}"] = hb.get(k)
                p = hb.profile(s < 39)       # the kernel's own event counters over these ten substeps of the four envs
                res[f"cand_per_env_substep_{s // 10}"] = np.array([p["n_cand"] / max(1, p["n_sub"])])
                res[f"mpr_per_env_substep_{s // 10}"] = np.array([p["n_mpr"] / max(1, p["n_sub"])])
    else:
        raise SystemExit(f"unknown case {case}")
    return res


if __name__ == "__main__":
    r = run(sys.argv[1])
    np.savez(sys.argv[2], **r)
    print(f"{os.environ.get('RSIM_LIB', 'default library')}: {sys.argv[1]}: {len(r)} arrays -> {sys.argv[2]}")
