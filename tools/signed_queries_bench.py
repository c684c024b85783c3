"""config_clearance(signed=True) and one solve_ik_avoid(signed=True) evaluation on the device, timed against the unsigned calls in one session, alternated: Lift
@4096 after a warm-up, the arm's default pair list without parent / child pairs (tools/penetration_bench.py's), K = 1 / 16 / 64 candidates per env, on two
workloads:
  1. the state as reset: every candidate is the env's own arm configuration shaken by 0.01 rad -- no overlaps, the signed call does what the unsigned one does;
  2. candidates over the whole joint ranges beside the table, tools/penetration_bench.py's workload: most wavefronts hold a lane that descends.
The IK rows time ONE evaluation (max_iters = 0: k_ika_init, one cost kernel, one step kernel) from workload 2's candidates at K = 1 / 16.
No ratio is promised.  Median of `rounds` rounds of `reps` calls, ms.

    python tools/signed_queries_bench.py [--envs 4096] [--out profiles/signed_queries_bench.txt]"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from robosuite_amd import clearance      # noqa: E402
from robosuite_amd.controllers import BatchState      # noqa: E402
from tests import clearance_scenes as S      # noqa: E402
from tests import raycast_scenes as R      # noqa: E402
from tests.util import make_hip      # noqa: E402
from tools.penetration_bench import alternate      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--d-safe", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("signed_queries_bench.py: no GPU visible (nothing here is measured on a CPU)")
    flat, cfg = R.lift()
    dofs, site = list(cfg["dof_idx"]), int(cfg["eef_site"])
    B = a.envs
    hm, hb = make_hip(flat, cfg, B=B)
    hb.set("qpos", np.tile(R.lift_init_qpos(flat, cfg), (B, 1)).astype(np.float32)); hb.set("qvel", 0); hb.forward(); hb.ctrl_reset()
    act = (torch.rand((B, hm.action_dim), device="cuda") * 2 - 1) * 0.3
    for _ in range(20):                     # warm-up: the envs leave the common reset pose
        hb.control_step(act, 25)
    hb.sync()
    parent, gb = clearance._I(flat, "body_parentid"), clearance._I(flat, "geom_bodyid")
    pairs = np.array([p for p in clearance.default_pairs(flat, dofs) if parent[gb[p[0]]] != gb[p[1]] and parent[gb[p[1]]] != gb[p[0]]], dtype=np.int32)
    qa = np.asarray(flat.arrays["jnt_qposadr"]).ravel()[[list(np.asarray(flat.arrays["jnt_dofadr"]).ravel()).index(d) for d in dofs]]
    arm = hb.get("qpos").astype(np.float64)[:, qa]
    lines = [f"Lift @{B}, {len(pairs)} pairs (the default list without parent / child pairs), {a.rounds} rounds x {a.reps} calls, alternated; ms per call",
             "config_clearance, automatic chunks:",
             f"{'workload':>10s} {'K':>3s} {'unsigned':>10s} {'signed':>10s} {'ratio':>6s} {'dist < 0 / candidate':>21s} {'status 2 / candidate':>21s}"]
    ranges = {}
    for name in ("reset", "ranges"):
        for K in (1, 16, 64):
            rng = np.random.default_rng(K)
            if name == "reset":
                q = arm[:, None, :] + rng.normal(0, 0.01, (B, K, 7))
            else:
                q = np.tile(S.candidates(flat, dofs, 1, K), (B, 1, 1)) + rng.normal(0, 0.05, (B, K, 7))
            q = torch.as_tensor(q, dtype=torch.float32, device="cuda")
            ranges[name, K] = q
            calls = {"plain": lambda: hb.config_clearance(dofs, q, pairs=pairs), "signed": lambda: hb.config_clearance(dofs, q, pairs=pairs, signed=True)}
            m = alternate(calls, a.rounds, a.reps)
            s, p = calls["signed"](), calls["plain"]()
            lines.append(f"{name:>10s} {K:3d} {m['plain']:10.3f} {m['signed']:10.3f} {m['signed'] / m['plain']:6.2f} {float((s[0] < 0).float().mean()):21.3f} "
                         f"{float((p[3] & 2 != 0).float().mean()):21.3f}")
            print(lines[-1], flush=True)
    lines += [f"solve_ik_avoid, ONE evaluation (max_iters 0), d_safe {a.d_safe}, position targets at the site's current place, starts: the `ranges` candidates:",
              f"{'K':>3s} {'unsigned':>10s} {'signed':>10s} {'ratio':>6s} {'dist < 0 / start':>17s}"]
    tip = BatchState(hb).site_pose(site)[0].float().clone()
    for K in (1, 16):
        q0, pos = ranges["ranges", K], tip[:, None, :].repeat(1, K, 1).contiguous()
        kw = dict(pairs=pairs, d_safe=a.d_safe, max_iters=0)
        calls = {"plain": lambda: hb.solve_ik_avoid(site, dofs, pos, None, q0, **kw), "signed": lambda: hb.solve_ik_avoid(site, dofs, pos, None, q0, signed=True, **kw)}
        m = alternate(calls, a.rounds, a.reps)
        s = calls["signed"]()
        lines.append(f"{K:3d} {m['plain']:10.3f} {m['signed']:10.3f} {m['signed'] / m['plain']:6.2f} {float(s[7].float().mean()):17.3f}")
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
