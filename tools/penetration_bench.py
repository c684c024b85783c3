"""The signed-overlap queries on the device, timed against the unsigned ones in one session, alternated: Lift @4096 after a warm-up,
  * geom_distance signed against unsigned on the collision pair list (tools/grad_bench.py's: the arm's default list without parent / child pairs), with the share
    of pairs that descend and their mean projection count;
  * config_collision_cost signed against unsigned at K = 1 / 16 / 64 candidates per env on the same list.
No ratio is promised: the descent is paid only by overlapping lanes, and a wavefront waits for its slowest lane.  Median of `rounds` rounds of `reps` calls, ms.

    python tools/penetration_bench.py [--envs 4096] [--out profiles/penetration_bench.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from robosuite_amd import clearance      # noqa: E402
from tests import clearance_scenes as S      # noqa: E402
from tests import raycast_scenes as R      # noqa: E402
from tests.util import make_hip      # noqa: E402


def alternate(calls, rounds, reps):
    for f in calls.values():      # warm-up: tables, scratch
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(rounds):
        for k, f in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                f()
            torch.cuda.synchronize()
            t[k].append((time.perf_counter() - t0) / reps * 1e3)
    return {k: float(np.median(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--d-safe", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("penetration_bench.py: no GPU visible (nothing here is measured on a CPU)")
    flat, cfg = R.lift()
    dofs = list(range(7))
    B = a.envs
    hm, hb = make_hip(flat, cfg, B=B)
    hb.set("qpos", np.tile(R.lift_init_qpos(flat, cfg), (B, 1)).astype(np.float32)); hb.set("qvel", 0); hb.forward(); hb.ctrl_reset()
    act = (torch.rand((B, hm.action_dim), device="cuda") * 2 - 1) * 0.3
    for _ in range(20):                     # warm-up: the envs leave the common reset pose
        hb.control_step(act, 25)
    hb.sync()
    parent, gb = clearance._I(flat, "body_parentid"), clearance._I(flat, "geom_bodyid")
    pairs = np.array([p for p in clearance.default_pairs(flat, dofs) if parent[gb[p[0]]] != gb[p[1]] and parent[gb[p[1]]] != gb[p[0]]], dtype=np.int32)
    lines = [f"Lift @{B}, {len(pairs)} pairs (the default list without parent / child pairs), {a.rounds} rounds x {a.reps} calls, alternated; ms per call"]
    _, _, st = hb.geom_distance(pairs)
    _, _, _, steps = hb.geom_distance(pairs, signed=True, steps=True)
    desc = steps[steps > 0].float()
    lines.append(f"geom_distance: {float((st & 2 != 0).float().mean()) * 100:.2f} % of the pairs overlap (status 2), {float((steps > 0).float().mean()) * 100:.2f} % descend, "
                 f"{float(desc.mean()) if desc.numel() else 0.0:.2f} projections each on average, worst {int(steps.max())}; wavefronts (pair, 64 envs) with a descending lane: "
                 f"{float((steps.reshape(-1, 64, steps.shape[1]) > 0).any(dim=1).float().mean()) * 100:.1f} %" if B % 64 == 0 else "")
    m = alternate({"plain": lambda: hb.geom_distance(pairs), "signed": lambda: hb.geom_distance(pairs, signed=True)}, a.rounds, a.reps)
    lines.append(f"geom_distance            unsigned {m['plain']:9.3f}   signed {m['signed']:9.3f}   ratio {m['signed'] / m['plain']:6.2f}")
    print("\n".join(lines), flush=True)
    lines.append(f"config_collision_cost, d_safe {a.d_safe}:")
    lines.append(f"{'K':>3s} {'unsigned':>10s} {'signed':>10s} {'ratio':>6s} {'near pairs / candidate':>23s} {'dist < 0 / candidate':>21s} {'status 2 / candidate':>21s}")
    for K in (1, 16, 64):
        q = torch.as_tensor(np.tile(S.candidates(flat, dofs, 1, K), (B, 1, 1)) + np.random.default_rng(K).normal(0, 0.05, (B, K, 7)), dtype=torch.float32, device="cuda")
        calls = {"plain": lambda: hb.config_collision_cost(dofs, q, pairs=pairs, d_safe=a.d_safe),
                 "signed": lambda: hb.config_collision_cost(dofs, q, pairs=pairs, d_safe=a.d_safe, signed=True)}
        m = alternate(calls, a.rounds, a.reps)
        s, p = calls["signed"](), calls["plain"]()
        lines.append(f"{K:3d} {m['plain']:10.3f} {m['signed']:10.3f} {m['signed'] / m['plain']:6.2f} {float(s[2].float().mean()):23.2f} {float(s[3].float().mean()):21.3f} "
                     f"{float(p[3].float().mean()):21.3f}")
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
