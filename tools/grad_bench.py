"""What the clearance gradient and the collision cost take beside the clearance query they are built on: Lift @4096, the default pair list without parent / child
pairs (tools/clearance_bench.py's list), K = 1, 16, 64.  config_clearance_grad against config_clearance, config_collision_cost against config_clearance, in one
session, alternated round by round; each figure is the median over the rounds of the mean over `--reps` back-to-back calls between two device syncs.

    python tools/grad_bench.py [--envs 4096] [--rounds 5] [--reps 5] [--out profiles/grad_bench.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch      # noqa: E402

from robosuite_amd import clearance      # noqa: E402
from tests import clearance_scenes as S      # noqa: E402
from tests import raycast_scenes as R      # noqa: E402
from tests.util import make_hip      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--d-safe", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    flat, cfg = R.lift()
    dofs = list(range(7))
    B = a.envs
    hm, hb = make_hip(flat, cfg, B=B)
    hb.set("qpos", np.tile(R.lift_init_qpos(flat, cfg), (B, 1)).astype(np.float32)); hb.set("qvel", 0); hb.forward()
    parent, gb = clearance._I(flat, "body_parentid"), clearance._I(flat, "geom_bodyid")
    pairs = np.array([p for p in clearance.default_pairs(flat, dofs) if parent[gb[p[0]]] != gb[p[1]] and parent[gb[p[1]]] != gb[p[0]]], dtype=np.int32)
    lines = [f"Lift @{B}, {len(pairs)} pairs (the default list without parent / child pairs), d_safe {a.d_safe}, {a.rounds} rounds x {a.reps} calls, alternated; ms per call",
             f"{'K':>3s} {'clearance':>10s} {'clearance_grad':>15s} {'ratio':>6s} {'collision_cost':>15s} {'ratio':>6s} {'near pairs / candidate':>23s}"]
    for K in (1, 16, 64):
        q = torch.as_tensor(np.tile(S.candidates(flat, dofs, 1, K), (B, 1, 1)) + np.random.default_rng(K).normal(0, 0.05, (B, K, 7)), dtype=torch.float32, device="cuda")
        calls = {"clear": lambda: hb.config_clearance(dofs, q, pairs=pairs, distmax=1.0), "grad": lambda: hb.config_clearance_grad(dofs, q, pairs=pairs, distmax=1.0),
                 "cost": lambda: hb.config_collision_cost(dofs, q, pairs=pairs, d_safe=a.d_safe)}
        for f in calls.values():      # warm-up: tables, scratch
            f()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k, f in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    f()
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) / a.reps * 1e3)
        m = {k: float(np.median(v)) for k, v in t.items()}
        near = float(calls["cost"]()[2].float().mean())
        lines.append(f"{K:3d} {m['clear']:10.3f} {m['grad']:15.3f} {m['grad'] / m['clear']:6.2f} {m['cost']:15.3f} {m['cost'] / m['clear']:6.2f} {near:23.2f}")
        print(lines[-1], flush=True)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
