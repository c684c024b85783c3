"""What the derivatives of the dynamics cost: Lift @4096, the arm's seven dofs, K = 1, 16, 64, in one session, alternated round by round:
  id        one config_inverse_dynamics call                       id again   the same a second time: the two-calls-of-one-kind spread
  4n id     4 n = 28 such calls back to back: what central differences in q and qd cost a user without the analytic blocks
  grad      one config_inverse_dynamics_grad call (tau and the two n x n blocks: 2 n tangent walks in a loop inside the lane, behind the primal walk)
  jvp       one config_inverse_dynamics_jvp call (one tangent walk)
  fd        one config_forward_dynamics call                       fd grad    one config_forward_dynamics_grad call
Each figure is the median over the rounds of the mean over `--reps` back-to-back calls between two device syncs, in ms; the ratios are of those medians.  At
K = 1 the 4096 candidates are 64 wavefronts on 256 compute units: every figure there is the latency of one wavefront's walk plus the launch chain, not
throughput -- the fill is printed beside K.  No threshold is attached to any figure.

    python tools/dyn_grad_bench.py [--envs 4096] [--rounds 5] [--reps 5] [--out profiles/dyn_grad_bench.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch      # noqa: E402

from tests import clearance_scenes as S      # noqa: E402
from tests import raycast_scenes as R      # noqa: E402
from tests.util import make_hip      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    flat, cfg = R.lift()
    dofs, n = list(range(7)), 7
    B = a.envs
    hm, hb = make_hip(flat, cfg, B=B)
    hb.set("qpos", np.tile(R.lift_init_qpos(flat, cfg), (B, 1)).astype(np.float32)); hb.set("qvel", 0); hb.forward()
    lines = [f"Lift @{B}, seven arm dofs, {a.rounds} rounds x {a.reps} calls, alternated; ms per call (4n id: ms per {4 * n} calls)",
             "id / id again (x id) / 4n id (x id) / grad (x id; x 4n id) / jvp (x id) / fd / fd grad (x fd)"]
    for K in (1, 16, 64):
        rng = np.random.default_rng(K)
        q = torch.as_tensor(np.tile(S.candidates(flat, dofs, 1, K), (B, 1, 1)) + rng.normal(0, 0.05, (B, K, n)), dtype=torch.float32, device="cuda")
        qd = torch.as_tensor(rng.uniform(-2, 2, (B, K, n)), dtype=torch.float32, device="cuda")
        qdd = torch.as_tensor(rng.uniform(-6, 6, (B, K, n)), dtype=torch.float32, device="cuda")
        tau = torch.as_tensor(rng.uniform(-20, 20, (B, K, n)), dtype=torch.float32, device="cuda")
        d = torch.as_tensor(rng.uniform(-1, 1, (B, K, n)), dtype=torch.float32, device="cuda")
        one = lambda: hb.config_inverse_dynamics(dofs, q, qd, qdd)      # noqa: E731

        def many():
            for _ in range(4 * n):
                one()

        calls = {"id": one, "again": one, "4n": many, "grad": lambda: hb.config_inverse_dynamics_grad(dofs, q, qd, qdd),
                 "jvp": lambda: hb.config_inverse_dynamics_jvp(dofs, q, qd, qdd, d, d, d), "fd": lambda: hb.config_forward_dynamics(dofs, q, qd, tau),
                 "fdg": lambda: hb.config_forward_dynamics_grad(dofs, q, qd, tau)}
        for g in calls.values():      # warm-up: tables, scratch, code objects
            g()
        torch.cuda.synchronize()
        t = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k, g in calls.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    g()
                torch.cuda.synchronize()
                t[k].append((time.perf_counter() - t0) / a.reps * 1e3)
        m = {k: float(np.median(v)) for k, v in t.items()}
        waves = (B * K + 63) // 64
        lines.append(f"K {K:3d} ({waves} wavefronts, {waves / 1024:.2f} per SIMD)  {m['id']:8.3f} / {m['again']:8.3f} ({m['again'] / m['id']:5.3f} x) / {m['4n']:8.3f} "
                     f"({m['4n'] / m['id']:5.2f} x) / {m['grad']:8.3f} ({m['grad'] / m['id']:5.2f} x; {m['grad'] / m['4n']:5.3f} x) / {m['jvp']:8.3f} "
                     f"({m['jvp'] / m['id']:5.2f} x) / {m['fd']:8.3f} / {m['fdg']:8.3f} ({m['fdg'] / m['fd']:5.2f} x)")
        print(lines[-1], flush=True)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
