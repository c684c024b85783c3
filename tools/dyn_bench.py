"""What the dynamics queries take beside the FK query they are built on: Lift @4096, the arm's seven dofs, K = 1, 16, 64.  config_inverse_dynamics (with qd and
qdd), config_mass_matrix and config_jacobian against config_fk of the same shape -- the floor: every chain starts with its kernel -- in one session, alternated
round by round; each figure is the median over the rounds of the mean over `--reps` back-to-back calls between two device syncs.

    python tools/dyn_bench.py [--envs 4096] [--rounds 5] [--reps 5] [--out profiles/dyn_bench.txt]"""
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
    dofs, site = list(range(7)), int(cfg["eef_site"])
    B = a.envs
    hm, hb = make_hip(flat, cfg, B=B)
    hb.set("qpos", np.tile(R.lift_init_qpos(flat, cfg), (B, 1)).astype(np.float32)); hb.set("qvel", 0); hb.forward()
    lines = [f"Lift @{B}, seven arm dofs, {a.rounds} rounds x {a.reps} calls, alternated; ms per call (ratio to config_fk), then million candidates per second",
             f"{'K':>3s} {'config_fk':>10s} {'inverse_dynamics':>24s} {'mass_matrix':>24s} {'jacobian':>24s}   {'Mcand/s: fk':>11s} {'id':>7s} {'M':>7s} {'J':>7s}"]
    for K in (1, 16, 64):
        rng = np.random.default_rng(K)
        q = torch.as_tensor(np.tile(S.candidates(flat, dofs, 1, K), (B, 1, 1)) + rng.normal(0, 0.05, (B, K, 7)), dtype=torch.float32, device="cuda")
        qd = torch.as_tensor(rng.uniform(-2, 2, (B, K, 7)), dtype=torch.float32, device="cuda")
        qdd = torch.as_tensor(rng.uniform(-6, 6, (B, K, 7)), dtype=torch.float32, device="cuda")
        calls = {"fk": lambda: hb.config_fk(dofs, q), "id": lambda: hb.config_inverse_dynamics(dofs, q, qd, qdd), "M": lambda: hb.config_mass_matrix(dofs, q),
                 "J": lambda: hb.config_jacobian(site, dofs, q)}
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
        rate = {k: B * K / (v * 1e-3) / 1e6 for k, v in m.items()}
        cell = lambda k: f"{m[k]:14.3f} ({m[k] / m['fk']:5.2f} x)"      # noqa: E731
        lines.append(f"{K:3d} {m['fk']:10.3f} {cell('id')} {cell('M')} {cell('J')}   {rate['fk']:11.1f} {rate['id']:7.1f} {rate['M']:7.1f} {rate['J']:7.1f}")
        print(lines[-1], flush=True)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
