"""What the M^-1 queries take beside what a user did before them: Lift @4096, the arm's seven dofs, K = 1, 16, 64.  Each new call -- config_forward_dynamics,
config_mass_solve (r = 6), config_opspace -- against the same result from the existing calls plus torch: config_mass_matrix (+ config_inverse_dynamics /
config_jacobian), torch.linalg.cholesky and torch.cholesky_solve in fp32 on the same tensors; and against config_mass_matrix alone, the floor (every chain
holds its kernels).  One session, alternated round by round; each figure is the median over the rounds of the mean over `--reps` back-to-back calls between two
device syncs.  Before timing, the two routes are compared on the timed inputs (largest difference relative to the largest entry).

Each route's entries that are not finite are counted and reported.

    python tools/dyn_solve_bench.py [--envs 4096] [--rounds 5] [--reps 5] [--out profiles/dyn_solve_bench.txt]      (the committed file: --reps 20)"""
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
    lines = [f"Lift @{B}, seven arm dofs, {a.rounds} rounds x {a.reps} calls, alternated; ms per call.  lib: the new call; torch: the existing calls + "
             "torch.linalg.cholesky + torch.cholesky_solve (fp32); floor: config_mass_matrix alone",
             f"{'K':>3s} {'floor':>8s} | {'fd lib':>8s} {'fd torch':>9s} {'ratio':>6s} | {'solve lib':>9s} {'solve torch':>11s} {'ratio':>6s} | {'opspace lib':>11s} "
             f"{'opspace torch':>13s} {'ratio':>6s} | {'lib / floor: fd':>15s} {'solve':>6s} {'opspace':>7s} | routes differ by (fd, solve, lambda_inv)"]
    for K in (1, 16, 64):
        rng = np.random.default_rng(K)
        q = torch.as_tensor(np.tile(S.candidates(flat, dofs, 1, K), (B, 1, 1)) + rng.normal(0, 0.05, (B, K, 7)), dtype=torch.float32, device="cuda")
        qd = torch.as_tensor(rng.uniform(-2, 2, (B, K, 7)), dtype=torch.float32, device="cuda")
        tau = torch.as_tensor(rng.uniform(-20, 20, (B, K, 7)), dtype=torch.float32, device="cuda")
        rhs = torch.as_tensor(rng.uniform(-1, 1, (B, K, 7, 6)), dtype=torch.float32, device="cuda")

        def fd_torch():
            b = (tau - hb.config_inverse_dynamics(dofs, q, qd))[..., None]
            return torch.cholesky_solve(b, torch.linalg.cholesky(hb.config_mass_matrix(dofs, q)))[..., 0]

        def solve_torch():
            return torch.cholesky_solve(rhs, torch.linalg.cholesky(hb.config_mass_matrix(dofs, q)))

        def opspace_torch():
            L = torch.linalg.cholesky(hb.config_mass_matrix(dofs, q))
            J = torch.cat(hb.config_jacobian(site, dofs, q), dim=-2)
            mjt = torch.cholesky_solve(J.transpose(-1, -2), L)
            return J @ mjt, mjt

        calls = {"floor": lambda: hb.config_mass_matrix(dofs, q), "fd": lambda: hb.config_forward_dynamics(dofs, q, qd, tau), "fd_t": fd_torch,
                 "solve": lambda: hb.config_mass_solve(dofs, q, rhs), "solve_t": solve_torch, "op": lambda: hb.config_opspace(site, dofs, q), "op_t": opspace_torch}
        out = {k: f() for k, f in calls.items()}      # warm-up: tables, scratch, torch's workspaces -- and the results of both routes
        torch.cuda.synchronize()
        diff = lambda x, y: float((x - y).abs().max() / y.abs().max())      # noqa: E731
        differ = (diff(out["fd"], out["fd_t"]), diff(out["solve"], out["solve_t"]), diff(out["op"][0], out["op_t"][0]))
        bad = {k: int((~torch.isfinite(v[0] if isinstance(v, tuple) else v)).sum()) for k, v in out.items()}
        if any(bad.values()):
            lines.append(f"    K = {K}: entries that are not finite, per route: {bad}")
            print(lines[-1], flush=True)
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
        lines.append(f"{K:3d} {m['floor']:8.3f} | {m['fd']:8.3f} {m['fd_t']:9.3f} {m['fd_t'] / m['fd']:5.2f}x | {m['solve']:9.3f} {m['solve_t']:11.3f} "
                     f"{m['solve_t'] / m['solve']:5.2f}x | {m['op']:11.3f} {m['op_t']:13.3f} {m['op_t'] / m['op']:5.2f}x | {m['fd'] / m['floor']:15.2f} "
                     f"{m['solve'] / m['floor']:6.2f} {m['op'] / m['floor']:7.2f} | {differ[0]:.1e} {differ[1]:.1e} {differ[2]:.1e}")
        print(lines[-1], flush=True)
    lines.append("ratio: torch route / library call (above 1: the library call is the faster one)")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
