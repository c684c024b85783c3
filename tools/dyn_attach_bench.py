"""What the carried payload costs in the dynamics queries: Lift @4096, the arm's seven dofs, the cube held on the eef body, K = 1, 16, 64.  Each of the six
calls three ways in one session, alternated round by round: plain; with attach and `held` all true (the payload); with attach and `held` all false (the cost
of the attached instantiation alone: its results are the plain call's bits).  Beside them the plain call a SECOND time -- two calls of one kind -- whose ratio
to the first is the spread any other ratio of the row is to be read against.  Each figure is the median over the rounds of the mean over `--reps` back-to-back
calls between two device syncs.

    python tools/dyn_attach_bench.py [--envs 4096] [--rounds 5] [--reps 5] [--out profiles/dyn_attach_bench.txt]"""
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
    att = [(flat.names["body"].index("cube_main"), int(np.asarray(flat.arrays["site_bodyid"]).ravel()[site]))]
    held = {"held": torch.ones(B, dtype=torch.bool, device="cuda"), "loose": torch.zeros(B, dtype=torch.bool, device="cuda")}
    lines = [f"Lift @{B}, seven arm dofs, cube_main on the eef body, {a.rounds} rounds x {a.reps} calls, alternated; ms per call",
             "plain / plain again (ratio: the two-calls-of-one-kind spread) / attach, held (ratio to plain) / attach, not held (ratio to plain)"]
    for K in (1, 16, 64):
        rng = np.random.default_rng(K)
        q = torch.as_tensor(np.tile(S.candidates(flat, dofs, 1, K), (B, 1, 1)) + rng.normal(0, 0.05, (B, K, 7)), dtype=torch.float32, device="cuda")
        qd = torch.as_tensor(rng.uniform(-2, 2, (B, K, 7)), dtype=torch.float32, device="cuda")
        qdd = torch.as_tensor(rng.uniform(-6, 6, (B, K, 7)), dtype=torch.float32, device="cuda")
        rhs = torch.as_tensor(rng.uniform(-1, 1, (B, K, 7)), dtype=torch.float32, device="cuda")
        six = {"inverse_dynamics": lambda **kw: hb.config_inverse_dynamics(dofs, q, qd, qdd, **kw), "mass_matrix": lambda **kw: hb.config_mass_matrix(dofs, q, **kw),
               "jacobian": lambda **kw: hb.config_jacobian(site, dofs, q, **kw), "forward_dynamics": lambda **kw: hb.config_forward_dynamics(dofs, q, qd, qdd, **kw),
               "mass_solve": lambda **kw: hb.config_mass_solve(dofs, q, rhs, **kw), "opspace": lambda **kw: hb.config_opspace(site, dofs, q, **kw)}
        for name, f in six.items():
            calls = {"plain": lambda f=f: f(), "again": lambda f=f: f(), "held": lambda f=f: f(attach=att, held=held["held"]),
                     "loose": lambda f=f: f(attach=att, held=held["loose"])}
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
            lines.append(f"K {K:3d} {name:17s} {m['plain']:9.3f} / {m['again']:9.3f} ({m['again'] / m['plain']:5.3f} x) / {m['held']:9.3f} ({m['held'] / m['plain']:5.3f} x) / "
                         f"{m['loose']:9.3f} ({m['loose'] / m['plain']:5.3f} x)")
            print(lines[-1], flush=True)
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
