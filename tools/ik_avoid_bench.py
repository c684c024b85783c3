"""Collision-aware IK on the device, timed: Lift @4096 (the Panda), the default pair list without parent / child pairs (tools/clearance_bench.py's list), K = 1
and 16 problems per env, pose targets drawn as in tools/ik_bench.py (the pose at joint angles drawn inside the ranges, start vectors 0.3 rad around them).

  * time per call and per evaluation of `solve_ik_avoid` (max_iters + 1 evaluations with check_every = 0), alternated round by round in one session against ONE
    `config_collision_cost` call of the same shape -- the floor of an evaluation; the ratio is reported, not fixed in advance;
  * check_every 0 against 8;
  * the share of targets where plain IK's answer has clearance below d_safe / 2 and the new call finishes.

Each figure is the median over the rounds of the mean over `--reps` back-to-back calls between two device syncs.

    python tools/ik_avoid_bench.py [--envs 4096] [--rounds 5] [--reps 3] [--out profiles/ik_avoid_bench.txt]"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch      # noqa: E402

from robosuite_amd import clearance, ik      # noqa: E402
from robosuite_amd.controllers import BatchState      # noqa: E402
from tests import raycast_scenes as R      # noqa: E402
from tests.util import make_hip      # noqa: E402
from tools.ik_bench import site_quat      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--d-safe", type=float, default=0.05)
    ap.add_argument("--max-iters", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ik_avoid_bench.py: no GPU visible (nothing here is measured on a CPU)")
    flat, cfg = R.lift()
    B, KMAX = a.envs, 16
    hm, hb = make_hip(flat, cfg, B=B)
    init = np.tile(R.lift_init_qpos(flat, cfg), (B, 1)).astype(np.float32)
    hb.set("qpos", init); hb.set("qvel", 0); hb.forward()
    st = BatchState(hb)
    site, dofs, qidx = int(cfg["eef_site"]), list(cfg["dof_idx"]), list(cfg["qpos_idx"])
    n = len(dofs)
    parent, gb = clearance._I(flat, "body_parentid"), clearance._I(flat, "geom_bodyid")
    pairs = np.array([p for p in clearance.default_pairs(flat, dofs) if parent[gb[p[0]]] != gb[p[1]] and parent[gb[p[1]]] != gb[p[0]]], dtype=np.int32)
    _, jid = ik.chain(flat, site, dofs)
    rng = np.asarray(flat.arrays["jnt_range"], dtype=np.float32).reshape(-1, 2)[jid]
    lo, hi = torch.as_tensor(rng[:, 0], device="cuda"), torch.as_tensor(rng[:, 1], device="cuda")
    saved = st.qpos.clone()
    g = torch.Generator(device="cuda").manual_seed(1)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    pos, quat, qi = [], [], []
    for _ in range(KMAX):
        qt = mid + 0.9 * half * (torch.rand((B, n), device="cuda", generator=g) * 2 - 1)
        st.qpos[:, qidx] = qt
        hb.forward()
        pos.append(st.site_pose(site)[0].clone()); quat.append(site_quat(st, site).clone())
        qi.append(torch.minimum(torch.maximum(qt + 0.3 * (torch.rand((B, n), device="cuda", generator=g) * 2 - 1), lo), hi))
    pos, quat, qi = torch.stack(pos, 1).contiguous(), torch.stack(quat, 1).contiguous(), torch.stack(qi, 1).contiguous()
    st.qpos.copy_(saved); hb.forward(); hb.sync()
    ev = a.max_iters + 1
    lines = [f"Lift @{B}, {len(pairs)} pairs (the default list without parent / child pairs), pose targets, d_safe {a.d_safe}, max_iters {a.max_iters} ({ev} evaluations), "
             f"{a.rounds} rounds x {a.reps} calls, alternated; ms",
             f"{'K':>3s} {'collision_cost':>15s} {'avoid / call':>13s} {'/ evaluation':>13s} {'ratio':>6s} {'check_every 8':>14s} {'plain solve_ik':>15s} | "
             f"{'grazing':>8s} {'repaired':>9s} {'finished':>9s} {'mean it':>8s}"]
    for K in (1, KMAX):
        p, qt, q0 = pos[:, :K].contiguous(), quat[:, :K].contiguous(), qi[:, :K].contiguous()
        kw = dict(pairs=pairs, d_safe=a.d_safe, max_iters=a.max_iters)
        calls = {"cost": lambda: hb.config_collision_cost(dofs, q0, pairs=pairs, d_safe=a.d_safe), "avoid": lambda: hb.solve_ik_avoid(site, dofs, p, qt, q0, **kw),
                 "avoid8": lambda: hb.solve_ik_avoid(site, dofs, p, qt, q0, check_every=8, **kw), "plain": lambda: hb.solve_ik(site, dofs, p, qt, q0, max_iters=a.max_iters)}
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
        out, plain = calls["avoid"](), calls["plain"]()
        d0 = hb.config_clearance(dofs, plain[0], pairs=pairs, distmax=1.0)[0]
        graze = plain[3] & (d0 < 0.5 * a.d_safe)
        fixed = graze & out[4]
        lines.append(f"{K:3d} {m['cost']:15.3f} {m['avoid']:13.3f} {m['avoid'] / ev:13.3f} {m['avoid'] / ev / m['cost']:6.2f} {m['avoid8']:14.3f} {m['plain']:15.3f} | "
                     f"{float(graze.float().mean()):8.3f} {float(fixed.sum()) / max(float(graze.sum()), 1.0):9.3f} {float(out[4].float().mean()):9.3f} "
                     f"{float(out[2].float().mean()):8.2f}")
        print(lines[-1], flush=True)
    lines.append("grazing: share of the targets where plain solve_ik converges and config_clearance at its answer is below d_safe / 2; repaired: the share of those that "
                 "solve_ik_avoid finishes; finished: of all targets.  A target whose only free configurations lie elsewhere than a null-space motion reaches stays unfinished.")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
