"""Swept clearance on the device, timed: Lift / Panda @4096 after a warm-up, K = 1, 16 and 64 joint-space segments per env (both ends uniform in the
joint ranges, or a fifth of such a segment) against the default pair list and against that list without its parent / child pairs.  Per K: the time of one config_sweep call, the mean and the largest number of samples a segment took,
segments per second, and what sampling would cost instead -- config_clearance on K S uniform samples per env with S the mean and S the largest step count
(samples at the resolution the certificate would need are far more than either).  Also the share of wavefronts that wait on one slow lane: a wavefront runs as
long as its slowest segment, so its 64 lanes cost 64 x the largest step count among them while the work is the sum.  Device events around >= 0.3 s of calls.

    python tools/sweep_bench.py [--envs 4096] [--out profiles/sweep_bench.txt]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robosuite_amd import mjcf  # noqa: E402
from robosuite_amd.backend import HipBatch, HipModel  # noqa: E402
from tools.clearance_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sweep_bench.py: no GPU visible (nothing here is measured on a CPU)")
    adir = os.path.join(ROOT, "robosuite_amd", "assets")
    flat = mjcf.load_model(os.path.join(adir, "lift_panda.rsim")); cfg = json.load(open(os.path.join(adir, "lift_panda.cfg.json")))
    hm = HipModel(flat); hm.set_controller(cfg)
    B = args.envs
    hb = HipBatch(hm, B, 0)
    hb.forward(); hb.ctrl_reset()
    act = (torch.rand((B, hm.action_dim), device="cuda") * 2 - 1) * 0.3
    for _ in range(20):                     # warm-up: the envs leave the common reset pose
        hb.control_step(act, 25)
    hb.sync()
    dofs = list(range(7))
    full = hb.config_pairs(dofs)
    parent, gb = (np.asarray(flat.arrays[k]).ravel().astype(int) for k in ("body_parentid", "geom_bodyid"))
    apart = np.ascontiguousarray(full[[not (parent[gb[x]] == gb[y] or parent[gb[y]] == gb[x]) for x, y in full]])      # without parent / child pairs
    rng = np.asarray(flat.arrays["jnt_range"], dtype=np.float64).reshape(-1, 2)[:7]
    lo, hi = (torch.as_tensor(rng[:, k], dtype=torch.float32, device="cuda") for k in (0, 1))
    lines = [f"sweep_bench: Lift @{B}, arm dofs 0..6, distmax 1.0, margin 0, slack 1e-3, max_steps 256; device events around >= 0.3 s of calls",
             f"  lists: the default pair list ({len(full)} pairs), and the same without its {len(full) - len(apart)} parent / child pairs ({len(apart)} pairs): Panda's link0 / link1",
             "  geoms stand 1.0 mm apart whatever the arm does, so with the default list and the default slack every segment is a HIT at its first sample.",
             "  segments: both ends uniform in the joint ranges (\"random\"), or the end a fifth of the way from the start towards such a draw (\"short\")"]
    for what, pairs, frac in (("default list, random", None, 1.0), ("no parent / child pairs, random", apart, 1.0), ("no parent / child pairs, short", apart, 0.2)):
        gen = torch.Generator(device="cuda"); gen.manual_seed(5)
        P = len(full) if pairs is None else len(pairs)
        for K in (1, 16, 64):
            q0 = lo + (hi - lo) * torch.rand((B, K, 7), device="cuda", generator=gen)
            q1 = q0 + frac * (lo + (hi - lo) * torch.rand((B, K, 7), device="cuda", generator=gen) - q0)
            st, t, d, tm, pair, ft, steps = hb.config_sweep(dofs, q0, q1, pairs=pairs); hb.sync()      # the first call builds the tables and grows the scratch
            kind, sn = (st & 3).cpu().numpy().ravel(), steps.cpu().numpy().ravel().astype(np.float64)
            L = hb.config_motion_bound(dofs, q0, q1, pairs=pairs).cpu().numpy()
            lines.append(f"  {what}, K = {K} ({P} pairs): {100 * (kind == 0).mean():.1f} % FREE, {100 * (kind == 1).mean():.1f} % HIT ({100 * (sn == 1).mean():.1f} % at the first "
                         f"sample), {100 * (kind == 2).mean():.1f} % UNDECIDED; steps mean {sn.mean():.2f} max {int(sn.max())}; L mean {L.mean():.2f} max {L.max():.2f}")
            pad = np.concatenate([sn, np.zeros(-len(sn) % 64)]).reshape(-1, 64)      # lane = env * K + k, 64 per wavefront
            busy = pad.sum() / (64 * pad.max(axis=1)).sum()
            waiting = (pad.max(axis=1) > 2 * np.sort(pad, axis=1)[:, -2]).mean()
            lines.append(f"    wavefronts: {len(pad)}; lanes busy {100 * busy:.1f} % of wavefront time (sum of steps / 64 x the wavefront's largest); "
                         f"{100 * waiting:.1f} % of wavefronts wait on ONE lane (its steps more than twice the next lane's)")
            s, calls = timed(lambda: hb.config_sweep(dofs, q0, q1, pairs=pairs))
            lines.append(f"    {'config_sweep':50s} {1e3 * s:9.3f} ms / call  ({calls} calls)  {B * K / s:.3e} segments/s  {B * K * sn.mean() / s:.3e} samples/s")
            s, calls = timed(lambda: hb.config_motion_bound(dofs, q0, q1, pairs=pairs))
            lines.append(f"    {'config_motion_bound':50s} {1e3 * s:9.3f} ms / call  ({calls} calls)")
            for which, S in (("mean", max(1, int(round(sn.mean())))), ("max", int(sn.max()))):
                part = min(S, max(1, (1 << 21) // (B * K)))      # samples per segment in one call: at most 2 M candidates; more is timed in part and scaled
                ts = torch.linspace(0, 1, S, device="cuda")[None, None, :part, None] if S > 1 else torch.zeros((1, 1, 1, 1), device="cuda")
                q = (q0[:, :, None] + ts * (q1 - q0)[:, :, None]).reshape(B, K * part, 7)
                s, calls = timed(lambda: hb.config_clearance(dofs, q, pairs=pairs))
                scaled = "" if part == S else f"  (= {S / part:.1f} x the {1e3 * s:.3f} ms of a call with {part} of them per segment)"
                s *= S / part
                lines.append(f"    {'config_clearance on K S = %d x %d (%s steps)' % (K, S, which):50s} {1e3 * s:9.3f} ms  ({calls} calls)  {B * K * S / s:.3e} samples/s{scaled}")
            print("\n".join(lines[-7:]), flush=True)
    s, calls = timed(lambda: hb.control_step(act, 25))
    lines.append(f"  {'control step (25 substeps)':52s} {1e3 * s:9.3f} ms / call  ({calls} calls)  {B / s:.3e} env-steps/s")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
