"""Geom distance on the device, timed: Lift @4096 after a warm-up, the pair list VecEnv.body_distance(robot bodies, table + cube) produces -- the last three links,
the hand, fingers and finger tips against every geom of the table and the cube -- with and without the nearest points, and the torch.min reduction on top.
Device events around >= 0.5 s of synchronised calls each; pairs per second and time per call.

    python tools/distance_bench.py [--envs 4096] [--out profiles/distance_bench.txt]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from robosuite_amd import distance, mjcf  # noqa: E402
from robosuite_amd.backend import HipBatch, HipModel  # noqa: E402

ROBOT = ("robot0_link5", "robot0_link6", "robot0_link7", "gripper0_right_right_gripper", "gripper0_right_leftfinger", "gripper0_right_finger_joint1_tip",
         "gripper0_right_rightfinger", "gripper0_right_finger_joint2_tip")
SCENE = ("table", "cube_main")


def timed(fn, min_seconds=0.5):
    """(seconds per call, calls): device events around at least min_seconds of calls, after two untimed ones"""
    fn(); fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
    n = max(3, int(np.ceil(min_seconds / max(time.perf_counter() - t0, 1e-5))))
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / n, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("distance_bench.py: no GPU visible (nothing here is measured on a CPU)")
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
    bn = flat.names["body"]
    pairs = distance.body_pairs(flat, [bn.index(n) for n in ROBOT], [bn.index(n) for n in SCENE])
    P = len(pairs)
    d, ft, st = hb.geom_distance(pairs); hb.sync()      # the first call uploads the pair table (and builds the scene table)
    st = st.cpu().numpy()
    lines = [f"distance_bench: Lift @{B}, {P} pairs (body_distance: {len(ROBOT)} robot bodies x table + cube), distmax 1.0, tol 1e-6, max_iters 64; device events around >= 0.5 s of calls",
             f"  status of this state: {int((st == 0).sum())} closer than distmax, {int((st == 1).sum())} beyond, {int((st == 2).sum())} overlapping, {int((st & 256 != 0).sum())} at the iteration cap"]

    def reduced():
        dd, ff, _ = hb.geom_distance(pairs)
        m, k = torch.min(dd, dim=1)
        return m, ff[torch.arange(B, device=ff.device), k]

    for name, fn in (("geom_distance, dist + fromto + status", lambda: hb.geom_distance(pairs)), ("geom_distance, fromto=False", lambda: hb.geom_distance(pairs, fromto=False)),
                     ("... + torch.min (body_distance)", reduced), ("geom_distance, one pair", lambda: hb.geom_distance(pairs[:1]))):
        s, calls = timed(fn)
        n = 1 if "one pair" in name else P
        lines.append(f"  {name:40s} {1e3 * s:9.3f} ms / call  ({calls} calls)  {B * n / s:.3e} pairs/s")
    s, calls = timed(lambda: hb.control_step(act, 25))
    lines.append(f"  {'control step (25 substeps)':40s} {1e3 * s:9.3f} ms / call  ({calls} calls)  {B / s:.3e} env-steps/s")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
