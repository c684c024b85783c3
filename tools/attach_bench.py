"""Carried objects on the device, timed: Lift / Panda @4096 after a warm-up, the cube attached to the eef body with a given grasp at the grip site, K = 1, 16
and 64 candidates / segments per env, held in all, half (every other env) and none of the envs, beside the plain call of the same session.  The plain and the
attached calls run different instantiations of the same kernels (k_clear_fk / k_clear_dist / k_sweep and their _att forms).  The sweep's list is the default
list of dofs 1..6: with joint 1 in it Panda's link0 / link1 pair, 1.0 mm apart, makes every segment a HIT at its first sample.  Device events around >= 0.3 s
of config_clearance calls; a config_sweep call takes seconds here (a wavefront runs as long as its slowest segment, and some segment of most wavefronts
grazes the scene for all 256 samples), so it is timed over two calls after one.  Reported, not gated.

    python tools/attach_bench.py [--envs 4096] [--out profiles/attach_bench.txt]
    python tools/attach_bench.py --order      # only: config_clearance at K = 1, plain and attached timed in turn, four rounds, the attached call FIRST
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


def timed_twice(fn):
    """(seconds per call, calls): device events around two calls, after one untimed -- for calls that take seconds"""
    out = fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn(); fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / 2, 2, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default=None)
    ap.add_argument("--order", action="store_true", help="only the K = 1 config_clearance order check")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("attach_bench.py: no GPU visible (nothing here is measured on a CPU)")
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
    eef = int(np.asarray(flat.arrays["site_bodyid"]).ravel()[int(cfg["eef_site"])])
    att = [(flat.names["body"].index("cube_main"), eef)]
    rel = torch.tensor([0, 0, 0, 1, 0, 0, 0], dtype=torch.float32, device="cuda").repeat(B, 1, 1)
    helds = (("all", None), ("half", (torch.arange(B, device="cuda") % 2 == 0)), ("none", torch.zeros(B, dtype=torch.bool, device="cuda")))
    rng = np.asarray(flat.arrays["jnt_range"], dtype=np.float64).reshape(-1, 2)[:7]
    lo, hi = (torch.as_tensor(rng[:, k], dtype=torch.float32, device="cuda") for k in (0, 1))
    lines = [f"attach_bench: Lift @{B}, cube_main attached to the eef body (rel given: the grip site), distmax 1.0; device events around >= 0.3 s of calls",
             f"  config_clearance: dofs 0..6, default lists: plain {len(hb.config_pairs(list(range(7))))} pairs, attached {len(hb.config_pairs(list(range(7)), attach=att))} pairs, automatic chunks",
             f"  config_sweep: dofs 1..6, default lists: plain {len(hb.config_pairs(list(range(1, 7))))} pairs, attached {len(hb.config_pairs(list(range(1, 7)), attach=att))} pairs; "
             "segments a fifth of the way between two uniform draws"]
    gen = torch.Generator(device="cuda"); gen.manual_seed(5)
    if args.order:      # does the figure of the plain call depend on being timed first in the session?
        q = lo + (hi - lo) * torch.rand((B, 1, 7), device="cuda", generator=gen)
        kw = dict(attach=att, held=None, rel=rel)
        for r in range(4):
            sa, ca = timed(lambda: hb.config_clearance(list(range(7)), q, **kw))
            sp, cp = timed(lambda: hb.config_clearance(list(range(7)), q))
            print(f"  K =  1  round {r}: config_clearance attached, held all {1e3 * sa:9.3f} ms / call ({ca} calls), then plain {1e3 * sp:9.3f} ms / call ({cp} calls)", flush=True)
        return
    for K in (1, 16, 64):
        q = lo + (hi - lo) * torch.rand((B, K, 7), device="cuda", generator=gen)
        q1 = q + 0.2 * (lo + (hi - lo) * torch.rand((B, K, 7), device="cuda", generator=gen) - q)
        d7, d6 = list(range(7)), list(range(1, 7))
        a6, b6 = q[..., 1:].contiguous(), q1[..., 1:].contiguous()
        s, calls = timed(lambda: hb.config_clearance(d7, q))
        lines.append(f"  K = {K:2d}  {'config_clearance, plain':44s} {1e3 * s:9.3f} ms / call  ({calls} calls)")
        base_c = s
        s, calls, st = timed_twice(lambda: hb.config_sweep(d6, a6, b6))
        lines.append(f"  K = {K:2d}  {'config_sweep, plain':44s} {1e3 * s:9.3f} ms / call  ({calls} calls)  steps mean {st[6].float().mean():.2f} max {int(st[6].max())}")
        base_s = s
        for name, held in helds:
            kw = dict(attach=att, held=held, rel=rel)
            s, calls = timed(lambda: hb.config_clearance(d7, q, **kw))
            lines.append(f"  K = {K:2d}  {'config_clearance, attached, held ' + name:44s} {1e3 * s:9.3f} ms / call  ({calls} calls)  {s / base_c:.3f} x plain")
            s, calls, st = timed_twice(lambda: hb.config_sweep(d6, a6, b6, **kw))
            lines.append(f"  K = {K:2d}  {'config_sweep, attached, held ' + name:44s} {1e3 * s:9.3f} ms / call  ({calls} calls)  {s / base_s:.3f} x plain  "
                         f"steps mean {st[6].float().mean():.2f} max {int(st[6].max())}")
        print("\n".join(lines[-8:]), flush=True)
    text = "\n".join(lines)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
