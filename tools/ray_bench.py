"""Ray casting on the device, timed: Lift @4096 after a warm-up -- render_depth at 84 x 84 and 256 x 256, raycast with 64 rays per env, and beside them the
control step of the same batch.  Device events around >= 0.5 s of calls each; rays/s, and the ray-geom tests per second counted from the shapes (every ray
against every geom the filters leave in: what the kernel would do without its bounding-sphere cull, an upper count of the work, not a measured one).

    python tools/ray_bench.py [--envs 4096] [--out profiles/raycast_bench.txt]
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
from robosuite_amd import mjcf  # noqa: E402
from robosuite_amd.backend import HipBatch, HipModel  # noqa: E402
from robosuite_amd.raycast import Camera  # noqa: E402


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
        sys.exit("ray_bench.py: no GPU visible (nothing here is measured on a CPU)")
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
    gt, did = np.asarray(flat.arrays["geom_type"]).ravel(), np.asarray(flat.arrays["geom_dataid"]).ravel()
    alpha = np.asarray(flat.arrays["geom_rgba"]).reshape(-1, 4)[:, 3]
    live = int(((alpha != 0) & ~((gt == mjcf.GEOM_MESH) & (did < 0))).sum())       # geoms a ray is tested against with every group on
    eye, at = np.array([1.3, 0.25, 1.55]), np.array([0.0, 0.0, 0.85])
    z = (eye - at) / np.linalg.norm(eye - at); x = np.cross([0, 0, 1.0], z); x /= np.linalg.norm(x)
    cam = Camera(0, tuple(eye), tuple(mjcf.mat2quat(np.stack([x, np.cross(z, x), z], axis=1))), 45.0)
    lines = [f"ray_bench: Lift @{B}, {int(flat.ngeom)} geoms ({live} take part), device events around >= 0.5 s of calls"]
    o = torch.tensor([0.0, 0.0, 1.6], device="cuda") + torch.rand((B, 64, 3), device="cuda") * 0.4
    d = torch.tensor([0.0, 0.0, -1.0], device="cuda") + (torch.rand((B, 64, 3), device="cuda") - 0.5)
    hb.raycast(o, d); hb.sync()             # the first ray call builds the scene table
    for name, n, fn in (("render_depth 84 x 84", 84 * 84, lambda: hb.render_depth(cam, 84, 84)), ("render_depth 256 x 256", 256 * 256, lambda: hb.render_depth(cam, 256, 256)),
                        ("render_depth 84 x 84 + segmentation", 84 * 84, lambda: hb.render_depth(cam, 84, 84, segmentation=True)), ("raycast 64 rays / env", 64, lambda: hb.raycast(o, d))):
        s, calls = timed(fn)
        lines.append(f"  {name:38s} {1e3 * s:9.3f} ms / call  ({calls} calls)  {B * n / s:.3e} rays/s  {B * n * live / s:.3e} ray-geom tests/s (counted from shapes)")
    s, calls = timed(lambda: hb.control_step(act, 25))
    lines.append(f"  {'control step (25 substeps)':38s} {1e3 * s:9.3f} ms / call  ({calls} calls)  {B / s:.3e} env-steps/s")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
