"""Configuration clearance on the device, timed: Lift / Panda @4096 after a warm-up, K = 1, 16 and 64 candidate arm configurations per env (uniform in the
joint ranges) against the default pair list, with the chunk count chosen automatically and swept from 1 to the list length, and config_fk alone.  The composed baseline is what a
caller had before: geom_distance over the same list on the current state + torch.min -- the answer of the K = 1 identity case, one configuration per env.
Device events around >= 0.3 s of calls each; candidates per second and pair evaluations per second (candidates x list length: what the composed route would
have to evaluate; the kernel's running minimum lets most of them leave early).

    python tools/clearance_bench.py [--envs 4096] [--out profiles/clearance_bench.txt]
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


def timed(fn, min_seconds=0.3):
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
        sys.exit("clearance_bench.py: no GPU visible (nothing here is measured on a CPU)")
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
    pairs = hb.config_pairs(dofs)
    P = len(pairs)
    rng = np.asarray(flat.arrays["jnt_range"], dtype=np.float64).reshape(-1, 2)[:7]
    lo, hi = (torch.as_tensor(rng[:, k], dtype=torch.float32, device="cuda") for k in (0, 1))
    gen = torch.Generator(device="cuda"); gen.manual_seed(5)
    lines = [f"clearance_bench: Lift @{B}, arm dofs 0..6, the default pair list ({P} of the model's {len(flat.arrays['pair_geom1'])} collision pairs), distmax 1.0, tol 1e-6, "
             f"max_iters 64; device events around >= 0.3 s of calls"]
    s0, calls = timed(lambda: torch.min(hb.geom_distance(pairs)[0], dim=1))
    lines.append(f"  {'composed: geom_distance(list) + torch.min':52s} {1e3 * s0:9.3f} ms / call  ({calls} calls)  {B / s0:.3e} configurations/s  {B * P / s0:.3e} pair evaluations/s")
    for K in (1, 16, 64):
        q = lo + (hi - lo) * torch.rand((B, K, 7), device="cuda", generator=gen)
        d, pair, ft, st = hb.config_clearance(dofs, q); hb.sync()      # the first call builds the tables and grows the scratch
        d = d.cpu().numpy()
        lines.append(f"  K = {K}: {100 * (d > 1e-4).mean():.1f} % free (d > 1e-4), {100 * (d <= 0).mean():.1f} % colliding (d <= 0), {int((st.cpu().numpy() & 256 != 0).sum())} at the iteration cap")
        sweep = [(f"config_clearance K {K}, chunks {c}", (lambda c: lambda: hb.config_clearance(dofs, q, chunks=c))(c)) for c in (1, 2, 4, 8, 16, 32, 64, P)]
        for name, fn in [(f"config_clearance K {K}, chunks automatic", lambda: hb.config_clearance(dofs, q))] + sweep + [
                         (f"config_clearance K {K}, fromto=False", lambda: hb.config_clearance(dofs, q, fromto=False)),
                         (f"config_fk K {K}", lambda: hb.config_fk(dofs, q))]:
            s, calls = timed(fn)
            tail = "" if "config_fk" in name else f"  {B * K * P / s:.3e} pair evaluations/s  ({s0 * K / s:.1f} x the composed route per configuration)"
            lines.append(f"  {name:52s} {1e3 * s:9.3f} ms / call  ({calls} calls)  {B * K / s:.3e} candidates/s{tail}")
    s, calls = timed(lambda: hb.control_step(act, 25))
    lines.append(f"  {'control step (25 substeps)':52s} {1e3 * s:9.3f} ms / call  ({calls} calls)  {B / s:.3e} env-steps/s")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
