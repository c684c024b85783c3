#!/usr/bin/env python3
"""profiles/ik_avoid_parity.txt: the records behind collision-aware IK (rsim_ik_site_avoid).

  --sweep   CPU only, the fp64 mirror alone (robosuite_amd/ik_avoid.py): how many cases of the two test scenes finish per avoid_gain -- scene A's 24 sphere cases
            (tests/ik_avoid_scenes.py cases(4, 6)) and its carried-box draws (plain IK's answer free without the box, inside the scene with it held).  The default
            RSIM_IK_AVOID_GAIN is the gain with the most finished cases over both, the smaller one on a tie.
  --device  the worst figures of the device tests (tests/test_ik_avoid.py figures()), for its MEASURED table.

Usage: python tools/ik_avoid_parity.py --sweep [--gains 10 20 30 ...] | --device"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def sweep(gains, ncargo):
    from robosuite_amd import clearance, ik, ik_avoid
    from tests import ik_avoid_scenes as A
    from tests import ik_scenes

    a = A.scene_a()
    flat, site, dofs = a["flat"], a["site"], a["dofs"]
    c = A.cases(4, 6)
    att = A.cargo_attach()
    cp = clearance.default_pairs(flat, dofs, att)
    q0 = np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel()
    rng, cargo = np.random.default_rng(A.SEED + 78), []
    while len(cargo) < ncargo:
        d = ik_scenes.cases(flat, site, dofs, 1, int(rng.integers(1 << 30)), quat=False)
        q, _, _, ok = ik.solve(flat, q0, site, dofs, d["pos"][0], None, d["q_init"][0], max_iters=A.MAX_ITERS)
        if ok and clearance.clearance(flat, q0, dofs, q, a["pairs"])[0] >= A.FREE_MIN and \
                clearance.clearance(flat, q0, dofs, q, cp, attach=att, held=[True], rel=A.CARGO_REL[None])[0] <= -A.HIT_MIN:
            cargo.append(d)
    print(f"avoid_gain sweep, fp64 mirror alone, d_safe {A.D_SAFE}, max_iters {A.MAX_ITERS}: finished cases of scene A (24) and of its carried-box draws ({ncargo})")
    rows = []
    for g in gains:
        fa = sum(bool(A.solve_case(c, e, k, avoid_gain=g)[4]) for e in range(4) for k in range(6))
        fc = sum(bool(ik_avoid.solve(flat, q0, site, dofs, d["pos"][0], None, d["q_init"][0], cp, attach=att, held=[True], rel=A.CARGO_REL[None],
                                     **dict(A.OPTS, avoid_gain=g))[4]) for d in cargo)
        rows.append((fa + fc, -g))
        print(f"  avoid_gain {g:6.1f}: scene A {fa:2d} / 24, carried box {fc:2d} / {ncargo}, total {fa + fc}")
    best = max(rows)
    print(f"  chosen: {-best[1]:g} (most finished, the smaller gain on a tie)")


def device():
    from tests import test_ik_avoid as T

    for k, v in T.figures().items():
        print(f"  {k}: {v:.3e}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--gains", type=float, nargs="*", default=[10, 20, 30, 45, 60, 80, 100, 150, 200])
    ap.add_argument("--ncargo", type=int, default=12)
    args = ap.parse_args()
    if args.sweep:
        sweep(args.gains, args.ncargo)
    if args.device:
        device()
