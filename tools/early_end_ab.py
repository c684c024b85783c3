"""What the early episode end (rsim_set_early_end, csrc/rsim_episode.hip) costs a lockstep control step once it is armed.

Drives the task batch the way bench.py's headline region does -- same build_env, same action tape, same staggered pre-roll and warm-up, events on the
stream the control step is launched on -- in one of three modes:

    off      nothing armed (the tool's own baseline: must agree with `python bench.py` on the same library)
    idle     success rule armed with min_steps above the horizon: k_end_episodes runs behind every step and never ends an episode
    firing   success rule armed, min_steps = 1; before every step a rotating 1/64 of the envs is put into a succeeding state by a write on the batch's stream
             (Lift: the cube 0.25 m above the table; Stack: cubeA resting on cubeB), so that those envs end their episode in that step and restart from
             the ring.  min_steps = 1 also makes the ring upkeep synchronous (reset_bank.py): the figure includes its blocking read per step

Prints one JSON line.  RSIM_LIB names the library, as everywhere.  Under `rocprofv3 --kernel-trace --stats -- python tools/early_end_ab.py ...` the kernel
statistics carry the duration of k_end_episodes (no counters are collected in such a run).

    python tools/early_end_ab.py --config lift --mode idle
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from robosuite_amd import factory, lift  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=("lift", "stack"), default="lift")
    ap.add_argument("--mode", choices=("off", "idle", "firing"), default="idle")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--preroll", type=int, default=bench.HORIZON)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    label, stem, _, dr, _ = bench.CONFIGS[args.config]
    flat, cfg = factory.load_shipped(stem)
    B, K, W, P = args.envs, args.steps, args.warmup, args.preroll
    ids = np.arange(B)
    # firing: every env ends an episode every 64 steps on top of the horizon -- the ring is sized for it, and min_steps = 1 makes the upkeep synchronous
    env = bench.build_env(args.config, flat, cfg, ids, 0, 3 + (P + W + K) // bench.HORIZON + (4 if args.mode == "firing" else 0))
    tape = torch.tensor(lift.env_actions(ids, P + W + K, action_dim=env.model.action_dim), device=dev)
    stream = torch.cuda.ExternalStream(env.batch.stream(), device=dev)
    if P:
        env.batch.set("ep_step", ((197 * ids) % bench.HORIZON).astype(np.int32))
    for t in range(P):
        env.step(tape[t])
    if args.mode == "idle":
        env.set_early_end(success=True, min_steps=bench.HORIZON + 1)
    elif args.mode == "firing":
        env.set_early_end(success=True, min_steps=1)
    qpos = env.batch.tensor("qpos")
    # free joints behind the arm (7) and gripper (2) coordinates: Lift's cube at 9; Stack's cubeA at 9 (half size 0.02) and cubeB at 16 (0.025)
    groups = [torch.arange(g, B, 64, device=dev) for g in range(64)]

    def step(t):
        if args.mode == "firing":
            with torch.cuda.stream(stream):
                g = groups[t % 64]
                if args.config == "lift":
                    qpos[g, 11] = 0.8 + 0.25
                else:
                    qpos[g, 9:11] = qpos[g, 16:18]
                    qpos[g, 11] = qpos[g, 18] + 0.0445       # half a millimetre into cubeB: in contact, not grasped, above the lift height
        env.step(tape[P + t])

    for t in range(W):
        step(t)
    env.batch.sync(); torch.cuda.synchronize()
    ep0 = env.batch.get("ep_index").astype(np.int64).sum()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(K)]
    t0 = time.perf_counter()
    for t in range(K):
        ev[t][0].record(stream)
        step(W + t)
        ev[t][1].record(stream)
    env.batch.sync(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    env.bank_quiesce()
    reasons = np.bincount(env.batch.get("end_reason"), minlength=5).tolist() if args.mode != "off" else None
    print(json.dumps({"tool": "early_end_ab", "config": args.config, "mode": args.mode, "envs": B, "steps": K, "ms_per_step": 1e3 * dt / K,
                      "kernel_ms": float(np.mean([a.elapsed_time(b) for a, b in ev])), "env_steps_per_s": B * K / dt,
                      "episodes_ended_in_region": int(env.batch.get("ep_index").astype(np.int64).sum() - ep0), "bank_stale": int(env.batch.get("bank_stale").sum()),
                      "end_reason_hist_last_step": reasons, "lib": os.environ.get("RSIM_LIB", "in-tree")}), flush=True)


if __name__ == "__main__":
    main()
