"""What the sensors beyond force / torque (k_sensors, csrc/rsim_sensors.hip) cost a host-controlled control step.

A HostControlledEnv step (controllers.py: per substep rsim_step1, the part controllers in torch, rsim_step2) of Lift / Panda with the joint-torque and
grip plugins, in one of two modes:

    plain     the golden Lift model: force / torque only, nothing new is launched (runs on a checkout from before the sensors too)
    sensors   the same model with a gyro and an accelerometer at the hand and a jointpos appended: k_sensors behind every step1 / step2, and the three
              device-to-device copies ahead of every integrating launch

Prints one JSON line.  RSIM_LIB names the library, as everywhere.

    python tools/sensors_ab.py --mode sensors
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

from robosuite_amd import lift  # noqa: E402
from robosuite_amd.controllers import HostControlledEnv  # noqa: E402
from tests.test_controllers_plugin import _parts  # noqa: E402
from tests.util import load_golden  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("plain", "sensors"), default="plain")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    B, K, W = args.envs, args.steps, args.warmup
    g, cfg, flat = load_golden("ctl_joint_torque")
    if args.mode == "sensors":
        from robosuite_amd import mjcf
        from tests.sensors_scenes import add_sensors
        site, jnt = flat.names["site"].index("gripper0_right_grip_site"), int(cfg["qpos_idx"][3])
        j = int(np.flatnonzero(np.asarray(flat.jnt_qposadr) == jnt)[0])
        flat = add_sensors(flat, [("hand_gyro", "gyro", mjcf.SENSOR_OBJ_SITE, site, 3), ("elbow_pos", "jointpos", mjcf.SENSOR_OBJ_JOINT, j, 1),
                                  ("hand_acc", "accelerometer", mjcf.SENSOR_OBJ_SITE, site, 3)])
    task = lift.LiftBatch(flat, cfg, np.arange(B), seed0=4)
    st, parts = _parts(task, cfg, flat)
    env = HostControlledEnv(task, parts)
    tape = torch.tensor(lift.env_actions(np.arange(B), W + K, action_dim=env.action_dim), device="cuda")
    for t in range(W):
        env.step(tape[t])
    task.batch.sync(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for t in range(K):
        env.step(tape[W + t])
    task.batch.sync(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    sd = task.batch.get("sensordata")
    print(json.dumps({"tool": "sensors_ab", "mode": args.mode, "envs": B, "steps": K, "n_sub": env.n_sub, "ms_per_step": 1e3 * dt / K,
                      "env_steps_per_s": B * K / dt, "nsensordata": int(sd.shape[1]), "sensordata_absmax": float(np.abs(sd).max()),
                      "lib": os.environ.get("RSIM_LIB", "in-tree")}), flush=True)


if __name__ == "__main__":
    main()
