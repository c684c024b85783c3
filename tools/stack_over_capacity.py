"""Records tests/golden/stack_over_capacity.npz: Stack states whose next control step needs more than the native 64 constraint rows.

Runs the 4096-env Stack / Panda / OSC_POSE workload the way tests/test_full_size_parity.py::test_stack_4096_reached_states does (StackBatch with
seed0 = 0, horizon 500, bank_episodes = 2, the per-env action streams of lift.env_actions(ids, 400)) and, from control step `t_from` on, keeps every
env's state before each step.  When a step's demand (RSIM_CAP_NEED, zeroed before the step) is above 64 rows in an env, that env's pre-step qpos,
qvel, qacc_warmstart, ctrl and cstate are saved with its actions for that step and the two after it; envs are taken in the order the steps reach
them (lowest env index first within a step), up to `k`.  Nothing in the run is random beyond the seeded per-env streams, so the same arguments give
the same file bit for bit.

Recorded with:  python tools/stack_over_capacity.py tests/golden/stack_over_capacity.npz        (defaults: t_from 50, k 16; needs a GPU)
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("qpos", "qvel", "qacc_warmstart", "ctrl", "cstate")
NATIVE_ROWS = 64       # constraint rows of the native Stack configuration (32 x 32, RSIM_CFG 1)


def record(t_from=50, k=16, B=4096, n_steps=400):
    import torch

    from robosuite_amd import lift, mjcf, stack

    adir = os.path.join(ROOT, "robosuite_amd", "assets")
    flat = mjcf.load_model(os.path.join(adir, "stack_panda.rsim"))
    cfg = json.load(open(os.path.join(adir, "stack_panda.cfg.json")))
    ids = np.arange(B)
    env = stack.StackBatch(flat, cfg, ids, seed0=0, horizon=500, bank_episodes=2)
    tape = lift.env_actions(ids, n_steps)
    tape_d = torch.tensor(tape, device="cuda")
    b = env.batch
    picked, rows = [], {f: [] for f in FIELDS + ("actions", "step", "cap_need")}
    for t in range(n_steps - 2):
        pre = {f: b.get(f).copy() for f in FIELDS} if t >= t_from else None
        b.set("cap_need", 0)
        env.step(tape_d[t])
        if pre is None:
            continue
        need = b.get("cap_need")
        for e in np.nonzero(need[:, 1] > NATIVE_ROWS)[0]:
            if len(picked) == k or e in picked:
                continue
            picked.append(int(e))
            for f in FIELDS:
                rows[f].append(pre[f][e])
            rows["actions"].append(tape[t:t + 3, e])
            rows["step"].append(t)
            rows["cap_need"].append(need[e])
        if len(picked) == k:
            break
    assert int(b.get("overflow").sum()) == 0 and int(b.get("diverged").sum()) == 0
    env.bank_quiesce(); env._bank_stop()
    out = {f: np.asarray(v) for f, v in rows.items()}
    out["envs"] = np.asarray(picked, dtype=np.int64)
    out["n_sub"] = np.int64(env.n_sub)
    return out


def save_npz(path, arrays):
    """np.savez_compressed with a fixed member timestamp: the same arrays give the same bytes."""
    import io
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


if __name__ == "__main__":
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    path = sys.argv[1]
    t_from = int(sys.argv[2]) if len(sys.argv) > 2 else 50
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 16
    out = record(t_from, k)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    save_npz(path, out)
    print(f"saved {len(out['envs'])} envs to {path}: steps {out['step'].tolist()}, demand (contacts, rows) {out['cap_need'].tolist()}")
