"""Inverse kinematics on the device, timed: Panda (the Lift asset) @4096, reachable gripper poses (the pose at joint angles drawn inside the ranges), start
vectors 0.3 rad around them, default options -- `HipBatch.solve_ik` with K = 1 and K = 16 problems per env: solves/s and mean iterations.  Beside it the
same algorithm done the only way the build before this kernel allowed: per iteration write qpos, run `forward` on the whole batch, build the Jacobian with
`BatchState.site_jacobian` and solve in torch (fp32), until every env has converged (it overwrites the simulation state, which is put back afterwards).

    python tools/ik_bench.py [--envs 4096] [--out profiles/ik_bench.txt]
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
from robosuite_amd import ik, mjcf  # noqa: E402
from robosuite_amd.backend import HipBatch, HipModel  # noqa: E402
from robosuite_amd.controllers import BatchState  # noqa: E402


def qmul(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], dim=-1)


def site_quat(st, site):
    q = qmul(st.xquat[:, int(st._site_body[site])], st._site_quat[site].expand(st.B, 4))
    return q / torch.linalg.norm(q, dim=-1, keepdim=True)


def rotvec(qt, qs):
    d = qmul(qt, qs * torch.tensor([1.0, -1.0, -1.0, -1.0], device=qs.device))
    d = torch.where(d[:, :1] < 0, -d, d)
    s = torch.linalg.norm(d[:, 1:], dim=-1, keepdim=True)
    return d[:, 1:] * torch.where(s > 1e-12, 2.0 * torch.atan2(s, d[:, :1]) / s.clamp_min(1e-30), torch.full_like(s, 2.0))


def torch_solve(hb, st, site, qidx, didx, lo, hi, pos, quat, q_init, o):
    """the mirror's loop on the debug entries: -> (q, iterations per env, converged)"""
    B = st.B
    q = torch.minimum(torch.maximum(q_init.clone(), lo), hi)
    it = torch.zeros(B, dtype=torch.int32, device=q.device)
    conv = torch.zeros(B, dtype=torch.bool, device=q.device)
    eye = torch.eye(6, device=q.device)[None]
    for k in range(o["max_iters"] + 1):
        st.qpos[:, qidx] = q
        hb.forward()
        p, _ = st.site_pose(site)
        jp, jr = st.site_jacobian(site)
        J = torch.cat([jp[:, :, didx], jr[:, :, didx]], dim=1)
        e = torch.cat([pos - p, rotvec(quat, site_quat(st, site))], dim=1)
        conv = conv | ((torch.linalg.norm(e[:, :3], dim=1) < o["pos_tol"]) & (torch.linalg.norm(e[:, 3:], dim=1) < o["rot_tol"]))
        if k == o["max_iters"] or bool(conv.all()):
            break
        A = torch.einsum("bij,bkj->bik", J, J) + o["damping"] * eye
        dq = torch.einsum("bji,bj->bi", J, torch.linalg.solve(A, e))
        big = dq.abs().amax(dim=1, keepdim=True)
        dq = dq * torch.where(big > o["max_dq"], o["max_dq"] / big, torch.ones_like(big))
        live = ~conv
        q = torch.where(live[:, None], torch.minimum(torch.maximum(q + dq, lo), hi), q)
        it = it + live.to(torch.int32)
    return q, it, conv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ik_bench.py: no GPU visible (nothing here is measured on a CPU)")
    adir = os.path.join(ROOT, "robosuite_amd", "assets")
    flat = mjcf.load_model(os.path.join(adir, "lift_panda.rsim")); cfg = json.load(open(os.path.join(adir, "lift_panda.cfg.json")))
    hm = HipModel(flat); hm.set_controller(cfg)
    B, KMAX = args.envs, 16
    hb = HipBatch(hm, B, 0)
    hb.forward()
    st = BatchState(hb)
    site, dofs, qidx = int(cfg["eef_site"]), list(cfg["dof_idx"]), list(cfg["qpos_idx"])
    n = len(dofs)
    _, jid = ik.chain(flat, site, dofs)
    rng = np.asarray(flat.arrays["jnt_range"], dtype=np.float32).reshape(-1, 2)[jid]
    lo, hi = torch.as_tensor(rng[:, 0], device="cuda"), torch.as_tensor(rng[:, 1], device="cuda")
    saved = st.qpos.clone()
    g = torch.Generator(device="cuda").manual_seed(1)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    pos, quat, qi = [], [], []
    for _ in range(KMAX):                   # reachable targets: the pose at joint angles drawn in the middle 90 % of the ranges
        qt = mid + 0.9 * half * (torch.rand((B, n), device="cuda", generator=g) * 2 - 1)
        st.qpos[:, qidx] = qt
        hb.forward()
        pos.append(st.site_pose(site)[0].clone()); quat.append(site_quat(st, site).clone())
        qi.append(torch.minimum(torch.maximum(qt + 0.3 * (torch.rand((B, n), device="cuda", generator=g) * 2 - 1), lo), hi))
    pos, quat, qi = torch.stack(pos, 1).contiguous(), torch.stack(quat, 1).contiguous(), torch.stack(qi, 1).contiguous()
    st.qpos.copy_(saved); hb.forward(); hb.sync()
    lines = [f"ik_bench: Panda (Lift asset) @{B}, site {site}, {n} dofs, pose targets, default options, start vectors within 0.3 rad of a solution"]
    for K in (1, KMAX):
        args_k = (pos[:, :K].contiguous(), quat[:, :K].contiguous(), qi[:, :K].contiguous())
        for _ in range(3):
            q, err, it, conv = hb.solve_ik(site, dofs, *args_k)
        torch.cuda.synchronize()
        reps = 50
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            hb.solve_ik(site, dofs, *args_k)
        b.record(); torch.cuda.synchronize()
        s = a.elapsed_time(b) * 1e-3 / reps
        lines.append(f"  k_ik, K = {K:2d}: {1e3 * s:9.3f} ms / call ({reps} calls)  {B * K / s:.3e} solves/s  mean iterations {it.float().mean().item():.2f} "
                     f"(max {int(it.max())})  converged {int(conv.sum())}/{B * K}")
    o = ik.options()
    torch_solve(hb, st, site, qidx, dofs, lo, hi, pos[:, 0], quat[:, 0], qi[:, 0], o)      # untimed: first-use costs
    torch.cuda.synchronize()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        q, it, conv = torch_solve(hb, st, site, qidx, dofs, lo, hi, pos[:, 0], quat[:, 0], qi[:, 0], o)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    s = float(np.median(times))
    lines.append(f"  torch on the debug entries, K = 1 (set qpos -> forward -> site_jacobian -> torch.linalg.solve, until all envs converged or {o['max_iters']} updates): "
                 f"{1e3 * s:9.3f} ms / call (median of 5: {1e3 * min(times):.1f} .. {1e3 * max(times):.1f})  {B / s:.3e} solves/s  mean iterations {it.float().mean().item():.2f} (the loop runs {int(it.max())})  converged {int(conv.sum())}/{B}")
    st.qpos.copy_(saved); hb.forward(); hb.sync()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
