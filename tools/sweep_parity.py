"""Worst figures of the swept clearance kernel, per scene, in one GPU run: what tests/test_sweep.py keeps in MEASURED.  Runs the very functions the tests run
(identity_figure, certificate_figures, mirror_bounds, centre_displacement_figure) on the tests' scenes and shapes, asserts no bound, and prints one line per
figure; also the step-count ratio of the device to the fp64 mirror (robosuite_amd/sweep.py) on scene T (3, 5) and the kernel's registers, scratch and LDS.

    python tools/sweep_parity.py [--out profiles/sweep_parity.txt]"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from robosuite_amd import clearance, sweep      # noqa: E402
from tests import clearance_scenes as S      # noqa: E402
from tests import sweep_scenes as W      # noqa: E402
from tests import test_sweep as T      # noqa: E402
from tests.util import make_hip      # noqa: E402


def figures(scene, flat, hb, dofs, q0, q1, distmax, margin=0.0):
    pairs = clearance.default_pairs(flat, dofs)
    a, b = T.dev(q0), T.dev(q1)
    out = hb.config_sweep(dofs, a, b, distmax=distmax, margin=margin)
    fig = {}
    fig["ident"], same = T.identity_figure(hb, dofs, q0, q1, out, distmax)
    fig.update(T.certificate_figures(hb, dofs, q0, q1, out, distmax, margin))
    L = hb.config_motion_bound(dofs, a, b)
    rel = L.cpu().numpy().astype(np.float64) / T.mirror_bounds(flat, hb.get("qpos").astype(np.float64), dofs, q0, q1, pairs) - 1.0
    fig["bound_rel_min"], fig["bound_rel_max"] = float(rel.min()), float(rel.max())
    fig["centres"] = T.centre_displacement_figure(flat, hb, dofs, q0, q1, pairs, L, 0.0)
    kind, steps = out[0].cpu().numpy() & 3, out[6].cpu().numpy()
    tail = (f"bitwise {'yes' if same else 'NO'}; free {int((kind == 0).sum())} hit {int((kind == 1).sum())} undecided {int((kind == 2).sum())}; "
            f"steps mean {steps.mean():.1f} max {int(steps.max())}")
    return fig, tail, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    worst, lines = {}, []

    def note(scene, what, fig, tail=""):
        for k, v in fig.items():
            worst.setdefault(scene, {})[k] = max(worst.get(scene, {}).get(k, -np.inf), v)
        lines.append(f"{scene:7s} {what:30s} " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()) + ("  | " + tail if tail else ""))
        print(lines[-1], flush=True)

    flat = S.scene_t(tempfile.mkdtemp())
    for which, margin in (("all", 0.0), ("arm", 0.01)):
        for B, K in T.SHAPES:
            hm, hb = make_hip(flat, None, B=B)
            hb.set("qpos", S.scene_t_qpos(flat, B).astype(np.float32)); hb.forward()
            dofs = S.dofs_t(flat, which)
            q0, q1 = W.segments(flat, dofs, B, K)
            fig, tail, out = figures("T", flat, hb, dofs, q0, q1, S.DISTMAX_T, margin)
            note("T", f"{which} B {B} K {K} margin {margin}", fig, tail)
            if (B, K) == T.SHAPES[0] and which == "all":
                qpos = hb.get("qpos").astype(np.float64)
                ref = np.array([[sweep.sweep(flat, qpos[e], dofs, q0[e, k], q1[e, k], distmax=S.DISTMAX_T)[6] for k in range(K)] for e in range(B)])
                dev_steps = out[6].cpu().numpy()
                lines.append(f"T       steps, device against mirror, B {B} K {K}: device {dev_steps.sum()} mirror {ref.sum()} ratio {dev_steps.sum() / ref.sum():.4f}; "
                             f"per segment ratio {np.min(dev_steps / ref):.3f} .. {np.max(dev_steps / ref):.3f}")
                print(lines[-1], flush=True)
    for name in ("panda", "baxter_both"):
        s = S.arm(name)
        f, cfg, dofs = s["flat"], s["cfg"], s["dofs"]
        B, K = T.SHAPES[0]
        hm, hb = make_hip(f, cfg, B=B)
        hb.set("qpos", np.tile(s["qpos"], (B, 1)).astype(np.float32)); hb.set("qvel", 0); hb.forward()
        q0, q1 = W.segments(f, dofs, B, K)
        scene = "panda" if name == "panda" else "baxter"
        fig, tail, _ = figures(scene, f, hb, dofs, q0, q1, S.DISTMAX_ARM)
        note(scene, name, fig, tail)
    lines.append("")
    lines.append("worst per scene (tests/test_sweep.py MEASURED):")
    for scene, fig in worst.items():
        lines.append(f"{scene:7s} " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    try:
        from tools.kernel_resources import kernels
        for k, v in kernels(os.path.join(ROOT, "robosuite_amd", "librsim_hip.so")).items():
            if "k_sweep" in k:
                lines.append(f"k_sweep: {v['vgpr']} registers, {v['scratch']} B of scratch, {v['lds']} B of LDS")
    except Exception as e:      # (llvm-readelf not at hand)
        lines.append(f"k_sweep: resources not read ({e})")
    print("\n".join(lines[-len(worst) - 3:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("Swept clearance kernel held to config_clearance / config_fk and the fp64 mirror (tools/sweep_parity.py), one run on an MI355X.\n"
                     "ident m: |dist - config_clearance(q(t_min))|, one chunk (bitwise: dist, pair and fromto equal bit for bit); shortfall m: margin - the minimum of\n"
                     "config_clearance over 129 uniform samples of [0, t], where positive; hit m: a HIT's config_clearance at t above margin + slack, where positive;\n"
                     "bound_rel: device L / mirror L - 1, smallest and largest; centres m: geom-centre displacement between neighbouring samples at config_fk poses\n"
                     "minus L dt, worst pair (negative: inside the bound).\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
