"""Worst figures of the configuration clearance kernels against the fp64 mirror, per scene, in one GPU run: what tests/test_clearance.py keeps in MEASURED
and asserts four times.  Runs the very functions the tests run (fk_figures, step_fk_figure, clear_figures, ident_figure) on the tests' scenes, shapes, dof
lists and chunkings, asserts no bound, and prints one line per figure.

    python tools/clearance_parity.py [--out profiles/clearance_parity.txt]"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from robosuite_amd import clearance      # noqa: E402
from tests import clearance_scenes as S      # noqa: E402
from tests import distance_scenes as D      # noqa: E402
from tests import test_clearance as T      # noqa: E402
from tests.util import make_hip      # noqa: E402

EDGE = 4e-6      # the band about distmax in which "far or not" is not compared while measuring (the tests use 2 BOUND)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    worst, lines = {}, []

    def note(scene, what, fig):
        for k, v in fig.items():
            worst.setdefault(scene, {})[k] = max(worst.get(scene, {}).get(k, 0.0), v)
        lines.append(f"{scene:7s} {what:44s} " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()))
        print(lines[-1], flush=True)

    flat = S.scene_t(tempfile.mkdtemp())
    for which in ("all", "arm"):
        for B, K in T.SHAPES:
            hm, hb = make_hip(flat, None, B=B)
            hb.set("qpos", S.scene_t_qpos(flat, B).astype(np.float32)); hb.forward()
            dofs = S.dofs_t(flat, which)
            q = S.candidates(flat, dofs, B, K)
            pairs = clearance.default_pairs(flat, dofs)
            xp, xq, fig = T.fk_figures(flat, hb, dofs, q)
            note("T", f"fk {which} B {B} K {K}", fig)
            if (B, K) == T.SHAPES[0]:
                note("T", f"fk against forward() {which}", {"fk_step": T.step_fk_figure(flat, None, hb, dofs, q, xp)})
                note("T", f"identity {which}", {"ident": T.ident_figure(hb, flat, dofs, pairs, S.DISTMAX_T)})
                every = D.all_pairs(flat)
                note("T", f"every pair {which}", T.clear_figures(flat, hb.config_clearance(dofs, T.dev(q), pairs=every, distmax=1.0), xp, xq, every, 1.0, EDGE)[0])
            ref = S.pair_reference(flat, xp, xq, pairs, S.params32(flat))[0]
            for chunks in (1, 2, len(pairs), 0, 7):
                out = hb.config_clearance(dofs, T.dev(q), distmax=S.DISTMAX_T, chunks=chunks)
                note("T", f"clearance {which} B {B} K {K} chunks {chunks}", T.clear_figures(flat, out, xp, xq, pairs, S.DISTMAX_T, EDGE, ref=ref)[0])
    for name in ("panda", "baxter_right", "baxter_left", "baxter_both"):
        s = S.arm(name)
        f, cfg, dofs = s["flat"], s["cfg"], s["dofs"]
        scene = "panda" if name == "panda" else "baxter"
        B, K = T.SHAPES[0]
        hm, hb = make_hip(f, cfg, B=B)
        hb.set("qpos", np.tile(s["qpos"], (B, 1)).astype(np.float32)); hb.set("qvel", 0); hb.forward()
        q = S.candidates(f, dofs, B, K)
        pairs = clearance.default_pairs(f, dofs)
        xp, xq, fig = T.fk_figures(f, hb, dofs, q)
        note(scene, f"fk {name}", fig)
        note(scene, f"fk against forward() {name}", {"fk_step": T.step_fk_figure(f, cfg, hb, dofs, q, xp)})
        out = hb.config_clearance(dofs, T.dev(q), distmax=S.DISTMAX_ARM)
        note(scene, f"clearance {name} ({len(pairs)} pairs)", T.clear_figures(f, out, xp, xq, pairs, S.DISTMAX_ARM, EDGE)[0])
        note(scene, f"identity {name}", {"ident": T.ident_figure(hb, f, dofs, pairs, S.DISTMAX_ARM)})
    lines.append("")
    lines.append("worst per scene (tests/test_clearance.py MEASURED; the tests assert 4 x; witness is held to the dist bound, pick to twice it):")
    for scene, fig in worst.items():
        lines.append(f"{scene:7s} " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    print("\n".join(lines[-len(worst) - 1:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("Configuration clearance kernels against the fp64 mirror (tools/clearance_parity.py), one run on an MI355X.\n"
                     "fk_pos m / fk_rot rad: config_fk against clearance.fk, every body; fk_step m: against the step path's forward(); dist m: |dist - min_ref| at the\n"
                     "device's own poses; witness m: reported points outside their solids, |p2 - p1| against |dist|; pick m: the chosen pair's reference distance above\n"
                     "the minimum; ident m: K = 1 at the env's own joints against torch.min over geom_distance.\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
