"""Worst figures of the carried-object queries, per shape and rel mode, in one GPU run: what tests/test_attach.py keeps in MEASURED.  Runs the very functions
the tests run (fk_figures, clear_figures, transplant_figure, sweep_figures) on scene T with the sphere on the last link and the box on the side link
(tests/attach_scenes.py), asserts no bound beyond the exact properties inside those functions, and prints one line per figure; then the resources of the
clearance and sweep kernels, plain and attached.

    python tools/attach_parity.py [--out profiles/attach_parity.txt]"""
import argparse
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import attach_scenes as A      # noqa: E402
from tests import clearance_scenes as S      # noqa: E402
from tests import test_attach as T      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    worst, lines = {}, []

    def note(what, fig, tail=""):
        for k, v in fig.items():
            worst[k] = max(worst.get(k, -np.inf), v)
        lines.append(f"{what:28s} " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()) + ("  | " + tail if tail else ""))
        print(lines[-1], flush=True)

    scene = (S.scene_t(tempfile.mkdtemp()), {})
    flat = scene[0]
    for B, K in T.SHAPES:
        for mode in A.REL_MODES:
            c, m = T.mode_of(scene, B, K, mode)
            what = f"T B {B} K {K} rel {mode}"
            note(what + " fk", T.fk_figures(flat, c, m))
            for chunks in (0, 3):
                out = c["hb"].config_clearance(c["dofs"], T.dev(c["q"]), distmax=S.DISTMAX_T, chunks=chunks, **m["kw"])
                fig, _ = T.clear_figures(flat, out, m["xp"].astype(np.float64), m["xq"].astype(np.float64), c["pairs"], S.DISTMAX_T, T.BOUND["T"]["dist"], ref=m["ref"])
                far = int((out[1] < 0).sum())
                note(what + f" chunks {chunks}", fig, f"{far} of {B * K} far; evaluated pairs per env {int(c['on'].sum(axis=1).min())} .. {int(c['on'].sum(axis=1).max())} of {len(c['pairs'])}")
            if (B, K) == T.SHAPES[0]:
                note(what + " transplant", {"transplant": T.transplant_figure(flat, c, m)})
            out, fig = T.sweep_figures(flat, c, m)
            kind, steps = out[0].cpu().numpy() & 3, out[6].cpu().numpy()
            note(what + " sweep", fig, f"sample identity bitwise yes; free {int((kind == 0).sum())} hit {int((kind == 1).sum())} undecided {int((kind == 2).sum())}; "
                                       f"steps mean {steps.mean():.1f} max {int(steps.max())}")
    seen = dict(worst)
    for mode in A.REL_MODES:      # scene J: an attached SUBTREE (tool, jaw, tip, guard on the wrist); held to reasoned bounds, so it stays out of `worst`
        fj, c, m = T.batch_j(mode)
        what = f"J B {T.SHAPE_J[0]} K {T.SHAPE_J[1]} rel {mode}"
        note(what + " fk", T.fk_figures(fj, c, m))
        out = c["hb"].config_clearance(c["dofs"], T.dev(c["q"]), distmax=S.DISTMAX_T, **m["kw"])
        note(what + " chunks 0", T.clear_figures(fj, out, m["xp"].astype(np.float64), m["xq"].astype(np.float64), c["pairs"], S.DISTMAX_T, T.HOST_DIST_BOUND, ref=m["ref"])[0])
        out, fig = T.sweep_figures(fj, c, m)
        kind = out[0].cpu().numpy() & 3
        note(what + " sweep", fig, f"free {int((kind == 0).sum())} hit {int((kind == 1).sum())} undecided {int((kind == 2).sum())}")
    worst.clear(); worst.update(seen)
    lines.append("")
    lines.append("worst over scene T's shapes and rel modes (tests/test_attach.py MEASURED keeps held_pos, held_rot, transplant):")
    lines.append("  ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    try:
        from tools.kernel_resources import kernels
        for k, v in sorted(kernels(os.path.join(ROOT, "robosuite_amd", "librsim_hip.so")).items()):
            if "k_clear" in k or "k_sweep" in k:
                lines.append(f"{k}: {v['vgpr']} registers, {v['scratch']} B of scratch, {v['lds']} B of LDS")
    except Exception as e:      # (llvm-readelf not at hand)
        lines.append(f"kernel resources not read ({e})")
    print("\n".join(lines[-10:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("Carried objects (rsim_attach) on the device held to the fp64 mirror and to the plain queries (tools/attach_parity.py), one run on an MI355X.\n"
                     "Scene T, fsb on l2 and fbb on side, dofs all, held[e] = (e % 2 == 0, e % 3 != 0); rel from the env's state or given (tests/attach_scenes.py).\n"
                     "fk_pos m / fk_rot rad: config_fk against the mirror over the unattached bodies; held_pos / held_rot: over HELD attached bodies (bodies not held are\n"
                     "asserted bitwise the env's pose); dist / witness / pick m: config_clearance at the device's own poses against the mirror over the pairs each env\n"
                     "evaluates; transplant m: ||dist| - |plain config_clearance|| on a second batch with the free bodies written to the attached poses; shortfall / hit m,\n"
                     "bound_lo / bound_hi (1 - L / mirror L, L / mirror L - 1), centres m (negative: inside the bound), carried_share (the carried geoms' densest\n"
                     "displacement rate over L): the sweep, as tools/sweep_parity.py.  Each rel mode sweeps segments of its own (tests/attach_scenes.py SEGMENTS).\n"
                     "Scene J: the tool with jaw, tip and guard attached to the wrist, held in every other env -- the walk of an attached subtree.\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
