"""Worst figures of the clearance gradient and collision cost kernels against their fp64 references, per scene, in one GPU run: what
tests/test_clearance_grad.py keeps in MEASURED and asserts four times.  Runs the very functions the tests run (make_case, grad_figures, cost_figures) on the
tests' scenes, shapes and chunkings, asserts no bound, and prints one line per figure.

    python tools/grad_parity.py [--out profiles/grad_parity.txt]"""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from robosuite_amd import mjcf      # noqa: E402
from tests import attach_scenes as A      # noqa: E402
from tests import clearance_scenes as S      # noqa: E402
from tests import test_clearance_grad as T      # noqa: E402
from tests import test_clearance_grad_host as H      # noqa: E402
from tests.util import make_hip      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    worst, lines = {}, []

    def note(scene, what, fig, counts=None):
        for k, v in fig.items():
            worst.setdefault(scene, {})[k] = max(worst.get(scene, {}).get(k, 0.0), v)
        lines.append(f"{scene:6s} {what:46s} " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()) + ("  " + str(counts) if counts else ""))
        print(lines[-1], flush=True)

    def both(scene, what, c, distmax, pairs, **att):
        hb, q = c["hb"], T.dev(c["q"])
        note(scene, f"gradient {what}", *T.grad_figures(c, hb.config_clearance_grad(c["dofs"], q, pairs=pairs, distmax=distmax, **att), distmax))
        for chunks in (1, 2, len(c["plist"]), 0):
            out = hb.config_collision_cost(c["dofs"], q, pairs=pairs, d_safe=T.D_SAFE[scene], chunks=chunks, **att)
            note(scene, f"cost {what} chunks {chunks}", *T.cost_figures(c, out, T.D_SAFE[scene], T.DIST_BOUND[scene]))

    scene_t = (S.scene_t(tempfile.mkdtemp()), {})
    flat = scene_t[0]
    for which in ("all", "arm"):
        for B, K in T.SHAPES:
            both("T", f"{which} B {B} K {K}", T.case_t(scene_t, B, K, which), S.DISTMAX_T, None)
    B, K = 6, 5      # attachments, as tests/test_clearance_grad.py test_attachments_scene_t
    hm, hb = make_hip(flat, None, B=B)
    hb.set("qpos", S.scene_t_qpos(flat, B).astype(np.float32)); hb.forward()
    dofs = S.dofs_t(flat, "all")
    held = np.repeat((np.arange(B) % 2 == 0)[:, None], 2, axis=1)
    c = T.make_case(flat, hb, dofs, S.candidates(flat, dofs, B, K), attach=A.attach_t(flat), held=held, rel=A.rel_given(B))
    both("T", "attached, default list", c, S.DISTMAX_T, None, **c["att"])
    for B, K in T.SHAPES:
        c = T.case_panda(B, K)
        both("panda", f"B {B} K {K} ({len(c['plist'])} pairs)", c, S.DISTMAX_ARM, None)
        keep = [i for i in range(len(c["plist"])) if not T._static_near(c, i)]
        sub = dict(c, plist=c["plist"][keep], d=c["d"][..., keep], ft=c["ft"][:, :, keep], st=c["st"][..., keep])
        out = c["hb"].config_clearance_grad(c["dofs"], T.dev(c["q"]), pairs=sub["plist"], distmax=S.DISTMAX_ARM)
        note("panda", f"gradient B {B} K {K} without the static near pairs", *T.grad_figures(sub, out, S.DISTMAX_ARM))
    chain = mjcf.compile_mjcf(H.chain_xml())
    for ndof in (H.CHAIN_N, 1):
        dofs = S.dofs_of(chain, [f"cj{i}" for i in range(H.CHAIN_N)]) if ndof > 1 else S.dofs_of(chain, ["cj7"])
        hm, hb = make_hip(chain, None, B=2)
        hb.forward()
        c = T.make_case(chain, hb, dofs, S.candidates(chain, dofs, 2, 35), pairs=H.chain_pairs(chain))
        both("chain", f"{ndof} dofs", c, 5.0, c["plist"])
    lines.append("")
    lines.append("worst per scene (tests/test_clearance_grad.py MEASURED; the tests assert 4 x):")
    for scene, fig in worst.items():
        lines.append(f"{scene:6s} " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    print("\n".join(lines[-len(worst) - 1:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("Clearance gradient and collision cost kernels against their fp64 references (tools/grad_parity.py), one run on an MI355X.\n"
                     "formula: |grad - n . (s2 v(p2) - s1 v(p1))| per entry, the right side in fp64 from the device's own config_fk poses, fromto, dist and pair, every\n"
                     "candidate; mirror: |grad - mirror's grad| per entry at the mirror's own witnesses (status 0, |dist| >= 1e-3, the same pair); cost m^2 / cost_grad\n"
                     "m^2/rad: against the mirror's reduction of the reference distances at the device's poses.  Counts: candidates of the mirror check, dropped for another\n"
                     "pair, with a zero gradient by rule; cost: candidates with several near pairs.\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
