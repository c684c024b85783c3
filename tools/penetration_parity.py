"""Worst figures of the signed-overlap kernels against their fp64 references in one GPU run: what tests/test_penetration.py keeps in MEASURED and asserts four
times.  Runs the very functions the tests run (the scene and arm set-ups, figures, arm_figures), asserts no bound, and prints one line per figure.

    python tools/penetration_parity.py [--out profiles/penetration_parity.txt]"""
import argparse
import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_penetration as T      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for cast in ("P", "P2"):
        fig, counts = T.figures(T.make_scene(tempfile.mkdtemp(), cast))
        lines += [f"scene {cast}, B = 70, 28 pairs (tests/penetration_scenes.py), defaults pen_tol 1e-7, pen_iters 64, offset 4e-3:",
                  "  " + "  ".join(f"{k} {v}" if isinstance(v, int) else f"{k} {v:.2f}" for k, v in counts.items()),
                  "  " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items())]
        print("\n".join(lines[-3:]), flush=True)
    afig, acounts = T.arm_figures(T.make_arm())
    lines += [f"five-hinge arm, B = {T.AB}, K = {T.AK}, d_safe {T.Q.ARM_D_SAFE} (penetration_scenes.arm_cases), signed cost against the fp64 formula on the device's own dist / fromto:",
              "  " + "  ".join(f"{k} {v:.3e}" for k, v in afig.items()) + "  " + str(acounts)]
    print("\n".join(lines[-2:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("Signed distance of overlapping convex pairs on the device (csrc/rsim_pen.hip) against the fp64 mirror (robosuite_amd/penetration.py), one run on an\n"
                     "MI355X (tools/penetration_parity.py).  dist: worst |dist - mirror| over every pair outside the band (m); cert / cert_band: the certificate's worst\n"
                     "residual outside / inside the band, from the device's witnesses and n = (p2 - p1) / dist in fp64 (m); below_multistart: how far a band pair's depth is\n"
                     "below the multistart minimum (m); cost (m^2) / cost_grad (m^2 / rad): the signed collision cost against the formula.  tests/test_penetration.py\n"
                     "asserts 4 x these, floored at 4 x 2^-23 x the scale.\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
