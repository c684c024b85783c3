"""Worst figures of the signed clearance, its gradient and the signed collision-aware IK step against their fp64 references in one GPU run: what
tests/test_signed_queries.py keeps in MEASURED and asserts four times (floored).  Runs the very figure functions of the test modules, asserts no bound, and prints
one line per figure.

    python tools/signed_queries_parity.py [--out profiles/signed_queries_parity.txt]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import test_signed_ik_avoid as TI      # noqa: E402
from tests import test_signed_queries as TS      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    fig = TS.figures()
    print("  ".join(f"{k} {v:.3e}" for k, v in fig.items()), flush=True)
    fig.update(TI.figures())
    print(f"step {fig['step']:.3e}", flush=True)
    lines = [f"five-hinge arm, B = {TS.AB}, K = {TS.AK}, distmax {TS.DISTMAX} (penetration_scenes.arm_cases), config_clearance(signed=True) against the mirror on the device's poses:",
             f"  dist {fig['dist']:.3e}",
             "config_clearance_grad(signed=True) against clearance.pair_grad in fp64 on the device's own dist / fromto / poses:",
             f"  grad {fig['grad']:.3e}   (largest reference entry {fig['grad_largest']:.3f})",
             "the cargo box held by l4 in 2 of 4 envs, K = 16, the default list with the attachment, the holding envs against the mirror:",
             f"  dist_att {fig['dist_att']:.3e}",
             f"config_clearance(signed=True) at the {TI.SQ.B * TI.SQ.K} sunk starts of tests/signed_query_scenes.py, half of them box in box (the descent runs):",
             f"  dist_descend {fig['dist_descend']:.3e}",
             f"solve_ik_avoid(signed=True), one update from the {TI.SQ.B * TI.SQ.K} sunk starts of tests/signed_query_scenes.py against ik_avoid.update fed with the device's signed gradient:",
             f"  step {fig['step']:.3e}"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("Signed distances in config_clearance, config_clearance_grad and solve_ik_avoid on the device (csrc/rsim_pen_query.hip) against fp64, one run on an MI355X\n"
                     "(tools/signed_queries_parity.py).  dist / dist_att: worst |dist - mirror's smallest signed per-pair value| (m), dist_descend on the candidates of which half descend; grad: worst |grad - formula| per entry\n"
                     "(m / rad); step: worst |q_out - formula| per entry after one update (rad).  tests/test_signed_queries.py and tests/test_signed_ik_avoid.py assert\n"
                     "max(4 x these, floor): 4 x 2^-23 x 1.5 m, x the largest reference entry, x pi.\n\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
