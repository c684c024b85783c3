"""Prints the worst figures of the dynamics queries WITH CARRIED PAYLOADS on the device against the fp64 statement (robosuite_amd/dynamics.py with attach /
held / rel), from the functions of tests/test_dynamics_attach.py -- scene P with per-env masses and scene J's subtree at the three shapes and both rel modes --
beside the reasoned bound each is held to and the host rehearsal's worst figure; then the registers of the kernels involved (tools/kernel_resources.py on the
built library).  The host rehearsal's figures come from `pytest -s tests/test_dynamics_attach_core_host.py`.

    python tools/dyn_attach_parity.py [--out profiles/dyn_attach_parity.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import dynamics_attach_scenes as P      # noqa: E402
from tests import dynamics_scenes as D      # noqa: E402
from tests import test_dynamics_attach as T      # noqa: E402
from tools.kernel_resources import kernels      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["worst absolute error on the device against the scale (max |tau_ref|, max |M_ref|, 1 for J at load_tip) -- the reasoned bound -- the host rehearsal's worst"]
    for scene in ("P", "J"):
        for B, K in P.SHAPES:
            for mode in P.REL_MODES:
                c = T.case(scene, B, K, mode)
                fig = D.errors(c["got"], c["ref"])
                lines.append(f"scene {scene} {str((B, K)):8s} rel {mode:5s} " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()) + f"   bound {c['bound']:.1e}   rehearsal " +
                             "  ".join(f"{k} {v:.3e}" for k, v in T.REHEARSAL[scene].items()))
                print(lines[-1], flush=True)
    lines.append("")
    lines.append("registers (VGPR + AGPR) / LDS bytes / scratch bytes")
    ks = kernels(os.path.join(ROOT, "robosuite_amd", "librsim_hip.so"))
    for n in sorted(ks):
        if "k_dyn_" in n or "k_clear_fk" in n or "k_clear_joints" in n:
            lines.append(f"{n:32s} {ks[n]['vgpr'] + ks[n]['agpr']:4d} / {ks[n]['lds']} / {ks[n]['scratch']}")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
