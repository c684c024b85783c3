"""Prints the worst figures of the dynamics queries on the device against the fp64 statement / the fp64 oracle, from the functions of tests/test_dynamics.py
(scene D with per-env parameters, Lift / Panda, Baxter with both arms), beside the reasoned bound each is held to; then the registers of the kernels involved
(tools/kernel_resources.py on the built library).  The host rehearsal's figures come from `pytest -s tests/test_dynamics_core_host.py`.

    python tools/dyn_parity.py [--out profiles/dyn_parity.txt]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import test_dynamics as T      # noqa: E402
from tools.kernel_resources import kernels      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["worst absolute error on the device against the scale (max |tau_ref|, max |M_ref|, 1 for J) -- and the reasoned bound"]
    rows = []
    for which in ("arm", "all"):
        fig, _, bound = T.scene_d_figures(which)
        rows.append((f"scene D {which} (5, 13), per-env parameters", fig, bound))
    fig, bound = T.lift_figures()
    rows.append(("Lift / Panda (3, 22), against the oracle", fig, bound))
    fig, bound, _ = T.baxter_figures()
    rows.append(("Baxter, both arms (2, 33), against the oracle", fig, bound))
    for name, fig, bound in rows:
        lines.append(f"{name:48s} " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()) + f"   bound {bound:.1e}")
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
