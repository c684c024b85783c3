"""Prints the worst figures of the DERIVATIVES of the dynamics on the device against the fp64 statement by the definition of a derivative
(robosuite_amd/dynamics.py inverse_dynamics_grad / inverse_dynamics_jvp), from the functions of tests/test_dynamics_grad.py -- scene D with per-env tables
(arm, all), Lift, the 16-hinge chain -- beside the reasoned bound each is held to; then the fp64 figure KAPPA rounds up, per scene
(tests/dynamics_grad_scenes.py kappa_of), and the registers of the kernels involved (tools/kernel_resources.py on the built library).  The host rehearsal's
figures come from `pytest -s tests/test_dynamics_grad_core_host.py`; --rehearsal FILE copies the lines of such a run into the output.

    python tools/dyn_grad_parity.py [--out profiles/dyn_grad_parity.txt] [--rehearsal FILE]"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import dynamics_grad_scenes as G      # noqa: E402
from tests import test_dynamics_grad as T      # noqa: E402
from tools.kernel_resources import kernels      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rehearsal", default=None)
    a = ap.parse_args()
    lines = ["worst absolute error on the device against the scale (max |dtau_dq_ref|, max |dtau_dqd_ref|; the JVP: n times the largest of the three blocks' scales)"
             " -- the reasoned bound"]
    for name in T.CASES:
        c = T.case(name)
        fig = T.figures(c)
        kq, kv = G.kappa_of(c["flat"], c["qpos"], c["dofs"], c["q"], c["qd"], c["qdd"], overrides=c["over"])
        lines.append(f"{name:8s} {str((c['B'], c['K'])):8s} n {c['n']:2d}  " + "  ".join(f"{k} {v:.3e}" for k, v in fig.items()) + f"   bound {c['bound']:.1e}   "
                     f"largest intermediate / scale in fp64: d/dq {kq:.2f}, d/dqd {kv:.2f} (KAPPA {G.KAPPA:g})")
        print(lines[-1], flush=True)
    if a.rehearsal:
        lines += ["", "the host rehearsal (the same source, g++ on the host under ASan + UBSan):"]
        lines += [ln.rstrip().lstrip(".") for ln in open(a.rehearsal) if "fp32 tangent core on the host" in ln]
    lines += ["", "registers (VGPR + AGPR) / LDS bytes / scratch bytes"]
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
