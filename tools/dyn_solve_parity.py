"""Prints the worst figures of the M^-1 queries beside the bounds they are held to, from the functions of tests/test_dynamics_solve.py (the device) and
tests/test_dynamics_solve_core_host.py (the host rehearsal of the same source): per scene the error of each quantity against numpy's fp64 solve on the device's
own M, b and J, relative to ||x_ref|| per column, and the share of the reasoned bound it uses (tests/dynamics_solve_scenes.py); end to end against the fp64
statement and the oracle; the round trip through config_inverse_dynamics; then the registers of the kernels involved.

    python tools/dyn_solve_parity.py [--out profiles/dyn_solve_parity.txt]"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from robosuite_amd import dynamics      # noqa: E402
from tests import dynamics_scenes as D      # noqa: E402
from tests import dynamics_solve_scenes as V      # noqa: E402
from tests import test_dynamics_solve as T      # noqa: E402
from tests import test_dynamics_solve_core_host as H      # noqa: E402
from tools.kernel_resources import kernels      # noqa: E402

SCENES = {"d_arm": "scene D arm (5, 13), per-env parameters", "d_all": "scene D all (5, 13), per-env parameters", "lift": "Lift / Panda (3, 22)",
          "chain16": "16-hinge chain (2, 5)"}


def row(what, fig):
    return f"  {what:44s} error {fig[0]:.3e}   share of its bound {fig[1]:.3e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["error: worst over candidates and columns of ||x - x_ref|| / ||x_ref|| (lambda_inv: worst entry error); share: worst error / its bound"]
    for name, title in SCENES.items():
        c = T.case(name)
        rel = c["rel"]
        lines.append(f"{title}: kappa_2(M_dev) <= {V.kappa(c['M']).max():.1f}, bound of the solve {rel.min():.1e} .. {rel.max():.1e}")
        lines.append(" device, against fp64 on the device's own M, b, J")
        lines += [row(k, v) for k, v in T.solve_figures(c).items()]
        fd, ms = T.end_to_end(c, "the fp64 statement", c["ref"]["M"], c["ref"]["tau"])
        lines.append(" device, end to end against the fp64 statement (allowance: ||M_ref^-1|| (||dM|| ||x|| + ||db||) + the bound of the solve)")
        lines += [row("forward dynamics", fd), row("mass solve r = 16", ms)]
        if name in ("lift", "chain16"):
            ref = D.oracle_reference(dynamics.model32(c["flat"]), c["qpos"], c["dofs"], c["q"], c["qd"], None)
            fd, ms = T.end_to_end(c, "the oracle", ref["M"], ref["tau"])
            lines.append(" device, end to end against the oracle")
            lines += [row("forward dynamics", fd), row("mass solve r = 16", ms)]
        lines.append(" device, round trip through config_inverse_dynamics (allowance: ||M_ref^-1|| sqrt(n) 2 beta S_tau + the bound of the solve)")
        lines.append(row("forward dynamics of inverse dynamics", T.round_trip_figures(c)))
    lines.append("")
    with tempfile.TemporaryDirectory() as tmp:
        exe, err = H.build(tmp)
        if exe is None:
            lines.append(f"host rehearsal: not built ({err.strip().splitlines()[-1] if err.strip() else 'g++ failed'})")
        else:
            for what, args in (("scene D arm (5, 13)", H.scene_d_inputs("arm")), ("scene D all (5, 13)", H.scene_d_inputs("all")), ("16-hinge chain (2, 5)", H.chain_inputs())):
                lines.append(f"host rehearsal under ASan + UBSan, {what}, against fp64 on the same fp32 inputs")
                lines += [row(k, v) for k, v in H.hold(what, H.run(exe, tmp, *args), *args).items()]
    lines.append("")
    lines.append("registers (VGPR + AGPR) / static LDS bytes / scratch bytes")
    ks = kernels(os.path.join(ROOT, "robosuite_amd", "librsim_hip.so"))
    for n in sorted(ks):
        if "k_dyn_" in n or "k_clear_fk" in n or "k_clear_joints" in n:
            lines.append(f"{n:32s} {ks[n]['vgpr'] + ks[n]['agpr']:4d} / {ks[n]['lds']} / {ks[n]['scratch']}")
    lines.append("k_dyn_solve's LDS is dynamic: (n (n + 1) / 2 + n) * 256 B per workgroup -- 8 960 B for n = 7, 38 912 B for n = 16")
    print("\n".join(lines))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
