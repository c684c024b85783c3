"""The two control-step kernels of the fused-tier builds (configurations 0-2), read from the code objects embedded in the in-tree library (no GPU needed):
k_step, the plain form, and k_full_step with the profiler, the MPR restart cone and the applied forces compiled in (csrc/rsim_step.hip fused_step).  The plain
form exists to execute fewer instructions under less register pressure: it must not need more registers than the one kernel did before the split, and neither
form may touch the private segment (a spill inside the 25-substep loop is HBM traffic of every env at every substep: profiles/r04_y_ab_spills.txt)."""
import os

import pytest

from tools.kernel_resources import LLVM, kernels

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robosuite_amd", "librsim_hip.so")
pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the built library and llvm-readelf")

# k_step<NB, NJ, NV, NG, NS, NCON, NEFC, NPAIR> of configurations 0-2: VGPR + AGPR of the single kernel before the split (a condition, not a measurement)
FUSED = {"ILi32ELi16ELi16ELi24ELi16ELi16ELi64ELi192E": 250, "ILi32ELi16ELi32ELi24ELi16ELi32ELi64ELi192E": 254, "ILi64ELi16ELi16ELi32ELi32ELi32ELi64ELi320E": 252}
OTHER = ("ILi64ELi32ELi48ELi64ELi32ELi32ELi128ELi640E", "ILi64ELi32ELi64ELi64ELi32ELi32ELi128ELi640E", "ILi64ELi32ELi48ELi64ELi32ELi64ELi256ELi640E")


@pytest.fixture(scope="module")
def ks():
    return kernels(LIB)


def test_both_forms_exist_for_the_fused_tier_builds_only(ks):
    full = [n for n in ks if n.startswith("_Z11k_full_stepI")]
    assert len(full) == 3
    for tag in FUSED:
        assert len([n for n in full if tag in n]) == 1 and len([n for n in ks if n.startswith("_Z6k_stepI") and tag in n]) == 1, tag
    for tag in OTHER:
        assert not [n for n in full if tag in n] and len([n for n in ks if n.startswith("_Z6k_stepI") and tag in n]) == 1, tag


def test_the_plain_kernel_needs_no_scratch_and_no_more_registers_than_the_single_kernel_did(ks):
    for tag, regs in FUSED.items():
        (name,) = [n for n in ks if n.startswith("_Z6k_stepI") and tag in n]
        r = ks[name]
        assert r["scratch"] == 0 and r["vgpr"] <= regs, (name, r)


def test_the_full_kernel_keeps_two_wavefronts_per_simd_without_scratch(ks):
    for tag in FUSED:
        (name,) = [n for n in ks if n.startswith("_Z11k_full_stepI") and tag in n]
        r = ks[name]
        assert r["scratch"] == 0 and r["vgpr"] <= 256, (name, r)
        (plain,) = [n for n in ks if n.startswith("_Z6k_stepI") and tag in n]
        assert r["lds"] == ks[plain]["lds"], (name, r, ks[plain])       # same LDS layout: the same occupancy whichever form a launch takes
