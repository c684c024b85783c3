"""The dynamics query kernels with carried payloads (csrc/rsim_dyn_att.hip), read from the code objects embedded in the in-tree library (no GPU needed): the
three are present, and none touches the private segment or LDS.  Every kernel they run beside or behind -- the plain dynamics kernels, the FK and joint walks,
k_dyn_solve, the control step -- reports the registers it reported before this code object existed (the Makefile's figures: a code object of its own changes no
other).  ELF metadata only."""
import os

import pytest

from tools.kernel_resources import LLVM, kernels

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robosuite_amd", "librsim_hip.so")
pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the built library and llvm-readelf")

NEW = ("_Z13k_dyn_rne_att4DDyn", "_Z13k_dyn_crb_att4DDyn", "_Z13k_dyn_jac_att4DDyni")
STEP = "ILi{}ELi16ELi{}ELi{}ELi{}ELi{}ELi64ELi{}EEv6DModel6DBatchPKfii"
CFG = {0: STEP.format(32, 16, 24, 16, 16, 192), 1: STEP.format(32, 32, 24, 16, 32, 192), 2: STEP.format(64, 16, 32, 32, 32, 320)}
# registers (VGPR + AGPR) as before this code object: robosuite_amd/csrc/Makefile
OLD = {"_Z9k_dyn_rne4DDyn": 78, "_Z9k_dyn_crb4DDyn": 51, "_Z9k_dyn_jac4DDyn": 26,
       "_Z10k_clear_fk6DClear": 49, "_Z14k_clear_fk_att6DClear": 56, "_Z14k_clear_joints5DGrad": 55, "_Z11k_dyn_solve6DSolve": 57,
       "_Z6k_step" + CFG[0]: 247, "_Z6k_step" + CFG[1]: 251, "_Z6k_step" + CFG[2]: 250,
       "_Z11k_full_step" + CFG[0]: 250, "_Z11k_full_step" + CFG[1]: 254, "_Z11k_full_step" + CFG[2]: 252}


def waves(r):
    return min(8, 512 // (8 * -(-(r["vgpr"] + r["agpr"]) // 8)))


@pytest.fixture(scope="module")
def ks():
    return kernels(LIB)


def test_every_new_kernel_is_there_without_scratch_and_lds(ks):
    for name in NEW:
        assert name in ks, name
        print(f"{name}: {ks[name]['vgpr'] + ks[name]['agpr']} registers, {waves(ks[name])} wavefronts per SIMD")
        assert ks[name]["scratch"] == 0 and ks[name]["lds"] == 0, (name, ks[name])


def test_every_kernel_beside_them_is_as_before(ks):
    for name, regs in OLD.items():
        assert name in ks, name
        assert ks[name]["vgpr"] + ks[name]["agpr"] == regs and ks[name]["scratch"] == 0, (name, ks[name])
