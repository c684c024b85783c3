"""The kernels of the dynamics derivatives (csrc/rsim_dyn_grad.hip), read from the code objects embedded in the in-tree library (no GPU needed): the two are
present, and neither touches the private segment or LDS.  Every kernel named in tests/test_dynamics_attach_kernel_resources.py -- the plain and the attached
dynamics kernels' neighbours, the FK and joint walks, k_dyn_solve, the control step -- keeps the registers the Makefile states: a code object of its own
changes no other.  ELF metadata only."""
import os

import pytest

from tests.test_dynamics_attach_kernel_resources import NEW as ATT, OLD, waves
from tools.kernel_resources import LLVM, kernels

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robosuite_amd", "librsim_hip.so")
pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the built library and llvm-readelf")

NEW = ("_Z13k_dyn_rne_jvp8DDynGrad", "_Z14k_dyn_rne_grad8DDynGrad")


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
    for name in ATT:
        assert name in ks and ks[name]["scratch"] == 0 and ks[name]["lds"] == 0, name
