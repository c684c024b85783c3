"""The collision-aware IK kernels (csrc/rsim_ik_avoid.hip), read from the code objects embedded in the in-tree library (no GPU needed): every one of them is
present, and none touches the private segment or LDS -- a spill in k_ika_cost's pair loop would be HBM traffic of every lane at every pair of every evaluation,
and k_ika_step carries the 6 x 6 factorisation, the step and both walks in one kernel.  k_ika_cost (_att) instantiates the loop of k_clear_cost (_att) behind one
more test and must reach at least its wavefronts per SIMD (512 registers per SIMD lane, allocated in blocks of 8).  ELF metadata only."""
import os

import pytest

from tools.kernel_resources import LLVM, kernels

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robosuite_amd", "librsim_hip.so")
pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the built library and llvm-readelf")

NEW = ("_Z10k_ika_init8DIkAvoid", "_Z14k_ika_init_att8DIkAvoid", "_Z10k_ika_cost8DIkAvoid", "_Z14k_ika_cost_att8DIkAvoid", "_Z10k_ika_step8DIkAvoid",
       "_Z14k_ika_step_att8DIkAvoid")


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


def test_the_cost_kernels_run_at_the_occupancy_of_the_collision_cost(ks):
    for name, like in (("_Z10k_ika_cost8DIkAvoid", "_Z12k_clear_cost5DGrad"), ("_Z14k_ika_cost_att8DIkAvoid", "_Z16k_clear_cost_att5DGrad")):
        assert waves(ks[name]) >= waves(ks[like]), (name, ks[name], ks[like])
