"""The clearance gradient and collision cost kernels (csrc/rsim_grad.hip), read from the code objects embedded in the in-tree library (no GPU needed): every
one of them is present, and none touches the private segment or LDS -- a spill in k_clear_cost's pair loop would be HBM traffic of every lane at every pair.
The cost kernel keeps its gradient in the lane's own words of the result, not in registers, and so runs at the occupancy of k_clear_dist, whose loop it shares
(512 registers per SIMD lane, allocated in blocks of 8).  ELF metadata only."""
import os

import pytest

from tools.kernel_resources import LLVM, kernels

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robosuite_amd", "librsim_hip.so")
pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the built library and llvm-readelf")

NEW = ("_Z14k_clear_joints5DGrad", "_Z12k_clear_grad5DGrad", "_Z16k_clear_grad_att5DGrad", "_Z12k_clear_cost5DGrad", "_Z16k_clear_cost_att5DGrad",
       "_Z16k_clear_cost_sum5DGrad")


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


def test_the_cost_kernels_run_at_the_occupancy_of_the_distance_kernel(ks):
    for name, like in (("_Z12k_clear_cost5DGrad", "_Z12k_clear_dist6DClear"), ("_Z16k_clear_cost_att5DGrad", "_Z16k_clear_dist_att6DClear")):
        assert waves(ks[name]) >= waves(ks[like]), (name, ks[name], ks[like])
