"""The signed clearance and signed IK cost kernels (csrc/rsim_pen_query.hip), read from the code objects embedded in the in-tree library (no GPU needed): each of
the four is present, and none touches the private segment or LDS -- the descent calls the GJK core up to pen_iters times per overlapping pair, and a spill there
would be HBM traffic of every descending lane at every projection.  Registers and wavefronts per SIMD are printed; asserted is only that two wavefronts fit a
SIMD (512 registers per SIMD lane, allocated in blocks of 8), the floor the signed kernels of csrc/rsim_pen.hip hold.  ELF metadata only."""
import os

import pytest

from tools.kernel_resources import LLVM, kernels

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robosuite_amd", "librsim_hip.so")
pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the built library and llvm-readelf")

NEW = ("_Z19k_clear_dist_signed9DPenClear", "_Z23k_clear_dist_signed_att9DPenClear", "_Z17k_ika_cost_signed7DPenIka", "_Z21k_ika_cost_signed_att7DPenIka")


def waves(r):
    return min(8, 512 // (8 * -(-(r["vgpr"] + r["agpr"]) // 8)))


@pytest.fixture(scope="module")
def ks():
    return kernels(LIB)


def test_every_new_kernel_is_there_without_scratch_and_lds(ks):
    for name in NEW:
        assert name in ks, (name, sorted(k for k in ks if "signed" in k))
        print(f"{name}: {ks[name]['vgpr'] + ks[name]['agpr']} registers, {waves(ks[name])} wavefronts per SIMD")
        assert ks[name]["scratch"] == 0 and ks[name]["lds"] == 0, (name, ks[name])
        assert waves(ks[name]) >= 2, (name, ks[name])
