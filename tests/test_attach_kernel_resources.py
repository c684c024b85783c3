"""The clearance and sweep kernels, plain and attached, read from the code objects embedded in the in-tree library (no GPU needed).  A call with attachments
runs k_clear_fk_att / k_clear_dist_att / k_sweep_att, the same bodies with the attachment branches compiled in; a call without runs the kernels it always
ran.  None of them may touch the private segment or LDS (a spill in the pair loop or the advancement loop is HBM traffic of every lane at every pair), the
plain kernels keep the registers they had before there were attachments, and an attached kernel runs at no fewer wavefronts per SIMD than its plain form
(512 registers per SIMD lane, allocated in blocks of 8)."""
import os

import pytest

from tools.kernel_resources import LLVM, kernels

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robosuite_amd", "librsim_hip.so")
pytestmark = pytest.mark.skipif(not (os.path.exists(LIB) and os.path.exists(os.path.join(LLVM, "llvm-readelf"))), reason="needs the built library and llvm-readelf")

PLAIN = {"_Z10k_clear_fk6DClear": 49, "_Z12k_clear_dist6DClear": 136, "_Z11k_clear_min6DClear": 10, "_Z7k_sweep6DSweep": 161}      # registers before attachments
ATTACHED = {"_Z14k_clear_fk_att6DClear": "_Z10k_clear_fk6DClear", "_Z16k_clear_dist_att6DClear": "_Z12k_clear_dist6DClear", "_Z11k_sweep_att6DSweep": "_Z7k_sweep6DSweep"}


def waves(r):
    return min(8, 512 // (8 * -(-(r["vgpr"] + r["agpr"]) // 8)))


@pytest.fixture(scope="module")
def ks():
    return kernels(LIB)


def test_no_scratch_and_no_lds_in_any_of_them(ks):
    for name in list(PLAIN) + list(ATTACHED):
        assert name in ks, name
        assert ks[name]["scratch"] == 0 and ks[name]["lds"] == 0, (name, ks[name])


def test_the_plain_kernels_keep_their_registers(ks):
    for name, regs in PLAIN.items():
        assert ks[name]["vgpr"] + ks[name]["agpr"] <= regs, (name, ks[name])


def test_an_attached_kernel_runs_at_the_occupancy_of_its_plain_form(ks):
    for name, plain in ATTACHED.items():
        print(f"{name}: {ks[name]['vgpr']} registers, {waves(ks[name])} wavefronts per SIMD; {plain}: {ks[plain]['vgpr']}, {waves(ks[plain])}")
        assert waves(ks[name]) >= waves(ks[plain]), (name, ks[name], ks[plain])
