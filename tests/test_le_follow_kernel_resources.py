"""Registers, LDS and scratch of the kernels of LE following from CONNECT_IND (le_follow.h), read from the built library as
tests/test_le_csa2_kernel_resources.py does for the selection: DESIGN 3.8.4 names thirteen kernels, none of them with scratch or a
spilled register, and states their VGPR and LDS figures; none needs more than 64 VGPRs -- eight waves per SIMD."""
import os

import pytest

from test_kernel_resources import _kernels, SO, READELF

# kernel -> (VGPRs, bytes of LDS), as DESIGN 3.8.4 lists them
DOCUMENTED = {
    "le_seed_join_kernel": (24, 0), "le_epoch_init_kernel": (7, 0), "le_epoch_slot_kernel": (26, 0), "le_epoch_open_kernel": (12, 0),
    "le_epoch_step_kernel": (23, 8), "le_epoch_stop_kernel": (18, 0), "le_epoch_mark_kernel": (24, 4), "le_epoch_list_kernel": (38, 16),
    "le_epoch_rekey_kernel": (6, 0), "le_epoch_gather_kernel": (8, 0), "le_epoch_predict_kernel": (26, 0),
    "le_epoch_verdict_kernel": (27, 0), "le_epoch_pkt_kernel": (14, 0),
}


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "the library has not been built"
    assert os.path.exists(READELF), "llvm-readelf of the ROCm installation is missing"
    return {n: k for n, k in _kernels().items() if "le_seed_" in n or "le_epoch_" in n}


def test_the_kernels_are_the_documented_ones(kernels):
    assert sorted(kernels) == sorted(DOCUMENTED)           # (extern "C": the symbols are the plain names)
    for n in kernels:                                      # the other families' resource tests count kernels by these substrings
        assert not any(s in n for s in ("follow_", "hop_", "le_track_", "le_disc_", "le_csa2_", "survey_", "acquire_", "le_decode_kernel",
                                        "header_flags_kernel")), n


def test_no_scratch_no_spills(kernels):
    for n, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert k["max_flat_workgroup_size"] == 256, (n, k)


def test_registers_and_lds_as_documented(kernels):
    for name, (vgprs, lds) in DOCUMENTED.items():
        k = kernels[name]
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == (vgprs, lds), (name, k["vgpr_count"], k["group_segment_fixed_size"])
        assert k["vgpr_count"] <= 64                       # eight waves per SIMD
