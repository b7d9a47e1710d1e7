"""Registers, LDS and scratch of the LE channel selection #2 kernels (le_csa2.h), read from the built library as
tests/test_le_track_kernel_resources.py does for the tracking: DESIGN 3.8.3 names five kernels, none of them with scratch or a
spilled register, and states their VGPR and LDS figures.  The scoring kernel tabulates expected() in LDS for a window of
counters (4 KiB beside 4 KiB of events), not for all 65 536 (64 KiB), so LDS does not decide its occupancy and the limit of 64 VGPRs
-- eight waves per SIMD -- holds for it as for the others."""
import os

import pytest

from test_kernel_resources import _kernels, SO, READELF

# kernel -> (VGPRs, bytes of LDS), as DESIGN 3.8.3 lists them
DOCUMENTED = {
    "le_csa2_base_kernel": (54, 32), "le_csa2_event_kernel": (8, 0), "le_csa2_score_kernel": (36, 8560),
    "le_csa2_verdict_kernel": (34, 0), "le_csa2_pkt_kernel": (12, 0),
}


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "the library has not been built"
    assert os.path.exists(READELF), "llvm-readelf of the ROCm installation is missing"
    return {n: k for n, k in _kernels().items() if "le_csa2_" in n}


def test_the_kernels_are_the_documented_ones(kernels):
    assert sorted(kernels) == sorted(DOCUMENTED)           # (extern "C": the symbols are the plain names)
    for n in kernels:                                      # the other families' resource tests count kernels by these substrings
        assert not any(s in n for s in ("le_track_", "le_disc_", "follow_", "hop_", "survey_", "acquire_")), n


def test_no_scratch_no_spills(kernels):
    for n, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert k["max_flat_workgroup_size"] == 256, (n, k)


def test_registers_and_lds_as_documented(kernels):
    for name, (vgprs, lds) in DOCUMENTED.items():
        k = kernels[name]
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == (vgprs, lds), (name, k["vgpr_count"], k["group_segment_fixed_size"])
        assert k["vgpr_count"] <= 64                       # eight waves per SIMD
