"""Registers, LDS and scratch of the LE tracking kernels (le_track.h), read from the built library as
tests/test_le_discover_kernel_resources.py does for the discovery: DESIGN 3.8.2 names thirteen kernels, none of them with scratch
or a spilled register, and states their VGPR and LDS figures."""
import os

import pytest

from test_kernel_resources import _kernels, SO, READELF

# kernel -> (VGPRs, bytes of LDS), as DESIGN 3.8.2 lists them
DOCUMENTED = {
    "le_track_init_kernel": (12, 0), "le_track_key_kernel": (11, 0), "le_track_rekey_kernel": (6, 0), "le_track_flag_kernel": (14, 4),
    "le_track_prefix_kernel": (22, 16), "le_track_event_kernel": (38, 16), "le_track_interval_kernel": (22, 0),
    "le_track_step_kernel": (22, 8), "le_track_prefix64_kernel": (34, 32), "le_track_count_kernel": (34, 32),
    "le_track_score_kernel": (20, 148), "le_track_verdict_kernel": (48, 0), "le_track_pkt_kernel": (26, 0),
}


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "the library has not been built"
    assert os.path.exists(READELF), "llvm-readelf of the ROCm installation is missing"
    return {n: k for n, k in _kernels().items() if "le_track_" in n}


def test_the_kernels_are_the_documented_ones(kernels):
    assert len(kernels) == len(DOCUMENTED), sorted(kernels)
    for name in DOCUMENTED:
        assert sum(name in n for n in kernels) == 1, (name, sorted(kernels))
    for n in kernels:                                      # the other families' resource tests count kernels by these substrings
        assert not any(s in n for s in ("le_disc_", "follow_", "hop_", "survey_", "acquire_")), n


def test_no_scratch_no_spills(kernels):
    for n, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert k["max_flat_workgroup_size"] == 256, (n, k)


def test_registers_and_lds_as_documented(kernels):
    for name, (vgprs, lds) in DOCUMENTED.items():
        k = [v for n, v in kernels.items() if name in n][0]
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == (vgprs, lds), (name, k["vgpr_count"], k["group_segment_fixed_size"])
        assert k["vgpr_count"] <= 64                       # eight waves per SIMD
