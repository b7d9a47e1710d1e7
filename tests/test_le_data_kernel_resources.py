"""Registers, LDS and scratch of the kernels of LE data extraction (le_data.h), read from the built library as
tests/test_le_span_kernel_resources.py does for the span stage: DESIGN 3.8.6 names eighteen kernels, none of them with scratch or
a spilled register, and states their VGPR and LDS figures; none needs more than 64 VGPRs -- eight waves per SIMD."""
import os
import re

import pytest

from test_kernel_resources import _kernels, SO, READELF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> (VGPRs, bytes of LDS), as DESIGN 3.8.6 lists them
DOCUMENTED = {
    "le_data_init_kernel": (12, 0), "le_data_slot_kernel": (10, 0), "le_data_open_sum_kernel": (28, 32), "le_data_open_prefix_kernel": (21, 32),
    "le_data_open_kernel": (29, 32), "le_data_prev_sum_kernel": (16, 16), "le_data_prev_prefix_kernel": (15, 16), "le_data_prev_kernel": (26, 16),
    "le_data_msg_sum_kernel": (33, 112), "le_data_msg_prefix_kernel": (38, 112), "le_data_msg_kernel": (46, 112),
    "le_data_close_kernel": (12, 0), "le_data_number_sum_kernel": (22, 48), "le_data_number_prefix_kernel": (27, 48),
    "le_data_number_kernel": (44, 48), "le_data_pkt_kernel": (18, 0), "le_data_conn_kernel": (22, 0), "le_data_gather_kernel": (40, 1024),
}


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "the library has not been built"
    assert os.path.exists(READELF), "llvm-readelf of the ROCm installation is missing"
    return {n: k for n, k in _kernels().items() if "le_data_" in n}


def test_the_kernels_are_the_documented_ones(kernels):
    assert sorted(kernels) == sorted(DOCUMENTED)           # (extern "C": the symbols are the plain names)
    for n in kernels:                                      # the other families' resource tests count kernels by these substrings
        assert not any(s in n for s in ("le_seed_", "le_epoch_", "le_span_", "le_track_", "le_disc_", "le_csa2_", "follow_", "hop_", "survey_",
                                        "acquire_", "order_", "le_decode_kernel", "header_flags_kernel", "decode_kernel", "replay_kernel")), n


def test_no_scratch_no_spills(kernels):
    for n, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert k["max_flat_workgroup_size"] == 256, (n, k)


def test_registers_and_lds_as_documented(kernels):
    for name, (vgprs, lds) in DOCUMENTED.items():
        k = kernels[name]
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == (vgprs, lds), (name, k["vgpr_count"], k["group_segment_fixed_size"])
        assert k["vgpr_count"] <= 64                       # eight waves per SIMD


def test_design_lists_the_same_figures():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("#### 3.8.6"):]
    for name, (vgprs, lds) in DOCUMENTED.items():
        assert re.search(r"`%s`\s*\|\s*%d\s*\|\s*%d\s*\|" % (name, vgprs, lds), section), name
