"""Registers, LDS and scratch of the kernels of keyed LE following (le_keyed.h), read from the built library as
tests/test_le_span_kernel_resources.py does for the span stage: DESIGN 3.8.9 names five kernels, none of them with scratch or a
spilled register, and states their VGPR and LDS figures.  Only le_keyed_open_kernel holds AES's round table (1 KiB) and a key
schedule in registers: 66 VGPRs, seven waves per SIMD; the others stay far below 64."""
import os
import re

import pytest

from test_kernel_resources import _kernels, SO, READELF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> (VGPRs, bytes of LDS), as DESIGN 3.8.9 lists them
DOCUMENTED = {
    "le_keyed_slot_kernel": (30, 0), "le_keyed_open_kernel": (66, 1024), "le_keyed_param_kernel": (26, 0),
    "le_keyed_pkt_epoch_kernel": (14, 0), "le_keyed_pkt_span_kernel": (17, 0),
}


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "the library has not been built"
    assert os.path.exists(READELF), "llvm-readelf of the ROCm installation is missing"
    return {n: k for n, k in _kernels().items() if "le_keyed_" in n}


def test_the_kernels_are_the_documented_ones(kernels):
    assert sorted(kernels) == sorted(DOCUMENTED)           # (extern "C": the symbols are the plain names)
    for n in kernels:                                      # the other families' resource tests count kernels by these substrings
        assert not any(s in n for s in ("le_seed_", "le_epoch_", "le_span_", "le_crypt_", "le_data_", "le_pair_", "le_track_", "le_disc_",
                                        "le_csa2_", "follow_", "hop_", "survey_", "acquire_", "order_", "le_decode_kernel",
                                        "header_flags_kernel", "decode_kernel", "replay_kernel")), n


def test_no_scratch_no_spills(kernels):
    for n, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert k["max_flat_workgroup_size"] == 256, (n, k)


def test_registers_and_lds_as_documented(kernels):
    for name, (vgprs, lds) in DOCUMENTED.items():
        k = kernels[name]
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == (vgprs, lds), (name, k["vgpr_count"], k["group_segment_fixed_size"])
        assert k["vgpr_count"] <= 72                       # seven waves per SIMD at the least


def test_design_lists_the_same_figures():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("#### 3.8.9"):]
    for name, (vgprs, lds) in DOCUMENTED.items():
        assert re.search(r"`%s`\s*\|\s*%d\s*\|\s*%d\s*\|" % (name, vgprs, lds), section), name
