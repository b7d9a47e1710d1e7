"""Registers, LDS and scratch of the kernels of LE legacy pairing key recovery (le_pair.h), read from the built library as
tests/test_le_crypt_kernel_resources.py does for the decryption stage: DESIGN 3.8.8 names twelve kernels, none of them with scratch
or a spilled register, and states their VGPR and LDS figures.  The search and finish kernels keep a key schedule of 44 words in
registers and may use up to 160 VGPRs, the budget of the decryption stage's trial kernels; every other kernel stays within 64."""
import os
import re

import pytest

from test_kernel_resources import _kernels, SO, READELF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("le_pair_init_kernel", "le_pair_find_kernel", "le_pair_prsp_kernel", "le_pair_mconf_kernel", "le_pair_sconf_kernel",
         "le_pair_mrand_kernel", "le_pair_srand_kernel", "le_pair_method_kernel", "le_pair_search_kernel", "le_pair_finish_kernel",
         "le_pair_slots_kernel", "le_pair_record_kernel")
SCHEDULE_IN_REGISTERS = ("le_pair_search_kernel", "le_pair_finish_kernel")
ROUND_TABLE_IN_LDS = SCHEDULE_IN_REGISTERS


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "the library has not been built"
    assert os.path.exists(READELF), "llvm-readelf of the ROCm installation is missing"
    return {n: k for n, k in _kernels().items() if "le_pair_" in n}


def test_the_kernels_are_the_documented_ones(kernels):
    assert sorted(kernels) == sorted(NAMES)                 # (extern "C": the symbols are the plain names)
    for n in kernels:                                      # the other families' resource tests count kernels by these substrings
        assert n.startswith("le_pair_")
        assert not any(s in n for s in ("le_data_", "le_seed_", "le_epoch_", "le_span_", "le_track_", "le_disc_", "le_csa2_", "le_crypt_",
                                        "follow_", "hop_", "survey_", "acquire_", "order_", "decode_kernel", "replay_kernel")), n


def test_no_scratch_no_spills(kernels):
    for n, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert k["max_flat_workgroup_size"] == 256, (n, k)


def test_registers_and_lds_within_their_budgets(kernels):
    for n, k in kernels.items():
        assert k["vgpr_count"] <= (160 if n in SCHEDULE_IN_REGISTERS else 64), (n, k["vgpr_count"])
        assert k["group_segment_fixed_size"] == (1024 if n in ROUND_TABLE_IN_LDS else (16 if n == "le_pair_slots_kernel" else 0)), n


def test_design_lists_the_figures_of_the_built_library(kernels):
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("#### 3.8.8"):text.index("### 3.9 ")]
    assert text.index("#### 3.8.7") < text.index("#### 3.8.8") < text.index("### 3.9 ")
    for n, k in kernels.items():
        assert re.search(r"`%s`\s*\|\s*%d\s*\|\s*%d\s*\|" % (n, k["vgpr_count"], k["group_segment_fixed_size"]), section), \
            (n, k["vgpr_count"], k["group_segment_fixed_size"])
    assert len(re.findall(r"^\| `le_pair_\w+` \|", section, re.M)) == len(NAMES)
