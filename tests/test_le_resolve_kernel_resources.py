"""Registers, LDS and scratch of the kernels of LE address resolution (le_resolve.h), read from the built library as
tests/test_le_pair_kernel_resources.py does for the pairing stage: DESIGN 3.8.10 names eleven kernels, none of them with scratch or a
spilled register, and states their VGPR and LDS figures.  The expand and trial kernels hold a key schedule of 44 words and may use up
to 160 VGPRs, the budget of the pairing search; every other kernel stays within 64.  The two run AES and have its round table, 1024
bytes, in LDS and nothing else there."""
import os
import re

import pytest

from test_kernel_resources import _kernels, SO, READELF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("le_resolve_init_kernel", "le_resolve_find_kernel", "le_resolve_table_kernel", "le_resolve_expand_kernel", "le_resolve_mark_kernel",
         "le_resolve_prefix_kernel", "le_resolve_rank_kernel", "le_resolve_tally_kernel", "le_resolve_trial_kernel", "le_resolve_addr_kernel",
         "le_resolve_peer_kernel")
HOLD_A_SCHEDULE = ("le_resolve_expand_kernel", "le_resolve_trial_kernel")
ROUND_TABLE_IN_LDS = HOLD_A_SCHEDULE
WAVE_SUMS_IN_LDS = ("le_resolve_table_kernel", "le_resolve_mark_kernel", "le_resolve_prefix_kernel", "le_resolve_rank_kernel")
OTHER_FAMILIES = ("le_data_", "le_seed_", "le_epoch_", "le_span_", "le_track_", "le_disc_", "le_csa2_", "le_crypt_", "le_pair_", "le_keyed_",
                  "follow_", "hop_", "survey_", "acquire_", "order_", "decode_kernel", "replay_kernel")


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "the library has not been built"
    assert os.path.exists(READELF), "llvm-readelf of the ROCm installation is missing"
    return {n: k for n, k in _kernels().items() if "le_resolve_" in n}


def test_the_kernels_are_the_documented_ones(kernels):
    assert sorted(kernels) == sorted(NAMES)                 # (extern "C": the symbols are the plain names)
    for n in kernels:                                      # the other families' resource tests count kernels by these substrings
        assert n.startswith("le_resolve_")
        assert not any(s in n for s in OTHER_FAMILIES), n


def test_no_scratch_no_spills(kernels):
    for n, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert k["max_flat_workgroup_size"] == 256, (n, k)


def test_registers_and_lds_within_their_budgets(kernels):
    for n, k in kernels.items():
        assert k["vgpr_count"] <= (160 if n in HOLD_A_SCHEDULE else 64), (n, k["vgpr_count"])
        assert k["group_segment_fixed_size"] == (1024 if n in ROUND_TABLE_IN_LDS else (16 if n in WAVE_SUMS_IN_LDS else 0)), n


def test_design_lists_the_figures_of_the_built_library(kernels):
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("#### 3.8.10"):text.index("### 3.9 ")]
    assert text.index("#### 3.8.9") < text.index("#### 3.8.10") < text.index("### 3.9 ")
    for n, k in kernels.items():
        assert re.search(r"`%s`\s*\|\s*%d\s*\|\s*%d\s*\|" % (n, k["vgpr_count"], k["group_segment_fixed_size"]), section), \
            (n, k["vgpr_count"], k["group_segment_fixed_size"])
    rows = re.findall(r"^\| `(\w+)` \|", section, re.M)
    assert sorted(rows) == sorted(NAMES)                    # this stage's kernels only: the sections in front count their rows to here
