"""Registers, LDS and scratch of the kernels of LE decryption (le_crypt.h), read from the built library as
tests/test_le_data_kernel_resources.py does for the data stage: DESIGN 3.8.7 names nineteen kernels (the other five of the
stage's 24 launches are the data stage's kernels, tests/test_le_data_kernel_resources.py), none of them with scratch or a spilled
register, and states their VGPR and LDS figures.  The trial kernels keep a key schedule of 44 words in registers and
may use up to 160 VGPRs (three waves per SIMD); every other kernel stays within 64 (eight)."""
import os
import re

import pytest

from test_kernel_resources import _kernels, SO, READELF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> (VGPRs, bytes of LDS), as DESIGN 3.8.7 lists them
DOCUMENTED = {
    "le_crypt_init_kernel": (44, 0),
    "le_crypt_find_kernel": (20, 0),
    "le_crypt_rsp_kernel": (6, 0),
    "le_crypt_begin_kernel": (6, 0),
    "le_crypt_sched_kernel": (71, 2048),
    "le_crypt_ord_sum_kernel": (24, 48),
    "le_crypt_ord_prefix_kernel": (23, 48),
    "le_crypt_ord_kernel": (30, 48),
    "le_crypt_probe_kernel": (147, 2048),
    "le_crypt_key_kernel": (8, 0),
    "le_crypt_first_kernel": (109, 2048),
    "le_crypt_retry_kernel": (121, 2048),
    "le_crypt_effect_kernel": (59, 2048),
    "le_crypt_number_sum_kernel": (22, 48),
    "le_crypt_number_prefix_kernel": (27, 48),
    "le_crypt_number_kernel": (42, 48),
    "le_crypt_pkt_kernel": (18, 0),
    "le_crypt_conn_kernel": (22, 0),
    "le_crypt_plain_kernel": (59, 2048),
}
SCHEDULE_IN_REGISTERS = ("le_crypt_sched_kernel", "le_crypt_probe_kernel", "le_crypt_first_kernel", "le_crypt_retry_kernel")


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "the library has not been built"
    assert os.path.exists(READELF), "llvm-readelf of the ROCm installation is missing"
    return {n: k for n, k in _kernels().items() if "le_crypt_" in n}


def test_the_kernels_are_the_documented_ones(kernels):
    assert sorted(kernels) == sorted(DOCUMENTED)           # (extern "C": the symbols are the plain names)
    for n in kernels:                                      # the other families' resource tests count kernels by these substrings
        assert n.startswith("le_crypt_")
        assert not any(s in n for s in ("le_data_", "le_seed_", "le_epoch_", "le_span_", "le_track_", "le_disc_", "le_csa2_", "follow_", "hop_",
                                        "survey_", "acquire_", "order_", "le_decode_kernel", "header_flags_kernel", "decode_kernel",
                                        "replay_kernel")), n


def test_no_scratch_no_spills(kernels):
    for n, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert k["max_flat_workgroup_size"] == 256, (n, k)


def test_registers_and_lds_as_documented(kernels):
    for name, (vgprs, lds) in DOCUMENTED.items():
        k = kernels[name]
        assert (k["vgpr_count"], k["group_segment_fixed_size"]) == (vgprs, lds), (name, k["vgpr_count"], k["group_segment_fixed_size"])
        assert k["vgpr_count"] <= (160 if name in SCHEDULE_IN_REGISTERS else 64), name
        assert lds <= 2048


def test_design_lists_the_same_figures():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = text[text.index("#### 3.8.7"):]
    for name, (vgprs, lds) in DOCUMENTED.items():
        assert re.search(r"`%s`\s*\|\s*%d\s*\|\s*%d\s*\|" % (name, vgprs, lds), section), name
