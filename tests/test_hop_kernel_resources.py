"""Registers, LDS and scratch of the single-piconet reversal's kernels that call the shared pieces of csrc/hop_core.h (table
build, agreement walk, block scan, verdict, ordered emit), read from the built library in the form of
tests/test_hop_batch_kernel_resources.py.  The figures are those of the build before the pieces were shared
(profiles/r10_hop): sharing a piece must not cost a kernel registers, LDS or scratch."""
import os
import re

import pytest

from test_kernel_resources import _kernels, _waves_per_simd, SO, READELF

# kernel -> (VGPRs of the build with one copy of each piece per kernel: a ceiling, LDS bytes: exact, workgroup size)
PINNED = {"hop_candidate_mask_kernel": (19, 272, 256),         # the table
          "hop_mask_prefix_kernel": (12, 4096, 1024),          # 1024 partial sums
          "hop_winnow_kernel": (27, 4384, 256),                # 272 table + 1025 histogram bins (+ pad)
          "hop_verdict_kernel": (5, 4100, 1024),               # 4096 prefix + first
          "hop_winnow_small_kernel": (28, 37208, 1024)}        # 272 table + 32768 agree + 4096 prefix + 16 wave counts + first + base


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "the library has not been built"
    assert os.path.exists(READELF), "llvm-readelf of the ROCm installation is missing"
    return _kernels()


@pytest.mark.parametrize("pattern", sorted(PINNED))
def test_reversal_kernel_no_scratch_no_spills_pinned_registers_and_lds(kernels, pattern):
    m = [n for n in kernels if re.search(r"\d" + pattern, n)]          # the mangled name: its length comes before it
    assert len(m) == 1, m
    k = kernels[m[0]]
    vgprs, lds, threads = PINNED[pattern]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["vgpr_count"] <= vgprs and _waves_per_simd(k["vgpr_count"]) == 8, k
    assert k["group_segment_fixed_size"] == lds and k["max_flat_workgroup_size"] == threads, k
