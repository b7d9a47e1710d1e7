"""Registers, LDS and scratch of the follow stage's kernels (follow.h), read from the built library as
tests/test_acquire_kernel_resources.py does: DESIGN 3.10 states these figures."""
import os
import re

import pytest

from test_kernel_resources import _kernels, _waves_per_simd, SO, READELF

# kernel -> (VGPRs of the build DESIGN describes: a ceiling, LDS bytes: exact, workgroup size)
PINNED = {"follow_stage_kernel": (8, 0, 256),
          "follow_clock_kernel": (35, 0, 256),
          "follow_tally_kernel": (11, 0, 256)}


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "the library has not been built"
    assert os.path.exists(READELF), "llvm-readelf of the ROCm installation is missing"
    return _kernels()


def test_the_three_follow_kernels_exist(kernels):
    names = [n for n in kernels if "follow_" in n]
    assert len(names) == 3 and all(any(p in n for n in names) for p in PINNED), names


@pytest.mark.parametrize("pattern", sorted(PINNED))
def test_follow_kernel_no_scratch_no_spills_pinned_registers_and_lds(kernels, pattern):
    m = [n for n in kernels if re.search(pattern, n)]
    assert len(m) == 1, m
    k = kernels[m[0]]
    vgprs, lds, threads = PINNED[pattern]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["vgpr_count"] <= vgprs and _waves_per_simd(k["vgpr_count"]) == 8, k
    assert k["group_segment_fixed_size"] == lds and k["max_flat_workgroup_size"] == threads, k
