"""Registers, LDS and scratch of the batch reversal's kernels, read from the built library (as tests/test_kernel_resources.py
does for the older kernels): DESIGN 3.6 states these figures -- nothing in scratch, eight waves per SIMD by registers, and
the LDS of the job's table, its staged observations and the two histogram rows."""
import os
import re

import pytest

from test_kernel_resources import _kernels, _waves_per_simd, SO, READELF, LDS_PER_CU

# kernel -> (VGPRs of the build DESIGN 3.6 describes: a ceiling, LDS bytes: exact, workgroup size)
PINNED = {"hop_batch_agree_kernel": (46, 16688, 256),          # 272 table + 8192 observations + 2 x 4100 histogram rows + pad
          "hop_batch_verdict_kernel": (12, 4104, 1024),        # 4096 prefix + first + best
          "hop_batch_emit_kernel": (33, 8532, 1024)}           # 272 table + 8192 observations + 16 wave counts + base


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "the library has not been built"
    assert os.path.exists(READELF), "llvm-readelf of the ROCm installation is missing"
    return _kernels()


def test_the_three_batch_kernels_exist(kernels):
    names = [n for n in kernels if "hop_batch_" in n]
    assert len(names) == 3 and all(any(p in n for n in names) for p in PINNED), names


@pytest.mark.parametrize("pattern", sorted(PINNED))
def test_batch_kernel_no_scratch_no_spills_pinned_registers_and_lds(kernels, pattern):
    m = [n for n in kernels if re.search(pattern, n)]
    assert len(m) == 1, m
    k = kernels[m[0]]
    vgprs, lds, threads = PINNED[pattern]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["vgpr_count"] <= vgprs and _waves_per_simd(k["vgpr_count"]) == 8, k
    assert k["group_segment_fixed_size"] == lds and k["max_flat_workgroup_size"] == threads, k


def test_agree_kernel_eight_workgroups_per_cu_by_lds(kernels):
    """256 lanes = one wave per SIMD: eight workgroups fill the CU's 32 wave slots, and their LDS fits beside each other."""
    k = kernels[[n for n in kernels if "hop_batch_agree_kernel" in n][0]]
    assert 8 * k["group_segment_fixed_size"] <= LDS_PER_CU, k
