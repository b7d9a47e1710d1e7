"""Registers and scratch of the survey kernels, read from the built library (as tests/test_kernel_resources.py does for the
older kernels): DESIGN 3.9 claims eight waves per SIMD and nothing in scratch for the walk."""
import os
import re

import pytest

from test_kernel_resources import _kernels, _waves_per_simd, SO, READELF


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "the library has not been built"
    assert os.path.exists(READELF), "llvm-readelf of the ROCm installation is missing"
    return _kernels()


def test_walk_kernel_eight_waves_per_simd_no_scratch(kernels):
    m = [n for n in kernels if re.search(r"survey_walk_kernel", n)]
    assert len(m) == 1, m
    k = kernels[m[0]]
    assert k["vgpr_count"] <= 64 and _waves_per_simd(k["vgpr_count"]) == 8, k
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 0 and k["max_flat_workgroup_size"] == 256, k


def test_survey_kernels_have_no_scratch(kernels):
    names = [n for n in kernels if "survey_" in n or "header_flags_kernel" in n]
    assert len(names) == 12, names
    for n in names:
        k = kernels[n]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (n, k)
        assert _waves_per_simd(k["vgpr_count"]) == 8, (n, k)
