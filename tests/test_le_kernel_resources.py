"""Registers, LDS and scratch of the LE kernels, read from the built library (as tests/test_survey_kernel_resources.py does for
the survey kernels): DESIGN 3.8 claims eight waves per SIMD for the access-address scan and nothing in scratch."""
import os
import re

import pytest

from test_kernel_resources import _kernels, _waves_per_simd, SO, READELF

LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "the library has not been built"
    assert os.path.exists(READELF), "llvm-readelf of the ROCm installation is missing"
    return _kernels()


def test_le_scan_kernels_eight_waves_per_simd_no_spill_no_scratch(kernels):
    names = [n for n in kernels if re.search(r"le_scan_kernel", n)]
    assert len(names) == 10, names                           # advertising AA / any AA x limits 0 .. 4
    for n in names:
        k = kernels[n]
        assert k["vgpr_count"] <= 64 and _waves_per_simd(k["vgpr_count"]) == 8, (n, k)
        assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, (n, k)
        assert k["max_flat_workgroup_size"] == 256 and 8 * k["group_segment_fixed_size"] <= LDS_PER_CU, (n, k)


def test_le_decode_kernel_has_no_scratch(kernels):
    names = [n for n in kernels if "le_decode_kernel" in n]
    assert len(names) == 1, names
    k = kernels[names[0]]
    assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
