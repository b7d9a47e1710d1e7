"""Registers, LDS and scratch of the LE discovery kernels (le_discover.h), read from the built library as
tests/test_le_kernel_resources.py does for the LE scan: DESIGN 3.8.1 states eight waves per SIMD, 9472 bytes of LDS for
le_disc_scan_kernel and nothing in scratch for any of them."""
import os

import pytest

from test_kernel_resources import _kernels, _waves_per_simd, SO, READELF

LDS_PER_CU = 160 * 1024
GROUPING = ("le_disc_key_kernel", "le_disc_rekey_kernel", "le_disc_mark_kernel", "le_disc_prefix_kernel", "le_disc_starts_kernel",
            "le_disc_qmark_kernel", "le_disc_emit_kernel", "le_disc_rewrite_kernel", "le_disc_copy_kernel")


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "the library has not been built"
    assert os.path.exists(READELF), "llvm-readelf of the ROCm installation is missing"
    return _kernels()


def test_discovery_scan_kernel_eight_waves_per_simd_no_spill_no_scratch(kernels):
    names = [n for n in kernels if "le_disc_scan_kernel" in n]
    assert len(names) == 1, names
    k = kernels[names[0]]
    assert k["vgpr_count"] <= 64 and _waves_per_simd(k["vgpr_count"]) == 8, k
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
    # the ring (4 waves x 128 x 16 bytes), the inverse CRC table (1 KiB) and the two whitening tables (2 x 128 bytes)
    assert k["max_flat_workgroup_size"] == 256 and k["group_segment_fixed_size"] == 4 * 128 * 16 + 1024 + 256, k
    assert 8 * k["group_segment_fixed_size"] <= LDS_PER_CU


def test_grouping_kernels_have_no_scratch(kernels):
    names = [n for n in kernels if "le_disc_" in n and "le_disc_scan_kernel" not in n]
    assert len(names) == len(GROUPING) and all(any(p in n for n in names) for p in GROUPING), names
    for n in names:
        k = kernels[n]
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)
        assert k["vgpr_count"] <= 32 and k["group_segment_fixed_size"] <= 16 and k["max_flat_workgroup_size"] == 256, (n, k)
