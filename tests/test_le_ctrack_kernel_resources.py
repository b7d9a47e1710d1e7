"""Registers, LDS and scratch of the two kernels of the LE Coded connection tracking (le_ctrack.h), read from the built library as
tests/test_le_cfind_kernel_resources.py does: no scratch, no spilled register; the figures DESIGN 3.8.13 states are upper bounds.
The duration kernel holds, per lane, six stream words and the five shifted ones (22 dwords at most at once), eight metrics and
their eight successors, and no LDS; the stand-in flag pass is le_track_flag_kernel with one more load, and its LDS is the tile's
one counter."""
import os
import re

import pytest

from test_kernel_resources import _kernels, SO, READELF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel -> (VGPRs at most, bytes of LDS at most, lanes per workgroup): 22 + 16 dwords and addresses; the flag pass of le_track.h
BOUNDS = {"le_ctrack_symbols_kernel": (48, 0, 256), "le_ctrack_flag_kernel": (24, 4, 256)}


@pytest.fixture(scope="module")
def kernels():
    assert os.path.exists(SO), "the library has not been built"
    assert os.path.exists(READELF), "llvm-readelf of the ROCm installation is missing"
    return {n: k for n, k in _kernels().items() if "le_ctrack_" in n}


def _name(symbol):
    return next(n for n in BOUNDS if n in symbol)


def test_the_kernels_are_the_documented_ones(kernels):
    assert len(kernels) == 2 and sorted(_name(n) for n in kernels) == sorted(BOUNDS), sorted(kernels)
    for n in kernels:                                      # the other families' resource tests find their kernels by these substrings
        assert not any(s in n for s in ("le_track_", "le_coded_", "le_cfind_", "le_disc_", "le_csa2_", "le_scan_kernel", "le_decode_kernel",
                                        "le_resolve_", "follow_", "hop_", "survey_", "acquire_")), n


def test_no_scratch_no_spills(kernels):
    for n, k in kernels.items():
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, (n, k)


def test_registers_and_lds_within_their_bounds(kernels):
    for n, k in kernels.items():
        vgprs, lds, lanes = BOUNDS[_name(n)]
        assert k["vgpr_count"] <= vgprs and k["group_segment_fixed_size"] <= lds and k["max_flat_workgroup_size"] == lanes, (n, k)


def test_design_lists_the_figures_of_the_built_library(kernels):
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert text.index("#### 3.8.12") < text.index("#### 3.8.13") < text.index("### 3.9 ")
    section = text[text.index("#### 3.8.13"):text.index("### 3.9 ")]
    for n, k in kernels.items():
        assert re.search(r"\| `%s` \|\s*%d\s*\|\s*%d\s*\|" % (_name(n), k["vgpr_count"], k["group_segment_fixed_size"]), section), \
            (n, k["vgpr_count"], k["group_segment_fixed_size"])
