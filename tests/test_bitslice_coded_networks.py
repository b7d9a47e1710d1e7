"""The wide bit-sliced counters behind the LE Coded PHY scan's pre-filter (libbtbb_amd/csrc/bitslice.h: bs_add, bs_shift_add,
bs_le, le_coded_filter), as they ship, on the CPU as tests/test_bitslice_networks.py does for the small networks: the adders over
every pair of values, the compare over every count and limit, and the composed filter against the plain count of equal symbol
pairs (tests/c/bitslice_coded_check.cpp)."""
import os
import subprocess

from _libs import ROOT


def test_adders_compare_and_filter_equal_the_count(tmp_path):
    exe = str(tmp_path / "bitslice_coded_check")
    src = os.path.join(ROOT, "tests", "c", "bitslice_coded_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", src, "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failing cases"), r.stdout + r.stderr
