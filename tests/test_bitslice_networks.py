"""The bit-sliced count <= limit networks of the pattern scans (libbtbb_amd/csrc/bitslice.h: top12_filter, top16_filter,
le_filter16), as they ship, against the plain count over every value of their planes -- on the CPU: the header compiles for
the host, tests/c/bitslice_check.cpp runs it.  (tests/test_known_lap_filter_model.py holds numpy transcriptions of two of
the networks against the count; this runs the code the kernels are built from, all limits, both classes, the LE network.)"""
import os
import subprocess

from _libs import ROOT


def test_every_network_equals_the_count_over_all_inputs(tmp_path):
    exe = str(tmp_path / "bitslice_check")
    src = os.path.join(ROOT, "tests", "c", "bitslice_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", src, "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failing cases"), r.stdout + r.stderr
