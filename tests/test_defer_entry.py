"""The sixteen-byte list entry of decode_hits_kernel's deferred payloads (libbtbb_amd/csrc/defer_entry.h: what defer_payload
packs and the lane-group phases take apart), as it ships, on the CPU: the header compiles for the host,
tests/c/defer_entry_check.cpp packs entries over the extremes and a seeded sample of every field and checks each accessor
against the layout written out as literal shifts, and the round trip."""
import os
import subprocess

from _libs import ROOT


def test_every_field_sits_where_the_layout_says_and_round_trips(tmp_path):
    exe = str(tmp_path / "defer_entry_check")
    src = os.path.join(ROOT, "tests", "c", "defer_entry_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", src, "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("0 failing cases"), r.stdout + r.stderr
