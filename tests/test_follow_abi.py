"""The ABI of the follow stage (include/btbbx.h btbbx_follow_hits_device / btbbx_follow_host): the two names are exported and
nothing else is new, the struct sizes, and the argument checks of both entries, which come before any device work and so hold
on a machine without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -3
NEW = {"btbbx_follow_hits_device", "btbbx_follow_host"}


@pytest.fixture(scope="module")
def lib():
    import libbtbb_amd
    if not os.path.exists(libbtbb_amd.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "libbtbb_amd", "csrc")], check=True)
    return libbtbb_amd.lib()


def test_the_two_names_are_exported_and_nothing_else_is_new(lib):
    import libbtbb_amd
    out = subprocess.run(["nm", "-D", "--defined-only", libbtbb_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NEW <= names
    # every exported name of this family is one of the two: no kernel handle, launcher or helper came with them
    assert {n for n in names if "follow" in n} == NEW
    header = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header) and n in libbtbb_amd.SIGNATURES, n


def test_struct_sizes_and_layout():
    import libbtbb_amd as bt
    assert bt.FOLLOW_PKT_DTYPE.itemsize == 16 and bt.FOLLOW_SUM_DTYPE.itemsize == 32
    assert [bt.FOLLOW_PKT_DTYPE.fields[n][1] for n in ("piconet", "clkn", "stage", "channel", "hop_channel", "on_hop", "job")] == \
           [0, 4, 8, 9, 10, 11, 12]
    assert list(bt.FOLLOW_SUM_DTYPE.names) == ["stage", "job", "n_hits", "n_header", "n_payload", "n_on_hop", "n_off_hop", "lt_addr_mask"]
    header = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    assert "} btbbx_follow_pkt;" in header and "} btbbx_follow_sum;" in header


def test_header_says_what_the_contract_needs():
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    assert "(cand0 + c - recs[g].first_pkt_time) & 0x7ffffff" in text
    assert "(recs[g].clk_offset + c) & 0x3f" in text
    assert "((ch + 24) % 25) + 26" in text
    assert "d_in is the only" in text and "Every d_sums[g], g < R, is written whole" in text


def test_device_entry_rejects_before_any_launch(lib):
    """Every listed argument error: BTBBX_E_ARG, whether or not a device is present (the device pointers below are never
    dereferenced)."""
    f = lib.btbbx_follow_hits_device
    p = 0x10000                                              # aligned, never touched
    table = np.arange(8, dtype=np.uint8)
    entry = np.zeros(16, np.uint8)
    ep = entry.ctypes.data_as(C.c_void_p)

    def call(words=p, n_streams=8, hits=p, count=p, cap=100, recs=p, rec_count=p, rec_cap=10, jobs=p, job_rec=p, results=p, n_jobs=p,
             job_cap=10, channels=None, entry=ep, clk_div=625, clk_phase=0, d_in=p, follow=p, out=p, lengths=p, sums=p):
        chp = None if channels is None else channels.ctypes.data_as(C.c_void_p)
        return f(words, 1024, 1024, n_streams, hits, count, cap, recs, rec_count, rec_cap, jobs, job_rec, results, n_jobs, job_cap, chp,
                 entry, clk_div, clk_phase, 3125, d_in, follow, out, lengths, sums, None)
    for name in ("words", "hits", "recs", "d_in", "follow", "out", "sums", "entry"):
        assert call(**{name: None}) == E_ARG, name
        assert b"btbbx_follow_hits_device" in lib.btbbx_last_error(), name
    for name in ("jobs", "job_rec", "results"):
        assert call(**{name: None}) == E_ARG, name
        assert b"btbbx_follow_hits_device" in lib.btbbx_last_error(), name
    assert call(clk_div=0) == E_ARG and call(clk_phase=625) == E_ARG and call(clk_phase=700) == E_ARG
    assert b"btbbx_follow_hits_device" in lib.btbbx_last_error()
    assert call(cap=0) == E_ARG and call(rec_cap=0) == E_ARG
    bad = table.copy()
    bad[5] = 79
    assert call(channels=bad) == E_ARG
    assert call(n_streams=80) == E_ARG
    assert call(n_streams=257, channels=np.zeros(257, np.uint8)) == E_ARG
    for name in ("words", "hits", "count", "recs", "rec_count", "jobs", "job_rec", "results", "n_jobs", "d_in", "follow", "out", "lengths",
                 "sums"):
        assert call(**{name: p + 2}) == E_ARG, name
    assert call(out=p + 4) == E_ARG                            # 8 bytes for d_out
    assert b"btbbx_follow_hits_device" in lib.btbbx_last_error()
    # what is NOT an argument error gets as far as the device: a machine without one says so, and not in this function's name
    import torch
    if not torch.cuda.is_available():
        for kw in (dict(), dict(job_cap=0, jobs=None, job_rec=None, results=None, n_jobs=None), dict(count=None, rec_count=None, n_jobs=None),
                   dict(lengths=None), dict(channels=table)):
            rc = call(**kw)
            assert rc < 0 and b"btbbx_follow_hits_device" not in lib.btbbx_last_error(), kw


def test_host_entry_rejects_bad_arguments(lib):
    f = lib.btbbx_follow_host
    words = np.zeros(64, np.uint64)
    recs = np.zeros(64 * 4, np.uint8)
    out = np.zeros(4096, np.uint32)
    n_jobs, n_hits = C.c_uint64(0), C.c_uint64(0)
    wp, rp, op = (a.ctypes.data_as(C.c_void_p) for a in (words, recs, out))

    def call(words=wp, channels=None, clk_div=625, flags=0, max_obs=1024, recs=rp, rec_cap=4, n_jobs=C.byref(n_jobs), hits=op, follow=op,
             hit_cap=4, n_hits=C.byref(n_hits), sums=op):
        return f(words, 64, 64, 1, 1000, 2, channels, 0, clk_div, 0, recs, rec_cap, flags, max_obs, None, None, 4, n_jobs, hits, follow,
                 None, hit_cap, n_hits, sums)
    assert call(words=None) == E_ARG
    assert call(channels=np.array([79], np.uint8).ctypes.data_as(C.c_void_p)) == E_ARG
    assert call(clk_div=0) == E_ARG
    assert call(max_obs=0) == E_ARG and call(max_obs=1025) == E_ARG and call(flags=4) == E_ARG
    assert b"btbbx_follow_host" in lib.btbbx_last_error()
    for name in ("recs", "n_jobs", "hits", "follow", "n_hits", "sums"):
        assert call(**{name: None}) == E_ARG, name
        assert b"btbbx_follow_host" in lib.btbbx_last_error()
    assert call(rec_cap=0) == E_ARG
