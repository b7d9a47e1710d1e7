"""The ABI of the clock acquisition (include/btbbx.h btbbx_survey_clock_jobs_device / btbbx_acquire_host): the two names
are exported and nothing else is new, and the argument checks of the device entry, which come before any device work and
so hold on a machine without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -3
NEW = {"btbbx_survey_clock_jobs_device", "btbbx_acquire_host"}


@pytest.fixture(scope="module")
def lib():
    import libbtbb_amd
    if not os.path.exists(libbtbb_amd.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "libbtbb_amd", "csrc")], check=True)
    return libbtbb_amd.lib()


def test_the_two_names_are_exported_and_nothing_else_is_new(lib):
    import libbtbb_amd
    text = open(os.path.join(ROOT, "libbtbb_amd", "csrc", "exports.map")).read()
    assert "btbbx_*;" in text and "local:" in text and "*;" in text.split("local:")[1]
    out = subprocess.run(["nm", "-D", "--defined-only", libbtbb_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert NEW <= names
    # every exported name of this family is one of the two: no kernel handle, launcher or helper came with them
    assert {n for n in names if "acquire_" in n or "clock_jobs" in n} == NEW
    header = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header) and n in libbtbb_amd.SIGNATURES, n
    assert "#define BTBBX_JOBS_AFH     1u" in header and "#define BTBBX_JOBS_ALIASED 2u" in header
    assert (libbtbb_amd.JOBS_AFH, libbtbb_amd.JOBS_ALIASED) == (1, 2)


def test_header_says_what_the_contract_needs():
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    assert "(cand0 << 1) - (first_pkt_time << 1)" in text           # the reference's CLKN offset from a result
    assert "READ, never written" in text                             # the survey's scratch


def test_device_entry_rejects_before_any_launch(lib):
    """Every listed argument error: BTBBX_E_ARG, whether or not a device is present (the device pointers below are never
    dereferenced)."""
    f = lib.btbbx_survey_clock_jobs_device
    cap = 100
    need = lib.btbbx_survey_scratch_bytes(cap)
    p = 0x10000                                              # aligned, never touched
    table = np.arange(8, dtype=np.uint8)

    def call(recs=p, rec_count=p, rec_cap=10, scratch=p, scratch_bytes=need, cap=cap, channels=None, n_streams=8, flags=3, max_obs=1024,
             jobs=p, job_cap=10, n_jobs=p, job_rec=p, off=p, ch=p, obs_hits=p, obs_cap=cap, n_obs=p):
        chp = None if channels is None else channels.ctypes.data_as(C.c_void_p)
        return f(recs, rec_count, rec_cap, scratch, scratch_bytes, cap, chp, n_streams, flags, max_obs, jobs, job_cap, n_jobs, job_rec,
                 off, ch, obs_hits, obs_cap, n_obs, None)
    for name in ("recs", "jobs", "n_jobs", "scratch", "off", "ch"):
        assert call(**{name: None}) == E_ARG, name
        assert b"btbbx_survey_clock_jobs_device" in lib.btbbx_last_error()
    assert call(scratch_bytes=need - 1) == E_ARG
    assert call(obs_cap=cap - 1) == E_ARG
    assert call(max_obs=0) == E_ARG and call(max_obs=1025) == E_ARG
    assert call(job_cap=0) == E_ARG
    assert call(flags=4) == E_ARG and call(flags=0x80000001) == E_ARG
    bad = table.copy()
    bad[5] = 79
    assert call(channels=bad) == E_ARG
    assert call(n_streams=0) == E_ARG and call(n_streams=80) == E_ARG
    for name in ("recs", "rec_count", "jobs", "n_jobs", "job_rec", "off", "obs_hits", "n_obs"):
        assert call(**{name: p + 2}) == E_ARG, name
    assert call(scratch=p + 8) == E_ARG


def test_host_entry_rejects_bad_arguments(lib):
    """NULL words, a channel above 78, max_obs out of range, unknown flags, no place for the job count: before any device work"""
    f = lib.btbbx_acquire_host
    words = np.zeros(64, np.uint64)
    recs = np.zeros(64 * 4, np.uint8)
    out = np.zeros(256, np.uint32)
    n_jobs = C.c_uint64(0)
    wp, rp, op = (a.ctypes.data_as(C.c_void_p) for a in (words, recs, out))

    def call(words=wp, channels=None, clk_div=625, flags=0, max_obs=1024, n_jobs=C.byref(n_jobs), job_rec=op, results=op):
        return f(words, 64, 64, 1, 1000, 2, channels, 0, clk_div, 0, rp, 4, None, flags, max_obs, None, job_rec, results, 4, n_jobs, None, 0)
    assert call(words=None) == E_ARG
    assert call(channels=np.array([79], np.uint8).ctypes.data_as(C.c_void_p)) == E_ARG
    assert call(clk_div=0) == E_ARG
    assert call(max_obs=0) == E_ARG and call(max_obs=1025) == E_ARG and call(flags=4) == E_ARG
    assert call(n_jobs=None) == E_ARG and call(job_rec=None) == E_ARG and call(results=None) == E_ARG
    assert b"btbbx_acquire_host" in lib.btbbx_last_error()
