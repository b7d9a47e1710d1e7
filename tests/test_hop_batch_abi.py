"""The batch CLK1-27 reversal's ABI (include/btbbx.h btbbx_clock_job / btbbx_clock_result / btbbx_hop_reversal_batch_*):
layouts through the ctypes classes and the numpy dtypes, the host-only scratch formula, and the argument checks of the
device entry, which come before any device work and so hold on a machine without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG = -3


@pytest.fixture(scope="module")
def lib():
    import libbtbb_amd
    if not os.path.exists(libbtbb_amd.LIB_PATH):
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "libbtbb_amd", "csrc")], check=True)
    return libbtbb_amd.lib()


def test_struct_sizes():
    import libbtbb_amd as bt
    assert C.sizeof(bt.ClockJob) == bt.CLOCK_JOB_DTYPE.itemsize == 104
    assert C.sizeof(bt.ClockResult) == bt.CLOCK_RESULT_DTYPE.itemsize == 24
    assert C.sizeof(bt.HopCfg) == bt.HOP_CFG_DTYPE.itemsize == 88


def test_field_offsets():
    import libbtbb_amd as bt
    want = {"cfg": 0, "clk6": 88, "aliased": 92, "obs_first": 96, "n_obs": 100}
    for name, off in want.items():
        assert getattr(bt.ClockJob, name).offset == off, name
        assert bt.CLOCK_JOB_DTYPE.fields[name][1] == off, name
    for i, name in enumerate(("status", "n_initial", "stop", "count", "cand0", "n_stored")):
        assert getattr(bt.ClockResult, name).offset == 4 * i and bt.CLOCK_RESULT_DTYPE.fields[name][1] == 4 * i, name
    for name in ("address", "afh", "used_channels", "bank"):
        assert getattr(bt.HopCfg, name).offset == bt.HOP_CFG_DTYPE.fields[name][1], name


def test_header_states_the_sizes():
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    assert "typedef struct btbbx_clock_job {        /* 104 bytes */" in text
    assert "typedef struct btbbx_clock_result {     /* 24 bytes */" in text


def test_job_table_builder():
    """clock_jobs lays the observations out one job after the other and copies a configuration byte for byte (host only:
    the configuration is filled by hand, btbbx_hop_cfg_init is not needed)."""
    import libbtbb_amd as bt
    a, b = bt.HopCfg(), bt.HopCfg()
    a.address, a.afh, a.used_channels = 0x1234567, 0, 79
    b.address, b.afh, b.used_channels = 0x7654321, 1, 3
    for i in range(80):
        a.bank[i], b.bank[i] = i, 79 - i
    jobs, off, ch = bt.clock_jobs([a, b], [5, 63], [([0, 7, 9], [1, 2, 3]), ([0], [200])], aliased=[False, True])
    assert jobs.dtype == bt.CLOCK_JOB_DTYPE and jobs.tobytes()[:88] == bytes(a) and jobs.tobytes()[104:192] == bytes(b)
    assert jobs["clk6"].tolist() == [5, 63] and jobs["aliased"].tolist() == [0, 1]
    assert jobs["obs_first"].tolist() == [0, 3] and jobs["n_obs"].tolist() == [3, 1]
    assert off.dtype == np.int32 and off.tolist() == [0, 7, 9, 0] and ch.dtype == np.uint8 and ch.tolist() == [1, 2, 3, 200]


def test_scratch_bytes_is_host_only_positive_and_monotone(lib):
    f = lib.btbbx_hop_reversal_batch_scratch_bytes
    assert f(1, 0) > 0 and f(1, 64) > 0
    sizes = [1, 2, 3, 48, 1024, 4096]
    for cand_cap in (0, 1, 64, 1 << 21):
        got = [f(n, cand_cap) for n in sizes]
        assert all(x > 0 for x in got) and got == sorted(got) and got[-1] > got[0], (cand_cap, got)
    for n in sizes:
        got = [f(n, c) for c in (0, 1, 64, 4096, 1 << 21)]
        assert got == sorted(got), (n, got)
    # the formula the header states, and the condition on the design: no room for a job's candidates (2^21 clocks = 8 MiB)
    assert f(3, 64) == (3 * (2 * 1028 + 1) * 4 + 255) // 256 * 256
    assert f(3, 64) < 8 << 20 and f(3, 1 << 21) < 8 << 20


def test_device_entry_rejects_before_any_launch(lib):
    """NULL jobs, job_cap = 0, a scratch one byte too small, NULL results / scratch, missing observation arrays and misaligned
    pointers: BTBBX_E_ARG, whether or not a device is present (the pointers below are never dereferenced)."""
    f = lib.btbbx_hop_reversal_batch_device
    need = lib.btbbx_hop_reversal_batch_scratch_bytes(4, 8)
    p = 0x10000                                              # aligned, never touched

    def call(jobs=p, n_jobs=None, job_cap=4, off=p, ch=p, n_obs_total=16, results=p, cand=p, cand_cap=8, scratch=p, scratch_bytes=need):
        return f(jobs, n_jobs, job_cap, off, ch, n_obs_total, results, cand, cand_cap, scratch, scratch_bytes, None)
    assert call(jobs=None) == E_ARG
    assert b"btbbx_hop_reversal_batch_device" in lib.btbbx_last_error()
    assert call(job_cap=0) == E_ARG
    assert call(scratch_bytes=need - 1) == E_ARG
    assert call(results=None) == E_ARG
    assert call(scratch=None) == E_ARG
    assert call(off=None) == E_ARG and call(ch=None) == E_ARG
    for name in ("jobs", "n_jobs", "off", "results", "cand"):
        assert call(**{name: p + 2}) == E_ARG, name
    assert call(scratch=p + 8) == E_ARG


def test_host_entry_rejects_null(lib):
    res = np.zeros(1, np.uint32)
    assert lib.btbbx_hop_reversal_batch_host(None, 1, None, None, 0, res.ctypes.data_as(C.c_void_p), None, 0) == E_ARG
