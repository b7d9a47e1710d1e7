"""The hop kernels on the lattice of tests/_hop_lattice.py: btbbx_hop_channels_device and btbbx_hop_sequence_device on every
configuration's clocks and slices (with a guard behind every slice), the single-piconet reversal call by call and the batch
reversal on the frozen scenarios, and the follow's hop check -- all against the numpy model, none against another kernel.
tests/test_hop_lattice_model.py keeps the model and the tables honest.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

import _hop_lattice as hl
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu
FILL = 0xA5A5A5A5


@pytest.fixture(scope="module", autouse=True)
def ready():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    bt.init(2)
    yield


def _cfg(c):
    lap, uap = hl.lap_uap(c)
    cfg = bt.hop_cfg(lap, uap, None if c.afh_map is None else np.array(c.afh_map, np.uint8))
    bank, used = hl.bank_of(c.afh_map)
    assert cfg.address == c.address and cfg.used_channels == used and list(cfg.bank)[:len(bank)] == bank.tolist(), c.tag
    return cfg


def test_channels_of_clock_sets():
    for i, c in enumerate(hl.configs()):
        clocks = hl.clock_set(i)
        got = bt.hop_channels(_cfg(c), clocks)
        want = hl.model_hops(c.address, c.afh_map, clocks)
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (c.tag, len(bad), hex(int(clocks[bad[0]])), int(got[bad[0]]), int(want[bad[0]]))


def test_sequence_slices_and_the_bytes_behind_them():
    lib = bt.lib()
    room = 64 * max(hl.SLICE_GROUPS) + hl.GUARD_BYTES
    buf = bt.DeviceBuffer(room)
    try:
        for i, c in enumerate(hl.configs()):
            cfg = _cfg(c)
            for kind, first, count in hl.slices(i):
                bt.check(lib.btbbx_memset(buf.ptr, hl.GUARD, room), "memset")
                bt.check(lib.btbbx_hop_sequence_device(C.byref(cfg), first, count, buf.ptr, None), "btbbx_hop_sequence_device")
                bt.check(lib.btbbx_sync(None), "sync")
                got = buf.download(np.uint8, room)
                want = hl.model_hops(c.address, c.afh_map, first + np.arange(count, dtype=np.int64))
                bad = np.nonzero(got[:count] != want)[0]
                assert len(bad) == 0, (c.tag, kind, first, count, len(bad), int(bad[0]))
                assert (got[count:] == hl.GUARD).all(), (c.tag, kind, first, count, "written behind the slice")
        # the argument checks of test_gpu_hop.py::test_argument_checks hold on a lattice configuration too
        assert lib.btbbx_hop_sequence_device(C.byref(cfg), 32, 64, buf.ptr, None) == hl.E_ARG
        assert lib.btbbx_hop_sequence_device(C.byref(cfg), hl.SEQ_LEN, 64, buf.ptr, None) == hl.E_ARG
    finally:
        buf.free()


def test_single_piconet_reversal_call_by_call():
    lib = bt.lib()
    for n_scn, s in enumerate(hl.SCENARIOS):
        c = hl.configs()[s["cfg"]]
        off, ch = hl.expand(s)
        opened, calls = hl.replayed(s["tag"])
        rev = bt.HopReversal(_cfg(c), s["c0"] & 63, int(ch[0]), s["aliased"])
        try:
            assert rev.count == len(opened), s["tag"]
            assert np.array_equal(rev.candidates(), opened), s["tag"]
            if n_scn in (0, 9):                                     # 1025 observations: refused, the list as it was
                o, h = np.zeros(1025, np.int32), np.zeros(1025, np.uint8)
                assert lib.btbbx_hop_reversal_winnow(rev.h, o.ctypes.data_as(C.c_void_p), h.ctypes.data_as(C.c_void_p), 1025, None, None,
                                                     None) == hl.E_ARG
                assert np.array_equal(rev.candidates(), opened), s["tag"]
            at = 0
            for k, (n, (n_before, stop, count, cand0, left)) in enumerate(zip(s["cuts"], calls)):
                assert rev.count == n_before
                got = rev.winnow(off[at:at + n], ch[at:at + n])
                assert got == (stop, count, cand0), (s["tag"], k, got, (stop, count, cand0))
                cand = rev.candidates()
                assert len(cand) == count and np.array_equal(cand, left), (s["tag"], k)
                at += n
            # nothing to apply: the list as it is
            assert rev.winnow([], []) == (0, len(left), int(left[0]) if len(left) else 0), s["tag"]
        finally:
            rev.close()


def _tiles_log2(job_cap):
    """the rule of btbbx_hop_reversal_batch_device (hop.hip), copied"""
    t = 9
    while t > 4 and (job_cap << t) > 16384:
        t -= 1
    return t


def test_batch_reversal_against_the_model():
    cand_cap = 16
    fit = [s for s in hl.SCENARIOS if sum(s["cuts"]) <= 1024]
    assert len(fit) >= 12
    cfgs = [_cfg(hl.configs()[s["cfg"]]) for s in fit]
    obs = [hl.expand(s) for s in fit]
    jobs1, offsets, channels = bt.clock_jobs(cfgs, [s["c0"] & 63 for s in fit], obs, [s["aliased"] for s in fit])
    want = [hl.one_call(s) for s in fit]
    seen = set()
    for times in (1, 3):                                            # the same jobs once and three times over: two tilings
        jobs = np.concatenate([jobs1] * times)
        seen.add(_tiles_log2(len(jobs)))
        res, cand = bt.hop_reversal_batch_raw(jobs, offsets, channels, cand_cap, np.full((len(jobs), cand_cap), FILL, np.uint32))
        for j in range(len(jobs)):
            s = fit[j % len(fit)]
            n_initial, stop, count, cand0, left = want[j % len(fit)]
            r = res[j]
            got = (int(r["status"]), int(r["n_initial"]), int(r["stop"]), int(r["count"]), int(r["cand0"]), int(r["n_stored"]))
            assert got == (0, n_initial, stop, count, cand0, min(count, cand_cap)), (s["tag"], j, got)
            k = min(count, cand_cap)
            assert np.array_equal(cand[j, :k], left[:k]) and (cand[j, k:] == FILL).all(), (s["tag"], j)
    assert len(seen) == 2


def test_follow_hop_check_against_the_model():
    """stage 2 of btbbx_follow_hits_device on the doctored tables of test_gpu_follow.py::test_doctored_tables: the job of every
    followed piconet is replaced by a lattice configuration (no map, 2, 32 and 79 channels) and its clock moved to the top of
    the sequence; hop_channel of every packet is the model's hop at the packet's clock."""
    import _follow as fw
    import _survey as sv
    planted, cap, kw, hits, hops = fw.hopping("three")
    args = dict(channels=cap.channels, clk_div=cap.clk_div, clk_phase=0, max_length=bt.MAX_SYMBOLS, n_words=cap.n_words)
    entry = sv.entry_state(kw["clkn0"])
    base = bt.run_follow_hits(cap.words(), hits, entry, zero_out=len(hits), **args)
    jobs, results = base["jobs"], base["results"]
    assert len(jobs) == 3 and (results["count"] == 1).all()
    two = base["follow"]["stage"] == 2
    assert two.sum() == 90
    for n, kind in enumerate(("none", "u2", "u32", "u79")):
        j2, q = jobs.copy(), results.copy()
        picked = []
        for j in range(3):
            c = hl.config_by_kind(kind, (n + j) % 2)
            picked.append(c)
            j2["cfg"][j] = np.frombuffer(bytes(_cfg(c)), dtype=bt.HOP_CFG_DTYPE)[0]
            j2["aliased"][j] = j == 2
        q["cand0"][1] = (int(q["cand0"][1]) & 63) + hl.SEQ_LEN - 64           # the last group: the clock passes 2^27 inside the packets
        out = bt.run_follow_hits(cap.words(), hits, entry, zero_out=len(hits), jobs=j2, results=q, **args)
        fol = out["follow"]
        assert ((fol["stage"] == 2) == two).all()
        checked = 0
        for j in range(3):
            mine = two & (fol["job"] == j)
            want = hl.observable(hl.model_hops(picked[j].address, picked[j].afh_map, fol["clkn"][mine]), j == 2)
            assert np.array_equal(fol["hop_channel"][mine], want.astype(np.uint8)), (kind, j, picked[j].tag)
            assert np.array_equal(fol["on_hop"][mine] != 0, fol["hop_channel"][mine] == fol["channel"][mine]), (kind, j)
            checked += int(mine.sum())
        assert checked == 90
        assert n != 0 or (fol["clkn"][two & (fol["job"] == 1)].min() < 4096 < hl.SEQ_LEN - 4096 < fol["clkn"][two & (fol["job"] == 1)].max())
