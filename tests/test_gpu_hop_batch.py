"""GPU parity of the batch CLK1-27 reversal (btbbx_hop_reversal_batch_*, hop_batch.h) with the single-piconet path
(btbbx_hop_reversal_open / _winnow / _candidates, pinned to the oracle and to the reference's traces by test_gpu_hop.py),
with the traces recorded from the reference (tests/golden/hop.json), and its handling of rejected jobs, of a job count
that lives in device memory and of a job whose candidates would not fit any scratch; and every tiling of pass 1 (tiles_log2 9
down to 4) with true clocks on the edges of its tiles."""
import ctypes as C
import json
import os
import zlib

import numpy as np
import pytest

import _hop
import _libs
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HOP = json.load(open(os.path.join(HERE, "golden", "hop.json")))
FILL = 0xA5A5A5A5


@pytest.fixture(scope="module", autouse=True)
def ready():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    bt.init(2)
    yield


class _Slice:
    """The part [first, first + len(data)) of a hop sequence, indexed by CLK1-27 as _hop.observations indexes the whole."""

    def __init__(self, cfg, c0, span):
        self.first = c0 & ~63
        assert self.first + span + 128 <= _hop.SEQ_LEN
        self.data = bt.hop_sequence(cfg, self.first, (span + 128) & ~63)

    def __getitem__(self, i):
        return self.data[i - self.first]


def _amap(case):
    return None if case["afh_map"] is None else np.array(case["afh_map"], np.uint8)


def _scenario(rng, used, alias, n_obs):
    """One piconet and n_obs of its hops from clock c0 on: (cfg, c0, offsets, channels)."""
    lap, uap = int(rng.integers(0, 1 << 24)), int(rng.integers(0, 256))
    cfg = bt.hop_cfg(lap, uap, _hop.afh_map_bytes(rng, used) if used else None)
    max_gap = 400 if n_obs > 30 else 2000
    c0 = int(rng.integers(0, _hop.SEQ_LEN - n_obs * max_gap - 256))
    obs = _hop.observations(rng, _Slice(cfg, c0, n_obs * max_gap), c0, n_obs, alias=bool(alias), max_gap=max_gap)
    return cfg, c0, [o[0] for o in obs], [o[1] for o in obs]


def _single(cfg, clk6, off, ch, aliased, cand_cap):
    """What the single-piconet path leaves for one job: (n_initial, stop, count, cand0, candidates[:cand_cap])."""
    rev = bt.HopReversal(cfg, clk6, ch[0], aliased)
    n_initial = rev.count
    stop, count, cand0 = rev.winnow(off, ch)
    cand = rev.candidates()[:cand_cap].copy() if count else np.zeros(0, np.uint32)
    rev.close()
    return n_initial, stop, count, cand0, cand


def test_parity_with_the_single_piconet_path():
    rng = np.random.default_rng(_libs.seed(6401))
    cand_cap = 16
    cfgs, clk6, obs, alias, c0s, unique = [], [], [], [], [], []

    def add(cfg, c0, off, ch, al, sure=False):
        cfgs.append(cfg)
        clk6.append(c0 & 63)
        obs.append((off, ch))
        alias.append(al)
        c0s.append(c0)
        unique.append(sure)
    for used in (None, 79, 66, 30, 5, 1):
        for al in (0, 1):
            for n_obs in (1, 2, 30, 1024):
                cfg, c0, off, ch = _scenario(rng, used, al, n_obs)
                add(cfg, c0, off, ch, al, sure=n_obs >= 30 and (used is None or used >= 21))
    for used, al in ((None, 0), (66, 1)):                       # a contradiction planted at observation 3
        cfg, c0, off, ch = _scenario(rng, used, al, 30)
        ch[3] = _hop.aliased((ch[3] + 7) % 79) if al else (ch[3] + 7) % 79
        add(cfg, c0, off, ch, al)
    for first in (79, 200):                                     # a first channel no clock hops on: empty initial list
        cfg, c0, off, ch = _scenario(rng, None, 0, 30)
        ch[0] = first
        add(cfg, c0, off, ch, 0)
    jobs, offsets, channels = bt.clock_jobs(cfgs, clk6, obs, alias)
    # two more jobs on the observation range of job 2 (basic hopping, 30 observations): the same piconet with the other
    # aliasing flag, and another piconet
    shared = np.zeros(2, bt.CLOCK_JOB_DTYPE)
    shared[0], shared[1] = jobs[2], jobs[6]
    shared["aliased"][0] = 1
    shared["obs_first"][1], shared["n_obs"][1] = jobs["obs_first"][2], jobs["n_obs"][2]
    jobs = np.concatenate([jobs, shared])
    for s in shared:
        cfgs.append(bt.HopCfg.from_buffer_copy(s["cfg"].tobytes()))
        clk6.append(int(s["clk6"]))
        obs.append(obs[2])
        alias.append(int(s["aliased"]))
        unique.append(False)
    assert jobs[2]["n_obs"] == 30 and len(jobs) == 54

    res, cand = bt.hop_reversal_batch_raw(jobs, offsets, channels, cand_cap, np.full((len(jobs), cand_cap), FILL, np.uint32))
    cut_short = 0
    for j in range(len(jobs)):
        off, ch = obs[j]
        n_initial, stop, count, cand0, want = _single(cfgs[j], clk6[j], off, ch, alias[j], cand_cap)
        r = res[j]
        assert (int(r["status"]), int(r["n_initial"]), int(r["stop"]), int(r["count"])) == (0, n_initial, stop, count), j
        assert int(r["cand0"]) == (cand0 if count else 0), j
        assert int(r["n_stored"]) == min(count, cand_cap) == len(want), j
        assert np.array_equal(cand[j, :len(want)], want), j
        assert (cand[j, len(want):] == FILL).all(), j
        if unique[j]:
            assert count == 1 and cand0 == c0s[j], j
        cut_short += int(stop == len(off) and count > cand_cap)
    assert cut_short >= 8                                       # the jobs of one and two observations, mostly
    for j in (48, 49):                                          # the contradictions: the true clock does not survive
        assert res[j]["stop"] < 30 and (res[j]["count"] == 0 or res[j]["cand0"] != c0s[j]), j
    for j in (50, 51):
        assert (res[j]["n_initial"], res[j]["stop"], res[j]["count"], res[j]["cand0"]) == (0, 0, 0, 0), j


def test_reference_traces():
    """Every recorded case as one job with all its observations, and cut after the first winnow step of the trace."""
    cases = HOP["cases"]
    cand_cap = max(c["trace"][1]["n"] for c in cases)
    cfgs = [bt.hop_cfg(c["lap"], c["uap"], _amap(c)) for c in cases] * 2
    clk6 = [c["c0"] & 63 for c in cases] * 2
    alias = [c["aliased"] for c in cases] * 2
    obs = [([o[0] for o in c["obs"]], [o[1] for o in c["obs"]]) for c in cases]
    obs += [(off[:2], ch[:2]) for off, ch in obs]
    res, cand = bt.hop_reversal_batch(cfgs, clk6, obs, alias, cand_cap)
    for i, c in enumerate(cases):
        trace = c["trace"]
        assert trace[1]["winnowed"] == 2                        # the first winnow step applied observations 0 and 1
        full, cut = res[i], res[len(cases) + i]
        assert full["status"] == 0 and full["count"] == 1 and full["cand0"] == c["c0"] and full["n_initial"] == trace[0]["n"], i
        assert cand[i].tolist() == [c["c0"]], i
        assert cut["status"] == 0 and cut["n_initial"] == trace[0]["n"] and cut["count"] == trace[1]["n"], i
        got = cand[len(cases) + i]
        assert len(got) == trace[1]["n"] and zlib.crc32(got.astype("<u4").tobytes()) == trace[1]["cand_crc"], i
        assert got[:8].tolist() == trace[1]["cand_head"] and cut["cand0"] == got[0], i


def _good_job(rng):
    cfg, c0, off, ch = _scenario(rng, None, 0, 30)
    return cfg, c0, off, ch


def test_rejected_jobs_leave_their_neighbours_alone():
    rng = np.random.default_rng(_libs.seed(6402))
    cand_cap = 4
    cfg, c0, off, ch = _good_job(rng)
    good, offsets, channels = bt.clock_jobs([cfg], [c0 & 63], [(off, ch)])
    n_total = len(offsets)

    def bad(**fields):
        j = good.copy()
        for k, v in fields.items():
            if k in ("afh", "used_channels"):
                j["cfg"][k] = v
            else:
                j[k] = v
        return j
    rejects = [bad(clk6=64), bad(clk6=0xFFFFFFFF), bad(n_obs=0), bad(n_obs=1025), bad(obs_first=1, n_obs=n_total),
               bad(obs_first=n_total + 1, n_obs=1), bad(obs_first=0xFFFFFFFF, n_obs=2), bad(obs_first=0xFFFFFFF0, n_obs=0x20),
               bad(afh=1, used_channels=0), bad(afh=1, used_channels=80), bad(afh=7, used_channels=255)]
    jobs = np.concatenate([good] + rejects + [good])
    n = len(jobs)
    slots = np.full((n + 3) * cand_cap, FILL, np.uint32)            # three jobs' worth of slots behind the call's own
    res, cand = bt.hop_reversal_batch_raw(jobs, offsets, channels, cand_cap, slots)
    assert res[0].tobytes() == res[n - 1].tobytes()
    assert (res[0]["status"], res[0]["count"], res[0]["cand0"], res[0]["n_stored"]) == (0, 1, c0, 1)
    want = _single(cfg, c0 & 63, off, ch, 0, cand_cap)
    assert (int(res[0]["n_initial"]), int(res[0]["stop"]), int(res[0]["count"]), int(res[0]["cand0"])) == want[:4]
    slots = slots.reshape(-1, cand_cap)
    for j in (0, n - 1):
        assert slots[j].tolist() == [c0, FILL, FILL, FILL], j
    for j in range(1, n - 1):
        assert res[j]["status"] == 1 and res[j]["count"] == 0 and res[j]["n_stored"] == 0, j
        assert (slots[j] == FILL).all(), j
    assert (slots[n:] == FILL).all()


def _device_call(jobs, n_jobs_word, job_cap, offsets, channels, cand_cap, stream=None):
    """btbbx_hop_reversal_batch_device with results and candidates preset to the fill -> (results, candidates) of job_cap jobs."""
    lib = bt.lib()
    scratch_bytes = lib.btbbx_hop_reversal_batch_scratch_bytes(job_cap, cand_cap)
    bufs = []

    def dev(a):
        bufs.append(bt.DeviceBuffer(max(a.nbytes, 16)).upload(a))
        return bufs[-1]
    try:
        d_jobs, d_n = dev(jobs), dev(np.array([n_jobs_word, 0], np.uint32))
        d_off, d_ch = dev(offsets), dev(channels)
        d_res = dev(np.full(job_cap * 6, FILL, np.uint32))
        d_cand = dev(np.full(job_cap * cand_cap + 64, FILL, np.uint32))
        d_scr = dev(np.full(scratch_bytes // 4, FILL, np.uint32))      # the call prepares its scratch itself
        bt.check(lib.btbbx_hop_reversal_batch_device(d_jobs.ptr, d_n.ptr, job_cap, d_off.ptr, d_ch.ptr, len(offsets), d_res.ptr,
                                                     d_cand.ptr, cand_cap, d_scr.ptr, scratch_bytes, stream),
                 "btbbx_hop_reversal_batch_device")
        bt.check(lib.btbbx_sync(stream), "sync")
        return d_res.download(np.uint32, job_cap * 6).view(bt.CLOCK_RESULT_DTYPE), d_cand.download(np.uint32, job_cap * cand_cap + 64)
    finally:
        for b in bufs:
            b.free()


def test_job_count_in_device_memory():
    import torch
    rng = np.random.default_rng(_libs.seed(6403))
    cand_cap, job_cap = 4, 8
    sc = [_scenario(rng, used, 0, n_obs) for used, n_obs in ((None, 30), (40, 30), (None, 2))] * 3
    jobs, offsets, channels = bt.clock_jobs([s[0] for s in sc[:job_cap]], [s[1] & 63 for s in sc[:job_cap]],
                                            [(s[2], s[3]) for s in sc[:job_cap]])
    want = [_single(s[0], s[1] & 63, s[2], s[3], 0, cand_cap) for s in sc[:3]]
    side = torch.cuda.Stream()
    for stream in (None, C.c_void_p(side.cuda_stream)):
        res, cand = _device_call(jobs, 3, job_cap, offsets, channels, cand_cap, stream)
        for j in range(3):
            r = res[j]
            assert (int(r["status"]), int(r["n_initial"]), int(r["stop"]), int(r["count"]), int(r["cand0"])) == (0,) + want[j][:4], j
            k = min(want[j][2], cand_cap)
            assert r["n_stored"] == k and np.array_equal(cand[j * cand_cap:j * cand_cap + k], want[j][4]), j
            assert (cand[j * cand_cap + k:(j + 1) * cand_cap] == FILL).all(), j
        assert (res[3:].view(np.uint32) == FILL).all()                 # records 3..7 keep their fill
        assert (cand[3 * cand_cap:] == FILL).all()
    assert want[0][2] == 1 and want[0][3] == sc[0][1] and want[2][2] > cand_cap
    # a count above job_cap is clamped to it
    res, _ = _device_call(jobs, 1000, job_cap, offsets, channels, cand_cap)
    assert (res["status"] == 0).all() and res[:3].tobytes() == res[3:6].tobytes()


def test_flat_scratch_with_every_clock_a_candidate():
    """used_channels = 1: all 2^21 clocks congruent to clk6 are candidates and both observations keep them all."""
    rng = np.random.default_rng(_libs.seed(6404))
    cand_cap = 64
    heavy = _scenario(rng, 1, 0, 2)
    sc = [_scenario(rng, None, 0, 30), heavy, _scenario(rng, 30, 1, 30)]
    alias = [0, 0, 1]
    assert bt.lib().btbbx_hop_reversal_batch_scratch_bytes(3, cand_cap) < 8 << 20      # 2^21 stored clocks alone are 8 MiB
    res, cand = bt.hop_reversal_batch([s[0] for s in sc], [s[1] & 63 for s in sc], [(s[2], s[3]) for s in sc], alias, cand_cap)
    want = [_single(s[0], s[1] & 63, s[2], s[3], a, cand_cap) for s, a in zip(sc, alias)]
    for j in range(3):
        r = res[j]
        assert (int(r["status"]), int(r["n_initial"]), int(r["stop"]), int(r["count"]), int(r["cand0"])) == (0,) + want[j][:4], j
        assert np.array_equal(cand[j], want[j][4]), j
    assert res[1]["n_initial"] == 2 ** 21 and res[1]["count"] == want[1][2] == 2 ** 21 and res[1]["stop"] == 2
    assert cand[1].tolist() == [(heavy[1] & 63) + 64 * i for i in range(cand_cap)]
    for j in (0, 2):
        assert res[j]["count"] == 1 and res[j]["cand0"] == sc[j][1], j


# ---- the tiling ladder ----------------------------------------------------------------------------------------------

LADDER_CAPS = (32, 33, 64, 65, 128, 129, 256, 257, 512, 513)
N_GROUPS = 1 << 21                                              # HOP_GROUPS: the clocks congruent to clk6


def _tiles_log2(job_cap):
    """the rule of btbbx_hop_reversal_batch_device (hop.hip), copied"""
    t = 9
    while t > 4 and (job_cap << t) > 16384:
        t -= 1
    return t


def _edge_scenario(rng, used, alias, n_obs, group):
    """As _scenario, with the true clock in group `group` of the 2^21 (c0 >> 6) and the hops from btbbx_hop_channels_device,
    which takes any clock: the observations may pass 2^27."""
    lap, uap = int(rng.integers(0, 1 << 24)), int(rng.integers(0, 256))
    cfg = bt.hop_cfg(lap, uap, _hop.afh_map_bytes(rng, used) if used else None)
    c0 = 64 * group + int(rng.integers(0, 64))
    off = np.concatenate([[0], np.cumsum(rng.integers(1, 400 if n_obs > 30 else 2000, n_obs - 1))]).astype(np.int64)
    ch = bt.hop_channels(cfg, (c0 + off) % _hop.SEQ_LEN).tolist()
    return cfg, c0, off.tolist(), [_hop.aliased(c) for c in ch] if alias else ch


def _ladder_call(jobs, n_jobs_word, job_cap, offsets, channels, cand_cap):
    """btbbx_hop_reversal_batch_device over fill; n_jobs_word None: a NULL d_n_jobs (job_cap jobs)."""
    lib = bt.lib()
    scratch_bytes = lib.btbbx_hop_reversal_batch_scratch_bytes(job_cap, cand_cap)
    bufs = []

    def dev(a):
        bufs.append(bt.DeviceBuffer(max(a.nbytes, 16)).upload(a))
        return bufs[-1]
    try:
        d_jobs, d_n = dev(jobs), dev(np.array([n_jobs_word or 0, 0], np.uint32))
        d_off, d_ch = dev(offsets), dev(channels)
        d_res = dev(np.full(job_cap * 6, FILL, np.uint32))
        d_cand = dev(np.full(job_cap * cand_cap, FILL, np.uint32))
        d_scr = dev(np.full(scratch_bytes // 4, FILL, np.uint32))
        bt.check(lib.btbbx_hop_reversal_batch_device(d_jobs.ptr, None if n_jobs_word is None else d_n.ptr, job_cap, d_off.ptr, d_ch.ptr,
                                                     len(offsets), d_res.ptr, d_cand.ptr, cand_cap, d_scr.ptr, scratch_bytes, None),
                 "btbbx_hop_reversal_batch_device")
        bt.check(lib.btbbx_sync(None), "sync")
        return (d_res.download(np.uint32, job_cap * 6).view(bt.CLOCK_RESULT_DTYPE),
                d_cand.download(np.uint32, job_cap * cand_cap).reshape(job_cap, cand_cap))
    finally:
        for b in bufs:
            b.free()


def test_tiling_ladder():
    """Every tiling of pass 1 (tiles_log2 9 down to 4: job_cap on both sides of every step) over the same scenarios, with true
    clocks on the edges of the tiles: group 0, the last group, and per - 1 / per for the tile length per of every tiling
    (2^17 - 1 and 2^17 end and open a tile of EVERY tiling).  Eight scenarios cover basic / AFH, aliased or not and 1, 2, 30 and
    1024 observations; ten more put a clock on per - 1 and per of the five finer tilings."""
    rng = np.random.default_rng(_libs.seed(6405))
    cand_cap = 16
    sc = [_edge_scenario(rng, None, 0, 30, 0) + (0, True),
          _edge_scenario(rng, None, 1, 1024, (1 << 17) - 1) + (1, True),
          _edge_scenario(rng, 40, 0, 30, 1 << 17) + (0, True),
          _edge_scenario(rng, 66, 1, 30, N_GROUPS - 1) + (1, True),
          _scenario(rng, None, 0, 1) + (0, False),
          _scenario(rng, 30, 1, 2) + (1, False),
          _scenario(rng, 5, 0, 1024) + (0, False),
          _scenario(rng, 79, 0, 2) + (0, False)]
    edges = {0, (1 << 17) - 1, 1 << 17, N_GROUPS - 1}
    for t in range(5, 10):
        per = N_GROUPS >> t
        for k, group in enumerate((per - 1, per)):
            sc.append(_edge_scenario(rng, (None, 50)[(t + k) & 1], 0, 30, group) + (0, True))
            edges.add(group)
    for t in range(4, 10):                                          # the edge clocks asked for, at every tiling
        per = N_GROUPS >> t
        assert {0, per - 1, per, N_GROUPS - 1} <= edges and {s[1] >> 6 for s in sc} >= edges
    wrap = sc[3]
    assert wrap[1] + wrap[2][-1] >= _hop.SEQ_LEN > wrap[1]          # candidate + offset passes 2^27
    assert sorted(len(s[2]) for s in sc[:8]) == [1, 2, 2, 30, 30, 30, 1024, 1024]
    jobs1, offsets, channels = bt.clock_jobs([s[0] for s in sc], [s[1] & 63 for s in sc], [(s[2], s[3]) for s in sc], [s[4] for s in sc])
    # the single-piconet path, once per scenario
    want_res = np.zeros(len(sc), bt.CLOCK_RESULT_DTYPE)
    want_cand = np.full((len(sc), cand_cap), FILL, np.uint32)
    for i, s in enumerate(sc):
        n_initial, stop, count, cand0, cand = _single(s[0], s[1] & 63, s[2], s[3], s[4], cand_cap)
        want_res[i] = (0, n_initial, stop, count, cand0 if count else 0, min(count, cand_cap))
        want_cand[i, :len(cand)] = cand
        assert len(cand) == min(count, cand_cap)
        if s[5]:                                                    # >= 30 observations on >= 21 channels
            assert (count, cand0) == (1, s[1]), (i, count, cand0, s[1])
    assert (want_res["count"] > cand_cap).sum() >= 3 and (want_res["count"] == 1).sum() >= 14
    seen = set()
    for n_call, job_cap in enumerate(LADDER_CAPS):
        seen.add(_tiles_log2(job_cap))
        which = np.arange(job_cap) % len(sc)
        jobs = jobs1[which]
        n = job_cap - 3 if n_call & 1 else None                     # every other call: the count is a device word below job_cap
        res, cand = _ladder_call(jobs, n, job_cap, offsets, channels, cand_cap)
        n = job_cap if n is None else n
        bad = [j for j in range(n) if res[j].tobytes() != want_res[which[j]].tobytes()]
        assert not bad, (job_cap, bad[:4], res[bad[0]], want_res[which[bad[0]]])
        bad = np.nonzero((cand[:n] != want_cand[which[:n]]).any(axis=1))[0]
        assert len(bad) == 0, (job_cap, bad[:4].tolist(), cand[bad[0]], want_cand[which[bad[0]]])
        assert (res[n:].view(np.uint32) == FILL).all() and (cand[n:] == FILL).all(), job_cap
    assert seen == {4, 5, 6, 7, 8, 9}
