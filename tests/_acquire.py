"""Helpers of the clock-acquisition tests (no test in here): the host model of the job builder
(btbbx_survey_clock_jobs_device, include/btbbx.h) in numpy, and hopping captures with known clocks.

The model takes the survey records from _survey.expected(OracleEngine(), ...) and header_present from the oracle port, so it
does not depend on the code under test (the hop configuration comes from btbbx_hop_cfg_init, a host function with tests of its
own against the reference's bank).

A settled record's observations: W = the header-bearing packets of its LAP in ascending (offset, stream); the walk stopped at
W[n_walked - 1] with packets_observed packets in the pattern memory, so the run btbb_init_hop_reversal + btbb_winnow see is
W[n_walked - packets_observed .. n_walked), and every later packet of W is what try_hop appends.
"""
import numpy as np

import _libs
import _survey as sv
import libbtbb_amd as bt
from libbtbb_amd import synth

JOBS_AFH, JOBS_ALIASED = 1, 2


class Walked:
    """The header-bearing packets of every LAP of `hits` (the header_present pass of the oracle port), group by group and only
    when asked for: group(g) -> (W = hit indices in ascending (offset, stream), {hit index: (stored clock, channel)}).  One
    Walked serves every rec_cap / job_cap / max_obs / flags variation of model() over the same list."""

    def __init__(self, engine, cap, hits, clkn0, clk_phase=0, max_length=bt.MAX_SYMBOLS):
        self.engine, self.cap, self.hits = engine, cap, np.asarray(hits)
        self.clkn0, self.clk_phase, self.max_length = clkn0, clk_phase, max_length
        hits = self.hits
        self.order = np.lexsort((hits["stream"], hits["offset"], hits["lap"]))
        laps = hits["lap"][self.order]
        self.starts = (np.concatenate([[0], np.nonzero(np.diff(laps.astype(np.int64)))[0] + 1, [len(self.order)]])
                       if len(self.order) else np.zeros(1, int))
        self._groups = {}

    def members(self, g):
        return self.order[self.starts[g]:self.starts[g + 1]]

    def group(self, g):
        if g not in self._groups:
            engine, cap, hits = self.engine, self.cap, self.hits
            walked, clocks = [], {}
            for k in self.members(g):
                h = hits[k]
                st = int(h["stream"])
                ch = st if cap.channels is None else int(cap.channels[st])
                clkn = (self.clkn0 + (int(h["offset"]) + self.clk_phase) // cap.clk_div) & 0xFFFFFFFF
                p = engine.packet(int(h["lap"]), int(h["ac_errors"]), sv.packet_symbols(cap, h, self.max_length), ch, clkn)
                if engine.header_present(p):
                    walked.append(int(k))
                    clocks[int(k)] = (clkn, ch)
                engine.free_packet(p)
            self._groups[g] = (walked, clocks)
        return self._groups[g]

    def present(self):
        """header_present of every hit, in sorted order (what survey_wmark / wlist compact)"""
        out = np.zeros(len(self.order), dtype=bool)
        where = {int(k): i for i, k in enumerate(self.order)}
        for g in range(len(self.starts) - 1):
            for k in self.group(g)[0]:
                out[where[k]] = True
        return out


def model(engine, cap, hits, recs, clkn0, clk_phase=0, max_length=bt.MAX_SYMBOLS, flags=0, max_obs=1024, job_cap=None, walked=None):
    """What the builder leaves for `recs` (the first len(recs) LAPs of `hits` in ascending order): dict(n_jobs = all settled
    records, jobs / job_rec = the first job_cap of them, offsets / channels / obs_hits = their observations, n_obs).
    walked: a Walked over the same list and arguments, to share the header pass between calls (None: one of this call's own)."""
    hits = np.asarray(hits)
    lists = Walked(engine, cap, hits, clkn0, clk_phase, max_length) if walked is None else walked
    assert lists.hits is hits or (len(lists.hits) == len(hits) and lists.hits.tobytes() == hits.tobytes())
    assert (lists.clkn0, lists.clk_phase, lists.max_length) == (clkn0, clk_phase, max_length)
    cfgs, clk6, obs, job_rec, oh = [], [], [], [], []
    n_jobs = 0
    for g, r in enumerate(recs):
        group = lists.members(g)
        lap = int(r["lap"])
        assert int(hits["lap"][group[0]]) == lap and len(group) == r["n_packets"]
        if not r["settled_by"]:
            continue
        n_jobs += 1
        if job_cap is not None and n_jobs > job_cap:
            continue
        walked_g, clocks = lists.group(g)
        first = int(r["n_walked"]) - int(r["packets_observed"])
        assert 0 <= first < int(r["n_walked"]) <= len(walked_g)
        assert walked_g[int(r["n_walked"]) - 1] == r["settled_hit"]
        run = walked_g[first:][:max_obs]
        t0 = clocks[run[0]][0]
        assert t0 == r["first_pkt_time"]
        off = np.array([(clocks[k][0] - t0) & 0xFFFFFFFF for k in run], dtype=np.uint32).view(np.int32)
        obs.append((off, np.array([clocks[k][1] for k in run], dtype=np.uint8)))
        oh.append(np.array(run, dtype=np.uint32))
        cfgs.append(bt.hop_cfg(lap, int(r["uap"]), r["afh_map"] if flags & JOBS_AFH else None))
        clk6.append((int(r["clk_offset"]) + t0) & 63)
        job_rec.append(g)
    jobs, offsets, channels = bt.clock_jobs(cfgs, clk6 if clk6 else 0, obs, aliased=bool(flags & JOBS_ALIASED))
    return dict(n_jobs=n_jobs, jobs=jobs, job_rec=np.array(job_rec, dtype=np.uint32), offsets=offsets, channels=channels,
                obs_hits=np.concatenate(oh) if oh else np.zeros(0, np.uint32), n_obs=len(offsets))


def assert_builder_equals(out, want, sentinel, ctx=""):
    """`out`: bt.run_survey_clock_jobs over buffers filled with `sentinel` bytes; `want`: model()."""
    nj, no = len(want["jobs"]), want["n_obs"]
    assert (out["n_jobs"], out["n_obs"]) == (want["n_jobs"], no), (ctx, out["n_jobs"], out["n_obs"], want["n_jobs"], no)
    assert out["jobs"][:nj].tobytes() == want["jobs"].tobytes(), (ctx, [j for j in range(nj) if out["jobs"][j].tobytes() != want["jobs"][j].tobytes()][:4])
    assert out["job_rec"][:nj].tolist() == want["job_rec"].tolist(), ctx
    assert out["offsets"][:no].tolist() == want["offsets"].tolist(), ctx
    assert out["channels"][:no].tolist() == want["channels"].tolist(), ctx
    assert out["obs_hits"][:no].tolist() == want["obs_hits"].tolist(), ctx
    # nothing behind what is reported
    for name, n in (("jobs", nj), ("job_rec", nj), ("offsets", no), ("channels", no), ("obs_hits", no)):
        rest = out[name][n:].view(np.uint8)
        assert (rest == sentinel).all(), (ctx, name, "written past", n)


# ---- hopping captures ---------------------------------------------------------------------------------------------

N_SLOTS = 104                                           # 64 * 1024 symbols = 104 slots of 625 (and 536 symbols)


class Planted:
    def __init__(self, lap, uap, c0, afh_map=None, n_packets=30):
        self.lap, self.uap, self.c0, self.afh_map, self.n_packets = lap, uap, c0, afh_map, n_packets
        self.slots = []                                 # slot of every packet, ascending


def hopping_capture(seed, planted, hop, clkn0):
    """79 streams with channel = stream, 64 * 1024 symbols each.  Every piconet of `planted` sends n_packets packets on free
    increasing slots; the packet of slot k goes on stream hop(piconet, [c0 + k]) and is built with CLK1-6 = (c0 + k) & 63, the
    master's clock c0 at slot 0 -- the receiver stores clkn0 + k for it.  POLL, DM1, DH1 and FHS, so a CRC settles the UAP.
    No packet is on two streams at one time.  hop(piconet, clocks) -> channels."""
    cap = sv.Capture(seed, 79, 64 * 1024)
    rng = cap.rng
    types = (synth.TYPE_POLL, synth.TYPE_DM1, synth.TYPE_DH1, synth.TYPE_FHS)
    for p in planted:
        chans = hop(p, (p.c0 + np.arange(N_SLOTS)) & (bt.SEQUENCE_LENGTH - 1))
        free = [k for k in range(N_SLOTS) if (int(chans[k]), k) not in cap.used]
        p.slots = sorted(int(k) for k in rng.choice(free, size=p.n_packets, replace=False))
        for i, k in enumerate(p.slots):
            cap.put(int(chans[k]), k, sv._pkt(p.lap, p.uap, (p.c0 + k) & 63, types[(i + (i >> 2)) % 4], rng))
    return cap, dict(clkn0=clkn0, clk_phase=0)


def three_piconets(seed=41):
    rng = np.random.default_rng(_libs.seed(seed))
    c0s = [int(rng.integers(0, 1 << 27)), int(rng.integers(0, 1 << 27)), (1 << 27) - 20]
    return [Planted(int(rng.integers(1, 1 << 24)), int(rng.integers(1, 256)), c0) for c0 in c0s]


def afh_piconet(seed=42, n_used=20, n_packets=60):
    import _hop
    rng = np.random.default_rng(_libs.seed(seed))
    return [Planted(int(rng.integers(1, 1 << 24)), int(rng.integers(1, 256)), int(rng.integers(0, 1 << 27)),
                    afh_map=_hop.afh_map_bytes(rng, n_used), n_packets=n_packets)]
