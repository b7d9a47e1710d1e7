"""Helpers of the crowd tests (no test in here): ONE deterministic capture of about 2300 piconets and 9000 packets, laid out so
that every carry and boundary of the survey's list stages (survey.hip: 2048-record group tiles of eight 256-record rounds,
4096-record sort tiles) and of the job builder (survey_jobs.h: one workgroup over the records 1024 at a time, a stride of 64
over a job's observations) decides a result -- and tags(), which says from the oracle's records which of those inputs are
there.  tests/test_crowd_model.py asserts every tag on the CPU; tests/test_gpu_crowd.py runs the capture through the device.

Records come in ascending LAP, so the LAP is an increasing function of the intended record index g and the KIND of a piconet
is a function of g alone (kind_of, plan): the seed only moves UAPs, clocks, payloads and places.

    crc    0-2 quiet headers (NULL / POLL), one DM1 / DH1 / FHS, 0-3 POLLs: settles on the CRC
    id     one ID packet: nothing walked, no job
    open   one POLL: walked, not settled
    elim   14 quiet headers: candidates go by UAP disagreement (the oracle's time goes here: a few dozen)
    reset  two devices under one LAP, then two DM1: settles with n_walked > packets_observed
    twin   the same packet at one time on two streams (the higher stream first in the list), then a POLL or a DM1
    long   a DM1 and 150 POLLs: a run of more than 128 observations
    huge   a DM1 and 1100 POLLs: a run that max_obs = 1024 cuts

Every packet fits in one slot of 625 symbols and lies on a (stream, slot) place of its own; the packets of one piconet take
their places in ascending (slot, stream), so "then" above is time.
"""
import functools
from collections import namedtuple

import numpy as np

import _acquire as aq
import _survey as sv
import libbtbb_amd as bt
from libbtbb_amd import synth

SEED, CLKN0 = 77, 4242
N_STREAMS, N_SYMBOLS, N_SLOTS = 79, 64 * 4096, 417
N_RECORDS = 2301
G_HUGE, G_LONG = 600, 1500                  # round 0 and round 1 of the builder's record loop
SLOT_ROUND = 1024                           # AQ_SLOT_THREADS
GRP_TILE, GRP_ROUND, SORT_TILE = 2048, 256, 4096   # SV_GRP_TILE, SV_THREADS, SV_SORT_TILE
REC_CAPS = (1, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049)

TAGS = frozenset((
    "settled_block_64", "unsettled_block_64", "alternating_block_64", "settled_1023_1024", "settled_2047_2048",
    "round_1_opens_unsettled", "last_settled", "rec_cap_prefix_ends_unsettled", "long_and_huge_in_different_rounds",
    "group_straddles_grp_tile", "group_straddles_round", "headers_in_every_round_of_a_tile", "two_sort_tiles", "four_grp_tiles",
    "wave_of_one_group_full", "wave_mixed", "run_over_64", "run_cut_at_1024", "reset_before_settle", "twin_sorted_by_stream"))


def lap_of(g):
    return 0x010000 + 0x1F3 * g


def kind_of(g):
    fixed = {0: "crc", 62: "open", G_HUGE: "huge", G_LONG: "long", 1023: "crc", 1024: "crc", 1025: "open", 1026: "id", 1027: "open",
             1028: "id", 2046: "id", 2047: "crc", 2048: "crc", N_RECORDS - 1: "crc"}
    if g in fixed:
        return fixed[g]
    if 64 <= g < 128:                                   # a wave of the builder's scan all settled
        return "crc"
    if 128 <= g < 192:                                  # ... none settled
        return "id" if g & 1 else "open"
    if 192 <= g < 256:                                  # ... every other one
        return "id" if g & 1 else "crc"
    if g % 80 == 40:
        return "elim"
    h = ((g * 2654435761) & 0xFFFFFFFF) >> 28
    return "crc" if h < 11 else "id" if h < 13 else "open" if h == 13 else "twin" if h == 14 else "reset"


def plan(g):
    """The packets of piconet g in time order: (type or None for an ID packet, device 0 / 1); a twin's first two are one packet."""
    kind = kind_of(g)
    quiet = (synth.TYPE_NULL, synth.TYPE_POLL)
    if kind == "crc":
        return ([(quiet[j & 1], 0) for j in range((g // 3) % 3)] + [((synth.TYPE_DM1, synth.TYPE_DH1, synth.TYPE_FHS)[g % 3], 0)] +
                [(synth.TYPE_POLL, 0)] * ((g // 7) % 4))
    if kind == "id":
        return [(None, 0)]
    if kind == "open":
        return [(synth.TYPE_POLL, 0)]
    if kind == "elim":
        return [(quiet[(j + g) & 1], 0) for j in range(14)]
    if kind == "reset":
        return [(synth.TYPE_POLL, j & 1) for j in range(6)] + [(synth.TYPE_DM1, 0)] * 2
    if kind == "twin":
        return [(synth.TYPE_POLL, 0)] * 2 + [(synth.TYPE_DM1 if (g >> 1) & 1 else synth.TYPE_POLL, 0)]
    return [(synth.TYPE_DM1, 0)] + [(synth.TYPE_POLL, 0)] * (150 if kind == "long" else 1100)


Crowd = namedtuple("Crowd", "cap kw hits kinds")


def build(seed=SEED):
    """-> Crowd(capture, its arguments, the hit list of the placements in the order the packets were placed (offset = slot *
    625, no access-code errors), the kind of every record)."""
    cap = sv.Capture(seed, N_STREAMS, N_SYMBOLS, clk_div=625)
    rng = cap.rng
    places = [(st, sl) for sl in range(N_SLOTS) for st in range(N_STREAMS)]
    perm = rng.permutation(len(places))
    at = [0]

    def take(m):
        out = []
        while len(out) < m:
            p = places[perm[at[0]]]
            at[0] += 1
            if p not in cap.used and p not in out:
                out.append(p)
        return sorted(out, key=lambda p: (p[1], p[0]))

    hits = []

    def put(place, lap, symbols):
        st, sl = place
        cap.put(st, sl, symbols)
        hits.append((sl * cap.clk_div, lap, 0, 0, st))

    def packet(lap, ptype, uap, off6, slot):
        if ptype is None:
            return synth.build_packet(lap)
        return sv._pkt(lap, uap, (CLKN0 + slot + off6) & 63, ptype, rng)

    kinds = []
    for g in range(N_RECORDS):
        lap, kind, pk = lap_of(g), kind_of(g), plan(g)
        dev = [(int(rng.integers(1, 256)), int(rng.integers(0, 64)))]
        dev.append(((dev[0][0] + 0x5b) & 0xff or 1, dev[0][1] + 7))
        kinds.append(kind)
        if kind == "twin":
            while True:
                a, b = take(2)
                other = [st for st in range(N_STREAMS) if st != a[0] and (st, a[1]) not in cap.used and (st, a[1]) != b]
                if b[1] > a[1] and other:
                    break
            st2 = other[int(rng.integers(0, len(other)))]
            s = packet(lap, pk[0][0], *dev[0], a[1])
            for st in sorted((a[0], st2), reverse=True):                # the higher stream first: list order is not sorted order
                put((st, a[1]), lap, s)
            put(b, lap, packet(lap, pk[2][0], *dev[0], b[1]))
            continue
        for place, (ptype, d) in zip(take(len(pk)), pk):
            put(place, lap, packet(lap, ptype, *dev[d], place[1]))
    return Crowd(cap, dict(clkn0=CLKN0, clk_phase=0), np.array(hits, dtype=bt.HIT_DTYPE), kinds)


@functools.lru_cache(maxsize=None)
def crowd():
    """the capture and its hit list: built once per process, never changed"""
    return build()


@functools.lru_cache(maxsize=None)
def oracle_records():
    """(records, candidates) of the survey loop over the oracle port, and the Walked (header pass) that every model() shares"""
    c = crowd()
    engine = sv.OracleEngine()
    recs, cands = sv.expected(engine, c.cap, c.hits, CLKN0)
    return recs, cands, aq.Walked(engine, c.cap, c.hits, CLKN0)


@functools.lru_cache(maxsize=None)
def model(rec_cap=None, flags=0, max_obs=1024, job_cap=None):
    """aq.model over the first rec_cap records of the crowd (None: all); cached, never changed"""
    c = crowd()
    recs, _, walked = oracle_records()
    return aq.model(walked.engine, c.cap, c.hits, recs if rec_cap is None else recs[:rec_cap], CLKN0, flags=flags, max_obs=max_obs,
                    job_cap=job_cap, walked=walked)


def runs(recs, walked):
    """observations of every record's run before any max_obs (0: not settled)"""
    out = np.zeros(len(recs), dtype=np.int64)
    for g in np.nonzero(recs["settled_by"])[0]:
        out[g] = len(walked.group(int(g))[0]) - (int(recs["n_walked"][g]) - int(recs["packets_observed"][g]))
    return out


def tags(recs, hits, walked):
    """Which of the inputs the lattice is built for are in (records of the oracle, the list they came from, its header pass)."""
    t = set()
    n = len(recs)
    settled = recs["settled_by"] != 0
    blocks = settled[:n // 64 * 64].reshape(-1, 64)
    if blocks.all(axis=1).any():
        t.add("settled_block_64")
    if (~blocks).all(axis=1).any():
        t.add("unsettled_block_64")
    even, odd = blocks[:, 0::2], blocks[:, 1::2]
    if ((even.all(axis=1) & ~odd.any(axis=1)) | (odd.all(axis=1) & ~even.any(axis=1))).any():
        t.add("alternating_block_64")
    for a in (1023, 2047):
        if n > a + 1 and settled[a] and settled[a + 1]:
            t.add("settled_%d_%d" % (a, a + 1))
    if n > 1028 and settled[1024] and not settled[1025:1029].any():
        t.add("round_1_opens_unsettled")
    if settled[-1]:
        t.add("last_settled")
    if any(c <= n and not settled[c - 1] for c in REC_CAPS):
        t.add("rec_cap_prefix_ends_unsettled")
    run = runs(recs, walked)
    longs, huges = np.nonzero((run > 128) & (run <= 1024))[0], np.nonzero(run > 1024)[0]
    if len(longs):
        t.add("run_over_64")
    if len(huges):
        t.add("run_cut_at_1024")
    if any(a // SLOT_ROUND != b // SLOT_ROUND for a in longs for b in huges):
        t.add("long_and_huge_in_different_rounds")
    if (settled & (recs["n_walked"] > recs["packets_observed"])).any():
        t.add("reset_before_settle")
    # the sorted list
    order, starts = walked.order, walked.starts
    lap, off, stream = hits["lap"][order], hits["offset"][order], hits["stream"][order]
    inner = np.zeros(len(order) + 1, dtype=bool)                        # positions strictly inside a LAP's run
    inner[:] = True
    inner[starts] = False
    if inner[GRP_TILE::GRP_TILE].any():
        t.add("group_straddles_grp_tile")
    if inner[[k for k in range(GRP_ROUND, len(order), GRP_ROUND) if k % GRP_TILE]].any():
        t.add("group_straddles_round")
    present = walked.present()
    full = present[:len(order) // GRP_TILE * GRP_TILE].reshape(-1, GRP_TILE // GRP_ROUND, GRP_ROUND)
    if len(full) >= 2 and full.any(axis=2).all():                        # of every full tile, and there is a carry between two
        t.add("headers_in_every_round_of_a_tile")
    if len(order) > SORT_TILE:
        t.add("two_sort_tiles")
    if len(order) > 3 * GRP_TILE:
        t.add("four_grp_tiles")
    waves = lap[:len(order) // 64 * 64].reshape(-1, 64)
    one = (waves == waves[:, :1]).all(axis=1)
    if one.any():
        t.add("wave_of_one_group_full")
    if (~one).any():
        t.add("wave_mixed")
    same = (lap[1:] == lap[:-1]) & (off[1:] == off[:-1]) & (stream[1:] != stream[:-1])
    if (same & (order[1:] < order[:-1])).any():                         # the list has the higher stream first
        t.add("twin_sorted_by_stream")
    return t
