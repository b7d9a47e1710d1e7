"""Test-side model of the LE Coded connection tracking (include/btbbx.h btbbx_le_ctrack_*), written from the four
rules of the duration and the changed rule 3 in plain Python -- not from the kernels (le_ctrack.h keeps eight metrics and 24
decision bits in registers and never traces a whole path).

* symbols: rules 1 to 4 of the duration, on tests/_le_coded.py's block-1 decode (its forward pass and its trace-back)
* track: the tracking with rule 3 taking durations; rules 4 to 7 restate tests/_le_track.py's track()
  (tests/test_le_ctrack_model.py holds the two against each other with 1M durations)
* Rules: the model's branch points as options; Rules() is the model, VARIANTS are deliberately wrong ones
* symbols_lattice / flag_list / chain_capture: the stream, the lists and the capture the CPU and GPU tests share
"""
import collections
import functools
import math

import numpy as np

import _le
import _le_coded as c
import _le_cfind as f
import _le_csa2 as c2
import _le_discover as ld
import _le_track as lt

UNIT, IFS, JITTER = lt.UNIT, lt.IFS, lt.JITTER


class Rules:
    def __init__(self, **kw):
        self.duration_1m = False         # 80 + 8 * length, whatever the stream holds
        self.s_always_8 = False
        self.n_without_3 = False         # N = 8 * (L + 5)
        self.no_376 = False              # S * N alone
        self.ci_swapped = False          # ci = bit 33 | bit 32 << 1
        self.rfu_as_8 = False            # an RFU ci taken as S = 8
        self.event_ge = False            # a new event at offset >= end + ifs
        self.own_duration = False        # end_(m-1) formed with the packet's own duration
        self.end_32bit = False           # end_(m-1) kept in 32 bits
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


MODEL = Rules()
SYMBOL_VARIANTS = ("duration_1m", "s_always_8", "n_without_3", "no_376", "ci_swapped", "rfu_as_8")
TRACK_VARIANTS = ("event_ge", "own_duration", "end_32bit")
VARIANTS = {k: {k: True} for k in SYMBOL_VARIANTS + TRACK_VARIANTS}


def coded_duration(s, length):
    return 376 + s * (8 * (length + 5) + 3)


# ---- the duration ------------------------------------------------------------------------------------------------------
def _block1_symbols(words, n_words, stream, offset):
    """The 296 symbols from offset + 80 of one stream; symbols past the stream's end read as 0.  words: indexed [stream, a:b]."""
    first, total = offset + 80, 64 * n_words
    out = np.zeros(296, np.uint8)
    if first >= total:
        return out
    w0, w1 = first >> 6, min(n_words, (first + 296 + 63) >> 6)
    bits = np.unpackbits(np.ascontiguousarray(words[stream, w0:w1], dtype=np.uint64).view(np.uint8), bitorder="little")
    seg = bits[first - 64 * w0:][:296]
    out[:len(seg)] = seg
    return out


def block1_ci(words, n_words, cands, n_streams):
    """Rule 2 for every candidate whose stream is in range: the decoder's rule 3 (37 steps of 8 symbols from o + 80, x = 0 on equal
    sums, traced back from state 0) -> (bit 32, bit 33), None for the others."""
    live = [i for i, cd in enumerate(cands) if cd.stream < n_streams]
    out = [None] * len(cands)
    if live:
        sym = np.concatenate([_block1_symbols(words, n_words, cands[i].stream, cands[i].offset) for i in live] + [np.zeros(8, np.uint8)])
        n = len(live)
        steps = np.full(n, 37)
        _, dec, _ = c._forward_many(sym, 296 * np.arange(n, dtype=np.int64), 8, steps)
        bits = c._trace_many(dec, steps, np.zeros(n, np.int64))
        for j, i in enumerate(live):
            out[i] = (int(bits[j, 32]), int(bits[j, 33]))
    return out


def symbols(words, n_words, cands, n_streams, rules=MODEL):
    """Rules 1 to 3: one duration per candidate, in the order of the list."""
    out = []
    for cd, ci_bits in zip(cands, block1_ci(words, n_words, cands, n_streams)):
        if ci_bits is None:                                                # rule 1
            out.append(0)
            continue
        if rules.duration_1m:
            out.append(80 + 8 * cd.length)
            continue
        ci = ci_bits[1] + 2 * ci_bits[0] if rules.ci_swapped else ci_bits[0] + 2 * ci_bits[1]
        s = c.FORMAT["s_of_ci"].get(ci, 8 if rules.rfu_as_8 else 0)        # rule 3
        if rules.s_always_8:
            s = 8
        out.append((0 if rules.no_376 else 376) + s * (8 * (cd.length + 5) + (0 if rules.n_without_3 else 3)))
    return out


# ---- the tracking with durations -----------------------------------------------------------------------------------------
def track(cands, n_conns, mhz, n_streams, unit_bits, ifs_bits, jitter_bits, flags, durations, rules=MODEL):
    """btbbx_le_ctrack_device: tests/_le_track.py's track() with end_m = offset_m + durations[m].  Returns (tracks, pkts) of
    lt.Track and lt.Pkt (None: no member)."""
    assert len(durations) == len(cands)
    members = [[] for _ in range(n_conns)]
    chan = {}
    for i, cd in enumerate(cands):                                         # rule 1
        if cd.channel < n_conns and cd.stream < n_streams:
            ch = _le.channel_index(int(mhz[cd.stream]))
            if ch < 37:
                members[cd.channel].append(i)
                chan[i] = ch
    pkts = [None] * len(cands)
    tracks = []
    for g in range(n_conns):
        order = sorted(members[g], key=lambda i: (cands[i].offset, cands[i].stream, i))     # rule 2
        events = []                                                        # rule 3: [anchor, channel, [members]]
        for r, i in enumerate(order):
            new = r == 0
            if not new:
                p = order[r - 1]
                end = cands[p].offset + int(durations[i if rules.own_duration else p])
                if rules.end_32bit:
                    end &= 0xFFFFFFFF
                if chan[i] != chan[p]:
                    new = True
                if cands[i].offset >= end + ifs_bits if rules.event_ge else cands[i].offset > end + ifs_bits:
                    new = True
            if new:
                events.append([cands[i].offset, chan[i], []])
            events[-1][2].append(i)
        if not events:
            tracks.append(lt.Track(*([0] * 12)))
            continue
        map_mask = 0
        for e in events:
            map_mask |= 1 << e[1]
        used = [ch for ch in range(37) if (map_mask >> ch) & 1]
        D = [events[e + 1][0] - events[e][0] for e in range(len(events) - 1)]
        qs = []                                                            # rule 4
        for d in D:
            q = (d + unit_bits // 2) // unit_bits
            if q >= 1 and abs(d - q * unit_bits) <= jitter_bits:
                qs.append(q)
        interval = functools.reduce(math.gcd, qs) if qs else 0
        timed = 6 <= interval <= 3200
        n = [0] * len(events)
        hop = u0 = n_on = n_off = n_second = tflags = 0
        unmapped = [0xFF] * len(events)
        expected = [0xFF] * len(events)
        if timed:
            P = interval * unit_bits                                       # rule 5
            for e, d in enumerate(D):
                n[e + 1] = n[e] + (d + P // 2) // P
            V = {}                                                         # rule 6
            for ch in used:
                V[ch] = {ch}
                if flags & lt.REMAP:
                    V[ch] |= {v for v in range(37) if not (map_mask >> v) & 1 and used[v % len(used)] == ch}
            S = {(h, u): sum(1 for e in range(len(events)) if (u + h * n[e]) % 37 in V[events[e][1]]) for h in range(5, 17) for u in range(37)}
            best = max(S.values())
            hop, u0 = min(k for k, s in S.items() if s == best)
            n_second = max(s for k, s in S.items() if k != (hop, u0))
            tflags = lt.TIMED | (lt.HOPPING if best > n_second else 0)
            for e, ev in enumerate(events):                                # rule 7
                unmapped[e] = (u0 + hop * n[e]) % 37
                if (map_mask >> unmapped[e]) & 1:
                    expected[e] = unmapped[e]
                elif flags & lt.REMAP:
                    expected[e] = used[unmapped[e] % len(used)]
                if expected[e] != 0xFF:
                    if expected[e] == ev[1]:
                        n_on += 1
                    else:
                        n_off += 1
        rank = {i: r for r, i in enumerate(order)}
        for e, ev in enumerate(events):
            for i in ev[2]:
                pkts[i] = lt.Pkt(rank[i], e, n[e] & 0xFFFFFFFF if timed else 0, chan[i], unmapped[e], expected[e], int(timed and expected[e] == ev[1]))
        tracks.append(lt.Track(events[0][0], map_mask, len(events), len(qs), min(interval, 0xFFFFFFFF), n_on, n_off, n_second, hop, u0,
                               len(used), tflags))
    return tracks, pkts


def one_m_durations(cands):
    return [80 + 8 * cd.length for cd in cands]


def coded_durations_of(cands):
    """Durations for a list that no stream stands behind: S = 2 at an odd offset, S = 8 at an even one."""
    return [coded_duration(2 if cd.offset & 1 else 8, cd.length) for cd in cands]


# ---- the stream of the duration tests --------------------------------------------------------------------------------------
SYM_WORDS = 700
SYM_MHZ = np.array([2440], np.uint16)


@functools.lru_cache(maxsize=None)
def symbols_lattice():
    """One data-channel stream of SYM_WORDS words of seeded noise (pitch SYM_WORDS + 9, noise behind the stream's end) with coded
    packets, each cut behind its first 400 symbols (the duration reads block 1 alone), at all 64 offset residues, S = 8 and
    S = 2, L in {0, 1, 27, 255}, ci 2 and 3, and symbol errors in and around the CI's sixteen symbols; behind them candidates
    beyond the stream and on streams out of range (end_cases() has the block 1 that ends on and past the stream's last symbol).
    -> (words (1, pitch), candidates, notes); the candidates are ungrouped (conn = the channel index)."""
    mhz = SYM_MHZ
    b = f._Builder(1, SYM_WORDS, mhz, 6161)
    rng = np.random.default_rng(62)
    ch = _le.channel_index(int(mhz[0]))
    total = 64 * SYM_WORDS
    cands, notes = [], []

    def put(offset, s, length, note, ci=None, flips=(), stream=0):
        aa, init = ld.good_aa(rng), int(rng.integers(0, 1 << 24))
        payload = rng.integers(0, 256, length, dtype=np.uint8).tobytes()
        sym = c.coded_symbols(aa, ch & 0x3F, bytes([2 if length else 1, length]) + payload, init, s, ci=ci)[:400]
        b.plant(0, offset, aa, init, s, 2 if length else 1, length, note, ci=ci, flips=flips, symbols=sym)
        cands.append(ld.Cand(offset, aa, init, stream, 2 if length else 1, length, ch))
        notes.append(note)
        return offset + len(sym)

    at = 40
    lengths = (0, 1, 27, 255)
    for r in range(64):                                                    # every residue, S and L in turn
        at += (r - at) % 64
        at = put(at, (8, 2)[r & 1], lengths[(r >> 1) & 3], "residue %d" % r) + 1
    for ci in (2, 3):
        for s in (8, 2):
            at = put(at + 3, s, 1, "ci %d sent at S = %d" % (ci, s), ci=ci)
    for k in range(12):                                                    # one to four errors inside the CI's symbols 336 .. 351
        flips = 336 + rng.choice(16, 1 + k % 4, replace=False)
        at = put(at + 5, (8, 2)[k & 1], 3, "%d CI symbol errors" % len(flips), flips=flips)
    for k in range(6):                                                     # errors that straddle the CI and its neighbours
        flips = 328 + rng.choice(32, 6, replace=False)
        at = put(at + 5, (8, 2)[k & 1], 2, "6 errors around the CI", flips=flips)
    assert at < total - 3000, at
    for off, stream, note in ((total - 79, 0, "block 1 begins one symbol past the stream"), (total + 5, 0, "an offset beyond the stream"),
                              ((1 << 40) + 77, 0, "an offset far beyond the stream"), (100, 1, "stream == n_streams"), (100, 65535, "stream 65535")):
        cands.append(ld.Cand(off, 0x8E5A3C71, 0x123456, stream, 1, 0, ch))
        notes.append(note)
    words = b.words(SYM_WORDS + 9)
    words.flags.writeable = False
    return words, tuple(cands), tuple(notes)


@functools.lru_cache(maxsize=None)
def end_cases():
    """Four short streams whose last symbol is the last, or 1, 8 or 296 symbols before the last, of a planted packet's block 1, S = 8
    and S = 2 in turn -> [(words (1, pitch), n_words, candidates)]"""
    out = []
    rng = np.random.default_rng(63)
    for k, past in enumerate((0, 1, 8, 296)):
        n_words = 12
        total = 64 * n_words
        b = f._Builder(1, n_words, SYM_MHZ, 6200 + k)
        aa, init = ld.good_aa(rng), int(rng.integers(0, 1 << 24))
        s = (8, 2)[k & 1]
        o = total - 376 + past
        b.plant(0, o, aa, init, s, 1, 0, "ends %d past" % past, symbols=c.coded_symbols(aa, 17, bytes([1, 0]), init, s)[:400])
        words = b.words(n_words + 2)
        words.flags.writeable = False
        out.append((words, n_words, (ld.Cand(o, aa, init, 0, 1, 0, 17), ld.Cand(3, aa, init, 0, 1, 0, 17))))
    return out


# ---- the lists of the flag-pass tests, built without any stream ------------------------------------------------------------
REQ, REPLY = coded_duration(8, 0), coded_duration(2, 3)                   # 720 and 510 symbols


class _Laid:
    """Connections laid back to back on ascending access addresses (the grouping numbers them, and the tracking lays their slots
    out, in that order): self.slot is the slot the next one begins at.  Every candidate carries its duration."""

    def __init__(self):
        self.raw, self.dur, self.names, self.slot, self.k = [], {}, {}, 0, 0

    def conn(self, name, pkts):
        """pkts: (offset, stream, length, duration); a stream that is no data channel of lt.LATTICE_MHZ makes a non-member."""
        self.k += 1
        aa, ci = 0x20000000 + 0x1000 * self.k, (0x0A0B0C + 0x010203 * self.k) & 0xFFFFFF
        self.names[(aa, ci)] = name
        for o, s, n, dur in pkts:
            cd = ld.Cand(o, aa, ci, s, 1 if n == 0 else 2, n, _le.channel_index(int(lt.LATTICE_MHZ[s])) if s < lt.N_STREAMS else 0)
            self.raw.append(cd)
            self.dur[cd[:6]] = dur
            if s < lt.N_STREAMS and _le.channel_index(int(lt.LATTICE_MHZ[s])) < 37:
                self.slot += 1
        return self

    def events(self, name, n_events, h, u0, first=2, interval=6, base=4000):
        """Coded connection events on channel selection #1: a request (S = 8, empty) and a reply 150 symbols behind its end (S = 2,
        three octets); the first event has `first` packets (3: a second reply)."""
        pkts = []
        for n in range(n_events):
            ch = lt.csa1_at(u0, h, n, lt.FULL_MAP)
            at = base + n * interval * UNIT
            pkts.append((at, ch, 0, REQ))
            pkts.append((at + REQ + 150, ch, 3, REPLY))
            if n == 0 and first == 3:
                pkts.append((at + REQ + 150 + REPLY + 150, ch, 3, REPLY))
        return self.conn(name, pkts)

    def grouped(self, seed):
        rng = np.random.default_rng(seed)
        raw = [self.raw[i] for i in rng.permutation(len(self.raw))]
        conns, cands = ld.group(raw, 2)
        return conns, cands, [self.dur[cd[:6]] for cd in cands], [self.names[(x.access_address, x.crc_init)] for x in conns]


@functools.lru_cache(maxsize=None)
def flag_list():
    """-> (conns, cands, durations, names).  Slots: "wave a" 0 .. 79 (slot 63 a reply, 64 the next request), "wave b" from 80 with
    three packets in its first event (slot 127 a request, 128 its reply), "tile a" from 141 (2047 a request, 2048 its reply),
    "tile b" from 2341 with three packets first (4095 a reply, 4096 the next request); behind them the branch points of rule 3."""
    b = _Laid()
    b.events("wave a", 40, 7, 3)
    assert b.slot == 80
    b.events("wave b", 30, 11, 20, first=3)
    assert b.slot == 141
    b.events("tile a", 1100, 5, 9)
    assert b.slot == 2341
    b.events("tile b", 1000, 13, 30, first=3, interval=7)
    assert b.slot == 4342
    far = 40 * UNIT
    b.conn("gap of ifs: one event", [(1000, 3, 0, REQ), (1000 + REQ + IFS, 3, 3, REPLY), (1000 + far, 3, 0, REQ)])
    b.conn("gap of ifs + 1: two events", [(1000, 3, 0, REQ), (1000 + REQ + IFS + 1, 3, 3, REPLY), (1000 + far, 3, 0, REQ)])
    b.conn("duration 0, gap of ifs", [(1000, 5, 0, 0), (1000 + IFS, 5, 0, 0), (1000 + far, 5, 0, REQ)])
    b.conn("duration 0, gap of ifs + 1", [(1000, 5, 0, 0), (1000 + IFS + 1, 5, 0, 0), (1000 + far, 5, 0, REQ)])
    long_d = coded_duration(8, 255)
    assert long_d == 17040
    b.conn("17040 symbols reach past the next start", [(1000, 8, 255, long_d), (6000, 8, 0, REQ), (6000 + REQ + IFS + 1, 8, 0, REQ),
                                                         (1000 + long_d + IFS, 8, 0, REQ)])
    b.conn("17040 symbols, gap of ifs and of ifs + 1", [(1000, 8, 255, long_d), (1000 + long_d + IFS, 8, 0, REQ), (1000 + far, 8, 255, long_d),
                                                          (1000 + far + long_d + IFS + 1, 8, 0, REQ)])
    b.conn("channel change inside the gap", [(1000, 9, 0, REQ), (1000 + REQ + 150, 10, 3, REPLY), (1000 + far, 9, 0, REQ)])
    b.conn("a non-member between two members", [(1000, 12, 0, REQ), (1000 + REQ + 10, 37, 0, 0), (1000 + REQ + 20, 40, 0, 0),
                                                (1000 + REQ + 150, 12, 3, REPLY), (1000 + far, 12, 0, REQ)])
    top = (1 << 48) - (1 << 32)
    b.conn("end carries across 2^32", [(top - 300, 14, 0, REQ), (top - 300 + REQ + 150, 14, 3, REPLY), (top + 6 * UNIT - 300, 20, 0, REQ),
                                       (top + 6 * UNIT - 300 + REQ + IFS + 1, 20, 3, REPLY), (top - 6 * UNIT - 300, 2, 0, REQ)])
    b.conn("end reaches 2^32 exactly", [((1 << 32) - REQ, 15, 0, REQ), ((1 << 32) + IFS, 15, 3, REPLY), ((1 << 32) + far, 15, 0, REQ)])
    return b.grouped(17)


# ---- the chain capture -----------------------------------------------------------------------------------------------------
CHAIN_CHANNELS = (0, 4, 9, 13, 18, 22, 27, 36)
CHAIN_MAP = c2.mask_of(CHAIN_CHANNELS)
CHAIN_EVENTS = 13
Planted = collections.namedtuple("Planted", "aa crc_init interval algorithm hop u0 counter0 counters")
CHAIN_SEEDS = (1, 1)                                                       # (tests/test_le_ctrack_model.py shows what they give)


@functools.lru_cache(maxsize=None)
def chain_capture(seeds=CHAIN_SEEDS):
    """Two coded connections over eight data-channel streams of 1600 words of noise, interval 6, CHAIN_EVENTS events each, every
    event a request (S = 8, empty) and a reply 150 symbols behind its end (S = 2, three octets): the first hops by algorithm #1
    (lt.csa1), the second by algorithm #2 (c2.csa2) from a planted counter.  -> (Capture, planted)"""
    mhz = np.array([lt.DATA_MHZ[ch] for ch in CHAIN_CHANNELS], np.uint16)
    n_words = 1600
    b = f._Builder(8, n_words, mhz, 7070)
    planted = []
    for k, seed in enumerate(seeds):
        rng = np.random.default_rng(1000 * (k + 1) + seed)
        aa, init = ld.good_aa(rng), int(rng.integers(0, 1 << 24))
        hop, u0, counter0 = int(rng.integers(5, 17)), int(rng.integers(0, 37)), int(rng.integers(0, 1 << 16))
        base = 300 + 3000 * k
        for n in range(CHAIN_EVENTS):
            ch = lt.csa1(u0, hop, n, CHAIN_MAP) if k == 0 else c2.csa2(aa, counter0 + n, CHAIN_MAP)
            s = CHAIN_CHANNELS.index(ch)
            at = base + n * 6 * UNIT + int(rng.integers(-20, 21))
            at = b.plant(s, at, aa, init, 8, 1, 0, "connection %d request" % k)
            b.plant(s, at + 150, aa, init, 2, 2, 3, "connection %d reply" % k)
        planted.append(Planted(aa, init, 6, 1 + k, hop, u0, counter0, tuple(range(CHAIN_EVENTS))))
    words = b.words(n_words + 3)
    words.flags.writeable = False
    return f.Capture(words, n_words, n_words + 3, 64 * n_words - 335, mhz, b.planted), tuple(planted)


@functools.lru_cache(maxsize=None)
def chain_model(flags=lt.REMAP):
    """The chain on the chain capture, every stage by its model: (conns, cands, info by (stream, offset), durations, tracks, pkts,
    sels, sel_pkts)."""
    cap, _ = chain_capture()
    found = cap.candidates(27, 16)
    info = {(cd.stream, cd.offset): i for cd, i in found}
    conns, cands = ld.group([cd for cd, _ in found], 2)
    durations = symbols(cap.words, cap.n_words, cands, len(cap.mhz))
    tracks, pkts = track(cands, len(conns), cap.mhz, len(cap.mhz), UNIT, IFS, JITTER, flags, durations)
    sels, sel_pkts = c2.select(conns, cands, tracks, pkts, flags)
    return conns, cands, info, durations, tracks, pkts, sels, sel_pkts
