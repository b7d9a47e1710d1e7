"""Test-side model of the LE connection tracking (include/btbbx.h btbbx_le_track_*), written from the seven rules
of the contract in plain Python -- sorted(), a loop, math.gcd and a dictionary of scores over all 444 (hop increment, first
unmapped channel) pairs --, not from the kernels (le_track.h sorts by radix passes and votes into histograms).

* track: the model; Rules: its branch points as options, Rules() is the model, any other value a deliberately wrong one
  (tests/test_le_track_model.py shows that the lattice below tells each from the right one)
* csa1: the FORWARD channel selection algorithm #1 (Core v5.x Vol 6 Part B 4.5.8.2), written from the specification, one
  event after the other; it shares nothing with the model's inverse
* synth / lattice / seam_list / chain_capture: the lists and the capture the CPU and GPU tests share
* align_list / crowd_list / long_event_list: lists laid out on the kernels' waves, workgroups and tiles, for the path model of
  tests/_le_track_paths.py
"""
import collections
import functools
import math

import numpy as np

import _le
import _le_discover as ld

REMAP = 1
TIMED, HOPPING = 1, 2
DATA_MHZ = tuple(m for m in range(2404, 2480, 2) if m != 2426)        # data channel index c -> MHz
assert len(DATA_MHZ) == 37 and all(_le.channel_index(m) == c for c, m in enumerate(DATA_MHZ))

Track = collections.namedtuple("Track", "first_anchor map_mask n_events n_fit interval n_on_hop n_off_hop n_second hop_increment "
                               "first_unmapped n_used flags")
Pkt = collections.namedtuple("Pkt", "rank event counter channel unmapped expected on_hop")


class Rules:
    def __init__(self, **kw):
        self.event_ge = False            # a new event at offset >= end + ifs
        self.event_channel = True        # a channel change opens an event
        self.q_floor = False             # q_e by floor
        self.fit_strict = False          # the fit test with <
        self.interval_min = False        # min instead of gcd
        self.valid = (6, 3200)
        self.k_floor = False             # k_e by floor
        self.h_range = (5, 16)
        self.tie_h_largest = False
        self.tie_u_largest = False
        self.remap_mod37 = False         # the remapping index is v mod 37 (clamped to the table) instead of v mod n_used
        self.remap_descending = False    # the table of used channels in descending order
        self.second_other_h = False      # n_second over pairs with another h only
        self.count_packets = False       # scores and tallies count packets, not events
        self.tie_unstable = False        # members at one (offset, stream) in descending order of their index
        self.hop_truncated = False       # rule 7's unmapped channel from the counter as it is stored, 32 bits of it
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


MODEL = Rules()
VARIANTS = dict(event_ge=dict(event_ge=True), event_no_channel=dict(event_channel=False), q_floor=dict(q_floor=True),
                fit_strict=dict(fit_strict=True), interval_min=dict(interval_min=True), valid_from_5=dict(valid=(5, 3200)),
                valid_to_3199=dict(valid=(6, 3199)), k_floor=dict(k_floor=True), h_0_36=dict(h_range=(0, 36)),
                tie_h_largest=dict(tie_h_largest=True), tie_u_largest=dict(tie_u_largest=True), remap_mod37=dict(remap_mod37=True),
                remap_descending=dict(remap_descending=True), second_other_h=dict(second_other_h=True),
                count_packets=dict(count_packets=True), tie_unstable=dict(tie_unstable=True),
                hop_from_truncated_counter=dict(hop_truncated=True))


def _remap(v, used, rules):
    if rules.remap_mod37:
        return used[min(v % 37, len(used) - 1)]
    return used[v % len(used)]


def track(cands, n_conns, mhz, n_streams, unit_bits, ifs_bits, jitter_bits, flags, rules=MODEL):
    """cands: the candidates worked on (Cand tuples of tests/_le_discover.py, `channel` holding the connection index), n_conns:
    the stored connections.  Returns (tracks, pkts): one Track per connection, one Pkt or None (no member) per candidate."""
    members = [[] for _ in range(n_conns)]
    chan = {}
    for i, c in enumerate(cands):                                          # rule 1
        if c.channel < n_conns and c.stream < n_streams:
            ch = _le.channel_index(int(mhz[c.stream]))
            if ch < 37:
                members[c.channel].append(i)
                chan[i] = ch
    pkts = [None] * len(cands)
    tracks = []
    for g in range(n_conns):
        order = sorted(members[g], key=lambda i: (cands[i].offset, cands[i].stream, -i if rules.tie_unstable else i))   # rule 2
        events = []                                                        # rule 3: [anchor, channel, [members]]
        for r, i in enumerate(order):
            c = cands[i]
            new = r == 0
            if not new:
                p = cands[order[r - 1]]
                end = p.offset + 80 + 8 * p.length
                if rules.event_channel and chan[i] != chan[order[r - 1]]:
                    new = True
                if c.offset >= end + ifs_bits if rules.event_ge else c.offset > end + ifs_bits:
                    new = True
            if new:
                events.append([c.offset, chan[i], []])
            events[-1][2].append(i)
        if not events:
            tracks.append(Track(*([0] * 12)))
            continue
        map_mask = 0
        for e in events:
            map_mask |= 1 << e[1]
        used = [c for c in range(37) if (map_mask >> c) & 1]
        D = [events[e + 1][0] - events[e][0] for e in range(len(events) - 1)]
        qs = []                                                            # rule 4
        for d in D:
            q = d // unit_bits if rules.q_floor else (d + unit_bits // 2) // unit_bits
            rem = abs(d - q * unit_bits)
            if q >= 1 and (rem < jitter_bits if rules.fit_strict else rem <= jitter_bits):
                qs.append(q)
        interval = 0
        if qs:
            interval = min(qs) if rules.interval_min else functools.reduce(math.gcd, qs)
        timed = rules.valid[0] <= interval <= rules.valid[1]
        n = [0] * len(events)
        hop = u0 = n_on = n_off = n_second = 0
        tflags = 0
        unmapped = [0xFF] * len(events)
        expected = [0xFF] * len(events)
        if timed:
            P = interval * unit_bits                                       # rule 5
            for e, d in enumerate(D):
                n[e + 1] = n[e] + (d // P if rules.k_floor else (d + P // 2) // P)
            table = used[::-1] if rules.remap_descending else used
            V = {}                                                         # rule 6
            for c in used:
                V[c] = {c}
                if flags & REMAP:
                    V[c] |= {v for v in range(37) if not (map_mask >> v) & 1 and _remap(v, table, rules) == c}
            weight = [len(e[2]) if rules.count_packets else 1 for e in events]
            S = {}
            for h in range(rules.h_range[0], rules.h_range[1] + 1):
                for u in range(37):
                    S[(h, u)] = sum(w for e, w in zip(range(len(events)), weight) if (u + h * n[e]) % 37 in V[events[e][1]])
            best = max(S.values())
            winners = [k for k, s in S.items() if s == best]
            hop = (max if rules.tie_h_largest else min)(k[0] for k in winners)
            u0 = (max if rules.tie_u_largest else min)(k[1] for k in winners if k[0] == hop)
            n_second = max(s for k, s in S.items() if (k[0] != hop if rules.second_other_h else k != (hop, u0)))
            tflags = TIMED | (HOPPING if best > n_second else 0)
            for e, ev in enumerate(events):                                # rule 7
                unmapped[e] = (u0 + hop * (n[e] & 0xFFFFFFFF if rules.hop_truncated else n[e])) % 37
                if (map_mask >> unmapped[e]) & 1:
                    expected[e] = unmapped[e]
                elif flags & REMAP:
                    expected[e] = _remap(unmapped[e], table, rules)
                if expected[e] != 0xFF:
                    if expected[e] == ev[1]:
                        n_on += weight[e]
                    else:
                        n_off += weight[e]
        rank = {i: r for r, i in enumerate(order)}
        for e, ev in enumerate(events):
            for i in ev[2]:
                pkts[i] = Pkt(rank[i], e, n[e] & 0xFFFFFFFF if timed else 0, chan[i], unmapped[e], expected[e],
                              int(timed and expected[e] == ev[1]))
        tracks.append(Track(events[0][0], map_mask, len(events), len(qs), min(interval, 0xFFFFFFFF), n_on, n_off, n_second, hop, u0,
                            len(used), tflags))
    return tracks, pkts


def track_array(tracks, dtype):
    a = np.zeros(len(tracks), dtype)
    for i, t in enumerate(tracks):
        a[i] = tuple(t) + (0,)
    return a


def pkt_array(pkts, dtype):
    a = np.zeros(len(pkts), dtype)
    if not len(pkts):
        return a
    none = np.array([p is None for p in pkts], bool)
    rows = np.array([(0,) * len(Pkt._fields) if p is None else p for p in pkts], np.int64)
    for k, name in enumerate(Pkt._fields):
        a[name] = rows[:, k]
    a.view(np.uint8).reshape(len(pkts), dtype.itemsize)[none] = 0xFF
    return a


# ---- the forward channel selection ----------------------------------------------------------------------------------
def csa1(u0, h, n, chmap):
    """Channel selection algorithm #1: the data channel index of the n-th event behind the one whose unmappedChannel was u0.
    unmappedChannel = (lastUnmappedChannel + hopIncrement) mod 37, event after event; a used channel is taken as it is, an
    unused one is replaced by entry (unmappedChannel mod numUsedChannels) of the used channels in ascending order."""
    unmapped = u0
    for _ in range(n):
        unmapped = (unmapped + h) % 37
    if (chmap >> unmapped) & 1:
        return unmapped
    table = [c for c in range(37) if (chmap >> c) & 1]
    return table[unmapped % len(table)]


def csa1_at(u0, h, n, chmap):
    """csa1 without the walk over the events, for counters the walk cannot reach (tests/test_le_track_paths_model.py holds the
    two against each other)."""
    unmapped = (u0 + h * n) % 37
    if (chmap >> unmapped) & 1:
        return unmapped
    table = [c for c in range(37) if (chmap >> c) & 1]
    return table[unmapped % len(table)]


def synth(rng, n_events, chmap, interval, h, u0, loss=0.0, jitter=0, unit=1250, base=5000, aa=0x52A3C6D1, crc_init=0x3B5A17,
          conn=0, per_event=1, gap=150, lengths=(0,), stream_of=None):
    """The packets of a planted connection as Cand tuples (`channel` = conn, as the grouping leaves it): event n lies at
    base + n * interval * unit (+- jitter) on csa1(u0, h, n, chmap), and is lost as a whole with probability `loss`.  Returns
    (cands, seen): seen = the event counters that were not lost."""
    out, seen = [], []
    for n in range(n_events):
        if loss and rng.random() < loss:
            continue
        ch = csa1(u0, h, n, chmap)
        at = base + n * interval * unit + (int(rng.integers(-jitter, jitter + 1)) if jitter else 0)
        seen.append(n)
        for k in range(per_event):
            length = lengths[(n + k) % len(lengths)]
            out.append(ld.Cand(at, aa, crc_init, ch if stream_of is None else stream_of(ch, n, k), 1 if length == 0 else 2, length, conn))
            at += 80 + 8 * length + gap
    return out, seen


def popcount(x):
    return bin(x).count("1")


def random_map(rng, n_used):
    m = 0
    for c in rng.permutation(37)[:n_used]:
        m |= 1 << int(c)
    return m


# ---- the hand-built lattice -------------------------------------------------------------------------------------------
# Streams: 0..36 the data channels in order, 37 = 2402 MHz (advertising), 38 = channel 5 once more (two streams at one MHz),
# 39 = 2426 MHz (advertising).  N_STREAMS = 40; stream numbers >= 40 are out of range.
LATTICE_MHZ = np.array(DATA_MHZ + (2402, DATA_MHZ[5], 2426), np.uint16)
N_STREAMS = 40
UNIT, IFS, JITTER = 1250, 200, 50

Case = collections.namedtuple("Case", "name cands")
TIE_CASES = ("tie at one offset, long packet first", "tie at one offset, short packet first")
BEYOND_32 = (0, 1, 2, 3, (1 << 32) + 5, (1 << 32) + 6, (1 << 32) + 7, (1 << 32) + 9)


def _conn_ids():
    k = 0
    while True:
        k += 1
        yield 0x50000000 + 0x01010101 * (k % 7) + 0x1000 * k, (0x123456 + 0x010203 * k) & 0xFFFFFF


@functools.lru_cache(maxsize=None)
def lattice():
    """The hand-built connections of the tracking tests, one per branch point of the seven rules: a tuple of Case.  Every case is
    one (access address, CRCInit) group of ungrouped Cand tuples (`channel` = the data channel index, as the scan leaves it)."""
    rng = np.random.default_rng(11)
    ids = _conn_ids()
    cases = []
    full = (1 << 37) - 1

    def add(name, pkts):
        aa, ci = next(ids)
        cases.append(Case(name, tuple(ld.Cand(o, aa, ci, s, 1 if n == 0 else 2, n, _le.channel_index(int(LATTICE_MHZ[s])) if s < N_STREAMS else 0)
                                      for o, s, n in pkts)))

    def hop_events(n_events, chmap, interval, h, u0, base=3000, skip=(), counters=None, jit=None):
        out = []
        for n in (counters if counters is not None else range(n_events)):
            if n in skip:
                continue
            at = base + n * interval * UNIT + (jit(n) if jit else 0)
            out.append((at, csa1(u0, h, n, chmap), 0))
        return out

    # rule 3: one, two and three events; the gap at exactly ifs and one beyond; same-channel packets further apart
    add("one event, one packet", [(700, 3, 0)])
    add("one event, three packets", [(700, 3, 0), (700 + 80 + IFS, 3, 2), (700 + 80 + IFS + 96 + IFS, 3, 0)])
    add("gap of ifs + 1: two events", [(700, 3, 0), (700 + 80 + IFS + 1, 3, 2)])
    add("gap of ifs behind a long packet", [(700, 3, 27), (700 + 80 + 216 + IFS, 3, 0), (700 + 80 + 216 + IFS + 80 + IFS + 1, 3, 0)])
    add("same channel, far apart", [(1000, 9, 0), (1000 + 7 * 6 * UNIT, 9, 0), (1000 + 14 * 6 * UNIT, 9, 0)])
    add("channel change inside ifs", [(1000, 9, 0), (1100, 10, 0), (1000 + 6 * UNIT, 20, 0), (1000 + 12 * UNIT, 31, 0)])
    add("two channels at one offset", [(2000, 4, 0), (2000, 7, 0), (2000 + 8 * UNIT, 11, 0), (2000 + 16 * UNIT, 18, 0)])
    add("two streams at one MHz", [(2000, 5, 0), (2000 + 150, 38, 0), (2000 + 10 * UNIT, 38, 0), (2000 + 20 * UNIT, 5, 0),
                                   (2000 + 20 * UNIT, 38, 0)])
    add("three events", hop_events(3, full, 9, 7, 4))
    add("two events", hop_events(2, full, 9, 7, 4))
    # rule 4: the remainder at jitter and one beyond, on both sides; D at half a unit, both rounding directions
    for name, d in (("remainder +jitter", 7 * UNIT + JITTER), ("remainder +jitter+1", 7 * UNIT + JITTER + 1),
                    ("remainder -jitter", 7 * UNIT - JITTER), ("remainder -jitter-1", 7 * UNIT - JITTER - 1),
                    ("half a unit down", 7 * UNIT + UNIT // 2 - 1), ("half a unit up", 7 * UNIT + UNIT // 2),
                    ("below one unit", UNIT // 2 - 1), ("rounds to one unit", UNIT - JITTER)):
        add(name, [(4000, 1, 0), (4000 + d, 13, 0), (4000 + d + 14 * UNIT, 25, 0), (4000 + d + 35 * UNIT, 2, 0)])
    add("no fitting pair", [(4000, 1, 0), (4000 + 3 * UNIT + 300, 13, 0), (4000 + 9 * UNIT + 900, 25, 0)])
    add("min is not the gcd", hop_events(0, full, 6, 11, 3, counters=(0, 3, 5, 9, 10, 14)))
    add("one pair fits by rounding only", [(4000, 1, 0), (4000 + 12 * UNIT, 13, 0), (4000 + 12 * UNIT + 18 * UNIT + UNIT // 2 + 40, 25, 0),
                                           (4000 + 48 * UNIT + UNIT // 2 + 40, 2, 0)])
    # the validity range
    for iv in (5, 6, 3200, 3201):
        add("interval %d" % iv, hop_events(6, full, iv, 9, 0))
    # rule 5: D at half an interval, both rounding directions; missed events
    for name, d in (("half an interval down", 10 * 3 + 4), ("half an interval up", 10 * 3 + 5)):
        add(name, [(6000, 0, 0), (6000 + 10 * UNIT, 7, 0), (6000 + 20 * UNIT, 14, 0), (6000 + (20 + d) * UNIT, 2, 0),
                   (6000 + (30 + d) * UNIT, 9, 0)])
    for k in (2, 36, 37, 38):
        add("missed events, k = %d" % k, hop_events(0, full, 7, 13, 21, counters=(0, 1, 2, 3, 3 + k, 4 + k, 5 + k, 6 + k)))
    # rule 6: all twelve increments; the maps; ties
    for h in range(5, 17):
        add("increment %d" % h, hop_events(14, full, 6 + h, h, (3 * h) % 37, jit=lambda n: (n * 17) % 41 - 20))
    for n_used in (37, 36, 3, 2, 1):
        chmap = random_map(rng, n_used)
        add("map of %d" % n_used, hop_events(45, chmap, 8, 5 + n_used % 12, 6))
    add("map of 3, sparse", hop_events(0, 0b1001001 << 9, 8, 12, 30, counters=(0, 1, 2, 5, 11, 12, 30)))
    add("tie between two u", [(8000, 0, 0), (8000 + 10 * UNIT, 0, 0)])                        # one channel: every u that remaps ...
    add("tie between two h", [(8000, 3, 0), (8000 + 10 * UNIT, 30, 0), (8000 + 47 * 10 * UNIT, 4, 0)])
    add("events off the hop", hop_events(20, full, 10, 6, 2) + [(3000 + 3 * 10 * UNIT + 400, 33, 0), (3000 + 25 * 10 * UNIT, 1, 0)])
    add("two packets per event", [(o + k * 230, s, (0, 5)[k]) for o, s, _ in hop_events(9, full, 6, 16, 36) for k in range(2)])
    # offsets near 2^46
    add("offsets near 2^46", hop_events(8, full, 24, 8, 19, base=(1 << 46) - 8 * 24 * UNIT - 5000))
    add("two events 2^40 bits apart", [(1000, 2, 0), (1000 + (1 << 40), 9, 0)])                # (unit_bits 2: a gcd beyond 32 bits)
    # rule 1: a stream out of range and an advertising stream among the members
    add("foreign streams among the members", hop_events(7, full, 6, 10, 5) + [(3000 + 2 * 6 * UNIT + 90, 40, 0), (3000 + 3 * 6 * UNIT + 90, 37, 0),
                                                                              (3000 + 4 * 6 * UNIT + 90, 39, 0), (3000 + 5 * 6 * UNIT, 65535, 0)])
    add("only foreign streams", [(100, 37, 0), (100 + 6 * UNIT, 41, 0)])
    # rule 2: two members at one (offset, stream) stand in list order.  The packet behind them lies within ifs of the end of the long
    # one and beyond ifs of the end of the short one: one event where the long one is the later of the two, two where it is not
    # (lattice_list keeps the order the case names, whatever its shuffle does)
    add(TIE_CASES[0], [(9000, 6, 27), (9000, 6, 0), (9000 + 80 + 216 + IFS, 6, 0)])
    add(TIE_CASES[1], [(9000, 6, 0), (9000, 6, 27), (9000 + 80 + 216 + IFS, 6, 0)])
    # rule 5 / 7: event counters beyond 2^32 (2^32 mod 37 = 7: the hop needs the whole count, the record stores 32 bits of it)
    add("counter beyond 2^32", [(3000 + n * 6 * UNIT, csa1_at(29, 7, n, full), 0) for n in BEYOND_32])
    return tuple(cases)


def lattice_list(min_count=1, noise=40, seed=3):
    """The lattice as one candidate list: every case's packets, `noise` single candidates between them (non-members at
    min_count 2), shuffled, then grouped by the discovery's model.  Returns (conns, cands, names): names[g] = the case of
    connection g (None: noise)."""
    rng = np.random.default_rng(seed)
    raw, by_key = [], {}
    for case in lattice():
        raw += list(case.cands)
        by_key[(case.cands[0].access_address, case.cands[0].crc_init)] = case.name
    for k in range(noise):
        raw.append(ld.Cand(int(rng.integers(0, 1 << 24)), 0x40000000 + 0x2F1 * k + int(rng.integers(0, 1 << 28)), int(rng.integers(0, 1 << 24)),
                           int(rng.integers(0, 37)), 1, 0, 0))
        raw[-1] = raw[-1]._replace(channel=raw[-1].stream)
    raw = [raw[i] for i in rng.permutation(len(raw))]
    for case in lattice():                                                 # the tied pairs: in the order their case lists them
        if case.name in TIE_CASES:
            i, j = raw.index(case.cands[0]), raw.index(case.cands[1])
            if i > j:
                raw[i], raw[j] = raw[j], raw[i]
    conns, cands = ld.group(raw, min_count)
    return conns, cands, [by_key.get((c.access_address, c.crc_init)) for c in conns]


def lattice_tracks(flags, rules=MODEL, min_count=2):
    conns, cands, names = lattice_list(min_count)
    tracks, pkts = track(cands, len(conns), LATTICE_MHZ, N_STREAMS, UNIT, IFS, JITTER, flags, rules)
    return names, tracks, pkts


# ---- sizes that cross the kernels' seams ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam_list():
    """One connection of 5 000 events with two packets each beside 3 000 connections of 2 to 4 events: (conns, cands)."""
    rng = np.random.default_rng(21)
    raw, _ = synth(rng, 5000, (1 << 37) - 1, 6, 11, 8, jitter=20, aa=0x8E5A3C71, crc_init=0x5EED01, per_event=2, lengths=(0, 3))
    raw = [c._replace(channel=c.stream) for c in raw]
    for k in range(3000):
        iv = 6 + k % 30
        sm, _ = synth(rng, 2 + k % 3, random_map(rng, 37 if k % 4 else 5), iv, 5 + k % 12, k % 37, jitter=20, base=4000 + 97 * k,
                      aa=0x10000000 + 600 * int(rng.integers(0, 1 << 21)), crc_init=(7 * k + 1) & 0xFFFFFF)
        raw += [c._replace(channel=c.stream) for c in sm]
    raw = [raw[i] for i in rng.permutation(len(raw))]
    return ld.group(raw, 2)


# ---- the chain capture --------------------------------------------------------------------------------------------------
Planted = collections.namedtuple("Planted", "aa crc_init interval hop u0 chmap counters")


@functools.lru_cache(maxsize=None)
def chain_capture():
    """37 data-channel streams (stream c = channel c) and one advertising stream of 4 600 words of noise (38 events of interval
    6, which it takes to see all 37 channels, are 285 000 bits) with four planted connections: interval 6 on all channels with two
    packets per event 150 bits apart; interval 12 on a three-channel map, all its packets alike, which gives it a shifted alias on channel 3; interval 10 on a five-channel map with one event left
    out; one seen only at two events two intervals apart.  Returns (Capture, planted)."""
    n_words = 4600
    mhz = np.array(DATA_MHZ + (2402,), np.uint16)
    b = ld._Builder(38, n_words, mhz, 9090)
    rng = np.random.default_rng(91)
    total = 64 * n_words
    plans = [dict(interval=6, hop=7, u0=11, chmap=(1 << 37) - 1, counters=range(38), per_event=2),
             dict(interval=12, hop=13, u0=2, chmap=(1 << 3) | (1 << 17) | (1 << 30), counters=range(19), per_event=1, same=True),
             dict(interval=10, hop=5, u0=30, chmap=(1 << 1) | (1 << 8) | (1 << 19) | (1 << 25) | (1 << 33), counters=[n for n in range(22) if n != 5], per_event=1),
             dict(interval=7, hop=9, u0=0, chmap=(1 << 37) - 1, counters=(3, 5), per_event=1)]
    planted = []
    for k, p in enumerate(plans):
        aa, ci = ld.good_aa(rng), int(rng.integers(0, 1 << 24))
        # The second connection sends one packet again and again (h0 1, seventeen octets, the first of them 1) under an AA whose
        # three lowest bits are 101.  On channel 3 that packet is a candidate once more two bits later: bits 2 .. 9 alternate, the
        # AA read there (AA >> 2 with the first two whitened header bits, 0 and 1, on top) is made to have no offense, and the
        # header read there dewhitens to h0 0x1d and length 8 -- a shifted alias that ends inside the packet, so
        # that all its copies agree on a CRCInit and form a group.
        while p.get("same") and not ((aa & 7) == 5 and ld._offenses(aa) == 0 and ld._offenses((aa >> 2) | (1 << 31)) == 0):
            aa = (int(rng.integers(0, 1 << 32)) & ~7) | 5
        base = 900 + 2111 * k
        for n in p["counters"]:
            ch = csa1(p["u0"], p["hop"], n, p["chmap"])
            at = base + n * p["interval"] * UNIT + int(rng.integers(-20, 21))
            for j in range(p["per_event"]):
                length = 17 if p.get("same") else (0, 9, 3)[(n + j) % 3]
                assert at + 80 + 8 * length <= total
                b.plant(ch, at, aa, ci, 1 if length in (0, 17) else 2, length, "connection %d" % k,
                        payload=bytes(range(1, 18)) if p.get("same") else None)
                at += 80 + 8 * length + 150
        planted.append(Planted(aa, ci, p["interval"], p["hop"], p["u0"], p["chmap"], tuple(p["counters"])))
    # a valid data packet on the advertising stream: no candidate
    b.plant(37, 5000, planted[0].aa, planted[0].crc_init, 1, 0, "advertising channel")
    words = b.words(n_words + 5)
    words.flags.writeable = False
    return ld.Capture(words, n_words, n_words + 5, total - 39, mhz, tuple(b.planted), 27), tuple(planted)


@functools.lru_cache(maxsize=None)
def chain_model():
    """(conns, cands) of the discovery's model on the chain capture, min_count 2."""
    cap, _ = chain_capture()
    return ld.group(ld.capture_candidates(cap, 27), 2)


# ---- lists on the alignments of the kernels' waves, workgroups and tiles ------------------------------------------------------
# tests/_le_track_paths.py works out, from the model's own slot and event numbering, which paths of le_track.h a list drives.
# The grouping numbers the connections by (access address, CRCInit) and the tracking lays their slots and events out in that order,
# so a builder that hands out ascending access addresses decides where every connection begins.
FULL_MAP = (1 << 37) - 1
FIVE_MAP = (1 << 1) | (1 << 8) | (1 << 19) | (1 << 25) | (1 << 33)
OFF_HOP_EVENTS = 400
LT_SCORE_ALIGN = 1024                      # LT_SCORE_TILE of le_track.h (tests/test_le_track_paths_model.py holds the two together)


def off_hop_plan(slot0):
    """The events of the "off hop" connection of align_list (OFF_HOP_EVENTS events of two packets, the first at slot slot0) that are
    put one channel up: one in its first wave of slots and up to two in its last, which it shares with others; five in its second
    wave, one in its third, none in the rest, which are its own."""
    s, last = slot0 % 64, (slot0 % 64 + 2 * OFF_HOP_EVENTS - 1) // 64
    assert 0 < s <= 62 and (s + 2 * OFF_HOP_EVENTS) % 64 > 1 and last >= 5
    first_of = lambda k: (64 * k - s + 1) // 2                                  # noqa: E731  (the first event that opens in wave k)
    return (0,) + tuple(first_of(1) + i for i in (2, 5, 9, 20, 30)) + (first_of(2) + 7,) + tuple(range(max(first_of(last), OFF_HOP_EVENTS - 2), OFF_HOP_EVENTS))


class _Laid:
    """Connections laid back to back: conn() plants the next one (interval 6, stream = data channel index), on the next access
    address; self.ev and self.slot are the event and the slot it will begin at (stream c of LATTICE_MHZ is data channel c)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.raw, self.names, self.ev, self.slot, self.k = [], {}, 0, 0, 0

    def conn(self, name, counters, chmap=FULL_MAP, interval=6, h=7, u0=0, per_event=1, off_hop=(), jitter=20, gap=150, base=None):
        """Events with these counters, per_event packets `gap` bits apart in each; the events whose place in `counters` is in off_hop
        lie one channel up."""
        if isinstance(counters, int):
            counters = range(counters)
        self.k += 1
        aa, ci = 0x20000000 + 0x1000 * self.k, (0x0A0B0C + 0x010203 * self.k) & 0xFFFFFF
        self.names[(aa, ci)] = name
        base = 4000 + 97 * self.k if base is None else base
        for e, n in enumerate(counters):
            ch = csa1_at(u0, h, n, chmap)
            if e in off_hop:
                ch = (ch + 1) % 37
            at = base + n * interval * UNIT + (int(self.rng.integers(-jitter, jitter + 1)) if jitter else 0)
            for j in range(per_event):
                length = (0, 3)[(e + j) % 2]
                self.raw.append(ld.Cand(at, aa, ci, ch, 1 if length == 0 else 2, length, ch))
                at += 80 + 8 * length + gap
        self.ev += len(counters)
        self.slot += len(counters) * per_event
        return self

    def pad(self, unit, rest=0):
        """A filler connection that ends with the event count at `rest` modulo `unit` (two packets per event)."""
        n = (rest - self.ev) % unit
        if n:
            self.conn("filler", n, h=5 + self.k % 12, u0=self.k % 37, per_event=2)
        return self

    def lone(self, n):
        """n candidates with an access address of their own each: no members of anything (min_count 2); in front of all connections."""
        for k in range(n):
            ch = int(self.rng.integers(0, 37))
            self.raw.append(ld.Cand(int(self.rng.integers(0, 1 << 24)), 0x10000000 + 0x31 * k, 0x777 + k, ch, 1, 0, ch))
        return self

    def grouped(self):
        raw = [self.raw[i] for i in self.rng.permutation(len(self.raw))]
        conns, cands = ld.group(raw, 2)
        return conns, cands, [self.names[(c.access_address, c.crc_init)] for c in conns]


def _steps(*runs):
    """Event counters from runs of (pairs, counter step)."""
    out = [0]
    for pairs, step in runs:
        for _ in range(pairs):
            out.append(out[-1] + step)
    return out


@functools.lru_cache(maxsize=None)
def align_list(variant):
    """Connections whose first and last events lie on, one before and one behind the boundaries of a wave (64), a workgroup
    (256), a score tile (1024) and a scan tile (2048) of events -- sizes of one unit less one, the unit and the unit plus one, each
    group behind a filler that ends on a multiple of the unit; 127, 128 and 129 events, each from a multiple of 64; 3 071 and 1 --, with one and two packets per event in turn and a five-channel map on every third;
    among them the connections that the tags of tests/_le_track_paths.py name:
    * "beyond 2^32", first of all: every later connection rides on a step sum of 2^32 + 9;
    * "several a / b / c": three connections of three to four events in one wave of event pairs, with missed events;
    * "three waves": 193 events from a multiple of 64, the q of its three waves of pairs 36, 60 and 90: every two have a gcd above 6;
    * "lane 63" / "thread 255": all q 12 but the one of the pair at lane 63 of wave 0 / at thread 255 of a workgroup, which is 18;
    * "off hop": 400 events of two packets, those of off_hop_plan() one channel up: in its first and last wave of slots, which it
      shares with others, five in one wave of its own, one in another, none in the rest.
    variant "A" ends with the number of events at a multiple of 1024, "B" has one connection of one event more.
    -> (conns, cands, names)"""
    assert variant in ("A", "B")
    b = _Laid(31).lone(5)
    b.conn("beyond 2^32", BEYOND_32, h=7, u0=29, jitter=0)
    b.pad(64).conn("several a", (0, 2, 5)).conn("several b", (0, 1, 2, 3)).conn("several c", (0, 3, 5, 6))
    k = 0
    for unit in (64, 256, 1024, 2048):
        b.pad(unit)
        for n in (unit - 1, 2, unit, unit + 1) + ((-127, -128, -129) if unit == 64 else (3071, 1) if unit == 2048 else ()):
            if n < 0:                                                      # two waves less one, two waves, two waves and one: each from a
                n = -n                                                     # multiple of 64, so that they end one before, on and one
                b.pad(64)                                                  # behind the second wave boundary
            k += 1
            b.conn("%d events" % n, n, chmap=FIVE_MAP if k % 3 == 0 else FULL_MAP, interval=6 + k % 5, h=5 + k % 12, u0=(5 * k) % 37,
                   per_event=2 if n == 1 else 1 + k % 2)
    b.pad(64).conn("three waves", _steps((64, 6), (64, 10), (64, 15)), h=11, u0=3)
    b.pad(256).conn("lane 63", _steps((63, 2), (1, 3), (6, 2)), h=9, u0=20)
    b.pad(256).conn("thread 255", _steps((255, 2), (1, 3), (4, 2)), h=13, u0=1)
    b.conn("foreign", 3, per_event=2)
    b.raw += [b.raw[-1]._replace(offset=b.raw[-1].offset + 9 * UNIT, stream=37), b.raw[-1]._replace(offset=b.raw[-1].offset + 12 * UNIT, stream=39)]
    b.conn("off hop", OFF_HOP_EVENTS, h=10, u0=17, per_event=2, off_hop=off_hop_plan(b.slot))
    b.pad(LT_SCORE_ALIGN)
    if variant == "B":
        b.conn("one more", 1, per_event=2)
    return b.grouped()


CROWD = (1 << 16) + 4


@functools.lru_cache(maxsize=None)
def crowd_list():
    """More connections than sixteen bits number, 65 544 in all: CROWD = 65 540, the first eight of ten events, the others of one
    event of two packets, and behind them four that hop, in the same stretch of time as the first eight.  The connection indices from 65 536 on
    differ from the indices 65 536 below them in the third byte alone, so a sort of the connection index that stops after two radix
    passes leaves the members of connection 65 540 + i between those of connection 4 + i, in time order.
    -> (conns, cands, names)"""
    b = _Laid(51).lone(3)
    for k in range(CROWD):
        if k < 8:
            b.conn("front", 10, h=5 + k, u0=k, base=5000 + 40 * k)
        else:
            b.conn("one event", 1, per_event=2, jitter=0)
    b.conn("behind a", 12, h=6, u0=11, base=5013).conn("behind b", 9, per_event=2, h=16, u0=3, base=5450)
    b.conn("behind c", (0, 1, 2, 4, 7, 8), chmap=FIVE_MAP, h=12, u0=9, base=5777).conn("behind d", 70, h=9, u0=30, base=6000)
    return b.grouped()


@functools.lru_cache(maxsize=None)
def long_event_list():
    """More slots than 256 scan tiles hold, with few events: one connection of 40 events at interval 3200, each a train of 13 300
    empty packets 230 bits apart (3.06 Mbit of the 4 Mbit to the next event; the default ifs keeps a train in one event), and three
    small connections behind it, whose slots and events lie beyond tile 256.  -> (conns, cands, names, cand_arr): the candidate
    list as tuples for the model and, built with numpy, as the fields of the device's records (offset, access_address, crc_init,
    stream, header0, length, conn)."""
    b = _Laid(41).lone(3)
    n_events, train, spacing = 40, 13300, 230
    aa, ci = 0x20000000, 0x5A5A5A
    b.names[(aa, ci)] = "trains"
    anchors = 7000 + np.arange(n_events, dtype=np.int64) * (3200 * UNIT) + b.rng.integers(-20, 21, n_events)
    chans = np.array([csa1_at(5, 6, n, FULL_MAP) for n in range(n_events)], np.int64)
    off = (anchors[:, None] + spacing * np.arange(train, dtype=np.int64)[None, :]).reshape(-1)
    st = np.repeat(chans, train)
    b.raw += [ld.Cand(o, aa, ci, s, 1, 0, s) for o, s in zip(off.tolist(), st.tolist())]
    b.conn("behind a", 30, h=8, u0=2).conn("behind b", 5, per_event=2, h=15, u0=30).conn("behind c", (0, 1, 2, 4, 7), chmap=FIVE_MAP, h=12, u0=9)
    conns, cands = ld.group(b.raw, 2)                                       # (unshuffled: the grouping sorts the list anyway)
    names = [b.names[(c.access_address, c.crc_init)] for c in conns]
    fields = np.array(cands, dtype=np.int64)
    return conns, cands, names, fields
