"""Test-side model of the LE channel selection #2 stage (include/btbbx.h btbbx_le_csa2_*), written from the six
rules of the contract, not from the kernels (le_csa2.h splits the hypotheses into blocks and folds partial results).

* evaluate: rules 3 to 5 for one connection in plain Python, a loop over all 65 536 hypotheses; Rules: its branch points as
  options, Rules() is the model, any other value a deliberately wrong one (tests/test_le_csa2_model.py shows that the lattice
  below tells each from the right one)
* evaluate_np: the same in numpy, for the large lists
* select: rules 1, 2 and 6 around either of them, on what tests/_le_track.py's model of the tracking leaves
* csa2: the FORWARD channel selection algorithm #2 (Core v5.x Vol 6 Part B 4.5.8.3), written from the specification; it shares
  nothing with the model
* lattice / lattice_list / seam_list / crowd_list / chain_capture: the lists and the capture the CPU and GPU tests share
"""
import collections
import functools

import numpy as np

import _le_discover as ld
import _le_track as lt

REMAP = 1
EVALUATED, UNIQUE, PREFERRED = 1, 2, 4

Sel = collections.namedtuple("Sel", "n_on n_off n_second channel_id counter0 flags")
SelPkt = collections.namedtuple("SelPkt", "counter prn unmapped expected on_hop")


class Rules:
    def __init__(self, **kw):
        self.reverse16 = False           # the bits reversed over all 16, not within each byte
        self.rounds = 3
        self.final_xor = True
        self.chid_low = False            # chId = AA & 0xffff
        self.remap_index = "scaled"      # (n_used * prn) >> 16; "prn_mod": prn mod n_used; "unmapped_mod": unmapped mod n_used
        self.wrap = True                 # c0 + n_e modulo 2^16; False: a sum beyond 65535 has no prediction
        self.tie_largest = False         # ties to the largest c0
        self.second_below = False        # n_second leaves out the hypotheses that tie the winner
        self.count_packets = False       # scores and tallies count packets, not events
        self.preferred_ge = False        # PREFERRED with >=
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


MODEL = Rules()
VARIANTS = dict(reverse16=dict(reverse16=True), two_rounds=dict(rounds=2), four_rounds=dict(rounds=4), no_final_xor=dict(final_xor=False),
                chid_low=dict(chid_low=True), remap_prn_mod=dict(remap_index="prn_mod"), remap_unmapped_mod=dict(remap_index="unmapped_mod"),
                no_wrap=dict(wrap=False), tie_largest=dict(tie_largest=True), second_below=dict(second_below=True),
                count_packets=dict(count_packets=True), preferred_ge=dict(preferred_ge=True))

_REV8 = [sum(((b >> i) & 1) << (7 - i) for i in range(8)) for b in range(256)]


def channel_id(aa, rules=MODEL):
    return aa & 0xFFFF if rules.chid_low else (aa >> 16) ^ (aa & 0xFFFF)


def prn_e(c, chid, rules=MODEL):
    """Rule 3."""
    x = c ^ chid
    for _ in range(rules.rounds):
        if rules.reverse16:
            x = (_REV8[x & 0xFF] << 8) | _REV8[x >> 8]
        else:
            x = (_REV8[x >> 8] << 8) | _REV8[x & 0xFF]
        x = (17 * x + chid) % 65536
    return x ^ chid if rules.final_xor else x


def predict(c, chid, map_mask, flags, rules=MODEL):
    """Rule 4: (prn, unmapped, expected) of counter c."""
    prn = prn_e(c, chid, rules)
    unmapped = prn % 37
    if (map_mask >> unmapped) & 1:
        return prn, unmapped, unmapped
    used = [ch for ch in range(37) if (map_mask >> ch) & 1]
    if not (flags & REMAP) or not used:
        return prn, unmapped, 0xFF
    index = {"scaled": (len(used) * prn) >> 16, "prn_mod": prn % len(used), "unmapped_mod": unmapped % len(used)}[rules.remap_index]
    return prn, unmapped, used[index]


def evaluate(aa, events, map_mask, flags, n_on_hop, rules=MODEL):
    """Rules 3 to 5 for one EVALUATED connection.  events: (n_e, C_e, packets) per event.  Returns (Sel, counter0)."""
    chid = channel_id(aa, rules)
    table = [predict(c, chid, map_mask, flags, rules)[2] for c in range(65536)]
    scores = []
    for c0 in range(65536):                                                # rule 5
        s = 0
        for n, ch, packets in events:
            c = c0 + n % 65536
            if c > 65535:
                if not rules.wrap:
                    continue
                c -= 65536
            if table[c] == ch:
                s += packets if rules.count_packets else 1
        scores.append(s)
    best = max(scores)
    winners = [c0 for c0 in range(65536) if scores[c0] == best]
    counter0 = winners[-1] if rules.tie_largest else winners[0]
    if rules.second_below:
        n_second = max([s for s in scores if s != best], default=0)
    else:
        n_second = max(s for c0, s in enumerate(scores) if c0 != counter0)
    return _record(aa, events, table, best, counter0, n_second, n_on_hop, rules)


def _record(aa, events, table, best, counter0, n_second, n_on_hop, rules):
    n_off = 0
    for n, ch, packets in events:
        c = counter0 + n % 65536
        if c > 65535 and not rules.wrap:
            continue
        if table[c % 65536] not in (0xFF, ch):
            n_off += packets if rules.count_packets else 1
    flags = EVALUATED
    if best > n_second:
        flags |= UNIQUE
        if best >= n_on_hop if rules.preferred_ge else best > n_on_hop:
            flags |= PREFERRED
    return Sel(int(best), n_off, int(n_second), (aa >> 16) ^ (aa & 0xFFFF), int(counter0), flags)


@functools.lru_cache(maxsize=64)
def _prn_table(chid, rules):
    c = np.arange(65536, dtype=np.uint32)
    rev = np.array(_REV8, np.uint32)
    x = c ^ chid
    for _ in range(rules.rounds):
        x = (rev[x & 0xFF] << 8) | rev[x >> 8] if rules.reverse16 else (rev[x >> 8] << 8) | rev[x & 0xFF]
        x = (17 * x + chid) & 0xFFFF
    return x ^ chid if rules.final_xor else x


def expected_table(aa, map_mask, flags, rules=MODEL):
    """expected(c) of rule 4 for every c, as bytes."""
    prn = _prn_table(channel_id(aa, rules), rules)
    unmapped = prn % 37
    in_map = ((np.uint64(map_mask) >> unmapped.astype(np.uint64)) & np.uint64(1)).astype(bool)
    used = np.array([ch for ch in range(37) if (map_mask >> ch) & 1], np.uint32)
    out = np.full(65536, 0xFF, np.uint8)
    if (flags & REMAP) and len(used):
        index = {"scaled": (len(used) * prn) >> 16, "prn_mod": prn % len(used), "unmapped_mod": unmapped % len(used)}[rules.remap_index]
        out = used[index].astype(np.uint8)
    out[in_map] = unmapped[in_map]
    return out


def scores_np(aa, events, map_mask, flags, rules=MODEL):
    """(S(c0) for every c0, the table of expected(c)) in numpy: the table, doubled, shifted by n_e and compared event after event."""
    table = expected_table(aa, map_mask, flags, rules)
    twice = np.concatenate([table, table if rules.wrap else np.full(65536, 0xFE, np.uint8)])
    scores = np.zeros(65536, np.int64)
    for n, ch, packets in events:
        n %= 65536
        scores += (twice[n:n + 65536] == ch) * (packets if rules.count_packets else 1)
    return scores, table


def evaluate_np(aa, events, map_mask, flags, n_on_hop, rules=MODEL):
    """evaluate in numpy."""
    scores, table = scores_np(aa, events, map_mask, flags, rules)
    best = int(scores.max())
    winners = np.flatnonzero(scores == best)
    counter0 = int(winners[-1] if rules.tie_largest else winners[0])
    if rules.second_below:
        below = scores[scores != best]
        n_second = int(below.max()) if len(below) else 0
    else:
        n_second = best if len(winners) > 1 else int(np.delete(scores, counter0).max())
    return _record(aa, events, table, best, counter0, n_second, n_on_hop, rules)


def select(conns, cands, tracks, pkts, flags, rules=MODEL, core=evaluate_np):
    """Rules 1, 2 and 6.  conns, cands: as ld.group leaves them (a candidate's `channel` = its connection); tracks, pkts: what
    lt.track returned for them (so len(tracks) = K, len(pkts) = N, None: no member).  Returns (sels, sel_pkts): one Sel per
    connection, one SelPkt or None per candidate."""
    k = len(tracks)
    sel_pkts = [None] * len(pkts)
    members = [[] for _ in range(k)]
    for i, p in enumerate(pkts):                                               # rule 1
        if p is not None and cands[i].channel < k:
            members[cands[i].channel].append(i)
    sels = []
    for g in range(k):
        aa, t = conns[g].access_address, tracks[g]
        if not t.flags & lt.TIMED:                                             # rule 2
            sels.append(Sel(0, 0, 0, (aa >> 16) ^ (aa & 0xFFFF), 0, 0))
            for i in members[g]:
                sel_pkts[i] = SelPkt(0, 0, 0xFF, 0xFF, 0)
            continue
        events = {}
        for i in members[g]:
            p = pkts[i]
            n, ch, packets = events.get(p.event, (p.counter % 65536, p.channel, 0))
            assert (n, ch) == (p.counter % 65536, p.channel)
            events[p.event] = (n, ch, packets + 1)
        sel = core(aa, [events[e] for e in sorted(events)], t.map_mask, flags, t.n_on_hop, rules)
        sels.append(sel)
        chid = channel_id(aa, rules)
        for i in members[g]:                                                   # rule 6
            c = sel.counter0 + pkts[i].counter % 65536
            if c > 65535 and not rules.wrap:
                sel_pkts[i] = SelPkt(c % 65536, 0, 0xFF, 0xFF, 0)
                continue
            prn, unmapped, expected = predict(c % 65536, chid, t.map_mask, flags, rules)
            sel_pkts[i] = SelPkt(c % 65536, prn, unmapped, expected, int(expected == pkts[i].channel))
    return sels, sel_pkts


def sel_array(sels, dtype):
    a = np.zeros(len(sels), dtype)
    for i, s in enumerate(sels):
        a[i] = tuple(s) + (0,)
    return a


def sel_pkt_array(sel_pkts, dtype):
    a = np.zeros(len(sel_pkts), dtype)
    if not len(sel_pkts):
        return a
    none = np.array([p is None for p in sel_pkts], bool)
    rows = np.array([(0,) * len(SelPkt._fields) if p is None else p for p in sel_pkts], np.int64)
    for j, name in enumerate(SelPkt._fields):
        a[name] = rows[:, j]
    a.view(np.uint8).reshape(len(sel_pkts), dtype.itemsize)[none] = 0xFF
    return a


# ---- the forward channel selection ----------------------------------------------------------------------------------
def _perm(v):
    """4.5.8.3.3: the permutation operation -- the bits of each of the two octets in opposite order."""
    low, high = format(v & 0xFF, "08b"), format(v >> 8, "08b")
    return int(high[::-1] + low[::-1], 2)


def _mam(a, b):
    """4.5.8.3.3: multiply, add and modulo."""
    return (17 * a + b) % 65536


def csa2_steps(aa, counter, chmap):
    """Channel selection algorithm #2, step by step as 4.5.8.3 lays it out: (prn_e, unmappedChannel, remappingIndex or None,
    data channel index) of the event with this connEventCounter on a connection with this access address and channel map."""
    identifier = ((aa >> 16) & 0xFFFF) ^ (aa & 0xFFFF)
    v = counter ^ identifier
    for _ in range(3):
        v = _mam(_perm(v), identifier)
    prn = v ^ identifier
    unmapped = prn % 37
    if (chmap >> unmapped) & 1:
        return prn, unmapped, None, unmapped
    table = [c for c in range(37) if (chmap >> c) & 1]
    index = (len(table) * prn) // 65536
    return prn, unmapped, index, table[index]


def csa2(aa, counter, chmap):
    return csa2_steps(aa, counter % 65536, chmap)[3]


def mask_of(channels):
    m = 0
    for c in channels:
        m |= 1 << c
    return m


FULL_MAP = (1 << 37) - 1
NINE_MAP = mask_of((9, 10, 21, 22, 23, 33, 34, 35, 36))                   # the map of the specification's sample data
FIVE_MAP = mask_of((3, 8, 19, 25, 33))
UNIT, IFS, JITTER = lt.UNIT, lt.IFS, lt.JITTER


def plant(aa, crc_init, counter0, counters, chmap, interval=6, base=3000, per_event=1, jitter=None, channel_of=None):
    """The packets of a connection that hops by algorithm #2, as ungrouped Cand tuples (`channel` = the data channel index, stream c
    = data channel c): the event with relative counter n lies at base + n * interval * UNIT on csa2(aa, counter0 + n, chmap)."""
    out = []
    for e, n in enumerate(counters):
        ch = csa2(aa, counter0 + n, chmap) if channel_of is None else channel_of(n)
        at = base + n * interval * UNIT + (jitter(e) if jitter else 0)
        for j in range(per_event):
            length = (0, 5)[j % 2]
            out.append(ld.Cand(at, aa, crc_init, ch, 1 if length == 0 else 2, length, ch))
            at += 80 + 8 * length + 150
    return out


# ---- the hand-built lattice -------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name cands")
BEYOND_16 = (0, 1, 2, 3, (1 << 16) + 5, (1 << 16) + 6, (1 << 17) + 7, (1 << 17) + 9)
BEYOND_32 = (0, 1, 2, 3, (1 << 32) + 5, (1 << 32) + 6, (1 << 32) + (1 << 16) + 7, (1 << 33) + 9)
# (access address, counter0, events): three events on all channels whose best score two hypotheses share -- found by a search over
# random access addresses with evaluate_np; tests/test_le_csa2_model.py asserts where the two lie
BOTH = (0x61E7C392, 30666, 14, 11)                                         # (access address, counter0, hop increment, first unmapped)
TIE_ACROSS = (0xD2AC6FD2, 62170, 6)                                     # 62170 and 65048
TIE_INSIDE = (0x8EB2592E, 52801, 6)                                     # 52801 and 52903


def _ids():
    k = 0
    while True:
        k += 1
        yield 0x60000000 + 0x01010101 * (k % 5) + 0x1357 * k, (0x234567 + 0x010203 * k) & 0xFFFFFF


@functools.lru_cache(maxsize=None)
def lattice():
    """The hand-built connections of the selection tests: a tuple of Case, every case one (access address, CRCInit) group."""
    ids = _ids()
    cases = []

    def add(name, counter0, counters, chmap=FULL_MAP, aa=None, **kw):
        own_aa, ci = next(ids)
        cases.append(Case(name, tuple(plant(own_aa if aa is None else aa, ci, counter0, counters, chmap, **kw))))

    for n in (2, 3, 8, 40):
        add("%d events" % n, 4711 + n, range(n))
    for c0 in (0, 1, 65535):
        add("counter0 %d" % c0, c0, range(12))
    add("wrap inside", 65530, range(12))
    add("n_e beyond 2^16", 40000, BEYOND_16)
    add("n_e beyond 2^32", 123, BEYOND_32)
    add("missed events", 30000, (0, 1, 2, 5, 11, 12, 30, 31, 33, 40, 41, 45))
    add("map of 37", 77, range(14))
    add("map of 36", 78, range(40), chmap=FULL_MAP & ~(1 << 17))
    add("map of 9", 6, range(30), chmap=NINE_MAP)
    add("map of 2", 9000, range(30), chmap=mask_of((4, 29)))
    add("map of 1", 9001, range(10), chmap=mask_of((13,)))
    add("two packets per event", 555, range(9), per_event=2)
    add("two packets per event, map of 9", 556, (0, 1, 2, 4, 7, 8, 9, 13, 14, 15, 16, 20), chmap=NINE_MAP, per_event=2)
    add("not TIMED: interval 5", 100, range(8), interval=5)
    add("not TIMED: one event", 100, range(1), per_event=2)
    add("algorithm #1", 0, range(24), channel_of=lambda n: lt.csa1_at(11, 7, n, FULL_MAP))
    add("algorithm #1, map of 5", 0, range(24), channel_of=lambda n: lt.csa1_at(30, 12, n, FIVE_MAP))
    add("events off the prediction", 31000, range(20), channel_of=None, jitter=lambda e: (e * 13) % 31 - 15)
    # seven events of algorithm #2, then seven of #1 that continue at the same counters: each algorithm explains seven (no REMAP)
    aa, c0, h, u = BOTH
    add("both algorithms", c0, range(14), aa=aa, channel_of=lambda n: csa2(aa, c0 + n, FULL_MAP) if n < 7 else lt.csa1_at(u, h, n, FULL_MAP))
    aa, c0, n = TIE_ACROSS
    add("tie across two blocks", c0, range(n), aa=aa)
    aa, c0, n = TIE_INSIDE
    add("tie inside one block", c0, range(n), aa=aa)
    # a stored connection without members: candidates on an advertising stream and on one out of range
    aa, ci = next(ids)
    cases.append(Case("no members", (ld.Cand(100, aa, ci, 37, 1, 0, 0), ld.Cand(100 + 6 * UNIT, aa, ci, 41, 1, 0, 0))))
    # long gaps: within a tile of events the later ones lie beyond the window of counters the scoring pass tabulates
    add("missed events, far", 50000, (0, 1, 2, 20000, 20001, 45000, 45001, 45002, 65000))
    # three events of the "off the prediction" case moved one channel up
    k = [c.name for c in cases].index("events off the prediction")
    moved = tuple(c._replace(stream=(c.stream + 1) % 37, channel=(c.channel + 1) % 37) if e in (3, 4, 17) else c
                  for e, c in enumerate(cases[k].cands))
    cases[k] = Case(cases[k].name, moved)
    return tuple(cases)


def _grouped(raw, names_by_key, rng, noise):
    for k in range(noise):                                                 # single candidates: no members of anything at min_count 2
        ch = int(rng.integers(0, 37))
        raw.append(ld.Cand(int(rng.integers(0, 1 << 24)), 0x40000000 + 0x2F1 * k + int(rng.integers(0, 1 << 28)), int(rng.integers(0, 1 << 24)),
                           ch, 1, 0, ch))
    raw = [raw[i] for i in rng.permutation(len(raw))]
    conns, cands = ld.group(raw, 2)
    return conns, cands, [names_by_key.get((c.access_address, c.crc_init)) for c in conns]


@functools.lru_cache(maxsize=None)
def lattice_list():
    """The lattice as one candidate list with 40 non-members between the groups, shuffled and grouped: (conns, cands, names)."""
    raw, by_key = [], {}
    for case in lattice():
        raw += list(case.cands)
        by_key[(case.cands[0].access_address, case.cands[0].crc_init)] = case.name
    return _grouped(raw, by_key, np.random.default_rng(5), 40)


def tracked(conns, cands, flags, count=None, kept=None):
    """lt.track on the first `count` candidates and `kept` connections of a grouped list."""
    n = len(cands) if count is None else min(count, len(cands))
    k = len(conns) if kept is None else min(kept, len(conns))
    return lt.track(cands[:n], k, lt.LATTICE_MHZ, lt.N_STREAMS, UNIT, IFS, JITTER, flags)


@functools.lru_cache(maxsize=None)
def lattice_model(flags):
    conns, cands, names = lattice_list()
    tracks, pkts = tracked(conns, cands, flags)
    return tracks, pkts, select(conns, cands, tracks, pkts, flags)


# ---- sizes that cross the kernels' seams ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam_list():
    """One connection of 5 000 events of two packets each (ten LDS tiles of events in every one of its 64 work items; 1 000 events
    missed behind the first thousand, which widens the window of one tile, and 5 000 behind the third, which puts the rest of that
    tile beyond the window) beside 1 000 connections of 2 to 4 events, all hopping by algorithm #2: (conns, cands, names)."""
    rng = np.random.default_rng(23)
    counters = list(range(1000)) + [n + 1000 for n in range(1000, 3000)] + [n + 6000 for n in range(3000, 5000)]
    raw = plant(0x8E5A3C71, 0x5EED01, 60000, counters, FULL_MAP, per_event=2, jitter=lambda e: (e * 7) % 41 - 20)
    by_key = {(0x8E5A3C71, 0x5EED01): "large"}
    for k in range(1000):
        aa = 0x10000000 + 600 * int(rng.integers(0, 1 << 21))
        raw += plant(aa, (7 * k + 1) & 0xFFFFFF, int(rng.integers(0, 1 << 16)), range(2 + k % 3), FULL_MAP if k % 4 else FIVE_MAP,
                     interval=6 + k % 30, base=4000 + 97 * k)
        by_key[(aa, (7 * k + 1) & 0xFFFFFF)] = "small"
    return _grouped(raw, by_key, rng, 0)


CROWD = (1 << 16) + 4


@functools.lru_cache(maxsize=None)
def crowd_list():
    """More connections than sixteen bits number: CROWD of one event of two packets (not TIMED), among them -- every 4 099th -- 16 of
    ten events, and four of 9 to 70 events behind them, at connection indices beyond 65 535: (conns, cands, names)."""
    rng = np.random.default_rng(53)
    raw, by_key = [], {}
    for k in range(CROWD + 4):
        aa, ci = 0x20000000 + 0x1000 * k, (0x0A0B0C + 0x010203 * k) & 0xFFFFFF
        if k >= CROWD:
            n, name = (12, 9, 30, 70)[k - CROWD], "behind"
        elif k % 4099 == 7:
            n, name = 10, "ten events"
        else:
            n, name = 1, "one event"
        by_key[(aa, ci)] = name
        raw += plant(aa, ci, (k * 7919) % 65536, range(n), FULL_MAP if k % 2 else FIVE_MAP, base=5000 + 3 * (k % 1000), per_event=2 if n == 1 else 1)
    conns, cands = ld.group(raw, 2)                                         # (unshuffled: the grouping sorts the list anyway)
    return conns, cands, [by_key[(c.access_address, c.crc_init)] for c in conns]


# ---- the chain capture --------------------------------------------------------------------------------------------------
Planted = collections.namedtuple("Planted", "aa crc_init interval counter0 chmap counters algorithm")


@functools.lru_cache(maxsize=None)
def chain_capture():
    """37 data-channel streams (stream c = channel c) and one advertising stream of 5 000 words of noise with three planted
    connections: algorithm #2 on all channels, 42 events of interval 6 with two packets each; algorithm #2 on a five-channel map,
    interval 10 with one event left out, all its packets alike, which gives it a shifted alias on channel 3 (as the second connection
    of tests/_le_track.py's chain capture has one); algorithm #1 on all channels, interval 7.  Returns (Capture, planted)."""
    n_words = 5000
    mhz = np.array(lt.DATA_MHZ + (2402,), np.uint16)
    b = ld._Builder(38, n_words, mhz, 9191)
    rng = np.random.default_rng(92)
    total = 64 * n_words
    plans = [dict(interval=6, counter0=65520, chmap=FULL_MAP, counters=range(42), per_event=2, algorithm=2),
             dict(interval=10, counter0=1234, chmap=FIVE_MAP, counters=[n for n in range(25) if n != 6], per_event=1, same=True, algorithm=2),
             dict(interval=7, counter0=0, chmap=FULL_MAP, counters=range(30), per_event=1, algorithm=1)]
    planted = []
    for k, p in enumerate(plans):
        aa, ci = ld.good_aa(rng), int(rng.integers(0, 1 << 24))
        while p.get("same") and not ((aa & 7) == 5 and ld._offenses(aa) == 0 and ld._offenses((aa >> 2) | (1 << 31)) == 0):
            aa = (int(rng.integers(0, 1 << 32)) & ~7) | 5
        base = 900 + 2111 * k
        for n in p["counters"]:
            ch = csa2(aa, p["counter0"] + n, p["chmap"]) if p["algorithm"] == 2 else lt.csa1(9, 11, n, p["chmap"])
            at = base + n * p["interval"] * UNIT + int(rng.integers(-20, 21))
            for j in range(p["per_event"]):
                length = 17 if p.get("same") else (0, 9, 3)[(n + j) % 3]
                assert at + 80 + 8 * length <= total
                b.plant(ch, at, aa, ci, 1 if length in (0, 17) else 2, length, "connection %d" % k,
                        payload=bytes(range(1, 18)) if p.get("same") else None)
                at += 80 + 8 * length + 150
        planted.append(Planted(aa, ci, p["interval"], p["counter0"], p["chmap"], tuple(p["counters"]), p["algorithm"]))
    words = b.words(n_words + 5)
    words.flags.writeable = False
    return ld.Capture(words, n_words, n_words + 5, total - 39, mhz, tuple(b.planted), 27), tuple(planted)


@functools.lru_cache(maxsize=None)
def chain_model():
    """(conns, cands) of the discovery's model on the chain capture, min_count 2."""
    cap, _ = chain_capture()
    return ld.group(ld.capture_candidates(cap, 27), 2)
