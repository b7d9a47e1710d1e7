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
* pair_list / wide_list: the lists that put winner and runner-up where the kernels split the work (tests/_le_csa2_paths.py)
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


# ---- lists that pin how the kernels split the work (tests/_le_csa2_paths.py holds the conditions) ------------------------------
# Hypothesis c0 is block c0 / 1024, thread (c0 mod 1024) / 4, register c0 mod 4 of le_csa2_score_kernel; the numbers below are
# written out, tests/test_le_csa2_paths_model.py holds them against the constants of the header.
def at(block, thread, r=0):
    return 1024 * block + 4 * thread + r


PAIR_AA = 0x5A17C3E9
PAIR_EVENTS = 32
# name -> (A, B, tie): PAIR_EVENTS events at the counters from 0 on (pair_counters), 18 of them on csa2(PAIR_AA, A + e) and 14 on csa2(PAIR_AA, B + e)
# -- A wins, B is the runner-up, wherever the two lie --, or 16 and 16 for an exact tie, which the smaller of the two wins
PAIRS = collections.OrderedDict([
    ("same lane, runner-up at the smaller r", (at(9, 77, 3), at(9, 77, 0), False)),
    ("same lane, runner-up at the larger r", (at(40, 200, 1), at(40, 200, 2), False)),
    ("same lane, high block, r 0 and 3", (at(61, 3, 0), at(61, 3, 3), False)),
    ("same wave, lanes 0 and 63, runner-up above", (at(12, 64, 2), at(12, 127, 1), False)),
    ("same wave, lanes 63 and 0, runner-up below", (at(45, 255, 0), at(45, 192, 3), False)),
    ("same wave, lanes 31 and 32", (at(33, 128 + 31, 1), at(33, 128 + 32, 1), False)),
    ("same wave, lanes 32 and 31", (at(20, 64 + 32, 0), at(20, 64 + 31, 2), False)),
    ("same wave 0, lanes 5 and 6", (at(3, 5, 3), at(3, 6, 0), False)),
    ("threads 63 and 64", (at(7, 63, 3), at(7, 64, 0), False)),
    ("threads 64 and 63", (at(50, 64, 0), at(50, 63, 3), False)),
    ("threads 127 and 128", (at(26, 127, 2), at(26, 128, 2), False)),
    ("threads 192 and 191", (at(58, 192, 1), at(58, 191, 0), False)),
    ("waves 0 and 3", (at(5, 10, 1), at(5, 250, 2), False)),
    ("waves 3 and 0", (at(37, 230, 0), at(37, 0, 0), False)),
    ("waves 1 and 2", (at(44, 100, 2), at(44, 150, 3), False)),
    ("waves 2 and 1", (at(18, 140, 3), at(18, 70, 1), False)),
    ("waves 3 and 3 beside wave 0", (at(62, 201, 1), at(62, 254, 3), False)),
    ("blocks 0 and 63", (at(0, 17, 1), at(63, 200, 2), False)),
    ("blocks 63 and 0", (at(63, 255, 3), at(0, 0, 0), False)),
    ("blocks 31 and 32, j 1023 beside j 0", (at(31, 255, 3), at(32, 0, 0), False)),
    ("blocks 32 and 31, j 0 beside j 1023", (at(32, 0, 0), at(31, 255, 3), False)),
    ("blocks 10 and 11, j 1023 beside j 0", (at(10, 255, 3), at(11, 0, 0), False)),
    ("blocks 0 and 1, lanes alike", (at(0, 31, 2), at(1, 31, 2), False)),
    ("blocks 47 and 15", (at(47, 129, 0), at(15, 66, 1), False)),
    ("tie in one lane", (at(22, 91, 0), at(22, 91, 3), True)),
    ("tie in one lane, r 1 and 2, high block", (at(55, 160, 1), at(55, 160, 2), True)),
    ("tie in one wave, lanes 0 and 63", (at(1, 192, 1), at(1, 255, 1), True)),
    ("tie in wave 1, lanes 31 and 32", (at(39, 95, 3), at(39, 96, 0), True)),
    ("tie at threads 63 and 64", (at(14, 63, 3), at(14, 64, 0), True)),
    ("tie at threads 63 and 64, high block", (at(48, 63, 0), at(48, 64, 3), True)),
    ("tie in waves 0 and 3", (at(29, 1, 0), at(29, 255, 3), True)),
    ("tie in waves 1 and 2", (at(60, 65, 2), at(60, 190, 1), True)),
    ("tie in waves 0 and 1, high block", (at(35, 40, 1), at(35, 80, 1), True)),
    ("tie in blocks 0 and 63", (at(0, 0, 0), at(63, 255, 3), True)),
    ("tie in blocks 16 and 17, j 1023 beside j 0", (at(16, 255, 3), at(17, 0, 0), True)),
    ("tie in blocks 62 and 63, j 1023 beside j 0", (at(62, 255, 3), at(63, 0, 0), True)),
    ("tie in blocks 8 and 40", (at(8, 120, 2), at(40, 120, 2), True)),
])


def pair_counters(a, b):
    """The counters of a pair's events: the first PAIR_EVENTS from 0 on at which the predictions of A and B differ (where they
    agree -- one counter in 37 -- an event would lie on both, and no draw could give the planted scores)."""
    counters = [n for n in range(3 * PAIR_EVENTS) if csa2(PAIR_AA, a + n, FULL_MAP) != csa2(PAIR_AA, b + n, FULL_MAP)][:PAIR_EVENTS]
    assert counters[0] == 0, "choose another placement: the tracking counts from the first event it sees"
    return counters


def pair_events(a, b, tie, seed):
    """(counter, channel) of each of the PAIR_EVENTS events of a pair: a seeded subset of 18 (16 for a tie) on A's prediction, the
    rest on B's."""
    n_a = PAIR_EVENTS // 2 if tie else PAIR_EVENTS // 2 + 2
    on_a = set(np.random.default_rng(seed).choice(PAIR_EVENTS, n_a, replace=False).tolist())
    return [(n, csa2(PAIR_AA, (a if e in on_a else b) + n, FULL_MAP)) for e, n in enumerate(pair_counters(a, b))]


def pair_is_clean(a, b, tie, events):
    """Whether, with and without REMAP on the map the events show, A and B score exactly what was planted -- no event of the one
    lies on the other's prediction through the remapping -- and every third hypothesis scores at least 2 below B."""
    n_a = PAIR_EVENTS // 2 if tie else PAIR_EVENTS // 2 + 2
    for flags in (0, REMAP):
        scores, _ = scores_np(PAIR_AA, [(n, ch, 1) for n, ch in events], mask_of(ch for _, ch in events), flags)
        if (scores[a], scores[b]) != (n_a, PAIR_EVENTS - n_a):
            return False
        scores[[a, b]] = 0
        if scores.max() > PAIR_EVENTS - n_a - 2:
            return False
    return True


@functools.lru_cache(maxsize=None)
def pair_plan():
    """name -> (A, B, tie, seed, events): for every pair the first seed (from a base of its own) whose draw is clean."""
    plan = collections.OrderedDict()
    for k, (name, (a, b, tie)) in enumerate(PAIRS.items()):
        for seed in range(1000 * k, 1000 * k + 200):
            events = pair_events(a, b, tie, seed)
            if pair_is_clean(a, b, tie, events):
                plan[name] = (a, b, tie, seed, tuple(events))
                break
        else:
            raise AssertionError("no clean draw for the pair %r" % name)
    return plan


@functools.lru_cache(maxsize=None)
def pair_list():
    """The pairs as one candidate list: one access address -- one chId --, consecutive CRCInits, 20 non-members between them:
    (conns, cands, names)."""
    raw, by_key = [], {}
    for k, (name, (a, b, tie, seed, events)) in enumerate(pair_plan().items()):
        raw += plant(PAIR_AA, 0x700000 + k, 0, [n for n, _ in events], FULL_MAP, interval=6 + k % 5, base=3000 + 977 * k,
                     channel_of=dict(events).get)
        by_key[(PAIR_AA, 0x700000 + k)] = name
    return _grouped(raw, by_key, np.random.default_rng(61), 20)


TWENTY_MAP = mask_of((0, 1, 3, 4, 6, 9, 10, 12, 15, 16, 19, 21, 22, 25, 27, 28, 30, 33, 34, 36))
Wide = collections.namedtuple("Wide", "name counter0 counters chmap moved b on_b")


def _wide(name, counter0, counters, chmap=FULL_MAP, moved=(), b=None, on_b=()):
    return Wide(name, counter0, tuple(counters), chmap, frozenset(moved), b, frozenset(on_b))


def _split(n, n_b, seed, keep=()):
    """n_b of the events 0 .. n - 1, seeded, none of `keep` among them."""
    free = [e for e in range(n) if e not in set(keep)]
    return np.random.default_rng(seed).choice(free, n_b, replace=False).tolist()


# The connections with gaps and many events.  Every one keeps adjacent counters, or the tracking's gcd would take a stride for the
# interval.  moved: events whose packets lie one used channel up, off every prediction; b / on_b: a second planted hypothesis and
# the events that lie on ITS prediction.  What each is for: tests/_le_csa2_paths.py's tags and WIDE_RUNS.
WINDOWS = (
    # the last byte of the window, 1023 + span, and the first: winners at j = 1023 and j = 0 of adjacent blocks; two tiles each
    _wide("tail, span 1711", at(20, 255, 3), list(range(300)) + [1500 + i for i in range(301)]),
    _wide("tail, span cut", at(52, 255, 3), list(range(511)) + [3072] + [3073 + i for i in range(102)]),
    _wide("head, span 1711", at(21, 0, 0), list(range(300)) + [1500 + i for i in range(301)]),
    _wide("head, span cut", at(53, 0, 0), list(range(511)) + [3072] + [3073 + i for i in range(102)]),
    # a tile that spans more than 2^16 counters; winners in block 63, where every window wraps
    _wide("tile spans 2^16", 65535, [0, 1] + [130 * i for i in range(2, 600)]),
    # (... and ten events behind a gap of 4 800 in the same tile: the second loop runs over a tile whose near events wrap)
    _wide("n_e wraps in tile two", 64512, list(range(512)) + [65400 + i for i in range(200)] + [70400 + i for i in range(10)]),
    # d_last around the cut
    _wide("d_last cut - 1", at(6, 63, 2), list(range(30)) + [3071]),
    _wide("d_last cut", at(6, 64, 1), list(range(30)) + [3072]),
    _wide("d_last cut + 1", at(41, 128, 3), list(range(30)) + [3072, 3073]),
    # far events alone lift A above B: 12 adjacent events, 4 on A and 8 on B, and 12 behind a gap of 5 000, all on A
    _wide("far decides, thread 0", at(13, 0, 1), list(range(12)) + [5000 + i for i in range(12)], b=at(30, 9, 0), on_b=_split(12, 8, 1)),
    _wide("far decides, thread 63", at(34, 63, 2), list(range(12)) + [5000 + i for i in range(12)], b=at(2, 99, 1), on_b=_split(12, 8, 2)),
    _wide("far decides, thread 64", at(57, 64, 0), list(range(12)) + [5000 + i for i in range(12)], b=at(57, 11, 3), on_b=_split(12, 8, 3)),
    _wide("far decides, thread 255", at(63, 255, 2), list(range(12)) + [5000 + i for i in range(12)], b=at(19, 255, 2), on_b=_split(12, 8, 4)),
)
COUNTS = (
    _wide("511 events", at(25, 100, 0), range(511)),
    _wide("512 events", at(38, 17, 3), range(512)),
    _wide("513 events", at(4, 63, 1), range(513)),
    _wide("1024 events", at(59, 64, 2), range(1024)),
    # (d_last on the cut in tile one, a third tile of one event)
    _wide("1025 events", 1023, list(range(511)) + [3072] + [3073 + i for i in range(513)], moved=(63, 64, 100, 511, 512, 513)),
    # a map of 20 channels: without REMAP 17 of 37 predictions are unknown, those of the moved events (the last among them) are not
    _wide("map of 20, last event off", at(46, 45, 1), range(603), chmap=TWENTY_MAP, moved=(70, 400, 602)),
    # B's events lie in the second tile alone
    _wide("second only in tile two", at(27, 180, 2), range(602), b=at(27, 20, 1), on_b=[512 + e for e in _split(90, 60, 5)]),
)
WIDE_AA = 0x8E5A3C00


def _wide_cands(k, w):
    used = [c for c in range(37) if (w.chmap >> c) & 1]
    event_of = {n: e for e, n in enumerate(w.counters)}

    def channel_of(n):
        e = event_of[n]
        ch = csa2(WIDE_AA + 0x10001 * k, (w.b if e in w.on_b else w.counter0) + n, w.chmap)
        return used[(used.index(ch) + 1) % len(used)] if e in w.moved else ch

    return plant(WIDE_AA + 0x10001 * k, 0x5EED00 + k, w.counter0, w.counters, w.chmap, base=3500 + 411 * k, channel_of=channel_of)


@functools.lru_cache(maxsize=None)
def wide_list(group):
    """WINDOWS or COUNTS ("windows", "counts") as one candidate list with 10 non-members: (conns, cands, names)."""
    raw, by_key = [], {}
    for k, w in enumerate(dict(windows=WINDOWS, counts=COUNTS)[group]):
        k += 32 * (group == "counts")
        raw += _wide_cands(k, w)
        by_key[(WIDE_AA + 0x10001 * k, 0x5EED00 + k)] = w.name
    return _grouped(raw, by_key, np.random.default_rng(71), 10)


@functools.lru_cache(maxsize=None)
def list_model(build, arg, flags):
    """(tracks, pkts, (sels, sel_pkts)) of the models on pair_list() or wide_list(arg), whole."""
    conns, cands, _ = globals()[build]() if arg is None else globals()[build](arg)
    tracks, pkts = tracked(conns, cands, flags)
    return tracks, pkts, select(conns, cands, tracks, pkts, flags)


def without_last_connection(conns, cands, want):
    """The model's (sels, sel_pkts) when the last connection is cut off: the others are unchanged (no rule looks across
    connections), its candidates are no members."""
    k = len(conns) - 1
    return want[0][:k], [None if c.channel >= k else p for c, p in zip(cands, want[1])]
