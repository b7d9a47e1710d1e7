"""Test-side model of LE following through connection parameter updates (include/btbbx.h btbbx_le_span_*), written from
the rules of the contract in plain Python on top of tests/_le_follow.py's pieces: loops over spans and events, no tables, no
searches (le_span.h works in rounds over the event table, with a prefix sum, atomic minima and binary searches).

* span_follow: the stage; Rules: its branch points as options, Rules() is the model, any other value a deliberately wrong one
  (tests/test_le_span_model.py shows that the lattice tells each from the right one)
* SpanWorld: lf.World with connections planted by a FORWARD WALK: the anchor of the event at an update's instant I is the anchor of
  I - 1 + P_old + WinOffset * unit + a chosen position inside the window, later events are P_new apart, on the forward selections
  lt.csa1_at / lc.csa2 at the absolute counter under the planted map.  The walk shares no arithmetic with the model's G.
* lattice / chain_world / wrap_world / crowd_world / seam_world: the lists the CPU and GPU tests share
"""
import collections
import functools

import numpy as np

import _le
import _le_csa2 as lc
import _le_discover as ld
import _le_follow as lf
import _le_track as lt

CAPPED, REFUSED = 32, 64
ST_GAP = 3
NONE = 0xFFFFFFFF
NO_STOP = lf.NO_STOP

Span = collections.namedtuple("Span", "map counter_first stop n_before n_on n_off n_beyond n_gap n_control n_map_updates n_param_updates "
                              "n_spans interval algorithm flags")
SPkt = collections.namedtuple("SPkt", "counter epoch span kind opcode expected on_hop state applied")
Rec = collections.namedtuple("Rec", "origin base first_event n_events pdu interval win_offset latency timeout win_size flags")


class Rules:
    def __init__(self, **kw):
        self.window_delay = False        # T' = G + unit_bits * (1 + WinOffset'), as for a CONNECT_IND
        self.allow_1x = False            # allowance jitter_bits in later spans
        self.g_from_pdu = False          # G from the PDU's own event instead of L
        self.base_plus_one = False       # B = I + 1
        self.first_round = False         # the first counter of a later span rounded instead of floored
        self.interval_from_pdu = False   # the new interval used from the PDU's event on
        self.instant_largest = False     # I_s the largest
        self.small_rank = False          # the smaller rank applies
        self.cap_off = 0                 # applies iff s < max_updates + this
        self.interval_min, self.interval_max = 6, 3200
        self.win_size_min, self.win_size_over, self.win_offset_over = 1, 0, 0
        self.gap_as_beyond = False
        self.later_maps_ignored = False  # map updates of later spans ignored
        self.win_offset_ignored = False
        self.count_packets = False       # tallies per packet
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


MODEL = Rules()
VARIANTS = dict(window_delay=dict(window_delay=True), allow_1x=dict(allow_1x=True), g_from_pdu=dict(g_from_pdu=True),
                base_plus_one=dict(base_plus_one=True), first_round=dict(first_round=True), interval_from_pdu=dict(interval_from_pdu=True),
                instant_largest=dict(instant_largest=True), small_rank=dict(small_rank=True), cap_plus_one=dict(cap_off=1),
                cap_minus_one=dict(cap_off=-1), interval_min_5=dict(interval_min=5), interval_min_7=dict(interval_min=7),
                interval_max_3201=dict(interval_max=3201), interval_max_3199=dict(interval_max=3199), win_size_min_0=dict(win_size_min=0),
                win_size_min_2=dict(win_size_min=2), win_size_max_plus=dict(win_size_over=1), win_size_max_minus=dict(win_size_over=-1),
                win_offset_max_plus=dict(win_offset_over=1), win_offset_max_minus=dict(win_offset_over=-1),
                gap_as_beyond=dict(gap_as_beyond=True), later_maps_ignored=dict(later_maps_ignored=True),
                win_offset_ignored=dict(win_offset_ignored=True), count_packets=dict(count_packets=True))


def params_valid(interval, win_size, win_offset, rules=MODEL):
    return (rules.interval_min <= interval <= rules.interval_max and
            rules.win_size_min <= win_size <= min(8, interval - 1) + rules.win_size_over and win_offset <= interval + rules.win_offset_over)


def span_follow(conns, cands, tracks, pkts, seeds, words, n_words, unit_bits, jitter_bits, max_updates, rules=MODEL, trace=None):
    """The arguments of lf.follow and max_updates.  Returns (spans, spkts, recs): one Span or None (zeros) per connection, one SPkt or
    None (0xff) per candidate, and per connection a list of max_updates + 1 Rec or None (zeros)."""
    k = len(tracks)
    spkts = [None] * len(pkts)
    members = [[] for _ in range(k)]
    for i, p in enumerate(pkts):
        if p is not None and cands[i].channel < k:
            members[cands[i].channel].append(i)
    spans, all_recs = [], []
    le16 = lambda pl, at: int.from_bytes(pl[at:at + 2], "little")                    # noqa: E731
    for g in range(k):
        order = sorted(members[g], key=lambda i: pkts[i].rank)
        s = seeds[g]
        ctl = {}
        for i in order:                                                        # the follow stage's rule 3
            c = cands[i]
            if (c.header0 & 3) == 3 and c.length >= 1:
                ctl[i] = lf.read_payload(words[c.stream], n_words, c.offset, c.length, pkts[i].channel)
        enc = [i for i in order if i in ctl and ctl[i][0] == 5 and cands[i].length == 1][:1]
        kind, opcode = {}, {}
        closed = False
        for i in order:
            kind[i], opcode[i] = lf.DATA, 0xFF
            if i in ctl:
                if closed:
                    kind[i] = lf.OPAQUE
                else:
                    kind[i], opcode[i] = lf.CONTROL, ctl[i][0]
                    if enc and i == enc[0]:
                        kind[i], closed = lf.ENC_START, True
                    elif ctl[i][0] == 2 and cands[i].length == 2:
                        kind[i] = lf.TERMINATE
        if s is None:
            spans.append(None)
            all_recs.append([None] * (max_updates + 1))
            for i in order:
                spkts[i] = SPkt(0, 0, 0, kind[i], opcode[i], 0xFF, 0, 0, 0)
            continue
        events = {}
        for i in order:
            events.setdefault(pkts[i].event, []).append(i)
        ev = sorted(events)
        A = {e: cands[events[e][0]].offset for e in ev}
        C = {e: pkts[events[e][0]].channel for e in ev}
        is_param = lambda i: kind[i] == lf.CONTROL and ctl[i][0] == 0 and cands[i].length == 12                 # noqa: E731
        # rules 1 to 6: span by span
        sp, Int, T, B, allow, start = 0, s.interval, s.t0, 0, jitter_bits, 0
        recs = [Rec(T, 0, NONE, 0, NONE, s.interval, s.win_offset, s.latency, s.timeout, s.win_size, 1)]
        cnt, span_of, early, applied = {}, {}, {}, set()
        stop, sflags = NO_STOP, 0
        while True:
            P = Int * unit_bits
            tail = ev[start:]
            prev = None
            for e in tail:
                span_of[e] = sp
                cnt.pop(e, None)
                early[e] = A[e] + allow < T
                if early[e]:
                    continue
                if prev is None:
                    cnt[e] = B + (A[e] + allow - T + (P // 2 if rules.first_round and sp else 0)) // P
                else:
                    cnt[e] = cnt[prev] + (A[e] - A[prev] + P // 2) // P
                prev = e
            counted = [e for e in tail if not early[e]]
            first = counted[0] if counted else NONE
            found = []
            for i in order:
                e = pkts[i].event
                if is_param(i) and e in span_of and span_of[e] == sp and e >= (tail[0] if tail else 0) and not early[e]:
                    delta = (le16(ctl[i], 10) - cnt[e]) % 65536
                    if delta < 32767:
                        found.append((cnt[e] + delta, pkts[i].rank, i, e))
            if not found:
                recs[sp] = recs[sp]._replace(first_event=first, n_events=len(counted))
                break
            at = (max if rules.instant_largest else min)(f[0] for f in found)
            mine = [e for e in counted if cnt[e] < at]
            able = [f for f in found if f[0] == at and cnt[f[3]] < at]
            pick = (min if rules.small_rank else max)(able, key=lambda f: f[1]) if able else None
            new = None
            if pick is not None and sp < max_updates + rules.cap_off:
                pl = ctl[pick[2]]
                new = dict(win_size=pl[1], win_offset=le16(pl, 2), interval=le16(pl, 4), latency=le16(pl, 6), timeout=le16(pl, 8))
                if not params_valid(new["interval"], new["win_size"], new["win_offset"], rules):
                    new = None
            if new is None:
                stop = at
                sflags = lf.STOPPED | (CAPPED if sp == max_updates else REFUSED)
                recs[sp] = recs[sp]._replace(first_event=first, n_events=len(mine))
                break
            last = mine[-1]
            if rules.interval_from_pdu:
                last = pick[3]
                mine = [e for e in mine if e <= last]
            src = pick[3] if rules.g_from_pdu else last
            G = A[src] + (at - cnt[src]) * P
            recs[sp] = recs[sp]._replace(first_event=first, n_events=len(mine))
            T = G + (0 if rules.win_offset_ignored else new["win_offset"] * unit_bits) + (unit_bits if rules.window_delay else 0)
            B = at + (1 if rules.base_plus_one else 0)
            Int, allow, start = new["interval"], jitter_bits if rules.allow_1x else 2 * jitter_bits, ev.index(last) + 1
            sp += 1
            applied.add(pick[2])
            recs.append(Rec(T, B & 0xFFFFFFFF, NONE, 0, pick[2], Int, new["win_offset"], new["latency"], new["timeout"], new["win_size"], 1))
        # rule 7: the follow stage's rules 3 to 7 over the final counters
        n_param = 0
        ups = []
        for i in order:
            e = pkts[i].event
            if kind[i] != lf.CONTROL or early[e]:
                continue
            pl, c = ctl[i], cnt[e]
            if pl[0] == 1 and cands[i].length == 8:
                m = int.from_bytes(pl[1:6], "little") & lf.MAP37
                delta = (le16(pl, 6) - c) % 65536
                if delta < 32767 and lt.popcount(m) >= 2 and c < stop and not (rules.later_maps_ignored and span_of[e]):
                    ups.append((c + delta, pkts[i].rank, m, i))
            elif pl[0] == 0 and cands[i].length == 12 and (le16(pl, 10) - c) % 65536 < 32767:
                kind[i] = lf.PARAM_UPDATE
                n_param += 1
        for u in ups:
            kind[u[3]] = lf.MAP_UPDATE
        state = {}
        for e in ev:
            if early[e]:
                state[e] = (lf.ST_BEYOND if rules.gap_as_beyond else ST_GAP) if span_of[e] else lf.ST_BEFORE
            else:
                state[e] = lf.ST_BEYOND if cnt[e] >= stop else lf.ST_COUNTED
        in_force, epoch = {}, {}
        for e in ev:
            epoch[e], in_force[e] = 0, s.map
            if e in cnt:
                mine = [u for u in ups if u[0] <= cnt[e]]
                epoch[e] = len(mine)
                if mine:
                    in_force[e] = max(mine, key=lambda u: u[:2])[2]
        exp, on = {1: {}, 2: {}}, {1: 0, 2: 0}
        weight = {e: len(events[e]) if rules.count_packets else 1 for e in ev}
        for e in ev:
            if state[e] == lf.ST_COUNTED:
                exp[1][e] = lf.predict1(s.hop, cnt[e], in_force[e], conns[g].access_address)
                exp[2][e] = lf.predict2(conns[g].access_address, cnt[e], in_force[e])
                for a in (1, 2):
                    on[a] += weight[e] * (exp[a][e] == C[e])
        algorithm = 2 if s.chsel and on[2] >= on[1] else 1
        tally = lambda st: sum(weight[e] for e in ev if state[e] == st)        # noqa: E731
        predicted = [e for e in ev if state[e] == lf.ST_COUNTED]
        flags = lf.SEEDED | (lf.COUNTED if cnt else 0) | sflags | (lf.ENCRYPTED if enc else 0)
        if any(kd == lf.TERMINATE for kd in kind.values()):
            flags |= lf.TERMINATED
        firsts = [e for e in ev if span_of[e] == 0 and not early[e]]
        if trace is not None:
            trace[g] = dict(cnt=dict(cnt), span_of=span_of, state=state, stop=stop, in_force=in_force)
        spans.append(Span(in_force[predicted[-1]] if predicted else s.map, cnt[firsts[0]] & 0xFFFFFFFF if firsts else 0, stop & 0xFFFFFFFF,
                          tally(lf.ST_BEFORE), on[algorithm], tally(lf.ST_COUNTED) - on[algorithm], tally(lf.ST_BEYOND), tally(ST_GAP),
                          len(ctl), len(ups), n_param, sp + 1, Int, algorithm, flags))
        all_recs.append((recs + [None] * (max_updates + 1))[:max(max_updates + 1, len(recs))])
        for e in ev:
            for i in events[e]:
                x = exp[algorithm].get(e, 0xFF)
                spkts[i] = SPkt(cnt.get(e, 0) & 0xFFFFFFFF, min(epoch[e], 0xFFFF), span_of[e], kind[i], opcode[i], x, int(x == C[e]), state[e],
                                int(i in applied))
    return spans, spkts, all_recs


def span_array(spans, dtype):
    a = np.zeros(len(spans), dtype)
    for i, f in enumerate(spans):
        if f is not None:
            a[i] = tuple(f)
    return a


def spkt_array(spkts, dtype):
    a = np.zeros(len(spkts), dtype)
    if not len(spkts):
        return a
    none = np.array([p is None for p in spkts], bool)
    rows = np.array([(0,) * len(SPkt._fields) if p is None else p for p in spkts], np.int64)
    for j, name in enumerate(SPkt._fields):
        a[name] = rows[:, j]
    a.view(np.uint8).reshape(len(spkts), dtype.itemsize)[none] = 0xFF
    return a


def rec_array(recs, dtype, max_updates):
    a = np.zeros((len(recs), max_updates + 1), dtype)
    for g, row in enumerate(recs):
        assert len(row) == max_updates + 1, (g, len(row))
        for s, r in enumerate(row):
            if r is not None:
                a[g, s] = tuple(r) + ((0,) * 6,)
    return a


# ---- planted connections ----------------------------------------------------------------------------------------------
def param_ind(instant, interval, win_offset=1, win_size=1, latency=0, timeout=100):
    """LL_CONNECTION_UPDATE_IND: (header0, payload)."""
    return 3, (bytes([0, win_size]) + win_offset.to_bytes(2, "little") + interval.to_bytes(2, "little") + latency.to_bytes(2, "little") +
               timeout.to_bytes(2, "little") + (instant % 65536).to_bytes(2, "little"))


class Up(collections.namedtuple("Up", "instant interval win_offset win_size pos said latency timeout")):
    """A planted parameter update: at counter `instant` the connection goes on with `interval`, the event of that counter `pos` bits
    into the transmit window.  said: the counter of the event that carries the PDU (None: no PDU is written)."""
    def __new__(cls, instant, interval, win_offset=1, win_size=1, pos=0, said=None, latency=0, timeout=100):
        return super().__new__(cls, instant, interval, win_offset, win_size, pos, said, latency, timeout)


class SpanWorld(lf.World):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.by_anchor = {}                # name -> {anchor: (counter, channel)}

    def walk(self, name, counters, ups=(), interval=6, dev=None, pdus=None, at=0, **kw):
        """The events with these absolute counters of a connection that applies the updates `ups` (ascending instants): the grid is
        walked forward from t0 + at over EVERY counter up to the last, seen or not; dev: counter -> the deviation of its seen anchor."""
        counters = list(counters)
        grid, iv, o, todo = {}, interval, None, list(ups)
        pdus = {c: list(v) for c, v in (pdus or {}).items()}
        for u in ups:
            if u.said is not None:
                pdus.setdefault(u.said, []).append(param_ind(u.instant, u.interval, u.win_offset, u.win_size, u.latency, u.timeout))
        first = counters[0]
        for c in range(first, counters[-1] + 1):
            if o is None:
                o = 0
            elif todo and todo[0].instant == c:
                u = todo.pop(0)
                o += iv * self.unit + u.win_offset * self.unit + u.pos
                iv = u.interval
            else:
                o += iv * self.unit
            grid[c] = o
        shift = lambda c: grid[c] - (c - first) * interval * self.unit + (dev(c) if dev else 0)            # noqa: E731
        # (World.conn puts counter c at t0 + c * P + at + jitter(c); the walk's grid starts at the first counter.)  A control PDU
        # that would overwrite another connection's bits: the whole connection a little later
        base = kw.pop("req_offset", None)
        base = 400 + 977 * (self.k + 1) if base is None else base
        for move in range(0, 1500, 37):
            keep = len(self.raw), len(self.adv), len(self.info), [len(x) for x in self.taken], self.k
            try:
                t0 = self.conn(name, counters, interval=interval, at=at, jitter=shift, pdus=pdus, req_offset=base + move, **kw)
                break
            except AssertionError:
                del self.raw[keep[0]:], self.adv[keep[1]:], self.info[keep[2]:]
                for x, n in zip(self.taken, keep[3]):
                    del x[n:]
                self.k = keep[4]
        else:
            raise AssertionError("no room for %s" % name)
        info = self.info[-1]
        P = interval * self.unit
        self.by_anchor[name] = {t0 + c * P + at + shift(c): (c, ch) for c, ch in zip(info.counters, info.channels)}
        return t0

    def stray(self, name, offset, ch, packet=lf.EMPTY):
        """One more packet of the connection `name` at `offset` on data channel ch (no planted event: by_anchor does not hold it)."""
        info = [i for i in self.info if i.name == name][0]
        h0, payload = packet
        self.raw.append(ld.Cand(offset, info.aa, info.crc_init, ch, h0, len(payload), _le.channel_index(int(lt.LATTICE_MHZ[ch]))))
        if (h0 & 3) == 3 and payload:
            end = offset + 80 + 8 * len(payload)
            assert end <= 64 * self.n_words
            for a, b in self.taken[ch]:
                assert end <= a or offset >= b, (name, ch, offset)
            self.taken[ch].append((offset, end))
            sym = _le.tx_bits(info.aa, _le.channel_index(int(lt.LATTICE_MHZ[ch])), bytes([h0, len(payload)]) + payload, info.crc_init)
            self.bits[ch, offset:offset + len(sym)] = sym

    def built(self, flags=lt.REMAP):
        b = super().built(flags)
        return SBuilt(*b, by_anchor=dict(self.by_anchor))


SBuilt = collections.namedtuple("SBuilt", lf.Built._fields + ("by_anchor",))


def model(b, max_updates, rules=MODEL, trace=None):
    """(seeds, spans, spkts, recs) of the model on a Built."""
    seeds = lf.seed(b.adv, b.conns, b.tracks, b.unit)
    return (seeds,) + span_follow(b.conns, b.cands, b.tracks, b.pkts, seeds, b.words, b.n_words, b.unit, b.jitter, max_updates, rules, trace)


def check_planted(b, seeds, spans, spkts, recs=None):
    """On EVERY planted seeded connection of a SpanWorld every event the model leaves COUNTED carries its planted absolute counter and
    lies on the planted channel, which is the prediction.  -> the number of packets checked."""
    n = 0
    for g, name in enumerate(b.names):
        if name is None or name not in b.by_anchor or seeds[g] is None or not name.startswith("planted"):
            continue
        want = b.by_anchor[name]
        mine = [i for i, c in enumerate(b.cands) if c.channel == g and spkts[i] is not None]
        anchor = {}
        for i in sorted(mine, key=lambda i: b.pkts[i].rank):
            anchor.setdefault(b.pkts[i].event, b.cands[i].offset)
        for i in mine:
            p = spkts[i]
            if p.state != lf.ST_COUNTED:
                continue
            assert anchor[b.pkts[i].event] in want, (name, i, p)
            c, ch = want[anchor[b.pkts[i].event]]
            assert p.counter == c & 0xFFFFFFFF and b.pkts[i].channel == ch and p.expected == ch and p.on_hop == 1, (name, p, c, ch)
            n += 1
    return n


NINE, FIVE, M36, FULL = lf.NINE, lf.FIVE, lf.M36, lc.FULL_MAP
J = lf.JITTER
MAX_UPDATES = (0, 1, 2, 3, 16)


@functools.lru_cache(maxsize=None)
def lattice():
    """The smallest shapes at which each rule can go wrong, as one shuffled, grouped list with non-members in between (unit_bits
    1250, jitter_bits 50, streams of 4096 words).  Names that begin with "planted" are connections every one of whose events lies
    on the forward walk with deviations inside the LIMIT of the contract."""
    w = SpanWorld(7)
    U = w.unit
    # ---- one update: the window's ends, the allowance, both directions
    for old, new in ((6, 8), (12, 6)):
        for wo in (0, 1, new):
            for ws in (1, min(8, new - 1)):
                for pos in (0, ws * U - 1):
                    for dl, df in ((-J, -J), (-J, J), (J, -J), (J, J)):
                        w.walk("planted: %d to %d, offset %d, size %d, pos %d, dev %d %d" % (old, new, wo, ws, pos, dl, df), range(10),
                               [Up(5, new, wo, ws, pos, said=2)], interval=old, dev=lambda c, dl=dl, df=df: {4: dl, 5: df}.get(c, 0),
                               alg=1 + (wo + ws) % 2)
    # ---- missed events around the instant
    w.walk("planted: the instant and the next two not seen", (0, 1, 2, 3, 4, 5, 9, 10, 11), [Up(6, 8, 2, 2, 700, said=1)])
    w.walk("planted: I - 1 and I - 2 not seen", (0, 1, 2, 3, 6, 7, 8, 9), [Up(6, 8, 1, 1, 300, said=2)], alg=2)
    w.walk("planted: only the PDU's event in front of the instant", (0, 7, 8, 9), [Up(7, 10, 3, 2, 100, said=0)])
    # ---- delta
    w.walk("planted: delta 0 behind an earlier event", range(8), pdus={3: [param_ind(3, 8)]})
    w.walk("planted: delta 0 in the span's first event", range(8), pdus={0: [param_ind(0, 8)]})
    w.walk("planted: delta 32766", range(8), pdus={2: [param_ind(2 + 32766, 8)]})
    w.walk("planted: delta 32767", range(8), pdus={2: [param_ind(2 + 32767, 8)]})
    # ---- invalid new parameters
    for what, kw in (("interval 5", dict(interval=5)), ("interval 3201", dict(interval=3201)), ("win_size 0", dict(interval=8, win_size=0)),
                     ("win_size 8 of interval 8", dict(interval=8, win_size=8)), ("win_size 9 of interval 12", dict(interval=12, win_size=9)),
                     ("win_offset interval + 1", dict(interval=8, win_offset=9))):
        w.walk("planted: refused, %s" % what, range(10), pdus={2: [param_ind(5, **kw)]})
    for what, iv, ws, wo in (("interval 3200", 3200, 8, 3200), ("win_size 7 of interval 8", 8, 7, 8), ("win_size 8 of interval 12", 12, 8, 0)):
        w.walk("planted: taken, %s" % what, range(10), [Up(5, iv, wo, ws, 17, said=2)])
    # ---- several updates in one span
    w.walk("planted: two instants, the smaller ends the span", range(12), [Up(5, 8, 1, 1, 40, said=3)], pdus={2: [param_ind(9, 10)]})
    w.walk("planted: one instant twice, the larger rank applies", range(12), [Up(5, 8, 2, 1, 40, said=3)], pdus={2: [param_ind(5, 10, 3)]})
    w.walk("planted: one instant twice in one event", range(12), [Up(5, 8, 2, 1, 40, said=3)], pdus={3: [param_ind(5, 10, 3)]})
    w.walk("planted: a valid update and an invalid one of larger rank", range(12), pdus={2: [param_ind(5, 8)], 3: [param_ind(5, 5)]})
    w.walk("planted: an invalid update and a valid one of larger rank", range(12), [Up(5, 8, 1, 1, 0, said=3)], pdus={2: [param_ind(5, 5)]})
    w.walk("planted: the update repeated at its own instant", range(12), [Up(5, 8, 1, 1, 0, said=3)], pdus={5: [param_ind(5, 8)]})
    # ---- GAP
    t0 = w.walk("planted: a stray event between L and T", range(10), [Up(5, 8, 8, 1, 0, said=2)])
    w.stray("planted: a stray event between L and T", t0 + 5 * 6 * U + 2 * U, 11)
    t0 = w.walk("planted: a PDU in a GAP event", range(10), [Up(5, 8, 8, 1, 0, said=2)])
    w.stray("planted: a PDU in a GAP event", t0 + 5 * 6 * U + 3 * U, 12, param_ind(7, 6))
    t0 = w.walk("planted: a map update in a GAP event", range(10), [Up(5, 8, 8, 1, 0, said=2)])
    w.stray("planted: a map update in a GAP event", t0 + 5 * 6 * U + 3 * U, 13, lf.map_ind(NINE, 7))
    # ---- the second update's instant, right only under the new counters: span 1's events stand 8 units apart
    w.walk("planted: two updates", range(16), [Up(4, 8, 1, 1, 10, said=1), Up(9, 6, 2, 2, 20, said=6)], alg=2)
    # ---- map updates and parameter updates together
    w.walk("planted: a map update announced in span 0 for span 1", range(14), [Up(5, 8, 1, 1, 0, said=2)], maps=[(8, NINE)],
           pdus={3: [lf.map_ind(NINE, 8)]})
    w.walk("planted: a map update announced in span 1", range(14), [Up(5, 8, 1, 1, 0, said=2)], maps=[(10, FIVE)], pdus={7: [lf.map_ind(FIVE, 10)]},
           alg=2)
    w.walk("planted: a map update in a BEYOND event", range(12), pdus={2: [param_ind(5, 5)], 7: [lf.map_ind(NINE, 9)]})
    w.walk("planted: a map update and the parameter update at one instant", range(14), [Up(5, 8, 1, 1, 0, said=2)], maps=[(5, M36)],
           pdus={1: [lf.map_ind(M36, 5)]})
    # ---- the algorithm through an update
    w.walk("planted: #2 through an update", range(16), [Up(6, 10, 1, 2, 900, said=3)], alg=2)
    w.walk("planted: #1 with ChSel 1 through an update", range(16), [Up(6, 10, 1, 2, 900, said=3)], alg=1, chsel=1)
    # ---- control PDUs
    w.walk("planted: ENC START in front of the update", range(12), pdus={1: [lf.ENC_REQ], 2: [param_ind(5, 8)]})
    w.walk("planted: TERMINATE behind an update", range(12), [Up(5, 8, 1, 1, 0, said=2)], pdus={8: [lf.TERMINATE_IND]})
    w.walk("planted: ENC START behind an update", range(12), [Up(5, 8, 1, 1, 0, said=2)], pdus={7: [lf.ENC_REQ], 8: [param_ind(10, 6)]})
    # ---- BEFORE, unseeded
    w.walk("events BEFORE t0 and an update", range(12), [Up(7, 8, 1, 1, 0, said=4)], win_offset=6, at=-7 * U)
    w.walk("unseeded with an update", range(10), [Up(5, 8, 1, 1, 0, said=2)], request=False)
    w.noise(40)
    return w.built()


@functools.lru_cache(maxsize=None)
def chain_world():
    """Chains of 1, 2 and 3 updates at unit_bits 120 (WinSize' 1: 120 + 4 * 50 bits is less than the shortest interval), each with
    a map update in the last span."""
    w = SpanWorld(11, unit=120)
    ups = [Up(6, 8, 1, 1, 30, said=2), Up(13, 7, 2, 1, 60, said=9), Up(21, 10, 0, 1, 0, said=16)]
    for n in (1, 2, 3):
        for alg in (1, 2):
            last = ups[n - 1].instant
            w.walk("planted: chain of %d, #%d" % (n, alg), range(30), ups[:n], alg=alg, maps=[(last + 5, NINE)],
                   pdus={last + 1: [lf.map_ind(NINE, last + 5)]}, dev=lambda c: (c * 29) % 101 - 50, hop=5 + n)
    w.walk("planted: chain of 3, events missed", [c for c in range(30) if c not in (5, 6, 12, 13, 14, 20)], ups, dev=lambda c: (c * 31) % 101 - 50)
    w.noise(20)
    return w.built()


@functools.lru_cache(maxsize=None)
def wrap_world():
    """lf.wrap_world's geometry (unit_bits 2, jitter_bits 0): an update announced at counter 65 530 for the instant 65 536 (the PDU
    says 0), one whose span begins at 65 535, and one announced behind 65 536 by the low sixteen bits."""
    w = SpanWorld(33, unit=2, n_words=12800, ifs=0, jitter=0)
    near = (65527, 65528, 65529, 65530, 65534, 65535, 65536, 65537, 65538, 65540)
    w.walk("planted: instant 65536", near, [Up(65536, 8, 1, 1, 1, said=65530)])
    w.walk("planted: instant 65535", near, [Up(65535, 8, 0, 2, 3, said=65529)], hop=11)
    w.walk("planted: announced at 65537 for 65540", near, [Up(65540, 7, 2, 1, 0, said=65537)], hop=9)
    w.walk("planted: counters from 0", range(0, 40, 3), [Up(21, 9, 1, 1, 0, said=3)])
    w.noise(10)
    return w.built()


CROWD_CONNS, CROWD_TILE = 1450, 2048


@functools.lru_cache(maxsize=None)
def crowd_world():
    """About 1 450 connections of 12 events side by side (unit_bits 120, ascending access addresses, so a world is laid out by counting
    packets), each with one parameter update (6 to 8 at counter 6) and one map update across it (announced at 3 for 9).  A connection
    lies across every scan tile seam (2048 events); for the one on the first seam L is the last event in front of the seam and f_1
    the first behind it; the one on the second seam has a GAP event -- a stray packet in front of the new window -- on the seam."""
    w = SpanWorld(43, unit=120, n_words=16384)
    p = 0
    for k in range(CROWD_CONNS):
        room = -p % CROWD_TILE                                                # table positions in front of the next seam
        second, stray = (), False
        if 18 <= room <= 30:
            second = tuple(range(room - 18))                                   # (the next connection begins six positions in front of the seam)
        elif room == 6:
            stray = p // CROWD_TILE == 1
        name = "planted: crowd %d" % k
        t0 = w.walk(name, range(12), [Up(6, 8, 4 if stray else 1, 1, 20, said=2)], alg=1 + k % 2, hop=5 + k % 12, maps=[(9, NINE)],
                    pdus={3: [lf.map_ind(NINE, 9)]}, second=second, req_offset=2000 + 700 * k, aa=0x20000000 + 0x3001 * k, request=k % 10 != 9)
        if stray:
            w.stray(name, t0 + 6 * 6 * 120 + 2 * 120, 3)
        p += 12 + len(second) + (1 if stray else 0)
    w.noise(40)
    return w.built()


@functools.lru_cache(maxsize=None)
def seam_world():
    """One connection of 5 000 events with 8 updates beside 1 000 small ones with one update each (unit_bits 120)."""
    w = SpanWorld(53, unit=120)
    ups = [Up(30 * (u + 1), (8, 6, 10, 7, 9, 6, 12, 8)[u], u % 3, 1, 10 * u, said=30 * (u + 1) - 8) for u in range(8)]
    w.walk("planted: large", range(5000), ups, alg=2, second=range(0, 5000, 3), req_offset=100, maps=[(20, NINE), (205, FIVE)],
           pdus={5: [lf.map_ind(NINE, 20)], 200: [lf.map_ind(FIVE, 205)]})
    for k in range(1000):
        w.walk("planted: small %d" % k, range(6), [Up(3, 8, 1, 1, 0, said=1)], alg=1 + k % 2, hop=5 + k % 12, request=k % 3 != 0,
               req_offset=2000 + 197 * k)
    return w.built()


@functools.lru_cache(maxsize=None)
def end_world():
    """An LL_CONNECTION_UPDATE_IND across the streams' end: its instant's low octet is the streams' last eight bits, the high octet
    is read as zeros (World.conn writes no packet that ends beyond the streams, so its first 144 bits are written here); beside it
    a connection whose update lies inside."""
    w = SpanWorld(59)
    U = w.unit
    at = 64 * lf.N_WORDS - 144
    w.walk("planted: inside", range(10), [Up(5, 8, 1, 1, 0, said=2)])
    w.walk("an update across the streams' end", range(28, 40), pdus={30: [param_ind(34, 8)]}, req_offset=at - 30 * 6 * U - 352 - 2 * U)
    last = w.info[-1]
    ch = last.channels[2]
    assert [c.offset for c in w.raw if c.access_address == last.aa and c.length == 12] == [at]
    w.bits[ch, at:] = _le.tx_bits(last.aa, ch, bytes((3, 12)) + param_ind(34, 8)[1], last.crc_init)[:144]
    w.noise(10)
    return w.built()


# ---- a capture for the host wrapper -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def span_capture():
    """37 data streams and three advertising streams of 4 600 words of noise with three seeded connections, each with one parameter
    update, their CONNECT_INDs on stream 37.  Every event is a PDU of the central and an empty PDU of the peripheral 150 bits behind
    it; the anchors are walked forward.  -> (Capture, planted: (aa, crc_init, alg, {anchor: counter}))"""
    n_words, U = 4600, lf.UNIT
    b = ld._Builder(40, n_words, lf.CHAIN_MHZ, 777)
    rng = np.random.default_rng(19)
    total = 64 * n_words
    plans = [dict(alg=1, hop=11, interval=6, up=Up(8, 8, 1, 1, 100, said=4), off=300),
             dict(alg=2, hop=9, interval=7, up=Up(6, 6, 2, 2, 400, said=3), off=1500),
             dict(alg=1, hop=5, interval=8, up=Up(10, 6, 0, 1, 0, said=5), off=2700)]
    planted = []
    for k, p in enumerate(plans):
        aa, ci = ld.good_aa(rng), int(rng.integers(0, 1 << 24))
        body = lf.connect_ind(aa, ci, FULL, p["hop"], p["interval"], win_size=2, win_offset=1, chsel=int(p["alg"] == 2))
        b.plant(37, p["off"], _le.ADV_AA, _le.ADV_CRC_INIT, body[4], 34, "CONNECT_IND %d" % k, payload=body[6:40])
        u, iv, o, anchors = p["up"], p["interval"], p["off"] + 352 + 2 * U + 300, {}
        for c in range(40):
            if c == u.instant:
                o += iv * U + u.win_offset * U + u.pos
                iv = u.interval
            elif c:
                o += iv * U
            ch = lt.csa1_at(0, p["hop"], c + 1, FULL) if p["alg"] == 1 else lc.csa2(aa, c, FULL)
            at = o + int(rng.integers(-20, 21))
            h0, payload = param_ind(u.instant, u.interval, u.win_offset, u.win_size) if c == u.said else \
                (2, bytes(rng.integers(0, 256, 1 + c % 5, dtype=np.uint8)))
            if at + 80 + 8 * len(payload) + 150 + 80 > total:
                break
            b.plant(ch, at, aa, ci, h0, len(payload), "connection %d" % k, payload=payload)
            b.plant(ch, at + 80 + 8 * len(payload) + 150, aa, ci, 1, 0, "connection %d" % k)
            anchors[at] = c
        planted.append((aa, ci, p["alg"], anchors))
    words = b.words(n_words + 5)
    words.flags.writeable = False
    return ld.Capture(words, n_words, n_words + 5, total - 39, lf.CHAIN_MHZ, tuple(b.planted), 27), tuple(planted)


@functools.lru_cache(maxsize=None)
def capture_model(max_updates):
    cap = span_capture()[0]
    conns, cands, tracks, pkts, adv, seeds, follows, fpkts = lf.capture_model(cap)
    return (conns, cands, tracks, pkts, adv, seeds, follows, fpkts) + span_follow(conns, cands, tracks, pkts, seeds, cap.words, cap.n_words,
                                                                                   lf.UNIT, lf.JITTER, max_updates)


@functools.lru_cache(maxsize=None)
def world_model(name, max_updates):
    return model(WORLDS[name](), max_updates)


WORLDS = dict(lattice=lattice, chain=chain_world, wrap=wrap_world, crowd=crowd_world, seam=seam_world, end=end_world)
