"""Test-side model of LE following from CONNECT_IND (include/btbbx.h btbbx_le_seed_* / btbbx_le_epoch_*), written
from the rules of the contract in plain Python on top of tests/_le_track.py's model of the tracking -- sorted(), loops and
dictionaries --, not from the kernels (le_follow.h lays slots and events out in tables, sums the counters with one prefix scan and
finds the map in force by a binary search of a radix-sorted list).

* parse_request / seed: the seed stage; follow: the follow stage; Rules: their branch points as options, Rules() is the model, any
  other value a deliberately wrong one (tests/test_le_follow_model.py shows that the lattice below tells each from the right one)
* connect_ind / adv_record: a CONNECT_IND as the 64 bytes and the record btbbx_le_decode_hits_device leaves
* World: planted connections -- they hop by the FORWARD selections of tests/_le_track.py (csa1_at) and tests/_le_csa2.py (csa2),
  which share nothing with the model's closed forms --, their requests and the stream bits of their control PDUs
* lattice / seam_world / wrap_world: the lists the CPU and GPU tests share; crowd_world / byte_world / tally_world: the worlds laid
  out by position for tests/_le_follow_paths.py, which names the kernels' paths they drive; cut_model: their cuts' models
"""
import collections
import functools

import numpy as np

import _le
import _le_csa2 as lc
import _le_discover as ld
import _le_track as lt

SEEDED, COUNTED, STOPPED, TERMINATED, ENCRYPTED = 1, 2, 4, 8, 16
ST_COUNTED, ST_BEFORE, ST_BEYOND = 0, 1, 2
DATA, CONTROL, MAP_UPDATE, PARAM_UPDATE, TERMINATE, ENC_START, OPAQUE = range(7)
MAP37 = (1 << 37) - 1
NO_STOP = (1 << 64) - 1
UNIT, IFS, JITTER = lt.UNIT, lt.IFS, lt.JITTER

Seed = collections.namedtuple("Seed", "t0 map access_address crc_init request interval win_offset latency timeout win_size hop sca "
                              "chsel init_a adv_a tx_add rx_add flags")
Follow = collections.namedtuple("Follow", "map counter_first stop n_before n_on n_off n_beyond n_control n_map_updates algorithm flags")
FPkt = collections.namedtuple("FPkt", "counter epoch kind opcode expected on_hop state")


class Rules:
    def __init__(self, **kw):
        self.first_round = False         # c_f rounded to the nearest interval instead of floored
        self.no_jitter = False           # rule 1 without the jitter allowance
        self.delta_limit = 32767         # an update is valid iff delta < this
        self.instant_strict = False      # an update is in force from I + 1 on (I < c instead of I <= c)
        self.equal_small_rank = False    # equal instants: the smaller rank wins
        self.remap_swapped = False       # each algorithm remaps by the other's index
        self.hop_no_plus_one = False     # #1: Hop * c without the + 1
        self.chsel_decides = False       # ChSel 1 means #2, whatever the events say
        self.tie_to_1 = False
        self.count_packets = False       # the tallies count packets, not events
        self.stop_largest = False        # stop = the largest I
        self.map_octets_0_4 = False      # map' from payload octets 0..4
        self.enc_open = False            # LL_START_ENC_REQ does not close the parse
        self.r_strict = False            # a request joins iff R < first_anchor
        self.earliest_request = False
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


MODEL = Rules()
VARIANTS = dict(first_round=dict(first_round=True), no_jitter=dict(no_jitter=True), delta_32768=dict(delta_limit=32768),
                instant_strict=dict(instant_strict=True), equal_small_rank=dict(equal_small_rank=True), remap_swapped=dict(remap_swapped=True),
                hop_no_plus_one=dict(hop_no_plus_one=True), chsel_decides=dict(chsel_decides=True), tie_to_1=dict(tie_to_1=True),
                count_packets=dict(count_packets=True), stop_largest=dict(stop_largest=True), map_octets_0_4=dict(map_octets_0_4=True),
                enc_open=dict(enc_open=True), r_strict=dict(r_strict=True), earliest_request=dict(earliest_request=True))


# ---- the seed stage ---------------------------------------------------------------------------------------------------
def connect_ind(aa, crc_init, chmap, hop, interval, win_size=2, win_offset=1, latency=0, timeout=100, sca=1, chsel=0, tx_add=0, rx_add=1,
                init_a=bytes(range(0x11, 0x17)), adv_a=bytes(range(0xA1, 0xA7)), adv_type=5, length=34, top_bits=0):
    """The 64 bytes of a CONNECT_IND as btbbx_le_pkt.bytes holds them: the advertising AA, the header, the payload, a CRC of zeros.
    top_bits: bits 37..39 of the map's fifth octet."""
    h0 = adv_type | (chsel << 5) | (tx_add << 6) | (rx_add << 7)
    ll = (aa.to_bytes(4, "little") + crc_init.to_bytes(3, "little") + bytes([win_size]) + win_offset.to_bytes(2, "little") +
          interval.to_bytes(2, "little") + latency.to_bytes(2, "little") + timeout.to_bytes(2, "little") +
          (chmap | (top_bits << 37)).to_bytes(5, "little") + bytes([hop | (sca << 5)]))
    b = _le.ADV_AA.to_bytes(4, "little") + bytes([h0, length]) + bytes(init_a) + bytes(adv_a) + ll
    return b.ljust(64, b"\0")[:64]


def adv_record(offset, stream, bytes64, mhz=2402, crc_ok=1, truncated=0):
    """The record of an advertising hit, as a dict keyed like LE_PKT_DTYPE."""
    rec = dict(offset=offset, stream=stream, aa_errors=0, crc_ok=crc_ok, crc_rx=0, crc_calc=0, pdu_bytes=2 + bytes64[5],
               truncated=truncated, bytes=bytes(bytes64))
    rec.update(_le.lell_fields(bytes64, mhz))
    return rec


def adv_array(recs, dtype):
    a = np.zeros(len(recs), dtype)
    for i, r in enumerate(recs):
        for k in _le.FIELDS:
            a[i][k] = r[k]
        a[i]["bytes"] = np.frombuffer(r["bytes"], np.uint8)
    return a


def parse_request(b):
    """Rule 1's fields of the 64 bytes."""
    le = lambda at, n: int.from_bytes(b[at:at + n], "little")              # noqa: E731
    return dict(init_a=bytes(b[6:12]), adv_a=bytes(b[12:18]), aa=le(18, 4), crc_init=le(22, 3), win_size=b[25], win_offset=le(26, 2),
                interval=le(28, 2), latency=le(30, 2), timeout=le(32, 2), map=le(34, 5) & MAP37, hop=b[39] & 0x1F, sca=b[39] >> 5,
                chsel=(b[4] >> 5) & 1, tx_add=(b[4] >> 6) & 1, rx_add=(b[4] >> 7) & 1)


def is_request(r):
    return r["crc_ok"] == 1 and r["truncated"] == 0 and r["is_data"] == 0 and r["adv_type"] == 5 and r["length"] == 34


def valid_request(f):
    return (5 <= f["hop"] <= 16 and 6 <= f["interval"] <= 3200 and lt.popcount(f["map"]) >= 2 and
            1 <= f["win_size"] <= min(8, f["interval"] - 1) and f["win_offset"] <= f["interval"])


def seed(adv, conns, tracks, unit_bits, rules=MODEL):
    """One Seed or None (not SEEDED) per stored connection."""
    reqs = []
    for j, r in enumerate(adv):
        if is_request(r):
            f = parse_request(r["bytes"])
            if valid_request(f):
                reqs.append((r["offset"], r["stream"], j, f))
    out = []
    for g, t in enumerate(tracks):
        c = conns[g]
        mine = [q for q in reqs if (q[3]["aa"], q[3]["crc_init"]) == (c.access_address, c.crc_init) and
                (q[0] + 352 < t.first_anchor if rules.r_strict else q[0] + 352 <= t.first_anchor)]
        if not mine:
            out.append(None)
            continue
        off, _, j, f = (min if rules.earliest_request else max)(mine, key=lambda q: q[:3])
        out.append(Seed(off + 352 + unit_bits * (1 + f["win_offset"]), f["map"], f["aa"], f["crc_init"], j, f["interval"], f["win_offset"],
                        f["latency"], f["timeout"], f["win_size"], f["hop"], f["sca"], f["chsel"], f["init_a"], f["adv_a"], f["tx_add"],
                        f["rx_add"], SEEDED))
    return out


def seed_array(seeds, dtype):
    a = np.zeros(len(seeds), dtype)
    for i, s in enumerate(seeds):
        if s is not None:
            for k in Seed._fields:
                a[i][k] = np.frombuffer(getattr(s, k), np.uint8) if k in ("init_a", "adv_a") else getattr(s, k)
    return a


# ---- the follow stage -------------------------------------------------------------------------------------------------
def read_payload(row, n_words, offset, length, ch):
    """Rule 3: the first min(length, 12) payload octets of the packet at `offset` of one stream, dewhitened."""
    take = min(length, 12)
    raw = _le.stream_bits(row, n_words, offset + 56, 8 * take)
    return _le.bits_octets(raw ^ _le.whitening_bits(ch, 16 + 8 * take)[16:])


def _used(m):
    return [c for c in range(37) if (m >> c) & 1]


def predict1(hop, c, m, aa, rules=MODEL):
    u = (hop * (c % 37 if rules.hop_no_plus_one else (c + 1) % 37)) % 37
    if (m >> u) & 1:
        return u
    used = _used(m)
    if rules.remap_swapped:
        return used[(len(used) * lc.prn_e(c % 65536, lc.channel_id(aa))) >> 16]
    return used[u % len(used)]


def predict2(aa, c, m, rules=MODEL):
    prn, unmapped, expected = lc.predict(c % 65536, lc.channel_id(aa), m, lc.REMAP)
    if rules.remap_swapped and not (m >> unmapped) & 1:
        used = _used(m)
        return used[unmapped % len(used)]
    return expected


def follow(conns, cands, tracks, pkts, seeds, words, n_words, unit_bits, jitter_bits, rules=MODEL, trace=None):
    """conns, cands: as ld.group leaves them; tracks, pkts: what lt.track returned (len(tracks) = K, len(pkts) = N); seeds: one Seed
    or None per connection; words: the streams, one row each.  Returns (follows, fpkts): one Follow or None (zeros) per
    connection, one FPkt or None (0xff) per candidate.  trace: a dict that takes, per seeded connection, what the records do not
    hold in full -- the 64-bit counters, the updates as (I, rank, map', candidate), stop, the map in force and the state of every
    event (tests/_le_follow_paths.py numbers the kernels' tables from them)."""
    k = len(tracks)
    fpkts = [None] * len(pkts)
    members = [[] for _ in range(k)]
    for i, p in enumerate(pkts):
        if p is not None and cands[i].channel < k:
            members[cands[i].channel].append(i)
    follows = []
    for g in range(k):
        order = sorted(members[g], key=lambda i: pkts[i].rank)
        s = seeds[g]
        # rule 3: the control PDUs
        ctl = {}
        for i in order:
            c = cands[i]
            if (c.header0 & 3) == 3 and c.length >= 1:
                ctl[i] = read_payload(words[c.stream], n_words, c.offset, c.length, pkts[i].channel)
        enc = [i for i in order if i in ctl and ctl[i][0] == 5 and cands[i].length == 1][:1]
        kind, opcode = {}, {}
        closed = False
        for i in order:
            kind[i], opcode[i] = DATA, 0xFF
            if i in ctl:
                if closed and not rules.enc_open:
                    kind[i] = OPAQUE
                else:
                    kind[i], opcode[i] = CONTROL, ctl[i][0]
                    if enc and i == enc[0]:
                        kind[i], closed = ENC_START, True
                    elif ctl[i][0] == 2 and cands[i].length == 2:
                        kind[i] = TERMINATE
        if s is None:
            follows.append(None)
            for i in order:
                fpkts[i] = FPkt(0, 0, kind[i], opcode[i], 0xFF, 0, 0)
            continue
        events = {}
        for i in order:
            events.setdefault(pkts[i].event, []).append(i)
        ev = sorted(events)
        A = {e: cands[events[e][0]].offset for e in ev}
        C = {e: pkts[events[e][0]].channel for e in ev}
        P = s.interval * unit_bits
        jit = 0 if rules.no_jitter else jitter_bits
        before = {e: A[e] + jit < s.t0 for e in ev}
        cnt = {}
        prev = None
        for e in ev:                                                           # rules 1 and 2
            if before[e]:
                continue
            if prev is None:
                cnt[e] = (A[e] + jit - s.t0 + (P // 2 if rules.first_round else 0)) // P
            else:
                cnt[e] = cnt[prev] + (A[e] - A[prev] + P // 2) // P
            prev = e
        ups, params = [], []                                                   # rule 3: the updates
        for i in order:
            if kind[i] != CONTROL or pkts[i].event not in cnt:
                continue
            pl, c = ctl[i], cnt[pkts[i].event]
            if pl[0] == 1 and cands[i].length == 8:
                m = int.from_bytes(pl[0:5] if rules.map_octets_0_4 else pl[1:6], "little") & MAP37
                delta = (int.from_bytes(pl[6:8], "little") - c) % 65536
                if delta < rules.delta_limit and lt.popcount(m) >= 2:
                    ups.append((c + delta, pkts[i].rank, m, i))
            elif pl[0] == 0 and cands[i].length == 12:
                delta = (int.from_bytes(pl[10:12], "little") - c) % 65536
                if delta < rules.delta_limit:
                    params.append((c + delta, i))
        stop = NO_STOP                                                         # rule 4
        if params:
            stop = (max if rules.stop_largest else min)(p[0] for p in params)
            for _, i in params:
                kind[i] = PARAM_UPDATE
        ups = [u for u in ups if cnt[pkts[u[3]].event] < stop]
        for u in ups:
            kind[u[3]] = MAP_UPDATE
        state = {e: ST_BEFORE if before[e] else (ST_BEYOND if cnt[e] >= stop else ST_COUNTED) for e in ev}
        in_force, epoch = {}, {}                                               # rule 5
        for e in ev:
            epoch[e] = 0
            in_force[e] = s.map
            if e in cnt:
                mine = [u for u in ups if (u[0] < cnt[e] if rules.instant_strict else u[0] <= cnt[e])]
                epoch[e] = len(mine)
                if mine:
                    in_force[e] = (max(mine, key=lambda u: (u[0], -u[1])) if rules.equal_small_rank else max(mine, key=lambda u: u[:2]))[2]
        exp = {1: {}, 2: {}}                                                   # rule 6
        on = {1: 0, 2: 0}
        weight = {e: len(events[e]) if rules.count_packets else 1 for e in ev}
        for e in ev:
            if state[e] == ST_COUNTED:
                exp[1][e] = predict1(s.hop, cnt[e], in_force[e], conns[g].access_address, rules)
                exp[2][e] = predict2(conns[g].access_address, cnt[e], in_force[e], rules)
                for a in (1, 2):
                    on[a] += weight[e] * (exp[a][e] == C[e])
        algorithm = 1
        if s.chsel:
            algorithm = 2 if rules.chsel_decides or on[2] > on[1] or (on[2] == on[1] and not rules.tie_to_1) else 1
        tally = lambda st: sum(weight[e] for e in ev if state[e] == st)        # noqa: E731
        predicted = [e for e in ev if state[e] == ST_COUNTED]
        flags = SEEDED | (COUNTED if cnt else 0) | (STOPPED if stop != NO_STOP else 0) | (ENCRYPTED if enc else 0)
        if any(kd == TERMINATE for kd in kind.values()):
            flags |= TERMINATED
        first = min(cnt) if cnt else None
        if trace is not None:
            trace[g] = dict(cnt=cnt, ups=ups, stop=stop, in_force=in_force, state=state)
        follows.append(Follow(in_force[predicted[-1]] if predicted else s.map, cnt[first] & 0xFFFFFFFF if cnt else 0, stop & 0xFFFFFFFF,
                              tally(ST_BEFORE), on[algorithm], tally(ST_COUNTED) - on[algorithm], tally(ST_BEYOND), len(ctl), len(ups),
                              algorithm, flags))
        for e in ev:
            for i in events[e]:
                x = exp[algorithm].get(e, 0xFF)
                fpkts[i] = FPkt(cnt.get(e, 0) & 0xFFFFFFFF, min(epoch[e], 0xFFFF), kind[i], opcode[i], x, int(x == C[e]), state[e])
    return follows, fpkts


def follow_array(follows, dtype):
    a = np.zeros(len(follows), dtype)
    for i, f in enumerate(follows):
        if f is not None:
            a[i] = tuple(f) + ((0,) * 6,)
    return a


def fpkt_array(fpkts, dtype):
    a = np.zeros(len(fpkts), dtype)
    if not len(fpkts):
        return a
    none = np.array([p is None for p in fpkts], bool)
    rows = np.array([(0,) * len(FPkt._fields) if p is None else p for p in fpkts], np.int64)
    for j, name in enumerate(FPkt._fields):
        a[name] = rows[:, j]
    a.view(np.uint8).reshape(len(fpkts), dtype.itemsize)[none] = 0xFF
    return a


# ---- planted connections ----------------------------------------------------------------------------------------------
def map_ind(chmap, instant, top_bits=0):
    """LL_CHANNEL_MAP_IND: (header0, payload)."""
    return 3, bytes([1]) + (chmap | (top_bits << 37)).to_bytes(5, "little") + (instant % 65536).to_bytes(2, "little")


def param_ind(instant, interval=12):
    """LL_CONNECTION_UPDATE_IND."""
    return 3, bytes([0, 2]) + (1).to_bytes(2, "little") + interval.to_bytes(2, "little") + bytes(2) + (100).to_bytes(2, "little") + \
        (instant % 65536).to_bytes(2, "little")


EMPTY = (1, b"")
ENC_REQ = (3, bytes([5]))
TERMINATE_IND = (3, bytes([2, 0x13]))
N_WORDS = 4096                                         # the streams of a World: 262 144 bits each
Info = collections.namedtuple("Info", "name aa crc_init alg counters channels stop")


class World:
    """Connections planted event by event.  Stream c < 37 is data channel c (lt.LATTICE_MHZ); only control PDUs are written into the
    stream bits -- nothing else is ever read from them --, and one that lies beyond the streams' end is read as zeros."""

    def __init__(self, seed=5, unit=UNIT, n_words=N_WORDS, ifs=IFS, jitter=JITTER):
        self.rng = np.random.default_rng(seed)
        self.unit, self.n_words, self.ifs, self.jitter = unit, n_words, ifs, jitter
        self.bits = self.rng.integers(0, 2, (lt.N_STREAMS, 64 * n_words), dtype=np.uint8)
        self.taken = [[] for _ in range(lt.N_STREAMS)]
        self.raw, self.adv, self.info, self.k = [], [], [], 0

    def ids(self):
        self.k += 1
        return 0x70000000 + 0x01010101 * (self.k % 6) + 0x2357 * self.k, (0x345678 + 0x010203 * self.k) & 0xFFFFFF

    def request(self, offset, aa, crc_init, stream=37, mhz=2402, crc_ok=1, **kw):
        self.adv.append(adv_record(offset, stream, connect_ind(aa, crc_init, **kw), mhz, crc_ok))

    def conn(self, name, counters, alg=1, chmap=lc.FULL_MAP, hop=7, interval=6, win_offset=1, win_size=2, at=0, req_offset=None,
             pdus=None, maps=(), stop=None, request=True, chsel=None, aa=None, jitter=None, second=(), stream_of=None, req_kw=None):
        """Events with these absolute counters: the event of counter c lies at t0 + c * P + at (+ jitter(c)) on the channel the
        forward selection `alg` gives for c under the map in force -- maps: (instant, map) pairs, what the planted connection does,
        whatever its PDUs say -- and keeps its channel from `stop` on (a planted connection goes on with another interval there; here
        it only must not be predicted).  pdus: counter -> the packets of that event as (header0, payload), EMPTY otherwise;
        second: counters whose event gets a second, empty packet."""
        own_aa, ci = self.ids()
        aa = own_aa if aa is None else aa
        req_offset = 400 + 977 * self.k if req_offset is None else req_offset
        t0 = req_offset + 352 + self.unit * (1 + win_offset)
        if request:
            kw = dict(chmap=chmap, hop=hop, interval=interval, win_size=win_size, win_offset=win_offset, chsel=(alg == 2) if chsel is None else chsel)
            kw.update(req_kw or {})
            self.request(req_offset, aa, ci, **kw)
        P, channels = interval * self.unit, []
        for c in counters:
            m = chmap
            for instant, new in sorted(maps):
                if instant <= c:
                    m = new
            ch = lt.csa1_at(0, hop, c + 1, m) if alg == 1 else lc.csa2(aa, c, m)
            channels.append(ch)
            o = t0 + c * P + at + (jitter(c) if jitter else 0)
            packets = list((pdus or {}).get(c, [EMPTY])) + ([EMPTY] if c in second else [])
            for h0, payload in packets:
                s = ch if stream_of is None else stream_of(ch, c)
                self.raw.append(ld.Cand(o, aa, ci, s, h0, len(payload), _le.channel_index(int(lt.LATTICE_MHZ[s])) if s < lt.N_STREAMS else 0))
                if (h0 & 3) == 3 and payload and s < lt.N_STREAMS and o + 80 + 8 * len(payload) <= 64 * self.n_words:
                    for a, b in self.taken[s]:
                        assert o + 80 + 8 * len(payload) <= a or o >= b, (name, s, o)
                    self.taken[s].append((o, o + 80 + 8 * len(payload)))
                    sym = _le.tx_bits(aa, _le.channel_index(int(lt.LATTICE_MHZ[s])), bytes([h0, len(payload)]) + payload, ci)
                    self.bits[s, o:o + len(sym)] = sym
                o += 80 + 8 * len(payload) + 150
        self.info.append(Info(name, aa, ci, alg, tuple(counters), tuple(channels), stop))
        return t0

    def words(self):
        w = np.stack([_le.pack(self.bits[s]) for s in range(lt.N_STREAMS)])
        w.flags.writeable = False
        return w

    def noise(self, n):
        for k in range(n):
            ch = int(self.rng.integers(0, 37))
            self.raw.append(ld.Cand(int(self.rng.integers(0, 1 << 24)), 0x40000000 + 0x2F1 * k + int(self.rng.integers(0, 1 << 28)),
                                    int(self.rng.integers(0, 1 << 24)), ch, 3, 1, ch))

    def built(self, flags=lt.REMAP):
        """-> Built: the shuffled list grouped, tracked and seeded by the models, the words, the adv records."""
        raw = [self.raw[i] for i in self.rng.permutation(len(self.raw))]
        conns, cands = ld.group(raw, 2)
        tracks, pkts = lt.track(cands, len(conns), lt.LATTICE_MHZ, lt.N_STREAMS, self.unit, self.ifs, self.jitter, flags)
        by = {(i.aa, i.crc_init): i for i in self.info}
        names = [by[(c.access_address, c.crc_init)].name if (c.access_address, c.crc_init) in by else None for c in conns]
        return Built(conns, cands, tracks, pkts, self.adv, self.words(), names, tuple(self.info), self.unit, self.n_words, self.ifs, self.jitter)


Built = collections.namedtuple("Built", "conns cands tracks pkts adv words names info unit n_words ifs jitter")


def model(b, rules=MODEL, trace=None):
    """(seeds, follows, fpkts) of the model on a Built."""
    seeds = seed(b.adv, b.conns, b.tracks, b.unit, rules)
    return (seeds,) + follow(b.conns, b.cands, b.tracks, b.pkts, seeds, b.words, b.n_words, b.unit, b.jitter, rules, trace)


def check_planted(b, seeds, follows, fpkts):
    """On every planted, seeded connection the model gives every event its planted counter and predicts the planted channel up to
    the planted stop."""
    n = 0
    for g, name in enumerate(b.names):
        info = [i for i in b.info if i.name == name]
        if not info or seeds[g] is None or not name.startswith("planted"):
            continue
        info = info[0]
        want = dict(zip(info.counters, info.channels))
        for i, c in enumerate(b.cands):
            if c.channel != g or fpkts[i] is None or fpkts[i].state == ST_BEFORE:
                continue
            p = fpkts[i]
            full = [x for x in info.counters if x & 0xFFFFFFFF == p.counter]
            assert full, (name, p)
            if p.state == ST_COUNTED:
                assert b.pkts[i].channel == want[full[0]] and p.on_hop == 1 and p.expected == want[full[0]], (name, p, want[full[0]])
                n += 1
    return n


NINE, FIVE, TWO = lc.NINE_MAP, lc.FIVE_MAP, lc.mask_of((4, 29))
M36 = lc.FULL_MAP & ~(1 << 17)


@functools.lru_cache(maxsize=None)
def lattice():
    """The smallest shapes at which each rule can go wrong, as one shuffled, grouped list with non-members in between.  Names that
    begin with "planted" are connections every one of whose counted events lies on the forward selection."""
    w = World(5)
    full = lc.FULL_MAP
    r12 = range(12)
    # ---- seeds: what makes a request valid, which request joins
    w.conn("planted: map bit 0 and bit 36, top bits set", r12, chmap=(1 << 0) | (1 << 36) | (1 << 20), req_kw=dict(top_bits=7))
    for hop in (4, 5, 16, 17):
        w.conn("hop %d" % hop, r12, hop=hop if 5 <= hop <= 16 else 7, req_kw=dict(hop=hop))
    for iv in (5, 6, 3200, 3201):
        w.conn("interval %d" % iv, range(4), interval=iv, win_size=1)
    for ws, iv in ((0, 6), (1, 6), (8, 12), (9, 12), (5, 6), (6, 6)):
        w.conn("win_size %d of interval %d" % (ws, iv), r12, interval=iv, win_size=ws)
    w.conn("win_offset = interval", r12, interval=6, win_offset=6)
    w.conn("win_offset = interval + 1", r12, interval=6, win_offset=7)
    w.conn("map of one channel", range(6), chmap=1 << 9)
    w.conn("crc_ok 0", r12, request=False)
    w.request(400 + 977 * w.k, w.info[-1].aa, w.info[-1].crc_init, crc_ok=0, chmap=full, hop=7, interval=6)
    for length in (33, 35):
        w.conn("length %d" % length, r12, req_kw=dict(length=length))
    w.conn("type 5 on a data-channel stream", r12, request=False)
    w.request(400 + 977 * w.k, w.info[-1].aa, w.info[-1].crc_init, stream=3, mhz=int(lt.LATTICE_MHZ[3]), chmap=full, hop=7, interval=6)
    w.conn("adv type 4", r12, req_kw=dict(adv_type=4))
    w.conn("equal AA with another CRCInit", r12, request=False)
    w.request(400 + 977 * w.k, w.info[-1].aa, w.info[-1].crc_init ^ 1, chmap=full, hop=7, interval=6)
    # two requests: the later wins (it names another hop increment, by which the connection hops)
    w.conn("planted: two requests, the later wins", r12, hop=9, req_offset=60000)
    w.request(60000 - 5000, w.info[-1].aa, w.info[-1].crc_init, chmap=full, hop=11, interval=6)
    w.request(60000, w.info[-1].aa, w.info[-1].crc_init, stream=39, mhz=2426, chmap=full, hop=9, interval=6)      # (the larger stream)
    # R = first_anchor (taken: win_offset such that t0 lies before R would need a negative delay, so the first packet is BEFORE and
    # stands at R itself) and R = first_anchor + 1 (not taken)
    for name, d in (("R = first_anchor", 0), ("R = first_anchor + 1", 1)):
        aa, ci = w.ids()
        w.request(90000 + d, aa, ci, chmap=full, hop=7, interval=6, win_size=2, win_offset=1)
        w.raw += [ld.Cand(90352 + n * 6 * UNIT, aa, ci, (7 * n) % 37, 1, 0, (7 * n) % 37) for n in range(5)]
        w.info.append(Info(name, aa, ci, 1, (), (), None))
    w.conn("planted: ChSel 0", r12, alg=1)
    w.conn("planted: ChSel 1", r12, alg=2)
    w.conn("no request", r12, request=False)
    # ---- counters: the first event around t0 and around the end of the first interval
    P = 6 * UNIT
    for name, at in (("A_f = t0", 0), ("A_f = t0 - jitter", -JITTER), ("A_f = t0 - jitter - 1", -JITTER - 1), ("A_f = t0 + win_size", 2 * UNIT),
                     ("A_f = t0 + P - jitter - 1", P - JITTER - 1), ("A_f = t0 + P - jitter", P - JITTER), ("A_f = t0 + P / 2", P // 2)):
        w.conn(name, r12, at=at)
    w.conn("planted: missed events", (0, 1, 2, 5, 11, 12, 30, 31, 33, 40, 41, 45), jitter=lambda c: (c * 17) % 41 - 20)
    w.conn("planted: counters across 2^16", (65530, 65531, 65534, 65535, 65536, 65537, 65540), alg=2)
    w.conn("planted: counters across 2^16, #1", (65530, 65531, 65534, 65535, 65536, 65537, 65540))
    w.conn("planted: counters beyond 2^32", (3, 4, (1 << 32) + 5, (1 << 32) + 6, (1 << 32) + (1 << 16) + 7, (1 << 33) + 9), alg=2)
    w.conn("planted: counters beyond 2^32, #1", (3, 4, (1 << 32) + 5, (1 << 32) + 6, (1 << 32) + 7, (1 << 33) + 9))
    # (win_offset 6: t0 lies 8 750 bits behind the request's end, room for two events in front of it)
    w.conn("every event BEFORE", range(2), win_offset=6, at=-7 * UNIT)
    w.conn("some events BEFORE", range(8), win_offset=6, at=-7 * UNIT)
    w.conn("two packets per event", r12, second=(0, 3, 4, 11), alg=2)
    # ---- updates
    for delta in (6, 32766, 32767, 32768):
        w.conn("planted: delta %d" % delta, (0, 1, 2, 3, 2 + delta - 1, 2 + delta, 2 + delta + 1), chmap=full,
               maps=[(2 + delta, NINE)] if delta < 32767 else [], pdus={2: [map_ind(NINE, 2 + delta)]})
    w.conn("planted: event at I - 1 and at I", (0, 1, 7, 8, 9), maps=[(8, NINE)], pdus={1: [map_ind(NINE, 8)]})
    w.conn("planted: two updates in order", range(24), maps=[(8, NINE), (16, FIVE)], pdus={1: [map_ind(NINE, 8)], 9: [map_ind(FIVE, 16)]}, alg=2)
    w.conn("planted: two updates out of order", range(24), maps=[(8, NINE), (16, FIVE)], pdus={1: [map_ind(FIVE, 16)], 2: [map_ind(NINE, 8)]})
    w.conn("planted: two with equal I", range(20), maps=[(10, FIVE)], pdus={1: [map_ind(NINE, 10)], 2: [map_ind(FIVE, 10)]})
    w.conn("planted: a retransmitted update", range(20), maps=[(10, NINE)], pdus={1: [map_ind(NINE, 10)], 2: [map_ind(NINE, 10)], 3: [map_ind(NINE, 10), EMPTY]})
    w.conn("planted: map' of one channel", range(16), pdus={1: [map_ind(1 << 5, 8)]})
    w.conn("planted: top bits in map'", range(16), maps=[(8, (1 << 36) | 1)], pdus={1: [map_ind((1 << 36) | 1, 8, top_bits=7)]}, alg=2)
    for n in (7, 9):
        w.conn("planted: length %d" % n, range(16), pdus={1: [(3, (map_ind(NINE, 8)[1] + b"\x00")[:n])]})
    w.conn("planted: opcode 1 under LLID 2", range(16), pdus={1: [(2, map_ind(NINE, 8)[1])]})
    w.conn("planted: an update behind ENC START", range(16), pdus={1: [ENC_REQ], 2: [map_ind(NINE, 8)], 3: [TERMINATE_IND]})
    w.conn("planted: an update in front of ENC START", range(16), maps=[(8, NINE)], pdus={1: [map_ind(NINE, 8)], 2: [ENC_REQ], 4: [ENC_REQ]})
    w.conn("update in a BEFORE event", range(16), win_offset=6, at=-7 * UNIT, pdus={0: [map_ind(NINE, 8)], 1: [param_ind(9)]})
    w.conn("planted: parameter update", range(16), stop=9, pdus={2: [param_ind(9)]}, alg=2)
    w.conn("planted: two parameter updates", range(16), stop=9, pdus={2: [param_ind(12)], 3: [param_ind(9)]})
    w.conn("planted: map update PDU in a BEYOND event", range(16), stop=6, maps=[(4, NINE)],
           pdus={1: [param_ind(6)], 2: [map_ind(NINE, 4)], 7: [map_ind(FIVE, 9)]})
    w.conn("planted: parameter update with delta 32767", range(8), pdus={2: [param_ind(2 + 32767)]})
    w.conn("planted: TERMINATE", range(8), pdus={6: [TERMINATE_IND]})
    w.conn("planted: TERMINATE of length 3", range(8), pdus={6: [(3, bytes([2, 0x13, 0]))]})
    w.conn("planted: other control PDUs", range(8), pdus={1: [(3, bytes([12, 9, 1, 2, 3, 4]))], 2: [(3, bytes([8]) + bytes(8))], 3: [(3, bytes(27))]})
    w.conn("unseeded with control PDUs", range(8), request=False, pdus={1: [map_ind(NINE, 5)], 2: [ENC_REQ], 3: [map_ind(NINE, 5)], 4: [TERMINATE_IND]})
    # ---- algorithm
    w.conn("ChSel 0 on a connection that #2 explains", range(20), alg=2, chsel=0)
    w.conn("planted: ChSel 1 with #1", range(20), alg=1, chsel=1)
    # an exact tie: event 0 lies where #2 puts it and #1 does not, event 1 where #1 puts it and #2 does not
    t0 = w.conn("an exact tie", (0,), alg=2)
    tie = w.info[-1]
    ch1 = lt.csa1_at(0, 7, 2, full)
    assert ch1 != lc.csa2(tie.aa, 1, full) and lt.csa1_at(0, 7, 1, full) != tie.channels[0]
    w.raw.append(ld.Cand(t0 + P, tie.aa, tie.crc_init, ch1, 1, 0, ch1))
    for m, nm in ((TWO, 2), (NINE, 9), (M36, 36), (full, 37)):
        for alg in (1, 2):
            w.conn("planted: map of %d, #%d" % (nm, alg), range(30), alg=alg, chmap=m, hop=5 + nm % 12)
    # ---- payload read: channels 0 and 36 (the first events of maps that hold only them), a stream out of range, the stream's end
    w.conn("planted: control PDUs on channels 0 and 36", range(10), chmap=(1 << 0) | (1 << 36), maps=[(6, NINE)],
           pdus={0: [map_ind(NINE, 6)], 1: [map_ind(NINE, 6)], 2: [map_ind(NINE, 6)], 3: [map_ind(NINE, 6)]})
    w.conn("foreign streams among the members", range(10), pdus={3: [map_ind(NINE, 6)]}, stream_of=lambda ch, c: (40, 37, 65535)[c % 3] if c in (3, 4, 5) else ch)
    w.conn("control PDU beyond the streams' end", (0, 1, 40, 41), pdus={40: [map_ind(NINE, 44)], 41: [TERMINATE_IND]})
    # control PDUs at stream offsets 0, 1 and 63 modulo 64; a packet whose last bit is the stream's last bit, and one a bit further
    for r in (0, 1, 63):
        req = 400 + 977 * (w.k + 1)
        first = req + 352 + 2 * UNIT + P
        w.conn("planted: control PDU at offset %d mod 64" % r, range(10), maps=[(6, NINE)], pdus={1: [map_ind(NINE, 6)]}, at=(r - first) % 64,
               req_offset=req)
    for name, d in (("planted: last bit is the stream's last bit", 0), ("one bit beyond the stream's end", 1)):
        end = 64 * N_WORDS - 144 + d
        w.conn(name, range(28, 40), maps=[(34, NINE)] if d == 0 else [], pdus={30: [map_ind(NINE, 34)]}, req_offset=end - 30 * P - 352 - 2 * UNIT)
    w.noise(40)
    return w.built()


@functools.lru_cache(maxsize=None)
def lattice_model():
    return model(lattice())


@functools.lru_cache(maxsize=None)
def seam_world():
    """One connection of 5 000 events with 40 map updates beside 1 000 connections of 2 to 4 events, some seeded and some not.
    unit_bits is 120 here, so that the first 360 events of the large connection -- and all its update PDUs -- lie inside the streams."""
    w = World(23, unit=120)
    rng = np.random.default_rng(29)
    maps, pdus, m = [], {}, lc.FULL_MAP
    for u in range(40):
        m = lt.random_map(rng, 5 + (7 * u) % 30)
        at = 100 + 120 * u
        maps.append((at, m))
        pdus[5 + 8 * u] = [map_ind(m, at)]
    w.conn("planted: large", range(5000), alg=2, maps=maps, pdus=pdus, second=range(0, 5000, 3), req_offset=100)
    for k in range(1000):
        w.conn("planted: small %d" % k, range(2 + k % 3), alg=1 + k % 2, interval=6 + k % 30, hop=5 + k % 12, chmap=lt.random_map(rng, 37 if k % 4 else 5),
               request=k % 3 != 0, req_offset=2000 + 97 * k)
    return w.built()


@functools.lru_cache(maxsize=None)
def wrap_world():
    """Update PDUs whose events have counters next to 2^16, INSIDE the streams: at unit_bits 2 and interval 6 an event is 12 bits, so
    counter 65 536 lies 786 432 bits behind t0 (at 1250 bits per unit it would be 490 Mbit).  jitter_bits 0, ifs_bits 0; the packets
    of neighbouring events overlap in time on different streams, which the rules do not mind: algorithm #1 on a full map never
    takes one channel twice in a row, so every event stays one event.  An instant across 65535 -> 0 (announced at 65 529 for 65 537: the PDU says 1), one
    announced at 65 534 for the event 65 536 itself, and a #2 connection with an instant of 0x10003."""
    w = World(31, unit=2, n_words=12800, ifs=0, jitter=0)
    near = (65527, 65528, 65529, 65530, 65534, 65535, 65536, 65537, 65538, 65540)
    w.conn("planted: instant across 65535 -> 0", near, maps=[(65537, M36)], pdus={65529: [map_ind(M36, 65537)]})
    w.conn("planted: instant 65536", near, maps=[(65536, M36)], pdus={65534: [map_ind(M36, 65536)]}, hop=11)
    w.conn("planted: instant 0x10003, #2", (65530, 65533, 65535, 65537, 65539, 65541, 65543, 65545), alg=2, maps=[(0x10003, NINE)],
           pdus={65533: [map_ind(NINE, 0x10003)]})
    w.conn("planted: counters from 0", range(0, 40, 3), maps=[(20, M36)], pdus={3: [map_ind(M36, 20)]})
    w.noise(10)
    return w.built()


@functools.lru_cache(maxsize=None)
def wrap_model():
    return model(wrap_world())


@functools.lru_cache(maxsize=None)
def seam_model():
    return model(seam_world())


# ---- the worlds of tests/_le_follow_paths.py: laid out by position ------------------------------------------------------------
# Their connections get ascending access addresses, so ld.group keeps them in the order they are planted in and connection g's
# slots and events begin at the sum of the packets in front of it: a world is laid out by counting packets.
CROWD_CONNS, CROWD_NOISE, CROWD_TILE = 1450, 40, 2048          # (CROWD_TILE: LT_TILE of le_track.h; tests/test_le_follow_paths_model.py holds them together)


@functools.lru_cache(maxsize=None)
def crowd_world():
    """1 450 connections of 12 events side by side, unit_bits 120, streams of 16 384 words; four in five are seeded, and all but one
    in twenty-five carry four LL_CHANNEL_MAP_IND in their events 1 to 4: I = 8 announced in front of I = 6, then two with I = 10.
    More than 4 096 listed updates, in every scan tile of slots but the third (the connections that begin there are not seeded);
    a connection begins on every tile seam but the fifth, which a seeded one lies across (the one in front of a seam gets as many
    second packets as it takes: holes in the event table); forty non-members lie between the two halves.  Every instant is shared
    by all connections with updates."""
    w = World(41, unit=120, n_words=16384)
    rng = np.random.default_rng(43)
    pool = [lt.random_map(rng, n) for n in (17, 23, 30, 33, 36, 25, 28, 35)]
    p = 0                                                                  # where the next connection's slots and events begin
    for k in range(CROWD_CONNS):
        if k == CROWD_CONNS // 2:
            p += CROWD_NOISE
        on_seam = p > 0 and p % CROWD_TILE == 0 or p < 5 * CROWD_TILE < p + 12
        seeded = (on_seam or k % 10 != 9) and not 2 * CROWD_TILE - 14 <= p < 3 * CROWD_TILE
        room = -(p + 12) % CROWD_TILE
        second = tuple(range(room)) if room < 12 and p + 12 + room != 5 * CROWD_TILE else ((0, 7) if k % 3 == 0 else ())
        a, b, c, d = (pool[(k + j) % 8] for j in range(4))
        pdus = {} if k % 25 == 7 else {1: [map_ind(a, 8)], 2: [map_ind(b, 6)], 3: [map_ind(c, 10)], 4: [map_ind(d, 10)]}
        for shift in range(0, 700, 37):                                    # (a control PDU that would overwrite another's bits: a little later)
            keep = len(w.raw), len(w.adv), len(w.info), [len(t) for t in w.taken], w.k
            try:
                w.conn("planted: crowd %d" % k, range(12), alg=1 + k % 2, hop=5 + k % 12, chmap=pool[(k + 5) % 8] if k % 4 else lc.FULL_MAP,
                       request=seeded, req_offset=2000 + 700 * k + shift, aa=(0x68000000 if k >= CROWD_CONNS // 2 else 0x20000000) + 0x3001 * k,
                       maps=[(6, b), (8, a), (10, d)] if pdus else [], pdus=pdus, second=second)
                break
            except AssertionError:
                del w.raw[keep[0]:], w.adv[keep[1]:], w.info[keep[2]:]
                for t, n in zip(w.taken, keep[3]):
                    del t[n:]
                w.k = keep[4]
        else:
            raise AssertionError("no room for connection %d" % k)
        p += 12 + len(second)
    w.noise(CROWD_NOISE)
    return w.built()


@functools.lru_cache(maxsize=None)
def crowd_model():
    trace = {}
    return model(crowd_world(), trace=trace) + (trace,)


M35 = lc.FULL_MAP & ~(1 << 5)


@functools.lru_cache(maxsize=None)
def byte_world():
    """wrap_world's geometry (unit_bits 2, jitter_bits 0, ifs_bits 0) with two connections that announce two updates each, the later
    instant first: 0x10001 in front of 0xFFFF -- the low sixteen bits order them the wrong way round, byte 2 alone decides -- and
    0x101 in front of 0xFF, which byte 1 decides."""
    w = World(37, unit=2, n_words=12800, ifs=0, jitter=0)
    w.conn("planted: byte 2 decides", (65527, 65528, 65529, 65530, 65534, 65535, 65536, 65537, 65538, 65540),
           maps=[(0xFFFF, M35), (0x10001, M36)], pdus={65529: [map_ind(M36, 0x10001)], 65530: [map_ind(M35, 0xFFFF)]})
    w.conn("planted: byte 1 decides", (250, 251, 252, 254, 255, 256, 257, 258, 260), hop=11,
           maps=[(0xFF, M35), (0x101, M36)], pdus={250: [map_ind(M36, 0x101)], 251: [map_ind(M35, 0xFF)]})
    w.noise(10)
    return w.built()


@functools.lru_cache(maxsize=None)
def byte_model():
    trace = {}
    return model(byte_world(), trace=trace) + (trace,)


@functools.lru_cache(maxsize=None)
def tally_world():
    """330 events laid out lane by lane for le_epoch_predict_kernel's tallies (a wave is 64 event positions): positions 0..3 a
    connection whose counters pass 2^33; 4..62 one with two BEFORE events; 63..133 one whose run begins at lane 63, fills wave 1 and
    leaves a BEYOND tail from lane 0 of wave 2 on (stop 65, an update in force before it and one behind it); 134..143 counted and
    BEYOND events in one run and two holes; 144..148 unseeded; 149..191 seeded; wave 3: sixteen connections of three events and one
    of sixteen; wave 4: one unseeded connection; 320..329 a seeded one behind it; 330..341 a connection whose update PDU lies across
    the streams' end: the map and the instant's low octet are the streams' last bits, the high octet is read as zeros, which dewhitened
    give an instant more than 32 767 events away: no update -- ones in their place give a valid one (World.conn writes no packet that
    ends beyond the streams, so its first 112 bits are written here)."""
    w = World(47)
    made = [0]

    def conn(name, counters, **kw):
        made[0] += 1
        w.conn(name, counters, aa=0x21000000 + 0x5003 * made[0], **kw)

    conn("planted: counters beyond 2^33 in front of all", (0, 1, (1 << 32) + 2, (1 << 33) + 3))
    conn("two BEFORE events, ends at lane 62", range(59), win_offset=6, at=-7 * UNIT)
    conn("planted: head at lane 63, wave 1, a BEYOND tail", range(71), stop=65, maps=[(10, NINE)],
         pdus={1: [map_ind(NINE, 10)], 2: [param_ind(65)], 3: [map_ind(FIVE, 67)]})
    conn("planted: counted and BEYOND in one run, two holes", range(8), stop=4, pdus={1: [param_ind(4)]}, second=(0, 5), alg=2)
    conn("unseeded between seeded runs", range(5), request=False)
    conn("planted: up to the end of wave 2", range(43), maps=[(5, NINE)], pdus={1: [map_ind(NINE, 5)]})
    for k in range(16):
        conn("planted: three events, %d" % k, range(3), alg=1 + k % 2, hop=5 + k % 12)
    conn("planted: up to the end of wave 3", range(16), alg=2)
    conn("unseeded, a wave of its own", range(64), request=False)
    conn("planted: behind the wave without a live lane", range(10), maps=[(4, FIVE)], pdus={1: [map_ind(FIVE, 4)]})
    at = 64 * N_WORDS - 112
    conn("planted: an instant's high octet behind the streams' end", range(28, 40), pdus={30: [map_ind(NINE, 34)]},
         req_offset=at - 30 * 6 * UNIT - 352 - 2 * UNIT)
    last = w.info[-1]
    ch = last.channels[2]
    assert [c.offset for c in w.raw if c.access_address == last.aa and c.length == 8] == [at]
    w.bits[ch, at:] = _le.tx_bits(last.aa, ch, bytes((3, 8)) + map_ind(NINE, 34)[1], last.crc_init)[:112]
    w.noise(30)
    return w.built()


@functools.lru_cache(maxsize=None)
def tally_model():
    trace = {}
    return model(tally_world(), trace=trace) + (trace,)


def cut_model(b, full, trace, work=None, kept=None):
    """What model_cut gives for the first `work` candidates and `kept` connections of a Built, from the whole list's model (`full`,
    `trace`): connections do not touch each other, so only the one the cut goes through is worked out again, alone.
    -> (pkts, seeds, follows, fpkts, trace).  (tests/test_le_follow_paths_model.py holds it against model_cut.)"""
    n = len(b.cands) if work is None else min(work, len(b.cands))
    k = len(b.conns) if kept is None else min(kept, len(b.conns))
    seeds, follows, fpkts, pkts = list(full[0][:k]), list(full[1][:k]), list(full[2][:n]), list(b.pkts[:n])
    trace = {g: t for g, t in trace.items() if g < k}
    for g, c in enumerate(b.conns):
        lo, hi = c.first, c.first + c.n_packets
        if g >= k:
            for i in range(lo, min(hi, n)):
                fpkts[i] = pkts[i] = None
        elif hi > n:
            m = max(n - lo, 0)
            sub = [x._replace(channel=0) for x in b.cands[lo:lo + m]]
            tracks, pk = lt.track(sub, 1, lt.LATTICE_MHZ, lt.N_STREAMS, b.unit, b.ifs, b.jitter, lt.REMAP)
            sd, own = seed(b.adv, [c], tracks, b.unit), {}
            fo, fp = follow([c], sub, tracks, pk, sd, b.words, b.n_words, b.unit, b.jitter, trace=own)
            seeds[g], follows[g] = sd[0], fo[0]
            fpkts[lo:lo + m], pkts[lo:lo + m] = fp, pk
            trace.pop(g, None)
            if 0 in own:
                trace[g] = dict(own[0], ups=[(at, rank, mp, i + lo) for at, rank, mp, i in own[0]["ups"]])
    return pkts, seeds, follows, fpkts, trace


def model_cut(b, work=None, kept=None, n_adv=None, rules=MODEL, flags=lt.REMAP):
    """(tracks, pkts, seeds, follows, fpkts) of the models on the first `work` candidates, `kept` connections and n_adv advertising
    records of a Built: what the device entries see through their caps and counts."""
    n = len(b.cands) if work is None else min(work, len(b.cands))
    k = len(b.conns) if kept is None else min(kept, len(b.conns))
    adv = b.adv if n_adv is None else b.adv[:n_adv]
    tracks, pkts = lt.track(b.cands[:n], k, lt.LATTICE_MHZ, lt.N_STREAMS, b.unit, b.ifs, b.jitter, flags)
    seeds = seed(adv, b.conns[:k], tracks, b.unit, rules)
    return (tracks, pkts, seeds) + follow(b.conns[:k], b.cands[:n], tracks, pkts, seeds, b.words, b.n_words, b.unit, b.jitter, rules)


# ---- the chain capture --------------------------------------------------------------------------------------------------
CHAIN_MHZ = np.array(lt.DATA_MHZ + _le.ADV_MHZ, np.uint16)                  # streams 0..36: the data channels; 37..39: advertising
Planted = collections.namedtuple("Planted", "name aa crc_init alg seeded stop first_update counters")


@functools.lru_cache(maxsize=None)
def chain_capture():
    """37 data streams and three advertising streams of 4 600 words of noise with a seeded #1 connection with one map update, a
    seeded #2 connection with two map updates and a parameter update, and an unseeded connection.  Every event is a control or
    data PDU of the central and an empty PDU of the peripheral 150 bits behind it.  -> (Capture, planted)"""
    n_words = 4600
    b = ld._Builder(40, n_words, CHAIN_MHZ, 4242)
    rng = np.random.default_rng(17)
    total = 64 * n_words
    plans = [dict(name="#1, one map update", alg=1, hop=11, interval=6, chmap=lc.FULL_MAP, req=(37, 300), maps=[(14, NINE)],
                  pdus={6: map_ind(NINE, 14), 7: map_ind(NINE, 14)}, n=36, stop=None),
             dict(name="#2, two map updates and a parameter update", alg=2, hop=9, interval=7, chmap=M36, req=(39, 1500),
                  maps=[(8, FIVE), (17, NINE)], pdus={2: map_ind(FIVE, 8), 10: map_ind(NINE, 17), 20: param_ind(26, 12)}, n=30, stop=26),
             dict(name="unseeded", alg=1, hop=5, interval=8, chmap=FIVE, req=None, maps=[], pdus={3: map_ind(NINE, 9)}, n=25, stop=None)]
    planted = []
    for k, p in enumerate(plans):
        aa, ci = ld.good_aa(rng), int(rng.integers(0, 1 << 24))
        if p["req"]:
            stream, off = p["req"]
            body = connect_ind(aa, ci, p["chmap"], p["hop"], p["interval"], win_size=2, win_offset=1, chsel=int(p["alg"] == 2))
            b.plant(stream, off, _le.ADV_AA, _le.ADV_CRC_INIT, body[4], 34, "CONNECT_IND %d" % k, payload=body[6:40])
            t0 = off + 352 + 2 * UNIT
        else:
            t0 = 3000
        counters = []
        for c in range(p["n"]):
            m = p["chmap"]
            for instant, new in p["maps"]:
                if instant <= c:
                    m = new
            ch = lt.csa1_at(0, p["hop"], c + 1, m) if p["alg"] == 1 else lc.csa2(aa, c, m)
            at = t0 + c * p["interval"] * UNIT + 300 + int(rng.integers(-20, 21))
            h0, payload = p["pdus"].get(c, (2, bytes(rng.integers(0, 256, 1 + c % 5, dtype=np.uint8))))
            if at + 80 + 8 * len(payload) + 150 + 80 > total:
                break
            b.plant(ch, at, aa, ci, h0, len(payload), p["name"], payload=payload)
            b.plant(ch, at + 80 + 8 * len(payload) + 150, aa, ci, 1, 0, p["name"])
            counters.append(c)
        planted.append(Planted(p["name"], aa, ci, p["alg"], p["req"] is not None, p["stop"], min([i for i, _ in p["maps"]], default=None),
                               tuple(counters)))
    words = b.words(n_words + 5)
    words.flags.writeable = False
    return ld.Capture(words, n_words, n_words + 5, total - 39, CHAIN_MHZ, tuple(b.planted), 27), tuple(planted)


def capture_model(cap, adv_errors=0):
    """(conns, cands, tracks, pkts, adv, seeds, follows, fpkts) of the models on a capture: discovery (min_count 2), tracking
    (REMAP), the advertising scan with up to adv_errors mismatches in (stream, offset) order, seed and follow."""
    conns, cands = ld.group(ld.capture_candidates(cap, 27), 2)
    tracks, pkts = lt.track(cands, len(conns), cap.mhz, len(cap.mhz), UNIT, IFS, JITTER, lt.REMAP)
    adv = []
    for s in range(len(cap.mhz)):
        offs, errs, _ = _le.match_all(cap.words[s], cap.n_words, cap.search_bits, _le.ADV_AA, adv_errors)
        adv += [_le.decode(cap.words[s], cap.n_words, s, int(o), int(e), int(cap.mhz[s]), _le.ADV_CRC_INIT) for o, e in zip(offs, errs)]
    seeds = seed(adv, conns, tracks, UNIT)
    return (conns, cands, tracks, pkts, adv, seeds) + follow(conns, cands, tracks, pkts, seeds, cap.words, cap.n_words, UNIT, JITTER)


@functools.lru_cache(maxsize=None)
def chain_model():
    return capture_model(chain_capture()[0])


@functools.lru_cache(maxsize=None)
def crowded_adv_capture():
    """One data stream and two advertising streams of 2 600 words: a connection of six events on data channel 5 behind its
    CONNECT_IND, and on each advertising stream 2 070 copies of preamble + advertising access address back to back -- more matches
    than the host wrapper's first advertising buffer holds (one per 16 384 offsets and stream + 4 096)."""
    n_words = 2600
    mhz = np.array((lt.DATA_MHZ[5], 2402, 2426), np.uint16)
    b = ld._Builder(3, n_words, mhz, 99)
    rng = np.random.default_rng(7)
    aa, ci = ld.good_aa(rng), 0x1F2E3D
    body = connect_ind(aa, ci, (1 << 5) | (1 << 9), 7, 6, chsel=0)
    b.plant(1, 200, _le.ADV_AA, _le.ADV_CRC_INIT, body[4], 34, "CONNECT_IND", payload=body[6:40])
    t0 = 200 + 352 + 2 * UNIT
    for c in range(6):
        b.plant(0, t0 + 400 + c * 6 * UNIT, aa, ci, 2, 3, "event %d" % c)
    pattern = np.tile(_le.pattern_bits(_le.ADV_AA), 2070)
    for s in (1, 2):
        b.bits[s, 1000:1000 + len(pattern)] = pattern
    words = b.words(n_words + 3)
    words.flags.writeable = False
    return ld.Capture(words, n_words, n_words + 3, 64 * n_words - 39, mhz, tuple(b.planted), 27)


@functools.lru_cache(maxsize=None)
def errors_capture():
    """The chain capture's first connection once more, alone, its CONNECT_IND received with one wrong bit in the access address (the
    CRC covers the PDU, not the access address, so it still holds): a scan without errors does not see the request, one that allows
    a mismatch seeds the connection.  -> (Capture, access address)"""
    n_words = 1300
    mhz = CHAIN_MHZ
    b = ld._Builder(40, n_words, mhz, 515)
    rng = np.random.default_rng(3)
    aa, ci = ld.good_aa(rng), 0x4D3C2B
    body = connect_ind(aa, ci, lc.FULL_MAP, 9, 6)
    b.plant(38, 150, _le.ADV_AA, _le.ADV_CRC_INIT, body[4], 34, "CONNECT_IND", payload=body[6:40])
    b.bits[38, 150 + 8 + 13] ^= 1
    t0 = 150 + 352 + 2 * UNIT
    for c in range(10):
        ch = lt.csa1_at(0, 9, c + 1, lc.FULL_MAP)
        b.plant(ch, t0 + 200 + c * 6 * UNIT, aa, ci, 1, 0, "event %d" % c)
    words = b.words(n_words + 2)
    words.flags.writeable = False
    return ld.Capture(words, n_words, n_words + 2, 64 * n_words - 39, mhz, tuple(b.planted), 27), aa


@functools.lru_cache(maxsize=None)
def payload_capture():
    """The payload read on a small capture built with tests/_le_discover._Builder: data channels 0 and 36 and one advertising
    stream, 1 300 words each; a connection on the map {0, 36} whose central sends an LL_CHANNEL_MAP_IND in every event, the
    packets at stream offsets 0, 1 and 63 modulo 64 among them, and the last one ending on the streams' last bit.  -> Capture"""
    n_words = 1300
    mhz = np.array((lt.DATA_MHZ[0], lt.DATA_MHZ[36], 2402), np.uint16)
    b = ld._Builder(3, n_words, mhz, 616)
    rng = np.random.default_rng(4)
    aa, ci = ld.good_aa(rng), 0x0F1E2D
    chmap, hop, total = (1 << 0) | (1 << 36), 11, 64 * n_words
    body = connect_ind(aa, ci, chmap, hop, 6)
    b.plant(2, 100, _le.ADV_AA, _le.ADV_CRC_INIT, body[4], 34, "CONNECT_IND", payload=body[6:40])
    t0 = 100 + 352 + 2 * UNIT
    last = (total - 144 - t0) // (6 * UNIT)
    seen = set()
    for c in range(last + 1):
        ch = lt.csa1_at(0, hop, c + 1, chmap)
        at = t0 + c * 6 * UNIT
        want = (0, 1, 63, 0, 1, 63)[c % 6]
        at = total - 144 if c == last else at + (want - at) % 64
        h0, payload = map_ind(chmap, c + 2)
        b.plant(1 if ch == 36 else 0, at, aa, ci, h0, len(payload), "event %d" % c, payload=payload)
        seen.add((ch, at % 64))
        if c != last:
            b.plant(1 if ch == 36 else 0, at + 144 + 150, aa, ci, 1, 0, "event %d, peripheral" % c)
    assert {m for _, m in seen} >= {0, 1, 63} and {ch for ch, _ in seen} == {0, 36}
    words = b.words(n_words + 1)
    words.flags.writeable = False
    return ld.Capture(words, n_words, n_words + 1, total - 39, mhz, tuple(b.planted), 27)
