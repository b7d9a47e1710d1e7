"""Test-side model of LE data extraction (include/btbbx.h btbbx_le_data_device, rules 1 to 7) -- plain Python over the tuples of
tests/_le_discover.py and tests/_le_track.py, written from the rules and not from the kernels: a connection is walked member by
member in time order with a dictionary per role, where libbtbb_amd/csrc/le_data.h runs four scans over a slot table.

* Rules: the model's branch points as options; VARIANTS are deliberately wrong models (tests/test_le_data_model.py shows that the
  lattice of this file tells each from the right one)
* data: the model -> Out(data, dpkts, msgs, payload, n_msgs, n_bytes)
* World: connections planted packet by packet, EVERY packet's bits written into the streams (_le.tx_bits), with what was planted:
  every seen packet's role and the messages of either direction, octet for octet
* H / hand_built: hand-made lists ("a list from elsewhere") with the tracking's records written directly; members may overlap
  in a small stream, since nothing but their payload bits is read
* the lattices of the GPU tests: planted_world, align_list, seam lists
"""
import collections
import functools

import numpy as np

import _le
import _le_discover as ld
import _le_track as lt

START, CONTINUATION, ORPHAN, EMPTY, CONTROL, IGNORED, RETRANSMIT, UNKNOWN = range(8)
CENTRAL, PERIPHERAL, ROLE_UNKNOWN = 0, 1, 2
COMPLETE, OVERRUN, RUNT, STORED = 1, 2, 4, 8
NONE = 0xFFFFFFFF

DPkt = collections.namedtuple("DPkt", "msg pos role kind bits")
Data = collections.namedtuple("Data", "bytes first_msg n_msgs n_complete n_central n_peripheral n_unknown n_retransmit n_orphan n_control "
                                      "n_empty")
Msg = collections.namedtuple("Msg", "byte_offset conn start n_fragments bytes l2cap_len cid role flags")
Out = collections.namedtuple("Out", "data dpkts msgs payload n_msgs n_bytes")


class Rules:
    """Rules() is the model; every other value is a wrong one."""

    def __init__(self, **kw):
        self.role_flip = False              # rule 3: the parity the other way round
        self.retx_any_role = False          # rule 4: sn compared with the previous member of ANY role
        self.cont_any_role = False          # rule 5: a continuation joins the latest START of either role
        self.whiten_restart = False         # rule 6: the whitening sequence restarted at the payload
        self.pos_all_members = False        # rule 5: pos counted over all members behind the START, not over the fragments
        self.order_by_index = False         # rule 6: messages ordered by the START's list index, not its rank
        # (told apart on the worlds of tests/_le_data_lattice.py: LATTICE_VARIANTS there)
        self.unknown_sets_sn = False        # rule 4: an UNKNOWN member's sn becomes the last sn of both roles
        self.empty_breaks = False           # rule 5: an EMPTY member closes the open message of its role
        self.retx_joins = False             # rule 5: a RETRANSMIT continuation's L is added to the open message once more
        self.end_reads_on = False           # rule 6: bits beyond a row's end taken from the words that follow in memory
        self.whiten_period_128 = False      # rule 6: the whitening sequence continued with period 128, not 127
        self.offset_mod_2_32 = False        # rule 6: byte_offset kept modulo 2^32
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


MODEL = Rules()
VARIANTS = dict(role_flip=dict(role_flip=True), retx_any_role=dict(retx_any_role=True), cont_any_role=dict(cont_any_role=True),
                whiten_restart=dict(whiten_restart=True), pos_all_members=dict(pos_all_members=True),
                order_by_index=dict(order_by_index=True))


def payload_octets(row, n_words, offset, length, ch, rules=MODEL):
    """Rule 6: the `length` payload octets of the packet at `offset` of one stream, dewhitened; zeros beyond the stream's end."""
    raw = _le.stream_bits(row, n_words, offset + 56, 8 * length, past_end=rules.end_reads_on)
    at = 0 if rules.whiten_restart else 16
    white = _le._whitening_2080(ch & 0x3F)
    if rules.whiten_period_128:
        return _le.bits_octets(raw ^ white[np.arange(at, at + 8 * length) % 128])
    return _le.bits_octets(raw ^ white[at:at + 8 * length])


def stream_row(rows, s, rules=MODEL):
    """The words of stream s; for the end_reads_on variant the memory from its first word on, the rows behind it included."""
    if not rules.end_reads_on:
        return rows[s]
    rows = np.asarray(rows)
    return rows.reshape(-1)[s * rows.shape[1]:]


def members_of(conns, cands, pkts):
    """Rule 0: per connection its members' list indices by rank."""
    n, k = len(cands), len(conns)
    out = [[] for _ in range(k)]
    for i, c in enumerate(cands):
        p = pkts[i]
        if c.channel >= k or p is None or p.rank == NONE:
            continue
        first = conns[c.channel].first
        if first >= n or p.rank >= n - first or p.event >= n - first:
            continue
        out[c.channel].append(i)
    for m in out:
        m.sort(key=lambda i: pkts[i].rank)
    return out


def data(conns, cands, pkts, rows, n_words, msg_cap, byte_cap, rules=MODEL):
    """rows[s]: the words of stream s.  -> Out: one Data per connection, one DPkt or None (no member) per candidate, the first msg_cap
    Msg records, the stored prefix of the octets, and the two counts."""
    dpkts = [None] * len(cands)
    per_conn, messages = [], []                 # messages: dicts, in (connection, rank of the START) order
    for g, order in enumerate(members_of(conns, cands, pkts)):
        counter, first_rank = {}, {}
        for i in order:                         # rule 2
            counter.setdefault(pkts[i].event, pkts[i].counter)
            first_rank.setdefault(pkts[i].event, pkts[i].rank)
        tally = collections.Counter()
        last_sn, open_msg, mine = {}, {}, []
        for i in order:
            c, p = cands[i], pkts[i]
            h0, L = c.header0, c.length         # rule 1
            llid, nesn, sn, md = h0 & 3, (h0 >> 2) & 1, (h0 >> 3) & 1, (h0 >> 4) & 1
            bits = sn | nesn << 1 | md << 2
            e = p.event
            head = e == 0 or counter.get(e - 1) != counter[e]
            role = ((p.rank - first_rank[e]) & 1) ^ int(rules.role_flip) if head else ROLE_UNKNOWN     # rule 3
            tally["role%d" % role] += 1
            for m in open_msg.values():
                m["all"] += L
            if role == ROLE_UNKNOWN:
                dpkts[i] = DPkt(NONE, 0, role, UNKNOWN, bits)
                if rules.unknown_sets_sn:
                    last_sn[CENTRAL] = last_sn[PERIPHERAL] = sn
                continue
            key = "any" if rules.retx_any_role else role                                             # rule 4
            new = key not in last_sn or last_sn[key] != sn
            last_sn[key] = sn
            if not new:
                tally["retransmit"] += 1
                dpkts[i] = DPkt(NONE, 0, role, RETRANSMIT, bits)
                if rules.retx_joins and llid == 1 and L >= 1 and role in open_msg:
                    open_msg[role]["bytes"] += L
                continue
            key = "any" if rules.cont_any_role else role                                             # rule 5
            if llid == 2 and L >= 1:
                m = dict(conn=g, start=i, role=role, frags=[(i, 0)], bytes=L, all=L, rank=p.rank)
                open_msg[key] = m
                mine.append(m)
                dpkts[i] = (m, 0, role, START, bits)
            elif llid == 1 and L >= 1:
                if key in open_msg:
                    m = open_msg[key]
                    pos = m["all"] - L if rules.pos_all_members else m["bytes"]
                    m["frags"].append((i, pos))
                    m["bytes"] += L
                    dpkts[i] = (m, pos, role, CONTINUATION, bits)
                else:
                    tally["orphan"] += 1
                    dpkts[i] = DPkt(NONE, 0, role, ORPHAN, bits)
            elif llid == 1:
                tally["empty"] += 1
                dpkts[i] = DPkt(NONE, 0, role, EMPTY, bits)
                if rules.empty_breaks:
                    open_msg.pop(key, None)
            elif llid == 3:
                tally["control"] += 1
                dpkts[i] = DPkt(NONE, 0, role, CONTROL, bits)
            else:
                dpkts[i] = DPkt(NONE, 0, role, IGNORED, bits)
        mine.sort(key=lambda m: m["start"] if rules.order_by_index else m["rank"])                       # rule 6
        per_conn.append((bool(order), tally, mine))
        messages += mine
    msgs, payload, offset = [], bytearray(), 0
    for M, m in enumerate(messages):
        m["M"] = M
        c = cands[m["start"]]
        flags, l2cap_len, cid = RUNT, 0xFFFF, 0xFFFF
        if c.length >= 4:
            hdr = payload_octets(stream_row(rows, c.stream, rules), n_words, c.offset, 4, pkts[m["start"]].channel, rules)
            l2cap_len, cid = hdr[0] | hdr[1] << 8, hdr[2] | hdr[3] << 8
            flags = COMPLETE if m["bytes"] == 4 + l2cap_len else (OVERRUN if m["bytes"] > 4 + l2cap_len else 0)
        m["complete"] = bool(flags & COMPLETE)
        if M < msg_cap and offset + m["bytes"] <= byte_cap:
            flags |= STORED
            buf = bytearray(m["bytes"] if not rules.pos_all_members else max(pos + cands[i].length for i, pos in m["frags"]))
            for i, pos in m["frags"]:
                f = cands[i]
                buf[pos:pos + f.length] = payload_octets(stream_row(rows, f.stream, rules), n_words, f.offset, f.length, pkts[i].channel, rules)
            payload[offset:offset + len(buf)] = buf
        if M < msg_cap:
            msgs.append(Msg(offset & 0xFFFFFFFF if rules.offset_mod_2_32 else offset, m["conn"], m["start"], len(m["frags"]),
                            m["bytes"] & 0xFFFFFFFF, l2cap_len, cid, m["role"], flags))
        offset += m["bytes"]
    records, before = [], 0
    for has, tally, mine in per_conn:
        if not has:
            records.append(Data(*([0] * 11)))
            continue
        records.append(Data(sum(m["bytes"] for m in mine), before, len(mine), sum(m["complete"] for m in mine), tally["role0"],
                            tally["role1"], tally["role2"], tally["retransmit"], tally["orphan"], tally["control"], tally["empty"]))
        before += len(mine)
    dpkts = [DPkt(d[0]["M"], *d[1:]) if d is not None and isinstance(d[0], dict) else d for d in dpkts]
    return Out(records, dpkts, msgs, bytes(payload), len(messages), offset)


def check_invariants(out, conns, cands, pkts, msg_cap, byte_cap):
    """What rules 6 and 7 promise of any output."""
    assert sum(d.n_msgs for d in out.data) == out.n_msgs and sum(d.bytes for d in out.data) == out.n_bytes
    before = 0
    mine = collections.Counter(c.channel for i, c in enumerate(cands) if out.dpkts[i] is not None)      # (one pass, whatever K)
    for g, d in enumerate(out.data):
        if d != Data(*([0] * 11)):
            assert d.first_msg == before
            assert d.n_central + d.n_peripheral + d.n_unknown == mine[g]
            before += d.n_msgs
    assert len(out.msgs) == min(out.n_msgs, msg_cap)
    stored = [bool(m.flags & STORED) for m in out.msgs]
    assert stored == sorted(stored, reverse=True)                        # a prefix
    at = 0
    for M, m in enumerate(out.msgs):
        assert m.byte_offset == at and (not m.flags & STORED or at + m.bytes <= byte_cap)
        assert not (m.flags & COMPLETE and m.flags & (OVERRUN | RUNT)) and (m.flags & RUNT) == (RUNT if cands[m.start].length < 4 else 0)
        assert out.dpkts[m.start][:4] == (M, 0, m.role, START)
        at += m.bytes
    kept = [m for m in out.msgs if m.flags & STORED]
    assert len(out.payload) == (kept[-1].byte_offset + kept[-1].bytes if kept else 0)
    for i, d in enumerate(out.dpkts):
        if d is not None and d.kind in (START, CONTINUATION):
            assert d.msg < out.n_msgs and d.role < 2
            if d.msg < len(out.msgs):
                assert d.pos + cands[i].length <= out.msgs[d.msg].bytes and out.msgs[d.msg].role == d.role
        elif d is not None:
            assert (d.msg, d.pos) == (NONE, 0)


# ---- records ---------------------------------------------------------------------------------------------------------------------
def data_array(records, dtype):
    a = np.zeros(len(records), dtype)
    for i, r in enumerate(records):
        a[i] = tuple(r)
    return a


def dpkt_array(dpkts, dtype):
    a = np.zeros(len(dpkts), dtype)
    for i, d in enumerate(dpkts):
        if d is None:
            a[i:i + 1].view(np.uint8)[:] = 0xFF
        else:
            a[i] = tuple(d) + (0,)
    return a


def msg_array(msgs, dtype):
    a = np.zeros(len(msgs), dtype)
    for i, m in enumerate(msgs):
        a[i] = tuple(m) + ((0, 0),)
    return a


# ---- planted worlds ----------------------------------------------------------------------------------------------------------------
UNIT, IFS, JITTER, INTERVAL = 1250, 200, 50, 6
N_WORDS = 4096
N_STREAMS = 37
MHZ = np.array(lt.DATA_MHZ, np.uint16)                      # stream c is data channel c
P = collections.namedtuple("P", "llid payload retx lost md")
P.__new__.__defaults__ = (b"", False, False, 0)
Planted = collections.namedtuple("Planted", "name aa crc_init roles messages")     # roles: offset -> role; messages: (role, octets)


def l2cap(cid, body, claim=None):
    """An L2CAP frame: length (claim: what the header says instead of the truth), CID, body."""
    n = len(body) if claim is None else claim
    return bytes([n & 0xFF, n >> 8, cid & 0xFF, cid >> 8]) + bytes(body)


class World:
    """Connections planted packet by packet; the packets of an event alternate central, peripheral, ... from its anchor, 150 bits
    apart.  Every packet that is not lost is written into its stream and listed as a raw candidate."""

    def __init__(self, seed=11, n_words=N_WORDS):
        self.rng = np.random.default_rng(seed)
        self.n_words = n_words
        self.bits = self.rng.integers(0, 2, (N_STREAMS, 64 * n_words), dtype=np.uint8)
        self.taken = [[] for _ in range(N_STREAMS)]
        self.raw, self.planted = [], []

    def conn(self, name, events, hop=7, u0=0, at=0, interval=INTERVAL, timed=True):
        """events: (counter, [P, ...]) pairs.  timed False: the connection will not be TIMED, so only its first event is HEAD."""
        aa, ci = ld.good_aa(self.rng), int(self.rng.integers(1, 1 << 24))
        sn, prev, cur = [0, 0], [None, None], [None, None]
        roles, messages = {}, []
        for n_ev, (c, packets) in enumerate(events):
            ch = (u0 + hop * c) % 37
            o = 3000 + at + c * interval * UNIT
            tail = not timed and n_ev > 0
            for k, p in enumerate(packets):
                role = k & 1
                if p.retx:
                    h0, payload = prev[role]
                else:
                    h0, payload = p.llid | (sn[role] << 3) | (sn[role ^ 1] << 2) | (p.md << 4), bytes(p.payload)
                    sn[role] ^= 1
                prev[role] = (h0, payload)
                end = o + 80 + 8 * len(payload)
                if p.lost:
                    tail = True                                    # what follows in this event cannot be given a role
                else:
                    assert end <= 64 * self.n_words, name
                    for a, b, whose in self.taken[ch]:                  # (another connection's packet within reach would join the event)
                        assert whose == name or end + 400 <= a or o >= b + 400, (name, c, ch, o)
                    self.taken[ch].append((o, end, name))
                    sym = _le.tx_bits(aa, ch, bytes([h0, len(payload)]) + payload, ci)
                    self.bits[ch, o:o + len(sym)] = sym
                    self.raw.append(ld.Cand(o, aa, ci, ch, h0, len(payload), ch))
                    roles[o] = ROLE_UNKNOWN if tail else role
                    if not tail and not p.retx:
                        if p.llid == 2 and payload:
                            cur[role] = [role, bytearray(payload)]
                            messages.append(cur[role])
                        elif p.llid == 1 and payload and cur[role] is not None:
                            cur[role][1] += payload
                o = end + 150
        self.planted.append(Planted(name, aa, ci, roles, [(r, bytes(b)) for r, b in messages]))

    def noise(self, n):
        for k in range(n):
            ch = int(self.rng.integers(0, 37))
            self.raw.append(ld.Cand(int(self.rng.integers(0, 64 * self.n_words - 400)), ld.good_aa(self.rng), int(self.rng.integers(0, 1 << 24)),
                                    ch, 1 + int(self.rng.integers(0, 3)), int(self.rng.integers(0, 28)), ch))

    def words(self):
        w = np.stack([_le.pack(self.bits[s]) for s in range(N_STREAMS)])
        w.flags.writeable = False
        return w

    def built(self):
        raw = [self.raw[i] for i in self.rng.permutation(len(self.raw))]
        conns, cands = ld.group(raw, 2)
        tracks, pkts = lt.track(cands, len(conns), MHZ, N_STREAMS, UNIT, IFS, JITTER, lt.REMAP)
        by = {(p.aa, p.crc_init): p.name for p in self.planted}
        names = [by.get((c.access_address, c.crc_init)) for c in conns]
        return Built(conns, cands, tracks, pkts, self.words(), names, tuple(self.planted), self.n_words)


Built = collections.namedtuple("Built", "conns cands tracks pkts words names planted n_words")
E = P(1)                                                            # an empty PDU


def _octets(rng, n):
    return bytes(rng.integers(0, 256, n, dtype=np.uint8).tolist())


@functools.lru_cache(maxsize=None)
def planted_world():
    """The lattice of the planted truth: a handful of connections that between them use every channel 0..36."""
    w = World()
    r = np.random.default_rng(5)
    a23, b40, c9 = l2cap(4, _octets(r, 19)), l2cap(4, _octets(r, 36)), l2cap(6, _octets(r, 5))
    # events of 1 to 5 packets; one-fragment messages; a two-fragment message across two events; both roles interleaved
    w.conn("planted: plain", [(0, [P(2, a23), E]), (1, [P(2, b40[:27]), P(2, c9), P(1, b40[27:]), E, E]), (2, [E]),
                              (3, [E, P(2, a23[:10]), E, P(1, a23[10:])]), (4, [P(2, c9), E, E]), (5, [E, E])] +
           [(c, [E, E]) for c in range(6, 30)], hop=7, u0=0, at=0)
    # a retransmission in each role, with a new packet after it; a control PDU and empty PDUs between the fragments
    w.conn("planted: retransmissions", [(0, [P(2, b40[:20]), P(2, a23[:12])]), (1, [P(0, retx=True), P(0, retx=True)]),
                                        (2, [P(3, bytes([0x12])), E]), (3, [P(1, b40[20:]), P(1, a23[12:])]), (4, [E, P(2, c9)]),
                                        (5, [P(2, c9), E])] + [(c, [E, E]) for c in range(6, 31)], hop=11, u0=3, at=1300)
    # a lost packet: air time left, no candidate -- a tail event whose members are UNKNOWN; the message goes on behind it
    w.conn("planted: a lost packet", [(0, [P(2, b40[:27]), E]), (1, [E, P(2, c9), P(1, b40[27:], lost=True), E, P(1, b"\x55\x66")]),
                                      (2, [P(1, b40[27:]), E])] + [(c, [E, E]) for c in range(3, 32)], hop=5, u0=20, at=2600)
    # ORPHAN, RUNT (L = 1, 3), OVERRUN, and a message cut short by the next START
    w.conn("planted: odd messages", [(0, [P(1, b"\x01\x02\x03"), P(1, b"\x09")]), (1, [P(2, b"\x07"), P(2, b"\x03\x00\x04")]),
                                     (2, [P(1, b"\x08\x09"), E]), (3, [P(2, l2cap(4, b"abcdefgh", claim=3)), P(2, b40[:27])]),
                                     (4, [E, P(2, c9)]), (5, [P(0, b"\x01"), P(2, b"")])] + [(c, [E, E]) for c in range(6, 33)],
           hop=13, u0=9, at=3900)
    # not TIMED: two events five units apart
    w.conn("planted: not timed", [(0, [P(2, a23[:11]), E]), (1, [P(1, a23[11:]), P(2, c9)])], hop=16, u0=30, at=5200, interval=5, timed=False)
    w.conn("planted: md", [(c, [P(2, c9, md=1), E, P(2, c9), P(2, a23)]) for c in range(0, 33)], hop=9, u0=14, at=5300)
    w.noise(60)
    b = w.built()
    assert {ld_.stream for ld_ in b.cands if ld_.channel != ld.NO_CONN} >= set(range(37))
    return b


def planted_model(msg_cap=1 << 20, byte_cap=1 << 30, rules=MODEL):
    b = planted_world()
    return data(b.conns, b.cands, b.pkts, b.words, b.n_words, msg_cap, byte_cap, rules)


def check_planted(b, out):
    """The model's roles and messages are the planted ones, octet for octet -> the number of messages checked."""
    n = 0
    for g, name in enumerate(b.names):
        if name is None:
            continue
        plant = [p for p in b.planted if p.name == name][0]
        mine = [i for i, c in enumerate(b.cands) if c.channel == g]
        assert {b.cands[i].offset: out.dpkts[i].role for i in mine} == plant.roles, name
        msgs = [m for m in out.msgs if m.conn == g]
        assert [(m.role, out.payload[m.byte_offset:m.byte_offset + m.bytes]) for m in msgs] == plant.messages, name
        assert out.data[g].n_msgs == len(msgs)
        n += len(msgs)
    return n


# ---- hand-made lists ---------------------------------------------------------------------------------------------------------------
H = collections.namedtuple("H", "event counter h0 length offset stream")    # one member, in time order


def hand_built(conn_members, n_words, n_streams=1, seed=3, gap=1, shuffle=True, words=None):
    """conn_members: per connection its H members in time order.  The list: the connections one behind the other, `gap` non-members
    between them, each connection's members in a shuffled list order (time order is `rank`, not the list's).  -> Built (no tracks)."""
    rng = np.random.default_rng(seed)
    conns, cands, pkts = [], [], []
    for g, members in enumerate(conn_members):
        for _ in range(gap if isinstance(gap, int) else gap[g]):             # (gap: one number, or one per connection)
            cands.append(ld.Cand(int(rng.integers(0, 64 * n_words)), 0x11110000 + g, 7, 0, 1, 0, ld.NO_CONN))
            pkts.append(None)
        order = rng.permutation(len(members)) if shuffle else np.arange(len(members))
        mask = 0
        for m in members:
            mask |= 1 << (m.stream % 37)
        conns.append(ld.Conn(0x50000000 + g, 0x100 + g, len(members), sum(m.length == 0 for m in members), mask, len(cands)))
        for rank in order.tolist():
            m = members[rank]
            cands.append(ld.Cand(m.offset, 0x50000000 + g, 0x100 + g, m.stream, m.h0, m.length, g))
            pkts.append(lt.Pkt(rank, m.event, m.counter, m.stream % 37, 0xFF, 0xFF, 0))
    if words is None:
        words = rng.integers(0, 1 << 64, (n_streams, n_words), dtype=np.uint64)
    return Built(conns, cands, None, pkts, words, None, (), n_words)


def _h0(llid, sn):
    return llid | sn << 3


ALIGN_LENGTHS = (1, 3, 4, 7, 8, 9, 15, 16, 17, 27, 251, 255)


@functools.lru_cache(maxsize=None)
def align_list():
    """One connection whose every event is a START of one of ALIGN_LENGTHS from the central and an empty packet back: packet offsets
    over every residue mod 64, byte_offset -- the lengths' running sum -- over every residue mod 8, two-fragment messages, and at
    the end a payload across the stream's end, whose trailing bits read as zeros."""
    n_words, members, sn, total, seen = 96, [], [0, 0], 0, set()
    e = 0
    while len(seen) < 8 or e < 64 * 3:
        L = ALIGN_LENGTHS[(e * 5 + e // 12) % 12]
        off = (e * 67) % (64 * n_words - 80 - 8 * 255 - 64)
        seen.add(total % 8)
        members.append(H(e, e, _h0(2, sn[0]), L, off, e % 37))
        sn[0] ^= 1
        total += L
        if e % 3 == 0:                                              # a second fragment, of the next length
            L2 = ALIGN_LENGTHS[(e + 1) % 12]
            members.append(H(e, e, _h0(1, sn[1]), 0, off + 11, e % 37))
            members.append(H(e, e, _h0(1, sn[0]), L2, (off + 29 * e) % (64 * n_words - 2200), e % 37))
            sn[0] ^= 1
            sn[1] ^= 1
            total += L2
        else:
            members.append(H(e, e, _h0(1, sn[1]), 0, off + 11, e % 37))
            sn[1] ^= 1
        e += 1
    assert {m.offset % 64 for m in members if m.length} == set(range(64))
    members.append(H(e, e, _h0(2, sn[0]), 27, 64 * n_words - 56 - 8 * 9 - 3, 5))      # nine octets and five bits inside
    members.append(H(e + 1, e + 1, _h0(2, sn[0] ^ 1), 255, 64 * n_words - 40, 6))    # wholly beyond the end
    return hand_built([members], n_words, n_streams=37, gap=3)


SEAM = 64                                                           # a wave of slots; 256 (a workgroup's round) and 2048 (a tile) are multiples
SEAM_PATTERN = ((-6, ("start", 17)), (-4, ("cont", 3)), (-2, ("cont", 4)), (0, ("cont", 8)), (2, ("cont", 1)),      # one role
                (-5, ("start", 9)), (-3, ("retx", 0)), (-1, ("retx", 0)), (1, ("retx", 0)), (3, ("cont", 5)))       # the other


def _long_members(n, first):
    """One connection of n members, two per event, whose first member lies in slot `first` of the list (slot = first + rank: the
    kernels' wave, workgroup and tile seams lie in SLOT space).  At EVERY multiple of 64 slots inside it, all three at once: one
    role's message of five fragments across the seam; the other role's START in front of it (inside that message), a run of three
    retransmissions of it across the seam -- one of them directly behind it, its previous member of the same role in front --, and
    its CONTINUATION behind: a START / CONTINUATION pair with the seam between them.  At every second seam the pattern lies one slot
    earlier, so that the seam's first slot holds a fragment at one seam and a retransmission at the next."""
    members, sn = [], [0, 0]
    want = {}
    for k, seam in enumerate(range((first // SEAM + 1) * SEAM, first + n - 8, SEAM)):
        r0 = seam - first - (k & 1)
        if r0 < 8:
            continue
        for off, what in SEAM_PATTERN:
            want[r0 + off] = what
    last = [None, None]
    for r in range(n):
        role = r & 1
        what, L = want.get(r, ("empty", 0))
        if what == "retx" and last[role] is not None:
            h0, L = last[role]
        else:
            llid = 2 if what == "start" else 1
            h0 = _h0(llid, sn[role])
            sn[role] ^= 1
        last[role] = (h0, L)
        members.append(H(r // 2, r // 2, h0, L, (r * 131) % (64 * 64 - 400), (r // 2) % 37))
    return members


@functools.lru_cache(maxsize=None)
def seam_list(which):
    """Hand-made lists on 64-word streams: 'long' -- one connection of 3 000 members from slot 5 on, across the tile seam at slot
    2048; 'crowd' -- 3 000 connections of 1 to 3 members; 'both' -- the two together, the long one from slot 3000 on across the tile
    seam at 4096, with K and N no multiples of any tile."""
    small = []
    for g in range(3000 if which != "both" else 2999):
        k = 1 + g % 3
        sn = g & 1
        small.append([H(0, 0, _h0(2 if j != 1 else 1, sn ^ (j >> 1)), 1 + (g + 5 * j) % 11 if j != 1 or g % 4 else 0, (g * 37 + j * 700) % 3600,
                        (g + j) % 37) for j in range(k)])
    if which == "long":
        conn_members, gap = [_long_members(3000, 5)], 5
    elif which == "crowd":
        conn_members, gap = small, 0
    else:
        conn_members, gap = small[:1500] + [_long_members(3001, sum(len(m) for m in small[:1500]))] + small[1500:], 0
    return hand_built(conn_members, 64, n_streams=37, gap=gap, seed=9)


def check_seams(b, out):
    """In SLOT space: at every multiple of 64 slots strictly inside the largest connection of a seam list -- 256 and 2048 among them
    -- a two-fragment message and one of four or more fragments have consecutive fragments on either side of the seam, and a
    RETRANSMIT in the seam's first or second slot has its previous member of the same role in front of the seam.  -> the seams
    checked, by class."""
    g = max(range(len(b.conns)), key=lambda x: b.conns[x].n_packets)
    first, n = b.conns[g].first, b.conns[g].n_packets
    at_slot = {first + b.pkts[i].rank: i for i in range(first, first + n)}
    assert len(at_slot) == n
    frags = collections.defaultdict(list)                           # message -> its fragments' slots
    for slot, i in at_slot.items():
        if out.dpkts[i].kind <= CONTINUATION:
            frags[out.dpkts[i].msg].append(slot)
    across = collections.defaultdict(set)                           # seam -> the fragment counts of the messages with a pair across it
    for M, slots in frags.items():
        slots.sort()
        for lo, hi in zip(slots, slots[1:]):
            if lo // SEAM != hi // SEAM:
                assert hi // SEAM == lo // SEAM + 1
                across[hi // SEAM * SEAM].add(out.msgs[M].n_fragments)
    seen = collections.Counter()
    for seam in range((first // SEAM + 1) * SEAM + SEAM, first + n - 8, SEAM):
        assert 2 in across[seam] and max(across[seam]) >= 4, (seam, across[seam])
        retx = [s for s in (seam, seam + 1) if out.dpkts[at_slot[s]].kind == RETRANSMIT]
        assert retx and all(out.dpkts[at_slot[s - 2]].role == out.dpkts[at_slot[s]].role and s - 2 < seam for s in retx), seam
        for cls in (64, 256, 2048):
            seen[cls] += seam % cls == 0
    return seen


def built_model(b, msg_cap=1 << 20, byte_cap=1 << 30, rules=MODEL):
    return data(b.conns, b.cands, b.pkts, b.words, b.n_words, msg_cap, byte_cap, rules)
