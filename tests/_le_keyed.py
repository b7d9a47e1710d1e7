"""Test-side model of keyed LE following (include/btbbx.h btbbx_le_keyed_epoch_* / btbbx_le_keyed_span_*), in plain
Python over the models of the unkeyed stages (tests/_le_follow.py follow, tests/_le_span.py span_follow) and tests/_le_crypt.py's
AES and CCM -- not from the kernels.

* keyed_follow / keyed_span: the keyed stages.  The contract's rules 1 to 3 become a VIEW of the input -- a READABLE member has
  length L' and its plaintext as payload, a member that stays unread reads as opcode 0xff, ENC_START closes nothing -- which the
  unkeyed models follow as they are; kind, opcode and the two flags are set behind them.  Rules: the branch points as options
* KeyedWorld: tests/_le_span.py's SpanWorld whose connections send control PDUs through cm.ccm_encrypt with their true packet
  counters; the data_pkts / crypt / crypt_pkts records that go with them are written by hand, so nothing here needs the data stage
  or the decryption stage
* twin: the independent check.  Capture T is capture S with every READABLE PDU replaced by its PLANTED plaintext PDU at the same
  offset, the ENC_START's opcode replaced by 0x12 and opcode 0xff in what stays OPAQUE; the unkeyed models on T must give what the
  keyed model gives on S
* lattice / end_world / crowd_world / span_world / wrap_world / chain_capture: the lists and the capture the CPU and GPU tests share
"""
import collections
import functools

import numpy as np

import _le
import _le_crypt as cm
import _le_csa2 as lc
import _le_data as dm
import _le_follow as lf
import _le_span as ls
import _le_track as lt

DECRYPTED = 128
CENTRAL, PERIPHERAL, UNKNOWN = 0, 1, 2
NONE = 0xFFFFFFFF


class Rules:
    """Rules() is the model; every other value is a wrong one."""

    def __init__(self, **kw):
        self.dir_flip = False               # rule 2: the direction bit the other way round
        self.s0_for_s1 = False              # rule 2: the keystream block of the MIC
        self.length_kept = False            # rule 3: parsed with L, not L - 4
        self.counter_hi_ignored = False     # rule 2: the packet counter's low 32 bits alone
        self.iv_swap = False                # rule 2: iv = IVs | IVm
        self.rank_ignored = False           # rule 1: READABLE whatever the rank
        self.failed_read = False            # rule 1: FAILED members read as well
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


MODEL = Rules()
VARIANTS = {name: {name: True} for name in ("dir_flip", "s0_for_s1", "length_kept", "counter_hi_ignored", "iv_swap", "rank_ignored",
                                            "failed_read")}
View = collections.namedtuple("View", "cands payload start readable opaque five")


def plaintext(row, n_words, cand, ch, role, cpkt, crypt, rules=MODEL):
    """Rule 2: the first min(L', 12) plaintext octets of a READABLE member."""
    c = cpkt.counter | (0 if rules.counter_hi_ignored else cpkt.counter_hi << 32)
    direction = int(role == CENTRAL) ^ int(rules.dir_flip)
    iv = bytes(crypt.iv[4:]) + bytes(crypt.iv[:4]) if rules.iv_swap else bytes(crypt.iv)
    nonce = bytes([c & 0xFF, (c >> 8) & 0xFF, (c >> 16) & 0xFF, (c >> 24) & 0xFF, ((c >> 32) & 0x7F) | direction << 7]) + iv
    s1 = cm.aes(bytes(crypt.session_key), bytes([1]) + nonce + bytes([0, 0 if rules.s0_for_s1 else 1]))
    length = cand.length if rules.length_kept else cand.length - 4
    raw = lf.read_payload(row, n_words, cand.offset, length, ch)
    return bytes(a ^ b for a, b in zip(raw, s1))


def view(cands, pkts, k, words, n_words, dpkts, crypt, cpkts, rules=MODEL):
    """Rules 1 to 3 -> View: the candidates with L' in a READABLE member's length; payload: (offset, channel, length) -> the octets
    the unkeyed models are to read there; per connection the ENC_START (or None); the READABLE members, those that stay OPAQUE and
    the READABLE members whose plaintext is opcode 5 with L' 1."""
    members = [[] for _ in range(k)]
    for i, p in enumerate(pkts):
        if p is not None and cands[i].channel < k:
            members[cands[i].channel].append(i)
    out, payload, start, readable, opaque, five = list(cands), {}, [None] * k, set(), set(), set()
    states = (cm.VERIFIED, cm.FAILED) if rules.failed_read else (cm.VERIFIED,)
    for g in range(k):
        order = sorted(members[g], key=lambda i: pkts[i].rank)
        ctl = [i for i in order if (cands[i].header0 & 3) == 3 and cands[i].length >= 1]
        raw = {i: lf.read_payload(words[cands[i].stream], n_words, cands[i].offset, cands[i].length, pkts[i].channel) for i in ctl}
        enc = [i for i in ctl if raw[i][0] == 5 and cands[i].length == 1][:1]
        start[g] = enc[0] if enc else None
        for i in ctl:
            c = cands[i]
            above = bool(enc) and pkts[i].rank > pkts[enc[0]].rank
            can = (crypt[g] is not None and crypt[g].flags & cm.F_KEYED and cpkts[i] is not None and cpkts[i].state in states and
                   c.length >= 5 and dpkts[i] is not None and dpkts[i].role in (CENTRAL, PERIPHERAL))
            if can and (above or rules.rank_ignored):
                plain = plaintext(words[c.stream], n_words, c, pkts[i].channel, dpkts[i].role, cpkts[i], crypt[g], rules)
                length = c.length if rules.length_kept else c.length - 4
                if plain[0] == 5 and length == 1:                     # never ENC_START: kept from the unkeyed models' sight
                    five.add(i)
                    plain = bytes([0x12])
                readable.add(i)
                out[i] = c._replace(length=length)
                payload[(c.offset, pkts[i].channel, length)] = plain
            elif above:
                opaque.add(i)
                payload[(c.offset, pkts[i].channel, c.length)] = bytes([0xFF]) * min(c.length, 12)
        if enc:
            payload[(cands[enc[0]].offset, pkts[enc[0]].channel, 1)] = bytes([0x12])
    return View(out, payload, start, readable, opaque, five)


class _Reading:
    """lf.read_payload, which both unkeyed models call, answering from a View's payload where it holds the member."""

    def __init__(self, payload):
        self.payload, self.saved = payload, lf.read_payload

    def __enter__(self):
        def read(row, n_words, offset, length, ch):
            got = self.payload.get((offset, ch, length))
            return got if got is not None else self.saved(row, n_words, offset, length, ch)
        lf.read_payload = read

    def __exit__(self, *exc):
        lf.read_payload = self.saved


def _close(v, cands, conn_recs, pkt_recs, seeds):
    """Behind the unkeyed model: kind and opcode of the members it was not to see as they are, the two flags."""
    pkt_recs = list(pkt_recs)
    for i in v.opaque:
        pkt_recs[i] = pkt_recs[i]._replace(kind=lf.OPAQUE, opcode=0xFF)
    for i in v.five:
        pkt_recs[i] = pkt_recs[i]._replace(opcode=5)
    for i in v.start:
        if i is not None:
            pkt_recs[i] = pkt_recs[i]._replace(kind=lf.ENC_START, opcode=5)
    conn_recs = list(conn_recs)
    for g, r in enumerate(conn_recs):
        if r is not None and seeds[g] is not None:
            extra = (lf.ENCRYPTED if v.start[g] is not None else 0) | (DECRYPTED if any(cands[i].channel == g for i in v.readable) else 0)
            conn_recs[g] = r._replace(flags=r.flags | extra)
    return conn_recs, pkt_recs


def keyed_follow(conns, cands, tracks, pkts, seeds, words, n_words, unit_bits, jitter_bits, dpkts, crypt, cpkts, rules=MODEL):
    """lf.follow's arguments and the three keyed arrays (lists of dm.DPkt, cm.Crypt, cm.CPkt or None) -> (follows, fpkts)."""
    v = view(cands, pkts, len(tracks), words, n_words, dpkts, crypt, cpkts, rules)
    with _Reading(v.payload):
        follows, fpkts = lf.follow(conns, v.cands, tracks, pkts, seeds, words, n_words, unit_bits, jitter_bits)
    return _close(v, cands, follows, fpkts, seeds)


def keyed_span(conns, cands, tracks, pkts, seeds, words, n_words, unit_bits, jitter_bits, max_updates, dpkts, crypt, cpkts, rules=MODEL):
    """ls.span_follow's arguments and the three keyed arrays -> (spans, spkts, recs)."""
    v = view(cands, pkts, len(tracks), words, n_words, dpkts, crypt, cpkts, rules)
    with _Reading(v.payload):
        spans, spkts, recs = ls.span_follow(conns, v.cands, tracks, pkts, seeds, words, n_words, unit_bits, jitter_bits, max_updates)
    return _close(v, cands, spans, spkts, seeds) + (recs,)


# ---- planted connections ----------------------------------------------------------------------------------------------------
class Enc(collections.namedtuple("Enc", "h0 plain counter role state sent")):
    """A control PDU sent encrypted: its plaintext, its 39-bit packet counter, its sender and the state the decryption stage is
    said to have given it.  sent: the counter it was really encrypted under (None: `counter`)."""
    def __new__(cls, plain, counter=0, role=CENTRAL, state=cm.VERIFIED, h0=3, sent=None):
        return super().__new__(cls, h0, bytes(plain), counter, role, state, sent)


START = (3, bytes([5]))
KBuilt = collections.namedtuple("KBuilt", ls.SBuilt._fields + ("dpkts", "crypt", "cpkts", "twin_words", "twin_cands", "sent"))


def _link_keys(n):
    return (bytes([n & 0xFF, n >> 8]) + bytes((37 * n + 11 * j + 5) & 0xFF for j in range(14)),
            bytes((91 * n + 29 * j + 3 + (n >> 8)) & 0xFF for j in range(8)))


class KeyedWorld(ls.SpanWorld):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.links, self.sent, self.marks = {}, [], []

    def _packet(self, name, p):
        if not isinstance(p, Enc):
            return p
        sk, iv, _ = self.links[name]
        c = p.counter if p.sent is None else p.sent
        return p.h0, cm.ccm_encrypt(sk, iv, c, int(p.role == CENTRAL), p.h0, p.plain)

    def secure(self, name, counters, pdus, keyed=True, ups=(), second=(), **kw):
        """ls.SpanWorld.walk for a connection with a session key (KEYED in its crypt record unless keyed is False); an Enc among the
        packets of pdus[counter] goes out encrypted.  ups: planted updates WITHOUT a PDU of their own (said None)."""
        assert all(u.said is None for u in ups)
        self.links[name] = _link_keys(len(self.links) + 1) + (keyed,)
        sent = {c: [self._packet(name, p) for p in v] for c, v in pdus.items()}
        at = len(self.raw)
        t0 = self.walk(name, counters, ups=ups, pdus=sent, second=second, **kw)
        assert len(self.raw) >= at
        first = len(self.raw) - sum(len(pdus.get(c, [lf.EMPTY])) + (c in second) for c in counters)
        for c in counters:
            for p in pdus.get(c, [lf.EMPTY]):
                if isinstance(p, Enc):
                    self.sent.append((name, self.raw[first], p))
                first += 1
            first += c in second
        return t0

    def put(self, name, offset, ch, packet, role=CENTRAL, state=None, in_stream=None):
        """One more packet of `name` at `offset` on data channel ch, as ls.SpanWorld.stray plants one, but cut at the stream's end: the
        bits that do not fit are not written (in_stream: the bits that are written, when fewer still)."""
        info = [i for i in self.info if i.name == name][0]
        h0, payload = self._packet(name, packet)
        cand = lf.ld.Cand(offset, info.aa, info.crc_init, ch, h0, len(payload), _le.channel_index(int(lt.LATTICE_MHZ[ch])))
        self.raw.append(cand)
        sym = _le.tx_bits(info.aa, cand.channel, bytes([h0, len(payload)]) + payload, info.crc_init)
        room = max(0, min(len(sym), 64 * self.n_words - offset))
        self.bits[ch, offset:offset + room] = sym[:room]
        if isinstance(packet, Enc):
            self.sent.append((name, cand, packet))

    def built(self, flags=lt.REMAP):
        b = super().built(flags)
        k = len(b.conns)
        where = {(c.stream, c.offset, c.access_address): i for i, c in enumerate(b.cands)}
        dpkts = [None if p is None else dm.DPkt(NONE, 0, CENTRAL, 0, 0) for p in b.pkts]
        cpkts = [None if p is None else cm.CPkt(0, 0, cm.CLEAR, 0, 0xFF, 0) for p in b.pkts]
        crypt = []
        for g in range(k):
            link = self.links.get(b.names[g])
            if link is None:
                crypt.append(cm.Crypt(bytes(16), bytes(8), NONE, NONE, NONE, 0, 0, 0, 0, 0xFF, 0, 0))
            else:
                f = cm.F_REQ | cm.F_RSP | cm.F_START | cm.F_ARMED | (cm.F_KEYED if link[2] else 0)
                crypt.append(cm.Crypt(link[0], link[1], NONE, NONE, NONE, 0, 0, 0, 0, 0 if link[2] else 0xFF, 0, f))
        bits, tcands, sent = self.bits.copy(), list(b.cands), []
        for name, cand, p in self.sent:
            i = where[(cand.stream, cand.offset, cand.access_address)]
            assert b.pkts[i] is not None, (name, cand)
            dpkts[i] = dm.DPkt(NONE, 0, p.role, 0, 0)
            low = p.counter & 0xFFFFFFFF
            cpkts[i] = cm.CPkt(low, low, p.state, 0 if p.state == cm.VERIFIED else 0xFF, p.plain[0] if p.state == cm.VERIFIED else 0xFF,
                               (p.counter >> 32) & 0x7F)
            sent.append((i, p))
        # the twin: what the unkeyed stages would read had the connection sent the same PDUs in the clear.  Whether a PDU is READABLE
        # is the PLANTED truth here -- VERIFIED, a known sender, a KEYED connection, behind the start --, not the model's verdict
        info = {x.name: x for x in self.info}
        starts = {}
        for i, c in enumerate(b.cands):
            if b.pkts[i] is not None and c.channel < k and (c.header0 & 3) == 3 and c.length == 1:
                if lf.read_payload(b.words[c.stream], b.n_words, c.offset, 1, b.pkts[i].channel)[0] == 5:
                    g = c.channel
                    if g not in starts or b.pkts[i].rank < b.pkts[starts[g]].rank:
                        starts[g] = i
        read = set()
        for i, p in sent:
            c = b.cands[i]
            g = c.channel
            link = self.links[b.names[g]]
            if not (p.state == cm.VERIFIED and p.role in (CENTRAL, PERIPHERAL) and link[2] and g in starts and
                    b.pkts[i].rank > b.pkts[starts[g]].rank and p.sent is None):
                continue
            x = info[b.names[g]]
            sym = _le.tx_bits(x.aa, b.pkts[i].channel, bytes([p.h0, len(p.plain)]) + p.plain, x.crc_init)
            room = max(0, min(len(sym), 64 * self.n_words - c.offset))
            bits[c.stream, c.offset:c.offset + room] = sym[:room]
            tcands[i] = c._replace(length=len(p.plain))
            read.add(i)
        # (what stays OPAQUE in S -- ciphertext nobody VERIFIED, or a PDU sent in the clear behind the start -- must not act in T, whose
        # reader knows no start: opcode 0xff there)
        for i, c in enumerate(b.cands):
            g = c.channel
            if (b.pkts[i] is not None and g in starts and (c.header0 & 3) == 3 and c.length >= 1 and i not in read and
                    b.pkts[i].rank > b.pkts[starts[g]].rank and c.stream < lt.N_STREAMS):
                sym = _le.tx_bits(c.access_address, b.pkts[i].channel, bytes([c.header0, c.length]) + bytes([0xFF]) * c.length, c.crc_init)
                room = max(0, min(len(sym), 64 * self.n_words - c.offset))
                bits[c.stream, c.offset:c.offset + room] = sym[:room]
        for g, i in starts.items():
            c = b.cands[i]
            sym = _le.tx_bits(c.access_address, b.pkts[i].channel, bytes([c.header0, 1, 0x12]), c.crc_init)
            room = max(0, min(len(sym), 64 * self.n_words - c.offset))
            bits[c.stream, c.offset:c.offset + room] = sym[:room]
        twin_words = np.stack([_le.pack(bits[s]) for s in range(lt.N_STREAMS)])
        return KBuilt(*b, dpkts=dpkts, crypt=crypt, cpkts=cpkts, twin_words=twin_words, twin_cands=tcands, sent=tuple(sent))


def model_follow(b, rules=MODEL):
    """(seeds, follows, fpkts) of the keyed model on a KBuilt."""
    seeds = lf.seed(b.adv, b.conns, b.tracks, b.unit)
    return (seeds,) + keyed_follow(b.conns, b.cands, b.tracks, b.pkts, seeds, b.words, b.n_words, b.unit, b.jitter, b.dpkts, b.crypt, b.cpkts,
                                   rules)


def model_span(b, max_updates, rules=MODEL):
    """(seeds, spans, spkts, recs)."""
    seeds = lf.seed(b.adv, b.conns, b.tracks, b.unit)
    return (seeds,) + keyed_span(b.conns, b.cands, b.tracks, b.pkts, seeds, b.words, b.n_words, b.unit, b.jitter, max_updates, b.dpkts,
                                 b.crypt, b.cpkts, rules)


def twin_follow(b):
    """The unkeyed follow model on the twin capture, with S's tracking records."""
    seeds = lf.seed(b.adv, b.conns, b.tracks, b.unit)
    return (seeds,) + lf.follow(b.conns, b.twin_cands, b.tracks, b.pkts, seeds, b.twin_words, b.n_words, b.unit, b.jitter)


def twin_span(b, max_updates):
    seeds = lf.seed(b.adv, b.conns, b.tracks, b.unit)
    return (seeds,) + ls.span_follow(b.conns, b.twin_cands, b.tracks, b.pkts, seeds, b.twin_words, b.n_words, b.unit, b.jitter, max_updates)


def crosses_the_end(b):
    """The connections with a sent PDU whose plaintext octets, as rule 2 reads them, reach beyond the stream's end.  There the keyed
    reader has the keystream over zeros and no capture can hold that as a clear PDU: the twin says nothing about them."""
    return {b.cands[i].channel for i, p in b.sent if b.cands[i].offset + 56 + 8 * min(max(b.cands[i].length - 4, 0), 12) > 64 * b.n_words}


def same_as_twin(b, keyed, twin):
    """keyed / twin: (conn records, packet records[, span records]) of the keyed model on S and of the unkeyed model on T.  Field for
    field the same, but for the ENCRYPTED / DECRYPTED bits, the start packet's kind and opcode, the members that are OPAQUE in S and
    the connections of crosses_the_end.  -> the number of packet records compared."""
    out = crosses_the_end(b)
    for g, (x, y) in enumerate(zip(keyed[0], twin[0])):
        assert (x is None) == (y is None), b.names[g]
        if x is not None and g not in out:
            mask = ~(lf.ENCRYPTED | DECRYPTED)
            assert x._replace(flags=x.flags & mask) == y._replace(flags=y.flags & mask), (b.names[g], x, y)
    n = 0
    for i, (x, y) in enumerate(zip(keyed[1], twin[1])):
        assert (x is None) == (y is None), i
        if x is None or x.kind == lf.OPAQUE or b.cands[i].channel in out:
            continue
        if x.kind == lf.ENC_START:
            x, y = x._replace(kind=0, opcode=0), y._replace(kind=0, opcode=0)
        elif (x.kind, x.opcode, y.kind) == (lf.CONTROL, 5, lf.ENC_START) and b.twin_cands[i].length == 1:
            y = y._replace(kind=lf.CONTROL)          # (rule 3's "never ENC_START": T's reader knows no such rule.  Nothing lies behind it)
        assert x == y, (i, b.names[b.cands[i].channel], x, y)
        n += 1
    if len(keyed) > 2:
        per = len(keyed[2]) // max(len(keyed[0]), 1)
        assert len(keyed[2]) == len(twin[2])
        for j, (x, y) in enumerate(zip(keyed[2], twin[2])):
            assert x == y or j // per in out, j
    return n


# ---- the shared worlds --------------------------------------------------------------------------------------------------------
FULL, NINE, FIVE, M36 = lc.FULL_MAP, lf.NINE, lf.FIVE, lf.M36
RESIDUES = (0, 7, 8, 56, 57, 63)
LENGTHS = (1, 2, 8, 11, 12, 13, 23)
COUNTERS = (0, 1, (1 << 32) - 1, 1 << 32, (1 << 39) - 1)


def _control(length, instant, chmap=NINE, interval=8):
    """A plaintext control PDU of this length: opcode 5 (never ENC_START), TERMINATE, a map update, opcode 0 one octet short of a
    parameter update, a parameter update, opcode 1 longer than a map update, LL_ENC_REQ's length."""
    if length == 1:
        return bytes([5])
    if length == 2:
        return lf.TERMINATE_IND[1]
    if length == 8:
        return lf.map_ind(chmap, instant)[1]
    if length == 12:
        return ls.param_ind(instant, interval)[1]
    if length == 11:
        return ls.param_ind(instant, interval)[1][:11]
    if length == 13:
        return lf.map_ind(chmap, instant)[1] + bytes(5)
    return bytes([3]) + bytes((7 * j + 1) & 0xFF for j in range(length - 1))


def plant_at(w, name, residue, said, build):
    """build(dev) plants the connection `name` with the deviations dev (counter -> bits); it is planted again, moved by less than half
    a word, until the payload of the Enc in event `said` begins at `residue` modulo 64."""
    dev = {}
    for _ in range(8):
        keep = len(w.raw), len(w.adv), len(w.info), [len(x) for x in w.taken], w.k, len(w.sent), dict(w.links), w.bits.copy()
        build(lambda c: dev.get(c, 0))
        cand = [c for n, c, p in w.sent[keep[5]:] if n == name][0]
        off = (residue - (cand.offset + 56)) % 64
        if off == 0:
            return
        del w.raw[keep[0]:], w.adv[keep[1]:], w.info[keep[2]:], w.sent[keep[5]:]
        for x, n in zip(w.taken, keep[3]):
            del x[n:]
        w.k, w.links, w.bits = keep[4], keep[6], keep[7]
        w.by_anchor.pop(name, None)
        dev[said] = dev.get(said, 0) + (off if off < 32 else off - 64)
    raise AssertionError("no place for %s" % name)


@functools.lru_cache(maxsize=None)
def lattice():
    """Single connections: the payload's first bit at every residue modulo 64 at which the octet reads change, every length at which
    the parse changes, both senders, packet counters on both sides of bit 32 and at the top of the 39."""
    w = KeyedWorld(11)
    r14 = range(14)
    n = 0
    for residue in RESIDUES:
        for length in LENGTHS:
            role, counter = (CENTRAL, PERIPHERAL)[n & 1], COUNTERS[n % 5]
            n += 1
            name = "planted: L' %d at %d, role %d, counter %d" % (length, residue, role, counter)
            kw = dict(alg=1 + (n & 1), hop=5 + n % 12)
            if length == 8:                                           # the map update is what the connection does from counter 7 on
                kw["maps"] = ((7, NINE),)
            ups = (ls.Up(8, 8, win_offset=2),) if length == 12 else ()
            pdu = Enc(_control(length, 7 if length == 8 else 8), counter, role)
            packets = [lf.EMPTY, pdu] if role == PERIPHERAL else [pdu]
            plant_at(w, name, residue, 4, lambda dev, name=name, ups=ups, packets=packets, kw=kw: w.secure(
                name, r14, {1: [START], 4: packets}, ups=ups, dev=dev, **kw))
    # ---- rule 1's conditions, one connection each
    w.secure("planted: FAILED map update is not read", r14, {1: [START], 3: [Enc(lf.map_ind(FIVE, 5)[1], 1, state=cm.FAILED)]})
    w.secure("planted: SKIPPED and SHORT are not read", r14, {1: [START], 3: [Enc(lf.map_ind(FIVE, 5)[1], 1, state=cm.SKIPPED)],
                                                             4: [Enc(lf.map_ind(NINE, 6)[1], 2, state=cm.SHORT)]})
    w.secure("planted: not KEYED", r14, {1: [START], 3: [Enc(lf.map_ind(FIVE, 5)[1], 1)]}, keyed=False)
    w.secure("planted: role UNKNOWN", r14, {1: [START], 3: [Enc(lf.map_ind(FIVE, 5)[1], 1, role=UNKNOWN)]})
    w.secure("planted: VERIFIED in front of the start", r14, {2: [Enc(lf.map_ind(FIVE, 4)[1], 1)], 6: [START]})
    w.secure("planted: VERIFIED without a start", r14, {2: [Enc(lf.map_ind(FIVE, 4)[1], 1)]})
    w.secure("planted: VERIFIED in the start's own event", r14, {2: [START, Enc(lf.map_ind(NINE, 5)[1], 0, PERIPHERAL)]}, maps=((5, NINE),))
    w.secure("planted: clear update behind the start stays OPAQUE", r14, {1: [START], 3: [lf.map_ind(FIVE, 5)]})
    w.secure("planted: two encrypted map updates, equal instants", r14,
             {1: [START], 3: [Enc(lf.map_ind(FIVE, 6)[1], 0)], 4: [lf.EMPTY, Enc(lf.map_ind(NINE, 6)[1], 0, PERIPHERAL)]}, maps=((6, NINE),))
    w.secure("planted: encrypted TERMINATE", r14, {1: [START], 9: [Enc(lf.TERMINATE_IND[1], 3)]})
    w.secure("planted: iv and direction matter", r14, {0: [START], 2: [lf.EMPTY, Enc(lf.map_ind(M36, 4)[1], (1 << 32) + 5, PERIPHERAL)]},
             maps=((4, M36),), alg=2)
    w.conn("planted: never encrypts", r14, pdus={3: [lf.map_ind(NINE, 6)]}, maps=((6, NINE),))
    w.noise(40)
    return w.built()


@functools.lru_cache(maxsize=None)
def end_world():
    """READABLE map and parameter updates whose last payload bit -- the last bit of plaintext octet L' - 1: rule 2 never reads the MIC
    as payload -- lies from 104 bits in front of the stream's end to 8 bits behind it, in steps of 8 and one bit either side, and 40
    bits behind it: from +1 on the Instant's octets cross the end and are read as zeros.  One connection, one more packet per distance."""
    w = KeyedWorld(13)
    end = 64 * w.n_words
    dists = sorted(set(range(-104, 9, 8)) | {-1, 1, 40})
    for kind, length in (("map", 8), ("param", 12)):
        for n, d in enumerate(dists):
            name = "%s update ending %d bits from the end" % (kind, d)
            ch = n + (len(dists) if kind == "param" else 0)            # (a stream of its own: the PDUs lie side by side)
            t0 = w.secure(name, range(3), {1: [START]}, req_offset=900 + 1300 * n + (400 if kind == "param" else 0))
            offset = end + d - (56 + 8 * length)                       # (L' octets of payload behind the header; the MIC behind them)
            c_est = (offset - t0) // (6 * w.unit)
            plain = lf.map_ind(NINE, c_est + 3)[1] if kind == "map" else ls.param_ind(c_est + 3, 8, 2, 1)[1]
            w.put(name, offset, ch, Enc(plain, n + 1, (CENTRAL, PERIPHERAL)[n & 1]))
    return w.built()


@functools.lru_cache(maxsize=None)
def crowd_world():
    """600 connections with distinct session keys -- more than two workgroups of a per-connection launch, members across the tile
    seams --, each with one encrypted map update that is VERIFIED and one that is FAILED; every third one is not KEYED."""
    w = KeyedWorld(17)
    for n in range(600):
        good, bad = (NINE, FIVE) if n & 1 else (M36, NINE)
        w.secure("planted: crowd %d" % n, range(5), {0: [START], 1: [Enc(lf.map_ind(bad, 3)[1], 0, state=cm.FAILED)],
                                                     2: [lf.EMPTY, Enc(lf.map_ind(good, 3)[1], (n << 20) + 1, PERIPHERAL)]},
                 keyed=n % 3 != 2, maps=((3, good),) if n % 3 != 2 else (), hop=5 + n % 12, alg=1 + (n & 1), interval=6 + n % 3,
                 req_offset=500 + 330 * n)
    w.noise(30)
    return w.built()


@functools.lru_cache(maxsize=None)
def span_world():
    """One connection that applies an encrypted parameter update, sends an encrypted map update in span 1 and then an encrypted
    TERMINATE and another encrypted map update; one whose encrypted parameters are invalid."""
    w = KeyedWorld(19)
    w.secure("planted: encrypted update, map update in span 1, TERMINATE, map update", range(40),
             {1: [START], 3: [Enc(ls.param_ind(7, 9, 2, 1)[1], 0)], 9: [lf.EMPTY, Enc(lf.map_ind(NINE, 14)[1], 0, PERIPHERAL)],
              16: [Enc(lf.TERMINATE_IND[1], 2)], 18: [Enc(lf.map_ind(FIVE, 24)[1], 3)]},
             ups=(ls.Up(7, 9, win_offset=2),), maps=((14, NINE), (24, FIVE)), alg=2)
    w.secure("refused: encrypted update, interval 5", range(20), {1: [START], 3: [Enc(ls.param_ind(8, 5, 1, 1)[1], 0)]})
    w.noise(10)
    return w.built()


@functools.lru_cache(maxsize=None)
def wrap_world():
    """ls.wrap_world's geometry (unit_bits 2, jitter_bits 0, streams of 12 800 words: counter 65 536 lies 786 432 bits behind t0 at the
    least): an encrypted map update and an encrypted parameter update announced in front of counter 65 536 for instants behind it."""
    w = KeyedWorld(23, unit=2, n_words=12800, ifs=0, jitter=0)
    near = (65527, 65528, 65529, 65530, 65534, 65535, 65536, 65537, 65538, 65540)
    w.secure("planted: encrypted updates next to 65536", near,
             {65527: [START], 65529: [Enc(ls.param_ind(65537, 8, 1, 1)[1], 1 << 32)], 65530: [Enc(lf.map_ind(NINE, 65536)[1], (1 << 32) + 1)]},
             ups=(ls.Up(65537, 8, 1, 1, 1),), maps=((65536, NINE),))
    w.secure("planted: clear beside it", near, {}, hop=11)
    w.noise(10)
    return w.built()


@functools.lru_cache(maxsize=None)
def lattice_models():
    b = lattice()
    out = {m: model_span(b, m) for m in (0, 1, 2)}
    out["follow"] = model_follow(b)
    return out


# ---- a capture for the host wrapper: pairing, encryption start, encrypted updates ----------------------------------------------
class _Placed(dm.World):
    """dm.World whose events lie where place(counter) -> (channel, offset) puts them, not on dm.World's fixed grid: the connection
    may change its map and its interval.  (dm.World.conn's loop, with the two lines that place an event replaced.)"""
    place = None

    def conn(self, name, events, **kw):
        aa, ci = lf.ld.good_aa(self.rng), int(self.rng.integers(1, 1 << 24))
        sn, prev, roles = [0, 0], [None, None], {}
        for c, packets in events:
            ch, o = self.place(c)
            for k, p in enumerate(packets):
                role = k & 1
                assert not p.retx and not p.lost
                h0, payload = p.llid | (sn[role] << 3) | (sn[role ^ 1] << 2) | (p.md << 4), bytes(p.payload)
                sn[role] ^= 1
                end = o + 80 + 8 * len(payload)
                assert end <= 64 * self.n_words, name
                for a, b, whose in self.taken[ch]:
                    assert whose == name or end + 400 <= a or o >= b + 400, (name, c, ch, o)
                self.taken[ch].append((o, end, name))
                sym = _le.tx_bits(aa, ch, bytes([h0, len(payload)]) + payload, ci)
                self.bits[ch, o:o + len(sym)] = sym
                self.raw.append(lf.ld.Cand(o, aa, ci, ch, h0, len(payload), ch))
                roles[o] = role
                o = end + 150
        self.planted.append(dm.Planted(name, aa, ci, roles, []))


class _ChainWorld(cm.CryptWorld, _Placed):
    pass


CHAIN_HOP, CHAIN_MAP_AT, CHAIN_PARAM_AT, CHAIN_INTERVAL, CHAIN_WIN_OFFSET, CHAIN_EVENTS = 7, 11, 14, 12, 6, 24
CHAIN_NAME, CHAIN_PLAIN = "pairs, encrypts, updates its map and its interval", "never encrypts"
Chain = collections.namedtuple("Chain", "cap stk t0")


@functools.lru_cache(maxsize=None)
def chain_capture():
    """A CONNECT_IND, a Just Works legacy pairing, an encryption start under the STK, then an encrypted LL_CHANNEL_MAP_IND (in force
    from counter 11) and an encrypted LL_CONNECTION_UPDATE_IND (interval 12 and WinOffset 6 from counter 14), both instants inside the
    capture; beside it a connection that never encrypts and sends its map update in the clear.  The new interval's events lie on the
    old interval's grid, so the tracking stays TIMED across the update: the data stage takes its roles, and so the decryption stage
    its counters, from the tracking's counters.  -> Chain: the ld.Capture (37 data streams, three advertising streams), the STK, the
    two connections' t0."""
    import _le_pair as pm
    P, E = dm.P, dm.E
    w = _ChainWorld(seed=71)
    U = dm.UNIT
    seeds = {CHAIN_NAME: pm.seed_of(1), CHAIN_PLAIN: pm.seed_of(2)}
    req = {CHAIN_NAME: 200, CHAIN_PLAIN: 1500}
    t0 = {n: req[n] + 352 + U * 2 for n in req}                         # (win_offset 1)

    def place(name, hop, updates):
        def at(c):
            m = FULL if c < CHAIN_MAP_AT else NINE
            ch = lt.csa1_at(0, hop, c + 1, m)
            if not updates or c < CHAIN_PARAM_AT:
                return ch, t0[name] + c * dm.INTERVAL * U + 7
            return ch, t0[name] + CHAIN_PARAM_AT * dm.INTERVAL * U + CHAIN_WIN_OFFSET * U + (c - CHAIN_PARAM_AT) * CHAIN_INTERVAL * U + 7
        return at

    messages, mrand, srand = pm.exchange(0, seeds[CHAIN_NAME], n=77)
    stk = pm.s1(0, mrand, srand, 16)
    smp = [dm.l2cap(pm.SMP_CID, body) for _, body in messages]
    pdus = {0: [E, E], 1: [P(2, smp[0]), P(2, smp[1])], 2: [P(2, smp[2]), P(2, smp[3])], 3: [P(2, smp[4]), P(2, smp[5])],
            4: [cm.REQ, cm.RSP], 5: [E, cm.BEGIN], 6: [P(3, b"\x06"), P(3, b"\x06")], 7: [P(3, lf.map_ind(NINE, CHAIN_MAP_AT)[1]), E],
            9: [P(3, ls.param_ind(CHAIN_PARAM_AT, CHAIN_INTERVAL, CHAIN_WIN_OFFSET, 1)[1]), E]}
    w.place = place(CHAIN_NAME, CHAIN_HOP, True)
    w.conn(CHAIN_NAME, [(c, pdus.get(c, [E, E])) for c in range(CHAIN_EVENTS)], ltk=stk)
    w.place = place(CHAIN_PLAIN, 11, False)
    w.conn(CHAIN_PLAIN, [(c, [P(3, lf.map_ind(NINE, CHAIN_MAP_AT)[1]), E] if c == 5 else [E, E]) for c in range(CHAIN_EVENTS)])
    w.noise(20)
    b = w.built()
    adv = np.random.default_rng(45).integers(0, 2, (3, 64 * b.n_words), dtype=np.uint8)
    for p in b.planted:
        s = seeds[p.name]
        body = lf.connect_ind(p.aa, p.crc_init, FULL, CHAIN_HOP if p.name == CHAIN_NAME else 11, dm.INTERVAL, tx_add=s.tx_add, rx_add=s.rx_add,
                              init_a=s.init_a, adv_a=s.adv_a)
        sym = _le.tx_bits(_le.ADV_AA, 37, body[4:40], _le.ADV_CRC_INIT)
        adv[0, req[p.name]:req[p.name] + len(sym)] = sym
    words = np.vstack([np.asarray(b.words)] + [_le.pack(row)[None, :] for row in adv])
    words.flags.writeable = False
    return Chain(lf.ld.Capture(words, b.n_words, b.n_words, 64 * b.n_words - 39, lf.CHAIN_MHZ, b.planted, 27), stk, t0)
