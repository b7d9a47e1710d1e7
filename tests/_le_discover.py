"""Test-side model of the promiscuous LE connection discovery (include/btbbx.h btbbx_le_discover_*), written
from the six rules of a candidate with the registers of tests/_le.py -- not from the kernels (le_discover.h runs the CRC
register backwards in its reflected byte form; here the spec's positions are shifted literally, one bit at a time).

* crc24_backward: the CRC register run backwards through data bits
* candidates: brute force over every offset of one packed stream
* group: the grouping stage as a plain sorted() and itertools.groupby
* Rules: the model's branch points as options; Rules() is the model, any other value a deliberately wrong one
  (tests/test_le_discover_model.py shows that the lattice below tells each from the right one)
* scan_lattice / chain_capture: the captures the CPU and GPU tests share
"""
import collections
import functools
import itertools

import numpy as np

import _le

NO_CONN = 0xFFFFFFFF
_TAPS = sum(1 << t for t in _le.CRC_TAPS)

Cand = collections.namedtuple("Cand", "offset access_address crc_init stream header0 length channel")
Conn = collections.namedtuple("Conn", "access_address crc_init n_packets n_empty channel_mask first")


class Rules:
    def __init__(self, **kw):
        self.len_strict = False          # h1 < max_len
        self.llid0 = False               # LLID 0 accepted
        self.rfu_mask = 0xE0
        self.end_strict = False          # rule 5 with <
        self.end_slack = 0               # rule 5 lets a packet end this many bits past the stream (None: no rule 5)
        self.preamble_aa_bit = 0         # the AA bit the preamble's first bit equals
        self.seed_shift = 0              # whitening seeded from channel index + this
        self.crc_octets_short = 0        # the CRC walked over 2 + h1 - this octets
        self.crc_init_reversed = False
        self.max_offenses = 0
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


MODEL = Rules()
VARIANTS = dict(len_strict=dict(len_strict=True), llid0=dict(llid0=True), rfu_mask=dict(rfu_mask=0xC0), end_strict=dict(end_strict=True),
                preamble_aa_bit=dict(preamble_aa_bit=1), seed_shift=dict(seed_shift=1), crc_octets_short=dict(crc_octets_short=1),
                crc_init_reversed=dict(crc_init_reversed=True), max_offenses=dict(max_offenses=1),
                end_permissive=dict(end_slack=1), end_absent=dict(end_slack=None))


def crc24_backward(bits, received):
    """The preset of the CRC register (Vol 6 Part B 3.1.1, figure 3.4) given the 24 CRC bits as received (position 23 first) and
    the data bits they cover: every clock of _le.crc24_register undone, last data bit first.  Position 0 took the feedback and
    no tap, so it names the feedback; the taps are taken out again, every position moves down by one, and position 23 was
    feedback XOR data bit."""
    pos = sum(int(b) << (23 - i) for i, b in enumerate(received))      # bit i = position i
    for b in reversed(np.asarray(bits, np.uint8).tolist()):
        fb = pos & 1
        if fb:
            pos ^= _TAPS
        pos = (pos >> 1) | ((fb ^ b) << 23)
    return pos


def _reverse24(x):
    return int("{:024b}".format(x)[::-1], 2)


@functools.lru_cache(maxsize=None)
def _offenses(aa):
    return _le.data_offenses(aa)


def candidates(words, n_words, search_bits, mhz, max_len, stream=0, rules=MODEL):
    """Every candidate of one packed stream (its row of LSB-first uint64 words), as Cand tuples in offset order."""
    ch = _le.channel_index(int(mhz))
    if ch >= 37:
        return []
    total = 64 * n_words
    bits = np.unpackbits(np.asarray(words[:n_words], np.uint64).view(np.uint8), bitorder="little")
    bits = np.concatenate([bits, np.zeros(8 * 262, np.uint8)])       # (what a wrong rule 5 would read behind the stream's end: zeros)
    wh = _le.whitening_bits((ch + rules.seed_shift) & 0x3F, 8 * 260)
    # rule 2 at every offset: eight relations between bits o .. o + 9
    n = min(search_bits, total - 10)
    ok = np.ones(n, bool)
    for j in range(7):
        ok &= bits[j:n + j] != bits[j + 1:n + j + 1]
    ok &= bits[:n] == bits[8 + rules.preamble_aa_bit:n + 8 + rules.preamble_aa_bit]
    out = []
    for o in np.nonzero(ok)[0].tolist():
        aa = _le.bits_value(bits[o + 8:o + 40])
        if _offenses(aa) > rules.max_offenses:
            continue
        hdr = bits[o + 40:o + 56] ^ wh[:16]
        h0, h1 = _le.bits_value(hdr[:8]), _le.bits_value(hdr[8:])
        if ((h0 & 3) == 0 and not rules.llid0) or (h0 & rules.rfu_mask):
            continue
        if h1 >= max_len if rules.len_strict else h1 > max_len:
            continue
        end = o + 40 + 8 * (2 + h1 + 3)
        if rules.end_slack is not None and (end >= total if rules.end_strict else end > total + rules.end_slack):
            continue
        n_pdu = 8 * (2 + h1 - rules.crc_octets_short)
        body = bits[o + 40:o + 40 + n_pdu + 24] ^ wh[:n_pdu + 24]
        init = crc24_backward(body[:n_pdu], body[n_pdu:])
        out.append(Cand(o, aa, _reverse24(init) if rules.crc_init_reversed else init, stream, h0, h1, ch))
    return out


def capture_candidates(cap, max_len, rules=MODEL):
    out = []
    for s in range(len(cap.mhz)):
        out += candidates(cap.words[s], cap.n_words, cap.search_bits, cap.mhz[s], max_len, s, rules)
    return out


def group(cands, min_count):
    """(conns, cands sorted with their connection index in place of the channel) of a candidate list."""
    order = sorted(cands, key=lambda c: ((c.access_address << 24) | c.crc_init, c.stream, c.offset))
    conns, out = [], []
    for key, members in itertools.groupby(order, key=lambda c: (c.access_address, c.crc_init)):
        members = list(members)
        ci = NO_CONN
        if len(members) >= min_count:
            ci = len(conns)
            mask = 0
            for m in members:
                mask |= 1 << (m.channel & 63)
            conns.append(Conn(key[0], key[1], len(members), sum(m.length == 0 for m in members), mask, len(out)))
        out += [m._replace(channel=ci) for m in members]
    return conns, out


def cand_array(cands, dtype):
    """Cand tuples -> LE_CAND_DTYPE records (the last field goes to `conn`)."""
    a = np.zeros(len(cands), dtype)
    for i, c in enumerate(cands):
        a[i] = (c.offset, c.access_address, c.crc_init, c.stream, c.header0, c.length, c.channel)
    return a


def conn_array(conns, dtype):
    a = np.zeros(len(conns), dtype)
    for i, c in enumerate(conns):
        a[i] = tuple(c)
    return a


def cand_tuples(arr):
    return [Cand(*(int(r[k]) for k in ("offset", "access_address", "crc_init", "stream", "header0", "length", "conn"))) for r in arr]


# ---- access addresses -----------------------------------------------------------------------------------------------
def good_aa(rng, low2=None):
    """A random access address without offense (low2: its two lowest bits)."""
    while True:
        aa = int(rng.integers(0, 1 << 32))
        if low2 is not None:
            aa = (aa & ~3) | low2
        if _offenses(aa) == 0:
            return aa


def _transitions(aa):
    return bin((aa ^ (aa >> 1)) & 0x7FFFFFFF).count("1")


OFFENSE_KINDS = dict(
    transitions=lambda aa: _transitions(aa) == 25,
    top6=lambda aa: bin(((aa >> 26) ^ (aa >> 27)) & 0x1F).count("1") < 2,
    equal_octets=lambda aa: len(set(aa.to_bytes(4, "little"))) == 1,
    adv_neighbour=lambda aa: bin(aa ^ _le.ADV_AA).count("1") == 1,
    run_window=lambda aa: any((aa >> s) & 0xFFF in _le.RUN_WINDOWS for s in range(0, 21, 4)),
)


def one_offense_aas(seed=7):
    """kind -> an access address with exactly one offense, of that kind."""
    rng = np.random.default_rng(seed)
    out = {}
    for kind, pred in OFFENSE_KINDS.items():
        if kind == "equal_octets":
            pool = [b * 0x01010101 for b in range(256)]
        elif kind == "adv_neighbour":
            pool = [_le.ADV_AA ^ (1 << b) for b in range(32)]
        else:
            pool = None
        for k in range(200000):
            if pool is not None and k >= len(pool):
                break
            aa = pool[k] if pool is not None else int(rng.integers(0, 1 << 32))
            if kind == "transitions" and pool is None:               # (random words rarely have 25 transitions: start from 0x55555555)
                aa = 0x55555555 ^ (int(rng.integers(0, 1 << 32)) & int(rng.integers(0, 1 << 32)) & int(rng.integers(0, 1 << 32)))
            if pred(aa) and _offenses(aa) == 1:
                out[kind] = aa
                break
    return out


# ---- the scan lattice --------------------------------------------------------------------------------------------------
Plant = collections.namedtuple("Plant", "stream offset aa crc_init header0 length note")
Capture = collections.namedtuple("Capture", "words n_words pitch_words search_bits mhz planted max_len")

LATTICE_MHZ = (2404, 2440, 2478, 2402, 2426, 2451)          # channel indices 0, 17, 36, 37 (adv), 38 (adv), 22 (an odd MHz value)
DATA_STREAMS = (0, 1, 2, 5)
N_WORDS = 1029                                             # two full 512-word tiles and a ragged one


class _Builder:
    def __init__(self, n_streams, n_words, mhz, seed):
        self.rng = np.random.default_rng(seed)
        self.n_words, self.mhz = n_words, mhz
        self.bits = self.rng.integers(0, 2, (n_streams, 64 * n_words + 4096), dtype=np.uint8)   # (the tail: room for what ends past the stream)
        self.used = [[] for _ in range(n_streams)]
        self.planted = []

    def plant(self, stream, offset, aa, crc_init, header0, length, note, payload=None):
        ch = _le.channel_index(int(self.mhz[stream])) & 0x3F
        if payload is None:
            payload = self.rng.integers(0, 256, length, dtype=np.uint8).tobytes()
        sym = _le.tx_bits(aa, ch, bytes([header0, length]) + bytes(payload), crc_init)
        assert len(sym) == 80 + 8 * length and offset >= 0
        for a, b in self.used[stream]:
            assert offset + len(sym) <= a or offset >= b, (note, stream, offset)
        self.used[stream].append((offset, offset + len(sym)))
        self.bits[stream, offset:offset + len(sym)] = sym
        self.planted.append(Plant(stream, offset, aa, crc_init, header0, length, note))

    def words(self, pitch_words):
        rows = [_le.pack(self.bits[s, :64 * self.n_words]) for s in range(len(self.bits))]
        out = self.rng.integers(0, 1 << 63, (len(rows), pitch_words), dtype=np.uint64)         # (what lies behind n_words is noise too)
        for s, r in enumerate(rows):
            out[s, :self.n_words] = r
        return out


@functools.lru_cache(maxsize=None)
def scan_lattice(max_len, tight):
    """The capture of the scan tests: six streams of N_WORDS words of seeded noise with packets at the kernel's seams and at the
    branch points of the six rules.  tight: pitch_words == n_words and search_bits as large as the
    entries allow (the stream less 39 bits); otherwise a larger pitch and search_bits 205 bits inside the stream, with packets at
    search_bits - 1 and at search_bits.  The packet that ends one bit past the stream starts below search_bits in both forms."""
    rng = np.random.default_rng(100 + max_len)
    b = _Builder(6, N_WORDS, LATTICE_MHZ, 1000 + max_len + (7 if tight else 0))
    total = 64 * N_WORDS
    search_bits = total - 39 if tight else total - 64 * 3 - 13
    lengths = [n for n in (0, 1, max_len, max_len + 1) if n < 256]
    inits = (0x555555, 0x000001, 0x800000, 0xABCDEF, 0x123456)
    k = 0

    def nxt():
        nonlocal k
        k += 1
        return good_aa(rng, k & 3), inits[k % len(inits)] ^ (k * 0x010203 & 0xFFFFFF), (1, 2, 3, 0x1D, 0x0A)[k % 5]

    # every bit phase of a word: stream 0, words 3 .. 194 (three words apart); lengths 0 and 1
    for ph in range(64):
        aa, ci, h0 = nxt()
        b.plant(0, 64 * (3 + 3 * ph) + ph, aa, ci, h0, min(ph & 1, max_len), "phase %d" % ph)
    # the seams of lane (words 1|2), wave (127|128) and tile (511|512, 1023|1024): the packet starts d bits in front of the seam
    for s, d, n in ((1, 1, lengths[1 % len(lengths)]), (2, 9, max_len), (5, 33, 0), (0, 45, min(2, max_len))):
        for w in (2, 128, 512, 1024):
            if s == 0 and w in (2, 128):
                continue                                                        # (the phase packets lie there)
            aa, ci, h0 = nxt()
            if 64 * w - d + 80 + 8 * n <= total:
                b.plant(s, 64 * w - d, aa, ci, h0, n, "seam %d - %d" % (w, d))
    # back to back, no bit between them: stream 1 from word 300, one packet of every length
    at = 64 * 300 + 5
    for n in lengths + lengths[:2]:
        aa, ci, h0 = nxt()
        b.plant(1, at, aa, ci, h0, n, "back to back, length %d" % n)
        at += 80 + 8 * n
    # every length once more, well apart: stream 2 from word 600
    at = 64 * 600 + 17
    for n in lengths:
        aa, ci, h0 = nxt()
        b.plant(2, at, aa, ci, h0, n, "length %d" % n)
        at += 80 + 8 * n + 300
    # the stream's end: ending at its last bit (stream 1), one bit past it (stream 5)
    aa, ci, h0 = nxt()
    b.plant(1, total - 80, aa, ci, h0, 0, "ends at the last bit")
    aa, ci, h0 = nxt()
    # (below search_bits in both forms, so that rule 5 alone keeps it out; the loose form needs sixteen octets for that)
    n = 16 if not tight and max_len >= 16 else 0
    b.plant(5, total - 79 - 8 * n, aa, ci, h0, n, "ends one bit past the stream")
    if not tight:
        aa, ci, h0 = nxt()
        b.plant(0, search_bits - 1, aa, ci, h0, 0, "at search_bits - 1")
        aa, ci, h0 = nxt()
        b.plant(1, search_bits, aa, ci, h0, 0, "at search_bits")
    # the header's branch points: LLID 0, each RFU bit; stream 5 from word 200
    at = 64 * 200 + 31
    for h0, note in ((0x00, "LLID 0"), (0x0C, "LLID 0, other bits set"), (0x21, "RFU bit 5"), (0x42, "RFU bit 6"), (0x83, "RFU bit 7"),
                     (0x1F, "every allowed bit")):
        aa, ci, _ = nxt()
        b.plant(5, at, aa, ci, h0, 0, note)
        at += 333
    # access addresses with exactly one offense of each kind, both preamble polarities (the two lowest AA bits in all four combinations)
    for kind, aa in sorted(one_offense_aas().items()):
        _, ci, h0 = nxt()
        b.plant(5, at, aa, ci, h0, 0, "one offense: " + kind)
        at += 333
    for low2 in range(4):
        _, ci, h0 = nxt()
        b.plant(5, at, good_aa(rng, low2), ci, h0, min(1, max_len), "AA low bits %d" % low2)
        at += 333
    # valid packets on the two advertising streams
    for s in (3, 4):
        for w in (10, 511, 900):
            aa, ci, h0 = nxt()
            b.plant(s, 64 * w + 50, aa, ci, h0, 0, "advertising channel")
    pitch = N_WORDS if tight else N_WORDS + 11
    words = b.words(pitch)
    words.flags.writeable = False
    return Capture(words, N_WORDS, pitch, search_bits, np.array(LATTICE_MHZ, np.uint16), tuple(b.planted), max_len)


def plant_expected(cap, p):
    """Whether a planted packet is a candidate by its own making (the model decides what the capture holds; this is what the
    lattice meant to build)."""
    ch = _le.channel_index(int(cap.mhz[p.stream]))
    return (ch < 37 and p.offset < cap.search_bits and p.offset + 80 + 8 * p.length <= 64 * cap.n_words and p.length <= cap.max_len and
            (p.header0 & 3) != 0 and (p.header0 & 0xE0) == 0 and _offenses(p.aa) == 0)


@functools.lru_cache(maxsize=None)
def lattice_model(max_len, tight):
    return tuple(capture_candidates(scan_lattice(max_len, tight), max_len))


# ---- the chain capture -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_capture():
    """Three connections hopping over twelve data-channel streams, empty and non-empty PDUs, in noise."""
    mhz = np.array([2404 + 2 * c for c in (0, 3, 5, 8, 9, 10)] + [2428 + 2 * c for c in (0, 2, 7, 11, 19, 25)], np.uint16)
    n_words = 700
    b = _Builder(12, n_words, mhz, 4242)
    rng = np.random.default_rng(77)
    conns = []
    for c, n_pkts in enumerate((30, 17, 9)):
        aa, ci = good_aa(rng), int(rng.integers(0, 1 << 24))
        for k in range(n_pkts):
            s = int(rng.integers(0, 12)) if c else k % 12                       # (the first connection visits every stream)
            n = 0 if k % 3 == 0 else int(rng.integers(1, 28))
            b.plant(s, 64 * (5 + 22 * k) + 7 * c * 64 + int(rng.integers(0, 64)), aa, ci, (1, 2, 3, 0x0D)[k & 3] if n else 1, n,
                    "connection %d" % c)
        conns.append((aa, ci))
    words = b.words(n_words + 3)
    words.flags.writeable = False
    return Capture(words, n_words, n_words + 3, 64 * n_words - 39, mhz, tuple(b.planted), 27), tuple(conns)
