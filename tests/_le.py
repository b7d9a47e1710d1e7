"""Test-side model of the Bluetooth LE 1M uncoded PHY (Core v5.x Vol 6 Part B 2.1, 3.1.1, 3.2) -- numpy and
bit-serial, written from the spec's register figures, not from the kernels (libbtbb_amd/csrc/le.hip runs both
registers in their reflected software form; here the positions 0..6 and 0..23 are shifted literally).

* whitening_bits / crc24: the two shift registers
* tx_bits: preamble + AA + whitened (PDU || CRC), one 0/1 symbol per bit in air order
* match_all: brute-force sliding 40-bit matcher over every offset
* decode: what btbbx_le_decode_hits_device derives for one hit, as a dict keyed like LE_PKT_DTYPE
* lell_fields: what lell_allocate_and_decode (reference bluetooth_le_packet.c:282-312) derives from bytes + MHz
* Rules: the model's own branch points as options; the default is the model, any other value a deliberately wrong
  decoder (tests/test_le_lattice_model.py shows that the lattice of tests/_le_lattice.py tells each from the right one)
* mhz_of / pack / compare: helpers shared by the GPU test files
"""
import ctypes as C
import functools

import numpy as np

ADV_AA = 0x8E89BED6
ADV_CRC_INIT = 0x555555
MAX_BYTES = 64
CRC_TAPS = (1, 3, 4, 6, 9, 10)          # x^24 + x^10 + x^9 + x^6 + x^4 + x^3 + x + 1: the feedback enters these positions
_CRC_TAP_MASK = sum(1 << t for t in CRC_TAPS)


# ---- registers ---------------------------------------------------------------------------------------------------
def whitening_bits(chan, n):
    """n whitening bits of channel index `chan` (Vol 6 Part B 3.2, figure 3.5): x^7 + x^4 + 1, position 0 preset to 1,
    positions 1..6 to the channel index with its MSB in position 1.  The output is position 6; on each clock position 0
    takes position 6 and position 4 takes position 3 XOR position 6."""
    pos = [1] + [(chan >> (5 - i)) & 1 for i in range(6)]
    out = np.zeros(n, np.uint8)
    for k in range(n):
        o = pos[6]
        out[k] = o
        pos = [o, pos[0], pos[1], pos[2], pos[3] ^ o, pos[4], pos[5]]
    return out


@functools.lru_cache(maxsize=64)
def _whitening_2080(chan):
    w = whitening_bits(chan, 8 * 260)
    w.flags.writeable = False
    return w


def crc24_register(bits, crc_init):
    """The CRC register after the data bits (Vol 6 Part B 3.1.1, figure 3.4): positions 0..23 preset with CRCInit (LSB in
    position 0); per bit the feedback = position 23 XOR the data bit enters position 0 and is XORed into CRC_TAPS."""
    pos = crc_init & 0xFFFFFF                       # bit i = position i
    for b in np.asarray(bits, np.uint8).tolist():
        fb = (pos >> 23) ^ b
        pos = ((pos << 1) & 0xFFFFFF) | fb          # every position moves up by one, the feedback enters position 0
        if fb:
            pos ^= _CRC_TAP_MASK
    return [(pos >> i) & 1 for i in range(24)]


def crc24_tx_bits(bits, crc_init):
    """The 24 CRC bits as transmitted: position 23 first, position 0 last."""
    pos = crc24_register(bits, crc_init)
    return np.array([pos[23 - i] for i in range(24)], np.uint8)


def bits_value(bits):
    """Bits in air order -> integer, first bit in bit 0 (the orientation of btbbx_le_pkt.crc_rx / crc_calc)."""
    return int(sum(int(b) << i for i, b in enumerate(bits)))


def octet_bits(data):
    """Octets -> bits, each octet LSB first."""
    return np.unpackbits(np.frombuffer(bytes(data), np.uint8), bitorder="little")


def bits_octets(bits):
    return np.packbits(np.asarray(bits, np.uint8), bitorder="little").tobytes()


# ---- transmitter ---------------------------------------------------------------------------------------------------
def preamble_bits(aa):
    """Eight alternating bits, the first equal to AA bit 0 (Vol 6 Part B 2.1.1)."""
    first = aa & 1
    return np.array([first ^ (i & 1) for i in range(8)], np.uint8)


def pattern_bits(aa):
    return np.concatenate([preamble_bits(aa), octet_bits(int(aa).to_bytes(4, "little"))])


def tx_bits(aa, chan, pdu, crc_init):
    """Preamble + AA + whitened PDU and CRC.  pdu = header (2 octets) + payload."""
    pdu_b = octet_bits(pdu)
    crc_b = crc24_tx_bits(pdu_b, crc_init)
    body = np.concatenate([pdu_b, crc_b])
    return np.concatenate([pattern_bits(aa), body ^ whitening_bits(chan, len(body))])


def make_pdu(header0, payload):
    payload = bytes(payload)
    assert len(payload) < 256
    return bytes([header0 & 0xFF, len(payload)]) + payload


# ---- channel mapping and the lell fields ----------------------------------------------------------------------------
def c_div(a, b):
    """C integer division (truncates toward zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b > 0) else -q


def channel_index(mhz, wrap=True):
    """le_channel_index of the reference, its integer arithmetic and unsigned-char conversion included (wrap=False: the
    value before that conversion)."""
    m = 0xFF if wrap else -1
    if mhz == 2402:
        return 37
    if mhz < 2426:
        return c_div(mhz - 2404, 2) & m
    if mhz == 2426:
        return 38
    if mhz < 2480:
        return (11 + c_div(mhz - 2428, 2)) & m
    return 39


def channel_k(mhz):
    return c_div(mhz - 2402, 2) & 0xFF


def _max_run(v, n):
    best = run = 1
    for i in range(1, n):
        run = run + 1 if ((v >> i) & 1) == ((v >> (i - 1)) & 1) else 1
        best = max(best, run)
    return best


def omitted_windows():
    """The 38 windows with a run of seven or more equal bits that the reference's case list does not name, as its five
    groups: a run of exactly seven ones at bits 0..6 or 5..11 with anything else in the window, seven ones at 4..10 with
    bit 2 clear, nine zeros at 0..8 unless bits 9..11 are ones, and 0x401."""
    return (frozenset(0x07F | (x << 8) for x in range(1, 16)), frozenset(0xFE0 | x for x in range(1, 16)),
            frozenset(0x7F0 | x for x in range(4)), frozenset(0x200 | (x << 10) for x in range(3)), frozenset([0x401]))


OMITTED_WINDOWS = frozenset().union(*omitted_windows())
assert len(OMITTED_WINDOWS) == 38


def _reference_run_windows():
    """The 12-bit windows the reference counts as an offense: those with a run of seven or more equal bits, minus the
    38 its case list does not name (omitted_windows)."""
    return frozenset(v for v in range(4096) if _max_run(v, 12) >= 7 and v not in OMITTED_WINDOWS)


RUN_WINDOWS = _reference_run_windows()


class Rules:
    """The branch points of the model as options.  Rules() is the model; every other value is a wrong decoder, used only
    to show that a set of test cases tells it from the right one."""

    def __init__(self, **kw):
        self.run_windows = RUN_WINDOWS      # the 12-bit windows that count as an offense
        self.transition_positions = 31      # bit pairs (i, i + 1) the transition count looks at (32: bit 31 against a zero)
        self.data_mask = 0x1F               # `length` on a data channel
        self.adv_mask = 0x3F                # `length` on an advertising channel
        self.truncated_ge = False           # truncated when the packet's end is at (not only behind) the stream's end
        self.read_past_end = False          # bits behind the stream's end come from the words that follow in memory
        self.second_word_above = 56         # an octet at bit phase > this takes its upper bits from the next word
        self.crc_init_mask = True           # CRCInit cut to 24 bits (False: the upper bits stay in a 32-bit reflected register)
        self.uchar_wrap = True              # the channel index goes through the reference's unsigned char
        self.seed_mask = True               # whitening seed = channel index & 0x3f (False: all eight bits enter the register)
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


MODEL = Rules()


def data_offenses(aa, rules=MODEL):
    """aa_data_channel_offenses of the reference (bluetooth_le_packet.c:100-242), from its rules as listed there."""
    bits = [(aa >> i) & 1 for i in range(32)] + [0]
    transitions = sum(bits[i] != bits[i + 1] for i in range(rules.transition_positions))
    n = max(transitions - 24, 0)
    top = bits[26:]
    n += 1 if sum(top[i] != top[i + 1] for i in range(5)) < 2 else 0
    octs = aa.to_bytes(4, "little")
    n += 1 if len(set(octs)) == 1 else 0
    n += 1 if aa == ADV_AA else 0
    n += 1 if bin(aa ^ ADV_AA).count("1") == 1 else 0
    n += sum(1 for s in range(0, 21, 4) if (aa >> s) & 0xFFF in rules.run_windows)
    return n


def lell_fields(bytes64, mhz, rules=MODEL):
    """What lell_allocate_and_decode(bytes64, mhz, 0, &p) leaves in p."""
    b = bytes(bytes64)
    aa = int.from_bytes(b[:4], "little")
    ci = channel_index(mhz, rules.uchar_wrap)
    f = dict(access_address=aa, channel_idx=ci & 0xFF, channel_k=channel_k(mhz), is_data=int(ci < 37))
    if ci < 37:
        off = data_offenses(aa, rules)
        f.update(length=b[5] & rules.data_mask, adv_type=0, adv_tx_add=0, adv_rx_add=0, access_address_offenses=off,
                 access_address_ok=int(off == 0))
    else:
        ok = aa == ADV_AA
        f.update(length=b[5] & rules.adv_mask, adv_type=b[4] & 0xF, adv_tx_add=int(bool(b[4] & 0x40)), adv_rx_add=int(bool(b[4] & 0x80)),
                 access_address_ok=int(ok), access_address_offenses=0 if ok else (1 if bin(aa ^ ADV_AA).count("1") == 1 else 32))
    return f


# ---- receiver model ------------------------------------------------------------------------------------------------
def match_all(words, n_words, search_bits, aa, max_errors):
    """Every offset in [0, search_bits) of one packed stream (LSB-first uint64 words) whose 40 bits are within max_errors
    of preamble + AA -> (offsets, mismatches, received AA) arrays.  Brute force over all offsets."""
    w = np.zeros(n_words + 2, np.uint64)
    w[:n_words] = np.asarray(words[:n_words], np.uint64)
    pat = bits_value(pattern_bits(aa))
    off = np.arange(search_bits, dtype=np.uint64)
    wi = (off >> np.uint64(6)).astype(np.int64)
    sh = off & np.uint64(63)
    lo = w[wi] >> sh
    hi = np.where(sh == 0, np.uint64(0), w[wi + 1] << ((np.uint64(64) - sh) & np.uint64(63)))
    win = (lo | hi) & np.uint64((1 << 40) - 1)
    err = np.bitwise_count(win ^ np.uint64(pat)).astype(np.int64)
    keep = np.nonzero(err <= max_errors)[0]
    return keep.astype(np.uint64), err[keep], ((win[keep] >> np.uint64(8)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def stream_bits(words, n_words, first, n, past_end=False):
    """n bits of a packed stream from bit `first`, zeros past the stream's end (past_end: zeros only past len(words))."""
    out = np.zeros(n, np.uint8)
    end = min(first + n, (len(words) if past_end else n_words) * 64)
    if end > first:
        w0, w1 = first // 64, (end + 63) // 64
        bits = np.unpackbits(np.asarray(words[w0:w1], np.uint64).view(np.uint8), bitorder="little")
        out[:end - first] = bits[first - 64 * w0:end - 64 * w0]
    return out


def _reverse24(x):
    return int("{:024b}".format(x & 0xFFFFFF)[::-1], 2)


_CRC_REFLECTED = _reverse24(_CRC_TAP_MASK | 1)         # 0xda6000


def _crc24_unmasked(pdu_bits, crc_init):
    """Rules(crc_init_mask=False): the reflected register (bit j = position 23 - j, shifted down) held in 32 bits, with
    CRCInit's bits 24..31 left above it: they move down into the register as it shifts."""
    s = _reverse24(crc_init) | (crc_init & 0xFF000000)
    for b in np.asarray(pdu_bits, np.uint8).tolist():
        fb = (s ^ b) & 1
        s >>= 1
        if fb:
            s ^= _CRC_REFLECTED
    return s


def _whitening_unmasked(state, n):
    """Rules(seed_mask=False): the reflected whitening register (bit j = position 6 - j) started from all eight bits of
    channel index | 0x40."""
    out = np.zeros(n, np.uint8)
    for k in range(n):
        o = state & 1
        out[k] = o
        if o:
            state ^= 0x88
        state >>= 1
    return out


def decode(words, n_words, stream, offset, errors, mhz, crc_init, rules=MODEL):
    """The record btbbx_le_decode_hits_device writes for a hit at `offset` (a dict keyed like LE_PKT_DTYPE).  `words` is
    the stream's row; only Rules(read_past_end=True) looks at what it holds behind n_words."""
    ci = channel_index(mhz, rules.uchar_wrap)
    past = rules.read_past_end
    head = stream_bits(words, n_words, offset, 56, past)
    aa = bits_value(head[8:40])
    if rules.seed_mask:
        wh = _whitening_2080(ci & 0x3F)
    else:
        wh = _whitening_unmasked((ci & 0xFF) | 0x40, 8 * 260)

    def body_bits(n_octets):
        raw = stream_bits(words, n_words, offset + 40, 8 * n_octets, past)
        for k in range(n_octets):                   # an octet's upper bits lie in the next word at bit phases above 56
            sh = (offset + 40 + 8 * k) & 63
            if 56 < sh <= rules.second_word_above:
                raw[8 * k + 64 - sh:8 * k + 8] = 0
        return raw ^ wh[:8 * n_octets]

    hdr = body_bits(2)
    L = bits_value(hdr[8:16])
    pdu_n = 2 + L
    body = body_bits(pdu_n + 3)
    pdu_b, crc_b = body[:8 * pdu_n], body[8 * pdu_n:]
    if rules.crc_init_mask:
        crc_calc = bits_value(crc24_tx_bits(pdu_b, crc_init & 0xFFFFFF))
    else:
        crc_calc = _crc24_unmasked(pdu_b, crc_init)
    crc_rx = bits_value(crc_b)
    end = offset + 40 + 8 * (pdu_n + 3)
    truncated = end >= n_words * 64 if rules.truncated_ge else end > n_words * 64
    raw = (int(aa).to_bytes(4, "little") + bits_octets(body))[:MAX_BYTES]
    raw = raw + bytes(MAX_BYTES - len(raw))
    rec = dict(offset=offset, stream=stream, aa_errors=errors, crc_ok=int(not truncated and crc_calc == crc_rx), crc_rx=crc_rx,
               crc_calc=crc_calc, pdu_bytes=pdu_n, truncated=int(truncated), bytes=raw)
    rec.update(lell_fields(raw, mhz, rules))
    return rec


FIELDS = ("offset", "stream", "aa_errors", "crc_ok", "crc_rx", "crc_calc", "pdu_bytes", "truncated", "channel_idx", "channel_k",
          "is_data", "length", "adv_type", "adv_tx_add", "adv_rx_add", "access_address_ok", "access_address_offenses",
          "access_address")


def record_dict(r):
    d = {k: int(r[k]) for k in FIELDS}
    d["bytes"] = bytes(np.asarray(r["bytes"], np.uint8))
    return d


# ---- shared by the GPU test files -------------------------------------------------------------------------------------
ADV_MHZ = (2402, 2426, 2480)


def mhz_of(n_streams):
    """Stream s: channels 37 / 38 / 39 first, then the data channels' MHz."""
    data = [m for m in range(2404, 2480, 2) if m != 2426]
    return np.array([(list(ADV_MHZ) + data)[s % 40] for s in range(n_streams)], np.uint16)


def pack(sym):
    sym = np.asarray(sym, np.uint8)
    pad = (-len(sym)) % 64
    return np.packbits(np.concatenate([sym, np.zeros(pad, np.uint8)]), bitorder="little").view(np.uint64)


def compare(got, want, phys, ref=None):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        gd = record_dict(g)
        assert gd == w, (gd, w)
        if ref is not None:
            rf = ref_lell_fields(ref, gd["bytes"], int(phys[gd["stream"]]))
            assert {k: gd[k] for k in rf} == rf


# ---- the compiled reference ------------------------------------------------------------------------------------------
class LellPacket(C.Structure):
    """struct lell_packet (reference bluetooth_le_packet.h:44-72)."""
    _fields_ = [("symbols", C.c_uint8 * 64), ("access_address", C.c_uint32), ("channel_idx", C.c_uint8),
                ("channel_k", C.c_uint8), ("length", C.c_int), ("clk100ns", C.c_uint32), ("adv_type", C.c_uint8),
                ("adv_tx_add", C.c_int), ("adv_rx_add", C.c_int), ("access_address_offenses", C.c_uint),
                ("refcount", C.c_uint32), ("flags", C.c_uint32)]


def ref_lell_fields(ref, bytes64, mhz):
    """lell_allocate_and_decode of the compiled reference (oracle/_ref/libbtbb_ref.so)."""
    fn = ref.lell_allocate_and_decode
    fn.restype, fn.argtypes = None, [C.c_char_p, C.c_uint16, C.c_uint32, C.POINTER(C.POINTER(LellPacket))]
    p = C.POINTER(LellPacket)()
    buf = bytes(bytes64)[:64].ljust(64, b"\0")
    fn(buf, mhz, 0, C.byref(p))
    s = p.contents
    f = dict(access_address=s.access_address, channel_idx=s.channel_idx, channel_k=s.channel_k, is_data=int(s.channel_idx < 37),
             length=s.length, adv_type=s.adv_type, adv_tx_add=s.adv_tx_add, adv_rx_add=s.adv_rx_add,
             access_address_ok=s.flags & 1, access_address_offenses=s.access_address_offenses)
    unref = ref.lell_packet_unref
    unref.restype, unref.argtypes = None, [C.c_void_p]
    unref(C.cast(p, C.c_void_p))
    return f
