"""One far capture for every stream-taking entry (no test in here): two streams of a little more than 2^29 words that are zero
except for copies of a short capture S, so that every offset an entry reports, cuts at or clocks needs bit 32 of a bit offset
(copy B, straddling word 2^26) or of a byte offset (copy C, straddling word 2^29 and ending the stream).

The expectation rests on translation: a scan, cut, decode or candidate rule depends only on the bits in and behind its window,
and all-zero words are quiet (tests/test_far_model.py asserts both on the CPU).  So the far result is the model's result on a
short stream moved by 64 * base:

* R_in  = 64 zero words, S, 64 zero words -- a copy inside the stream;
* R_end = 64 zero words, S               -- the copy that ends the stream (captured lengths, rule 5 of the LE candidate and
  the ragged last tile differ there).

S (stream 0 / stream 1; different content, so a stream mix-up shows):
  (a) the seam stream of test_gpu_scan.py -- noise with sync words of 0..2 errors, random LAPs and both barker classes;
  (b) packets of tests/_trial_lattice.py laid end to end up to S's end: every type at full length, the last ones cut by the
      end of S in the copy that ends the stream;
  (c) stream 1: tests/_survey.py capture_single's stream (625-symbol slots), above byte 2^32 as a whole in the last copy;
  (d) stream 0 (a data channel): LE data-channel packets -- lengths 0, 5, 27, 255, sixteen bit phases, two connections;
  (e) stream 1 (2402 MHz): advertising packets with 0..2 errors over preamble + access address.
At the words where the boundaries fall (CROSS), S holds what must cross them; S's last bits hold an LE packet that ends on the
last bit, with a sync word in the last 64 searchable offsets inside its payload, and in front of it the head of an LE packet
that would end one bit past.

Placement: the far copies start at multiples of 625 words -- a whole number of 625-symbol slots AND of words, which the
survey's clock needs; the near copy A starts at word 64, where R_in has it.  Copies lie at least 64 zero words apart.
"""
import collections
import functools

import numpy as np

import _le
import _le_discover as ld
import _libs
import _seams
import _survey
import _trial_lattice as tl
from libbtbb_amd import synth

PAD = 64                                   # zero words around S in the short references
BIT32_WORD = 1 << 26                       # bit 2^32 = word 2^26
BYTE32_WORD = 1 << 29                      # bit 2^35 = byte 2^32 = word 2^29
SLOT = 625
KNOWN_LAPS = (0x9E8B33, 0x1E8B33)
MHZ = (2440, 2402)                         # stream 0: data channel index 17; stream 1: advertising channel 37
LE_SCAN_ERRORS = 2
SEAM_WORDS = _seams.N_WORDS
# the word of S on which each far copy's boundary falls: (stream, boundary) -> word.  2^26 = 114 and 2^29 = 287 (mod 625).
CROSS = {(0, "bit32"): 3239, (0, "byte32"): 2787, (1, "bit32"): 4489, (1, "byte32"): 912}
assert all((BIT32_WORD - CROSS[s, "bit32"]) % SLOT == 0 and (BYTE32_WORD - CROSS[s, "byte32"]) % SLOT == 0 for s in (0, 1))

Plant = collections.namedtuple("Plant", "kind offset length meta")      # offsets in bits of S
Copy = collections.namedtuple("Copy", "name stream base ends")         # base in words; ends: S ends the stream there


class _Builder:
    def __init__(self, seed, n_bits):
        self.rng = np.random.default_rng(seed)
        self.bits = np.ascontiguousarray(synth.unpack_bits(synth.noise_words(seed, 0, (n_bits + 63) // 64))[:n_bits])
        self.used, self.plants = [], []

    def free(self, off, n):
        return off >= 0 and off + n <= len(self.bits) and all(off + n <= a or off >= b for a, b in self.used)

    def plant(self, kind, off, sym, meta=None, n_used=None):
        sym = np.asarray(sym, np.uint8)
        n = len(sym) if n_used is None else n_used
        assert self.free(off, n), (kind, off, n)
        self.used.append((off, off + n))
        self.bits[off:off + len(sym)] = sym[:max(0, len(self.bits) - off)]
        self.plants.append(Plant(kind, off, len(sym), meta))

    def sync(self, off, k, kind="sync", must=True, errors=None):
        """A sync word with (k // 3) % 3 errors below the barker bits; the LAP cycles through random and both barker classes."""
        if not self.free(off, 64):
            assert not must, (kind, off)
            return False
        lap = (int(self.rng.integers(0, 1 << 24)),) + KNOWN_LAPS
        sw = synth.syncword(lap[k % 3])
        for e in self.rng.choice(57, size=(k // 3) % 3 if errors is None else errors, replace=False):
            sw ^= 1 << int(e)
        self.plant(kind, off, synth.bits_lsb(sw, 64), lap[k % 3])
        return True


def _seam(b, first_word):
    """(a): sync words at the offsets right before, on and behind the seams of what the scan kernels hand out (a lane's run, a
    4096-offset segment, a wave's 63 / 128 words, tiles of 512 / 756 words), as the seam test of test_gpu_scan.py plants them."""
    deltas = _seams.DELTAS
    # the seam test's own bounds, and more of them: S is longer than that test's streams and other plants take some places
    bounds = tuple(sorted(_seams.BOUNDS + (300, 400, 600, 700, 900, 1100, 1300, 1700, 1900, 2048, 2268, 2400)))
    assert bounds == (1, 2, 63, 64, 126, 128, 189, 256, 300, 400, 512, 600, 700, 756, 900, 1024, 1100, 1300, 1512, 1700, 1900, 2048, 2268, 2400)
    n = 0
    for j, w in enumerate(bounds):
        for r in range(2):                              # two deltas per seam, far enough apart
            n += b.sync(64 * (first_word + w) + deltas[(5 * j + 7 * r) % len(deltas)] + 200 * r, j + r, must=False)
    assert n >= 40
    for j, errors in enumerate((3, 4, 5, 3, 4, 5)):      # ... and what only tables for more errors find
        b.sync(64 * (first_word + 1350 + 20 * j) + 11 * j, j, kind="sync%d" % errors, must=False, errors=errors)
    for k in range(3):                                   # ... and pairs 80 bits apart: a search that ends between them cuts a word in two
        at = 64 * (first_word + 2150 + 10 * k) + 13
        b.sync(at, k, kind="sync_pair")
        b.sync(at + 80, k + 3, kind="sync_pair")
    return n


def _le_packet(aa, ch, crc_init, header0, length, rng, embed=None):
    """Air bits of one LE packet; embed = (bit of the packet, 64 air bits to appear there, inside the payload)."""
    air = rng.integers(0, 2, 8 * length, dtype=np.uint8)
    if embed is not None:
        at, sw = embed
        assert 56 <= at and at + 64 <= 56 + 8 * length
        air[at - 56:at - 56 + 64] = sw
    payload = _le.bits_octets(air ^ _le.whitening_bits(ch, 16 + 8 * length)[16:])
    sym = _le.tx_bits(aa, ch, bytes([header0, length]) + payload, crc_init)
    assert len(sym) == 80 + 8 * length and (embed is None or np.array_equal(sym[embed[0]:embed[0] + 64], embed[1]))
    return sym


def _le_tail(b, aa, ch, crc_init, header0):
    """S's last bits: P1 (length 27) ends on the last bit and carries a sync word at the last-but-63 searchable offset in its
    payload; the head of P2 (length 37) lies 79 bits in front of it, so P2 would end one bit past S."""
    total = len(b.bits)
    sw = synth.bits_lsb(synth.syncword(KNOWN_LAPS[0]), 64)
    o1 = total - 80 - 8 * 27
    p1 = _le_packet(aa, ch, crc_init, header0, 27, b.rng, embed=(total - 127 - o1, sw))
    p2 = _le_packet(aa, ch, crc_init ^ 0x0F0F0F, header0, 37, b.rng)
    o2 = o1 - 79
    assert o2 + 80 + 8 * 37 == total + 1
    b.plant("le_past", o2, p2[:79], dict(aa=aa, length=37))
    b.plant("le_last", o1, p1, dict(aa=aa, crc_init=crc_init, length=27, sync=total - 127))
    return o2


def _lattice_pick():
    """(b): per type the whitened full-length packet with the longest body, DH5 first (it crosses a boundary); then cut ones."""
    lat = tl.lattice()
    best = {}
    for i, (name, what, n) in enumerate(lat.tags):
        if what == "full" and lat.air_white[i] and int(lat.pin["flags"][i]) & 1 and n >= best.get(name, (-1, 0))[0]:
            best[name] = (n, i)
    assert len(best) == 17, sorted(best)              # sixteen types, type 7 as HV3 and as EV3
    order = ["DH5"] + sorted(k for k in best if k != "DH5")
    idx = [best[k][1] for k in order]
    idx += [i for i, t in enumerate(lat.tags) if t[1].startswith(("end-1", "bitlen-1")) and t[0] in ("DM3", "DH3", "EV5") and t[2] in (7, 60)][:6]
    return lat, idx


def _lay_lattice(b, lat, idx, end):
    """The packets end to end with gaps of 0..47 noise bits, the last one ending at bit `end`."""
    gaps = [int(b.rng.integers(0, 48)) for _ in idx]
    at = end - sum(len(lat.syms[i]) + g for i, g in zip(idx, gaps)) + gaps[-1]
    first = at
    for i, g in zip(idx, gaps):
        b.plant("br", at, lat.syms[i], i)
        at += len(lat.syms[i]) + g
    return first


@functools.lru_cache(maxsize=None)
def short():
    """(S0, S1) as _Builder objects: .bits, .plants."""
    lat, idx = _lattice_pick()
    dh5, rest = idx[0], idx[1:]
    assert lat.tags[dh5][0] == "DH5" and len(lat.syms[dh5]) >= 1000
    lat_bits = sum(len(lat.syms[i]) + 48 for i in rest)

    # ---- stream 1: seam | survey | advertising | lattice | tail ----
    cap, _ = _survey.capture_single()
    slots = sorted(sl for st, sl in cap.used)
    want = 64 * CROSS[1, "bit32"] - 17                   # a survey packet begins 17 bits below bit 2^32
    k = max(sl for sl in slots if want - SLOT * sl >= 64 * (SEAM_WORDS + 3))
    q0 = want - SLOT * k
    seam1 = 0
    adv1 = (q0 + len(cap.sym[0]) + 63) // 64 + 3
    n1 = 64 * (adv1 + 160) + lat_bits + 512
    n1 = (n1 + 63) // 64 * 64
    b1 = _Builder(_libs.seed(7001), n1)
    b1.plant("survey", q0, cap.sym[0], dict(slots=slots, cross=k))
    assert seam1 < CROSS[1, "byte32"] < seam1 + SEAM_WORDS
    b1.sync(64 * CROSS[1, "byte32"], 3, kind="sync_on")              # begins exactly on bit 2^35
    _seam(b1, seam1)
    for j in range(8):                                               # (e)
        sym = _le.tx_bits(_le.ADV_AA, 37, _le.make_pdu((0x40, 0x02, 0xC6, 0x00)[j & 3], b1.rng.integers(0, 256, (6, 37, 12, 31)[j & 3], dtype=np.uint8).tobytes()),
                          _le.ADV_CRC_INIT).copy()
        for e in b1.rng.choice(40, size=j % 3, replace=False):
            sym[int(e)] ^= 1
        b1.plant("le_adv", 64 * (adv1 + 18 * j) + 9 * j + 1, sym, dict(errors=j % 3))
    tail1 = _le_tail(b1, _le.ADV_AA, 37, _le.ADV_CRC_INIT, 0x02)
    _lay_lattice(b1, lat, rest[::-1], tail1 - 11)

    # ---- stream 0: seam | DH5 across bit 2^35 | LE | noise | lattice | tail ----
    n0 = n1 + 64 * (CROSS[0, "byte32"] - CROSS[1, "byte32"])         # both C copies end the stream
    b0 = _Builder(_libs.seed(7000), n0)
    rng = np.random.default_rng(_libs.seed(7002))
    conns = [(ld.good_aa(rng), int(rng.integers(0, 1 << 24))) for _ in range(2)]
    b0.plant("br", 64 * CROSS[0, "byte32"] - 5, lat.syms[dh5], dh5)
    x = 64 * CROSS[0, "bit32"]
    sw = synth.bits_lsb(synth.syncword(0x2C7F91), 64)
    b0.plant("le", x - 1000, _le_packet(conns[0][0], 17, conns[0][1], 0x0E, 255, b0.rng, embed=(1001, sw)),
             dict(conn=0, length=255, sync=x + 1))                    # a sync word just behind bit 2^32, in its payload
    for j in range(18):                                              # (d)
        c = j & 1
        length = (0, 27, 5, 255, 0, 27)[j % 6]
        b0.plant("le", 64 * (2850 + (40 * j if j < 9 else 40 * j + 100)) + (4 * j + 1) % 64,
                 _le_packet(conns[c][0], 17, conns[c][1], (1, 2, 3, 0x0D, 0x1E)[j % 5] if length else 1, length, b0.rng), dict(conn=c, length=length))
    _seam(b0, 0)
    tail0 = _le_tail(b0, conns[1][0], 17, conns[1][1], 0x06)
    first = _lay_lattice(b0, lat, rest, tail0 - 7)
    assert first > 64 * (2850 + 40 * 17 + 100 + 40)
    for b in (b0, b1):
        b.bits.flags.writeable = False
    return b0, b1


Far = collections.namedtuple("Far", "S words R_in R_end copies n_words pitch_words plants lat")


@functools.lru_cache(maxsize=None)
def far():
    b0, b1 = short()
    S = tuple(np.ascontiguousarray(b.bits) for b in (b0, b1))
    words = tuple(synth.pack_bits(s) for s in S)
    W = [len(w) for w in words]
    zeros = np.zeros(PAD, np.uint64)
    copies = (Copy("A0", 0, 64, False), Copy("B0", 0, BIT32_WORD - CROSS[0, "bit32"], False),
              Copy("C0", 0, BYTE32_WORD - CROSS[0, "byte32"], True),
              Copy("B1", 1, BIT32_WORD - CROSS[1, "bit32"], False), Copy("C1", 1, BYTE32_WORD - CROSS[1, "byte32"], True))
    n_words = copies[2].base + W[0]
    assert n_words == copies[4].base + W[1] and BYTE32_WORD < n_words < BYTE32_WORD + (1 << 13)
    lat = tl.lattice()
    return Far(S, words, tuple(np.concatenate([zeros, w, zeros]) for w in words), tuple(np.concatenate([zeros, w]) for w in words),
               copies, n_words, n_words + 37, (tuple(b0.plants), tuple(b1.plants)), lat)


def copies_of(stream):
    return [c for c in far().copies if c.stream == stream]


def ref_words(stream, ends):
    f = far()
    return (f.R_end if ends else f.R_in)[stream]


def ref_sym(stream, ends):
    return np.ascontiguousarray(synth.unpack_bits(ref_words(stream, ends)))


def moved(offset_in_ref, copy):
    """An offset of R_in / R_end as the offset of that copy in the far stream."""
    return offset_in_ref - 64 * PAD + 64 * copy.base


def union(model, streams=(0, 1)):
    """model(stream, ends) -> tuples that begin with an offset of the short reference.  The far expectation: (stream, moved
    offset, rest...) over every copy, in (stream, offset) order."""
    out = []
    for s in streams:
        res = {ends: model(s, ends) for ends in (False, True)}
        for c in copies_of(s):
            out += [(s, moved(t[0], c)) + tuple(t[1:]) for t in res[c.ends]]
    return sorted(out)


# ---- the models on the short references ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def find_all(stream, ends, lap, max_err):
    """The oracle port's (offset, lap, errors) over every searchable offset of the short reference."""
    sym = ref_sym(stream, ends)
    return tuple(_libs.orc_find_all(sym, len(sym) - 63, _libs.LAP_ANY if lap == synth.LAP_ANY else lap, max_err))


def br_hits(stream):
    """(b): (offset in S, lattice index) of the packets laid into S, in offset order."""
    return sorted((p.offset, p.meta) for p in far().plants[stream] if p.kind == "br")


def br_slice(stream, ends, ref_offset, max_length=synth.MAX_SYMBOLS):
    """What btbbx_gather_packets_device cuts out at an offset of the short reference."""
    sym = ref_sym(stream, ends)
    return np.ascontiguousarray(sym[ref_offset:ref_offset + min(max_length, synth.MAX_SYMBOLS, max(len(sym) - ref_offset, 0))])


@functools.lru_cache(maxsize=None)
def le_matches(stream, ends):
    w = ref_words(stream, ends)
    off, err, aa = _le.match_all(w, len(w), 64 * len(w) - 39, _le.ADV_AA, LE_SCAN_ERRORS)
    return tuple((int(o), int(a), int(e)) for o, e, a in zip(off, err, aa))


@functools.lru_cache(maxsize=None)
def le_candidates(stream, ends, max_len):
    w = ref_words(stream, ends)
    return tuple(ld.candidates(w, len(w), 64 * len(w) - 39, MHZ[stream], max_len, stream))


def far_candidates(max_len):
    """Cand tuples of the far capture, every offset moved."""
    out = []
    for s in (0, 1):
        for c in copies_of(s):
            out += [k._replace(offset=moved(k.offset, c)) for k in le_candidates(s, c.ends, max_len)]
    return out


def survey_plant():
    p = [p for p in far().plants[1] if p.kind == "survey"]
    assert len(p) == 1
    return p[0]


def survey_clock(base):
    """(entry clock, clk_phase) with which the survey packets of S1 at `base` words carry the clocks they were built with:
    capture_single's first slot has the clock 77, and it begins at bit 64 * base + the plant's offset of the stream."""
    start = 64 * base + survey_plant().offset
    phase = (-start) % SLOT
    return (77 - (start + phase) // SLOT) & 0xFFFFFFFF, phase


# ---- the crossing conditions -------------------------------------------------------------------------------------------
def boundary_bit(copy, which):
    """The bit of S (may lie outside it) on which bit 2^32 / bit 2^35 of the far stream falls in that copy."""
    return 64 * ({"bit32": BIT32_WORD, "byte32": BYTE32_WORD}[which] - copy.base)


def crossings():
    """name -> True / False for every crossing condition, from the placement table and the hits the oracle finds."""
    f = far()
    far_copies = [c for c in f.copies if c.name != "A0"]
    lap_any = {c.name: [o - 64 * PAD for o, _, _ in find_all(c.stream, c.ends, synth.LAP_ANY, 2)] for c in far_copies}
    bounds = [(c, w, boundary_bit(c, w)) for c in far_copies for w in ("bit32", "byte32") if 0 < boundary_bit(c, w) < len(f.S[c.stream])]
    out = {}
    for w in ("bit32", "byte32"):
        out["sync begins in the 64 bits below " + w] = any(x - 64 <= o < x for c, ww, x in bounds if ww == w for o in lap_any[c.name])
    out["sync begins on a boundary"] = any(o == x for c, _, x in bounds for o in lap_any[c.name])
    out["sync begins just behind a boundary"] = any(o == x + 1 for c, _, x in bounds for o in lap_any[c.name])

    def spans(c, x, kinds, ok):
        return any(p.kind in kinds and p.offset < x < p.offset + p.length and ok(p) for p in f.plants[c.stream])
    out["BR data packet of >= 1000 symbols across a boundary"] = any(
        spans(c, x, ("br",), lambda p: p.length >= 1000 and f.lat.tags[p.meta][0] in ("DH5", "DM5", "DH3", "DM3")) for c, _, x in bounds)
    out["LE packet of length >= 27 across a boundary"] = any(spans(c, x, ("le",), lambda p: p.meta["length"] >= 27) for c, _, x in bounds)
    sp = survey_plant()
    out["survey packet across a boundary"] = any(c.stream == 1 and any(sp.offset + SLOT * sl < x < sp.offset + SLOT * sl + 68 for sl in sp.meta["slots"])
                                                 for c, _, x in bounds)
    for c in far_copies:
        if c.ends:
            total = len(f.S[c.stream])
            out[c.name + ": sync in the last 64 searchable offsets"] = any(total - 63 - 64 <= o < total - 63 for o in lap_any[c.name])
            out[c.name + ": LE packet ends on the last bit"] = any(p.kind == "le_last" and p.offset + p.length == total for p in f.plants[c.stream])
            out[c.name + ": LE packet would end one bit past"] = any(p.kind == "le_past" and p.offset + 80 + 8 * p.meta["length"] == total + 1
                                                                     for p in f.plants[c.stream])
    return out
