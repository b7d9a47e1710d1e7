"""Test-side model of the promiscuous LE Coded connection discovery (include/btbbx.h btbbx_le_cfind_*, rules 1..12; DESIGN
3.8.12), written from the twelve rules with the air format, encoder and decoders of tests/_le_coded.py, the registers of
tests/_le.py and the backward CRC and grouping of tests/_le_discover.py -- not from the kernels.

* StreamModel: one packed stream.  Block 1 at many offsets at once (branch metrics from a table of 4-symbol distances, one numpy
  step per trellis step), rule 4's count against the re-encoded decoded address, block 2 by _le_coded's _forward_many / _trace_many
* candidates: the twelve rules -> [(Cand, Info)] in offset order.  It skips offsets whose 80 preamble symbols alone mismatch in
  more than max_errors places (a lower bound of rule 4's count); every_offset=True decodes every offset with _le_coded's own
  decoder and compares literally with pattern_symbols(AA') -- tests/test_le_cfind_model.py shows that the two agree
* second_condition: the scan kernel's address-free bound, as DESIGN states it
* Rules: the model's branch points as options; Rules() is the model, VARIANTS are deliberately wrong ones
* lattice / chain_capture: the captures the CPU and GPU tests share
"""
import collections
import functools

import numpy as np

import _le
import _le_coded as c
import _le_discover as d

Cand = d.Cand
Info = collections.namedtuple("Info", "symbols metric2 metric1 errors ci s")
F = c.FORMAT
BLOCK2 = F["block2"]
LAG_STEP = 16 + c.LAG


class Rules:
    def __init__(self, **kw):
        self.given_aa = None             # rule 4 counted against this address instead of the decoded one
        self.match_symbols = c.PATTERN   # rule 4 over fewer symbols
        self.match_strict = False        # rule 4 with <
        self.max_offenses = 0
        self.rfu_ci = False              # an RFU ci accepted (as S = 8)
        self.s_swapped = False           # ci 0 -> 2, ci 1 -> 8
        self.header_final = False        # the header tests and the record's header from the final path, nothing compared
        self.ignore_moved = False        # header_moved not looked at
        self.fit_slack = 0               # rule 8 lets a packet end this many symbols past the stream
        self.len_strict = False          # h1 < max_len
        self.crc_octets_short = 0        # the CRC walked over 2 + L - this octets
        self.adv_accepted = False        # rule 1 absent
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


MODEL = Rules()
VARIANTS = dict(given_aa=None, match_320=dict(match_symbols=320), match_strict=dict(match_strict=True), one_offense=dict(max_offenses=1),
                rfu_ci=dict(rfu_ci=True), s_swapped=dict(s_swapped=True), header_final=dict(header_final=True),
                ignore_moved=dict(ignore_moved=True), fit_permissive=dict(fit_slack=1), len_strict=dict(len_strict=True),
                crc_octets_short=dict(crc_octets_short=1), adv_accepted=dict(adv_accepted=True))


@functools.lru_cache(maxsize=None)
def _offenses(aa):
    return _le.data_offenses(aa)


def _encode_many(bits):
    """c.encode for many messages at once: (n, k) input bits -> (n, k, 2) coded bits a0, a1, encoder from state 0."""
    n, k = bits.shape
    taps = np.zeros((4, n, k), np.uint8)
    for j in range(4):
        taps[j, :, j:] = bits[:, :k - j]
    out = np.zeros((n, k, 2), np.uint8)
    for which, g in enumerate((F["g0"], F["g1"])):
        for j in range(4):
            if g[j]:
                out[:, :, which] ^= taps[j]
    return out


class StreamModel:
    """One stream: what the rules read of it, computed once and kept."""

    def __init__(self, words, n_words, mhz, stream=0):
        self.n_words, self.total, self.mhz, self.stream = n_words, 64 * n_words, int(mhz), stream
        self.ch = _le.channel_index(int(mhz))
        self.words = np.asarray(words[:n_words], np.uint64)
        sym = np.unpackbits(self.words.view(np.uint8), bitorder="little")
        self.sym = np.concatenate([sym, np.zeros(BLOCK2 + 8 * 2100, np.uint8)])       # symbols past the stream's end read as 0
        self.wh = _le.whitening_bits(self.ch & 0x3F, 8 * 260)
        n = self.total
        pre = np.array(F["preamble"], np.uint8)
        self.pre_mis = np.zeros(n, np.int32)
        for k in range(80):
            self.pre_mis += self.sym[k:k + n] != pre[k]
        # d4[p, v] = the distance of the four symbols from p to the mapped coded bit v
        m = len(self.sym) - 4
        self.d4 = np.zeros((m, 2), np.int32)
        for v in (0, 1):
            for k in range(4):
                self.d4[:, v] += self.sym[k:k + m] != F["map8"][v][k]
        self._b1 = {}
        self._b2 = {}

    # ---- rule 3, and rule 4's count against the decoded address ----
    def block1(self, offsets):
        """offsets -> dict offset -> (AA', ci, metric1, errors); computed for those not yet known"""
        todo = np.array(sorted(set(int(o) for o in offsets) - set(self._b1)), np.int64)
        if len(todo):
            n = len(todo)
            metrics = np.full((n, 8), c.INF, np.int64)
            metrics[:, 0] = 0
            dec = np.zeros((37, n, 8), np.uint8)
            expect = [[c.branch((nxt >> 1) | (x << 2), nxt & 1, 2) for x in (0, 1)] for nxt in range(8)]      # the coded bits a0, a1
            for t in range(37):
                pos = todo + 80 + 8 * t
                new = np.empty_like(metrics)
                first, second = self.d4[pos], self.d4[pos + 4]
                bm = {(a0, a1): first[:, a0] + second[:, a1] for a0 in (0, 1) for a1 in (0, 1)}
                for nxt in range(8):
                    sums = []
                    for x in (0, 1):
                        sums.append(metrics[:, (nxt >> 1) | (x << 2)] + bm[tuple(expect[nxt][x])])
                    x1 = sums[1] < sums[0]                                              # x = 0 survives on equal sums
                    new[:, nxt] = np.minimum(np.where(x1, sums[1], sums[0]), c.INF + 100000)
                    dec[t, :, nxt] = x1
                metrics = new
            bits = c._trace_many(dec, np.full(n, 37), np.zeros(n, np.int64))
            coded = _encode_many(bits[:, :32])
            err = self.pre_mis[todo].astype(np.int64)
            err320 = err.copy()
            for i in range(32):
                e = self.d4[todo + 80 + 8 * i, coded[:, i, 0]] + self.d4[todo + 84 + 8 * i, coded[:, i, 1]]
                err += e
                if i < 30:
                    err320 += e
            for j, o in enumerate(todo.tolist()):
                self._b1[o] = (_le.bits_value(bits[j, :32]), int(bits[j, 32]) + 2 * int(bits[j, 33]), int(metrics[j, 0]), int(err[j]), int(err320[j]))
        return self._b1

    def block1_literal(self, offsets):
        """The same by _le_coded's decoder and a literal comparison with pattern_symbols(AA')."""
        offsets = np.asarray(offsets, np.int64)
        n = len(offsets)
        m1, d1, _ = c._forward_many(self.sym, offsets + 80, 8, np.full(n, 37))
        bits = c._trace_many(d1, np.full(n, 37), np.zeros(n, np.int64))
        out = {}
        for j, o in enumerate(offsets.tolist()):
            aa = _le.bits_value(bits[j, :32])
            diff = self.sym[o:o + c.PATTERN] != c.pattern_symbols(aa)
            out[o] = (aa, int(bits[j, 32]) + 2 * int(bits[j, 33]), int(m1[j, 0]), int(diff.sum()), int(diff[:320].sum()))
        return out

    # ---- rules 7 and 9: block 2 ----
    def block2(self, pairs):
        """(offset, S) pairs -> dict (offset, S) -> (lag header bits, metric2, final path bits, N)"""
        todo = sorted(set(pairs) - set(self._b2))
        for s in (8, 2):
            offs = np.array([o for o, ss in todo if ss == s], np.int64)
            if not len(offs):
                continue
            n = len(offs)
            base = offs + BLOCK2
            lag_steps = np.full(n, LAG_STEP)
            mlag, dlag, _ = c._forward_many(self.sym, base, s, lag_steps)
            best = np.array([min(range(8), key=lambda q: (mlag[i, q], q)) for i in range(n)])
            lag_header = c._trace_many(dlag, lag_steps, best)[:, :16]
            ls = np.array([_le.bits_value(h[8:16] ^ self.wh[8:16]) for h in lag_header])
            steps = 8 * (ls + 5) + 3
            m2, d2, _ = c._forward_many(self.sym, base, s, steps)
            paths = c._trace_many(d2, steps, np.zeros(n, np.int64))
            for j, o in enumerate(offs.tolist()):
                self._b2[(o, s)] = (lag_header[j].copy(), int(m2[j, 0]), paths[j, :int(steps[j]) - 3].copy(), int(steps[j]))
        return self._b2


def candidates(sm, search_bits, max_len, max_errors, rules=MODEL, every_offset=False):
    """The candidates of one stream (a StreamModel) as [(Cand, Info)] in offset order."""
    if sm.ch >= 37 and not rules.adv_accepted:                                          # rule 1
        return []
    n = min(search_bits, sm.total - c.PATTERN + 1)                                      # rule 2 (and its argument check)
    if every_offset:
        offs = np.arange(n)
        b1 = sm.block1_literal(offs)
    else:
        offs = np.nonzero(sm.pre_mis[:n] <= max_errors)[0]                              # (the preamble's mismatches bound rule 4's count from below)
        b1 = sm.block1(offs)                                                            # rule 3
    given = None
    if rules.given_aa is not None:
        given = c.mismatch_counts(sm.sym, rules.given_aa, n)
    keep = []
    for o in offs.tolist():
        aa, ci, metric1, err, err320 = b1[o]
        e = int(given[o]) if given is not None else (err if rules.match_symbols == c.PATTERN else err320)
        if e >= max_errors if rules.match_strict else e > max_errors:                   # rule 4
            continue
        if _offenses(aa) > rules.max_offenses:                                          # rule 5
            continue
        s = F["s_of_ci"].get(ci, 8 if rules.rfu_ci else 0)                              # rule 6
        if rules.s_swapped and s:
            s = 10 - s
        if s == 0:
            continue
        keep.append((o, s, aa, ci, metric1, err))
    b2 = sm.block2([(o, s) for o, s, *_ in keep])
    out = []
    for o, s, aa, ci, metric1, err in keep:
        lag_header, metric2, path, n_steps = b2[(o, s)]
        final_header = path[:16]
        moved = bool((final_header != lag_header).any())
        hdr = (final_header if rules.header_final else lag_header) ^ sm.wh[:16]          # rule 7
        h0, h1 = _le.bits_value(hdr[:8]), _le.bits_value(hdr[8:])
        if (h0 & 3) == 0 or (h0 & 0xE0):
            continue
        if h1 >= max_len if rules.len_strict else h1 > max_len:
            continue
        if o + BLOCK2 + s * n_steps > sm.total + rules.fit_slack:                       # rule 8 (N is the lag decision's, whatever the variant)
            continue
        if moved and not (rules.ignore_moved or rules.header_final):                    # rule 9
            continue
        body = path ^ sm.wh[:len(path)]
        n_pdu = len(path) - 24 - 8 * rules.crc_octets_short                             # rule 10
        init = d.crc24_backward(body[:n_pdu], body[n_pdu:n_pdu + 24])
        out.append((Cand(o, aa, init, sm.stream, h0, h1, sm.ch), Info(BLOCK2 + s * n_steps, metric2, metric1, err, ci, s)))
    return out


def pre_records(sm, search_bits, max_errors):
    """What the scan kernel leaves for the decoder, as DESIGN 3.8.12 states it: the offsets that pass the pre-filter (equal pairs
    among the 160 pairs of window symbols 0 .. 319 <= max_errors) and the second condition, with the second condition's bound."""
    if sm.ch >= 37:
        return []
    n = min(search_bits, sm.total - c.PATTERN + 1)
    eq = (sm.sym[:-2] == sm.sym[2:]).astype(np.int32)
    group = eq[:-1] + eq[1:]                                                            # the two pairs of the group of four that starts here
    first = np.zeros(n, np.int32)
    bound = sm.pre_mis[:n].copy()
    for g in range(84):
        if g < 80:
            first += group[4 * g:4 * g + n]
        if g >= 20:
            bound += group[4 * g:4 * g + n]
    keep = np.nonzero((first <= max_errors) & (bound <= max_errors))[0]
    return [(int(o), int(bound[o])) for o in keep]


def second_condition(sym, o):
    """The scan kernel's bound at offset o: the preamble's exact mismatches plus the equal pairs (k, k + 2), k mod 4 in {0, 1}, among
    the 64 groups of four of window symbols 80 .. 335."""
    w = np.asarray(sym[o:o + c.PATTERN], np.int64)
    bound = int((w[:80] != np.array(F["preamble"])).sum())
    for k in range(80, c.PATTERN):
        if k % 4 < 2:
            bound += int(w[k] == w[k + 2])
    return bound


# ---- captures --------------------------------------------------------------------------------------------------------
Plant = collections.namedtuple("Plant", "stream offset aa crc_init s ci header0 length note flips")
MHZ = d.LATTICE_MHZ                                        # channel indices 0, 17, 36, 37 (adv), 38 (adv), 22
DATA_STREAMS = d.DATA_STREAMS
N_WORDS = d.N_WORDS                                        # 1029: two full 512-word tiles and a ragged one
LIMITS = (0, 1, 16, 63)
MAX_LENS = (0, 27, 255)


class Capture:
    """words (n_streams, pitch_words), and one StreamModel per stream (made when first asked for)"""

    def __init__(self, words, n_words, pitch_words, search_bits, mhz, planted):
        self.words, self.n_words, self.pitch_words, self.search_bits = words, n_words, pitch_words, search_bits
        self.mhz, self.planted = np.array(mhz, np.uint16), tuple(planted)
        self._models = {}

    def model(self, s):
        if s not in self._models:
            self._models[s] = StreamModel(self.words[s], self.n_words, self.mhz[s], s)
        return self._models[s]

    def candidates(self, max_len, max_errors, rules=MODEL):
        out = []
        for s in range(len(self.mhz)):
            if _le.channel_index(int(self.mhz[s])) < 37 or rules.adv_accepted:
                out += candidates(self.model(s), self.search_bits, max_len, max_errors, rules)
        return out


class _Builder:
    def __init__(self, n_streams, n_words, mhz, seed):
        self.rng = np.random.default_rng(seed)
        self.n_words, self.mhz = n_words, mhz
        self.sym = self.rng.integers(0, 2, (n_streams, 64 * n_words + 20000), dtype=np.uint8)   # (the tail: room for what ends past the stream)
        self.used = [[] for _ in range(n_streams)]
        self.planted = []

    def free(self, stream, offset, n):
        return all(offset + n <= a or offset >= b for a, b in self.used[stream])

    def plant(self, stream, offset, aa, crc_init, s, header0, length, note, ci=None, flips=(), symbols=None):
        ch = _le.channel_index(int(self.mhz[stream])) & 0x3F
        if symbols is None:
            payload = self.rng.integers(0, 256, length, dtype=np.uint8).tobytes()
            symbols = c.coded_symbols(aa, ch, bytes([header0, length]) + payload, crc_init, s, ci=ci)
        if len(flips):
            symbols = c.flip(symbols, flips)
        assert offset >= 0 and self.free(stream, offset, len(symbols)), (note, stream, offset)
        self.used[stream].append((offset, offset + len(symbols)))
        self.sym[stream, offset:offset + len(symbols)] = symbols
        self.planted.append(Plant(stream, offset, aa, crc_init, s, {8: 0, 2: 1}[s] if ci is None else ci, header0, length, note, tuple(int(f) for f in flips)))
        return offset + len(symbols)

    def words(self, pitch_words):
        rows = [_le.pack(self.sym[s, :64 * self.n_words]) for s in range(len(self.sym))]
        out = self.rng.integers(0, 1 << 63, (len(rows), pitch_words), dtype=np.uint64)         # (what lies behind n_words is noise too)
        for s, r in enumerate(rows):
            out[s, :self.n_words] = r
        return out


def header_hit_symbols(rng, aa, ch, crc_init, mhz):
    """_le_coded.header_hit_case's recipe on a data channel: errors such that the lag decision's header (its length octet: 12 ^ 0x90)
    differs from the final path's, which is the header sent.  The first choice the model accepts."""
    for attempt in range(400):
        payload = rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
        sym = c.coded_symbols(aa, ch, bytes([0x02, 12]) + payload, crc_init, 2)
        diff = np.zeros((len(sym) - BLOCK2) // 2, np.uint8)
        diff[12:46:3] = 1
        apart = np.nonzero(np.array(c.encode(diff), np.uint8))[0]
        early = apart[apart < 80]
        k = len(early) // 2 + 1
        bad = c.flip(sym, BLOCK2 + rng.choice(early, k, replace=False))
        line = np.zeros(64 * 64, np.uint8)
        line[9:9 + len(bad)] = bad
        _, info = c.decode(_le.pack(line), 64, 0, 9, 0, mhz, crc_init)
        if info["header_moved"] and info["symbols"] == BLOCK2 + 2 * (8 * ((12 ^ 0x90) + 5) + 3):
            return bad
    raise AssertionError("no header hit found")


@functools.lru_cache(maxsize=None)
def lattice(tight):
    """The capture of the scan tests: six streams of N_WORDS words of seeded noise, four on data channels and two on advertising
    channels, with coded packets at the kernels' seams and at the branch points of the twelve rules.  tight: pitch_words == n_words
    and search_bits as large as the entries allow (the stream less 335 symbols); otherwise a larger pitch and search_bits 1500
    symbols inside the stream, with packets at search_bits - 1 and at search_bits."""
    b = _Builder(6, N_WORDS, MHZ, 2000 + (7 if tight else 0))
    rng = np.random.default_rng(300 + (1 if tight else 0))
    total = 64 * N_WORDS
    search_bits = total - 335 if tight else total - 1500
    inits = (0x555555, 0x000001, 0x800000, 0xABCDEF, 0x123456)
    k = 0

    def nxt():
        nonlocal k
        k += 1
        return d.good_aa(rng, k & 3), inits[k % len(inits)] ^ (k * 0x010203 & 0xFFFFFF), (1, 2, 3, 0x1D, 0x0A)[k % 5]

    # stream 0: every offset residue mod 64, S = 2 and S = 8 in turn, lengths 0 and 1; they lie across many lane seams (128
    # symbols) and the wave seams (8192 symbols), each right behind the one before it every fourth time (back to back)
    at = 70
    for r in range(64):
        aa, init, h0 = nxt()
        if r % 4:
            at += 1 + (r - at - 1) % 64                                                 # the next offset of residue r
        at = b.plant(0, at, aa, init, (2, 8)[r % 5 == 0], h0, r & 1, "residue %d%s" % (at % 64, "" if r % 4 else ", back to back"))
    residues = {p.offset % 64 for p in b.planted}
    for r in sorted(set(range(64)) - residues):                                         # (the back-to-back ones took what residue they got)
        aa, init, h0 = nxt()
        at += 1 + (r - at - 1) % 64
        at = b.plant(0, at, aa, init, 2, h0, 0, "residue %d" % r)
    assert {p.offset % 64 for p in b.planted} == set(range(64)) and at < 60000, at
    # stream 1: the long ones, S = 8: 254 and 255 octets; behind them packets whose 336 symbols lie on and against the wave seams
    at = 33
    for n in (255, 254):
        aa, init, h0 = nxt()
        at = b.plant(1, at, aa, init, 8, h0, n, "S 8 length %d" % n) + 11
    for o in (8192 * 5 - 100, 8192 * 6 - 335, 8192 * 7 - 1, 8192 * 7 + 1000):
        aa, init, h0 = nxt()
        b.plant(1, o, aa, init, 2, h0, 1, "wave seam")
    # stream 5 from word 330: lengths 27 and 28 at both S, across the tile seam 511 | 512 and in front of the ragged tile
    for s, n, o in ((2, 28, 64 * 1024 - 3000), (8, 28, 34200), (2, 27, 40000), (8, 27, 45000), (2, 1, 64 * 512 - 77), (8, 0, 64 * 512 - 900)):
        aa, init, h0 = nxt()
        b.plant(5, o, aa, init, s, h0, n, "S %d length %d" % (s, n))
    # stream 5: the long ones at S = 2, then the branch points of rules 5, 6, 7 and 9
    at = 21
    for n in (255, 254, 28):
        aa, init, h0 = nxt()
        at = b.plant(5, at, aa, init, 2, h0, n, "S 2 length %d" % n) + 7
    for kind, aa in sorted(d.one_offense_aas().items()):
        _, init, h0 = nxt()
        at = b.plant(5, at, aa, init, 2, h0, 0, "one offense: " + kind) + 13
    for ci in (2, 3):
        aa, init, h0 = nxt()
        at = b.plant(5, at, aa, init, (8, 2)[ci & 1], h0, 1, "ci %d" % ci, ci=ci) + 13
    for h0, note in ((0x00, "LLID 0"), (0x0C, "LLID 0, other bits set"), (0x21, "RFU bit 5"), (0x42, "RFU bit 6"), (0x83, "RFU bit 7"),
                     (0x1F, "every allowed bit")):
        aa, init, _ = nxt()
        at = b.plant(5, at, aa, init, 2, h0, 0, note) + 13
    aa, init, _ = nxt()
    hit = header_hit_symbols(rng, aa, _le.channel_index(MHZ[5]) & 0x3F, init, MHZ[5])
    at = b.plant(5, at, aa, init, 2, 0x02, 12, "header hit", symbols=hit)
    b.sym[5, at:at + 2700] = 0                                                          # (room, and quiet, for the 156 octets the lag decision reads)
    b.used[5].append((at, at + 2700))
    at += 2700
    # the stream's end: ending on its last symbol (stream 5), one symbol past it (stream 1)
    aa, init, h0 = nxt()
    b.plant(5, total - (BLOCK2 + 2 * 51), aa, init, 2, h0, 1, "ends on the last symbol")
    aa, init, h0 = nxt()
    b.plant(1, total + 1 - (BLOCK2 + 8 * 259), aa, init, 8, h0, 27, "ends one symbol past the stream")  # (below search_bits in both forms)
    if not tight:
        aa, init, h0 = nxt()
        b.plant(2, search_bits - 1, aa, init, 2, h0, 0, "at search_bits - 1")
        aa, init, h0 = nxt()
        b.plant(0, search_bits, aa, init, 2, h0, 0, "at search_bits")
    # stream 2: e mismatches for e one below, at and one above every limit, confined in turn to the preamble, each quarter of the
    # address, the sixteen symbols the pre-filter does not read, one symbol of e pre-filter pairs (its count equals e) and both
    # symbols of e / 2 pairs (it sees nothing of them).  Errors inside the address may make block 1 decode another one.
    at = 50
    regions = [("preamble", np.arange(0, 80))] + [("address quarter %d" % q, np.arange(80 + 64 * q, 144 + 64 * q)) for q in range(4)]
    pair_firsts = np.array([p for p in range(320) if p % 4 < 2])
    for e in sorted({max(E + dd, 0) for E in LIMITS for dd in (-1, 0, 1)}):
        kinds = [(name, rng.choice(reg, e, replace=False)) for name, reg in regions if e <= len(reg)]
        firsts = rng.choice(pair_firsts, e, replace=False)
        kinds.append(("one of a pair", firsts + 2 * rng.integers(0, 2, e)))
        both = rng.choice(pair_firsts, e // 2, replace=False)
        kinds.append(("both of a pair", np.concatenate([both, both + 2, [333] * (e % 2)]).astype(np.int64)))
        if e <= 16:
            kinds.append(("last sixteen", rng.choice(np.arange(320, 336), e, replace=False)))
        for name, flips in kinds:
            aa, init, h0 = nxt()
            at = b.plant(2, at, aa, init, 2, h0, 0, "%d errors: %s" % (e, name), flips=flips) + int(rng.integers(1, 20))
    assert at < search_bits - 500, at
    # coded data packets on the two advertising streams
    for s in (3, 4):
        for o in (64 * 10 + 50, 64 * 511 + 50, 64 * 900 + 50):
            aa, init, h0 = nxt()
            b.plant(s, o, aa, init, 2, h0, 0, "advertising channel")
    pitch = N_WORDS if tight else N_WORDS + 11
    words = b.words(pitch)
    words.flags.writeable = False
    return Capture(words, N_WORDS, pitch, search_bits, MHZ, b.planted)


def plant_expected(cap, p, max_len, max_errors):
    """Whether a planted packet without symbol errors is a candidate by its own making."""
    ch = _le.channel_index(int(cap.mhz[p.stream]))
    return (ch < 37 and p.offset < cap.search_bits and p.offset + BLOCK2 + p.s * (8 * (p.length + 5) + 3) <= 64 * cap.n_words and
            p.length <= max_len and (p.header0 & 3) != 0 and (p.header0 & 0xE0) == 0 and _offenses(p.aa) == 0 and p.ci < 2 and not p.flips)


@functools.lru_cache(maxsize=None)
def lattice_model(tight, max_len, max_errors):
    return tuple(lattice(tight).candidates(max_len, max_errors))


@functools.lru_cache(maxsize=None)
def chain_capture():
    """Three coded connections hopping over twelve data-channel streams, both S values, empty and non-empty PDUs, in noise."""
    mhz = np.array([2404 + 2 * ch for ch in (0, 3, 5, 8, 9, 10)] + [2428 + 2 * ch for ch in (0, 2, 7, 11, 19, 25)], np.uint16)
    n_words = 700
    b = _Builder(12, n_words, mhz, 4343)
    rng = np.random.default_rng(78)
    conns = []
    for cn, n_pkts in enumerate((24, 13, 7)):
        aa, init = d.good_aa(rng), int(rng.integers(0, 1 << 24))
        for k in range(n_pkts):
            s = int(rng.integers(0, 12)) if cn else k % 12                              # (the first connection visits every stream)
            n = 0 if k % 3 == 0 else int(rng.integers(1, 20))
            coded_s = (2, 8)[(k + cn) % 3 == 0]
            while True:                                                                 # (a free place: the longest of these packets has 1912 symbols)
                o = int(rng.integers(8, 64 * n_words - 2400))
                if b.free(s, o - 8, 2400):
                    break
            b.plant(s, o, aa, init, coded_s, (1, 2, 3, 0x0D)[k & 3] if n else 1, n, "connection %d" % cn)
        conns.append((aa, init))
    words = b.words(n_words + 3)
    words.flags.writeable = False
    return Capture(words, n_words, n_words + 3, 64 * n_words - 335, mhz, b.planted), tuple(conns)
