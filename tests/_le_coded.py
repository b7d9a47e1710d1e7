"""Test-side model of the Bluetooth LE Coded PHY (Core v5.x Vol 6 Part B 2.2, 3.1, 3.2, 3.3) and of the eight rules of
include/btbbx.h ("LE Coded PHY scan") -- plain Python and numpy, written from the spec text and the rules, not from the kernels.
CRC, whitening, the lell fields and the packing helpers are the 1M model's (tests/_le.py).

* FORMAT: the air format, stated once
* encode / map_symbols / coded_symbols / pattern_symbols: the transmitter
* match_all: brute-force sliding 336-symbol matcher (rule 1)
* Trellis / decode: rules 2 to 7 for one hit, literal and slow -> (btbbx_le_pkt dict, btbbx_le_coded_info dict)
* decode_many: the same for many hits at once (numpy over the hits, one Python step per trellis step); MODEL rules only
* Rules: the model's branch points as options; the default is the model, any other value a deliberately wrong decoder
* decode_cases / scan_cases: the inputs of tests/test_gpu_le_coded.py (tests/test_le_coded_model.py shows that they tell every
  wrong variant from the model)
"""
import numpy as np

import _le

PATTERN = 336
MAX_ERRORS = 63
LAG = 24
INF = 1 << 24

# ---- the air format, once ------------------------------------------------------------------------------------------
FORMAT = dict(
    preamble=(0, 0, 1, 1, 1, 1, 0, 0) * 10,         # 80 uncoded symbols in transmission order
    g0=(1, 1, 1, 1),                                # a0 = b ^ b1 ^ b2 ^ b3   (1 + x + x^2 + x^3)
    g1=(1, 0, 1, 1),                                # a1 = b ^ b2 ^ b3        (1 + x^2 + x^3)
    map8={0: (0, 0, 1, 1), 1: (1, 1, 0, 0)},        # S = 8: four symbols per coded bit; S = 2: coded bits as they are
    aa_bits=32, ci_bits=2, term_bits=3,             # block 1: AA LSB first, CI LSB first, TERM1; always S = 8
    s_of_ci={0: 8, 1: 2},                           # CI 2 and 3 are RFU
    block2=376,                                     # first symbol of block 2: 80 + 8 * 37
)


class Rules:
    """The branch points of the model.  Rules() is the model; every other value is a wrong decoder."""

    def __init__(self, **kw):
        self.swap_g = False             # G0 and G1 swapped
        self.a1_first = False           # a1 sent first
        self.mapper_inverted = False    # 0 -> 1100, 1 -> 0011
        self.ci_msb_first = False
        self.tie_x = 0                  # the predecessor that survives on equal sums
        self.lag_from_state0 = False    # rule 5's trace-back from state 0 instead of the best state
        self.final_from_best = False    # rule 6's trace-back from the best state instead of state 0
        self.revise_l = False           # L taken again from the final path's header
        self.whiten_block1 = False      # the whitening sequence starts at the AA
        self.s2_reads_8 = False         # at S = 2 a step still reads (and advances by) 8 symbols
        self.truncated_ge = False
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


MODEL = Rules()
WRONG = dict(swap_g=True, a1_first=True, mapper_inverted=True, ci_msb_first=True, tie_x=1, lag_from_state0=True, final_from_best=True,
             revise_l=True, whiten_block1=True, s2_reads_8=True, truncated_ge=True)


# ---- transmitter ---------------------------------------------------------------------------------------------------
def encode(bits, rules=MODEL):
    """Rate 1/2, K = 4, from state 0: the coded bits a0, a1 of every input bit, a0 first."""
    g0, g1 = (FORMAT["g1"], FORMAT["g0"]) if rules.swap_g else (FORMAT["g0"], FORMAT["g1"])
    reg = [0, 0, 0]
    out = []
    for b in bits:
        taps = [int(b)] + reg
        a0 = sum(t & g for t, g in zip(taps, g0)) & 1
        a1 = sum(t & g for t, g in zip(taps, g1)) & 1
        out += [a1, a0] if rules.a1_first else [a0, a1]
        reg = [int(b)] + reg[:2]
    return out


def map_symbols(coded, s, rules=MODEL):
    if s == 2:
        return list(coded)
    m = FORMAT["map8"]
    return [x for c in coded for x in m[c ^ 1 if rules.mapper_inverted else c]]


def int_bits(v, n):
    return [(v >> i) & 1 for i in range(n)]


def pattern_symbols(aa):
    """Rule 1's 336 symbols: preamble + mapped, coded AA (encoder from state 0, no CI)."""
    return np.array(list(FORMAT["preamble"]) + map_symbols(encode(int_bits(aa, 32)), 8), np.uint8)


def coded_symbols(aa, chan, pdu, crc_init, s, ci=None):
    """A whole packet in transmission order.  ci defaults to the one that announces s; an RFU ci (2, 3) sends block 2 at S = s anyway."""
    if ci is None:
        ci = {8: 0, 2: 1}[s]
    pdu_b = _le.octet_bits(pdu)
    body = np.concatenate([pdu_b, _le.crc24_tx_bits(pdu_b, crc_init)])
    body = body ^ _le.whitening_bits(chan, len(body))
    block1 = int_bits(aa, 32) + int_bits(ci, 2) + [0, 0, 0]
    block2 = [int(b) for b in body] + [0, 0, 0]
    return np.array(list(FORMAT["preamble"]) + map_symbols(encode(block1), 8) + map_symbols(encode(block2), s), np.uint8)


# ---- rule 1 ----------------------------------------------------------------------------------------------------------
def mismatch_counts(sym, aa, n_offsets):
    """The mismatch count of the 336-symbol window at every offset [0, n_offsets) of a symbol array (zeros behind its end)."""
    pat = pattern_symbols(aa)
    s = np.zeros(n_offsets + PATTERN, np.uint8)
    s[:min(len(sym), len(s))] = sym[:len(s)]
    err = np.zeros(n_offsets, np.int32)
    for k in range(PATTERN):
        err += s[k:k + n_offsets] != pat[k]
    return err


def match_all(words, n_words, search_bits, aa, max_errors):
    """Every offset in [0, search_bits) of one packed stream within max_errors of the pattern -> (offsets, mismatches)."""
    sym = np.unpackbits(np.asarray(words[:n_words], np.uint64).view(np.uint8), bitorder="little")
    err = mismatch_counts(sym, aa, search_bits)
    keep = np.nonzero(err <= max_errors)[0]
    return keep.astype(np.uint64), err[keep]


# ---- rules 2 to 7 ----------------------------------------------------------------------------------------------------
def branch(prev, b, s, rules=MODEL):
    """The symbols of the transition from state prev with input b."""
    g0, g1 = (FORMAT["g1"], FORMAT["g0"]) if rules.swap_g else (FORMAT["g0"], FORMAT["g1"])
    taps = [b, prev & 1, (prev >> 1) & 1, (prev >> 2) & 1]
    a0 = sum(t & g for t, g in zip(taps, g0)) & 1
    a1 = sum(t & g for t, g in zip(taps, g1)) & 1
    return map_symbols([a1, a0] if rules.a1_first else [a0, a1], s, rules)


class Trellis:
    """Rule 2.  metrics[s] after every step, decisions[t][s] = the x of the surviving predecessor (s >> 1) | x << 2."""

    def __init__(self, s, rules=MODEL):
        self.s, self.rules = s, rules
        self.metrics = [0] + [INF] * 7              # state 0 at metric 0, the others unreachable
        self.decisions = []
        self.expect = {(p, b): branch(p, b, s, rules) for p in range(8) for b in (0, 1)}

    def step(self, received):
        new, dec = [], []
        for nxt in range(8):
            b = nxt & 1
            sums = []
            for x in (0, 1):
                p = (nxt >> 1) | (x << 2)
                sums.append(self.metrics[p] + sum(int(r) != e for r, e in zip(received, self.expect[(p, b)])))
            x = self.rules.tie_x if sums[0] == sums[1] else int(sums[1] < sums[0])
            new.append(min(sums[x], INF + 100000))
            dec.append(x)
        self.metrics = new
        self.decisions.append(dec)

    def best(self):
        return min(range(8), key=lambda s: (self.metrics[s], s))

    def trace(self, state):
        """The input bits of the path that ends in `state` now."""
        bits = []
        for dec in reversed(self.decisions):
            bits.append(state & 1)
            state = (state >> 1) | (dec[state] << 2)
        return bits[::-1]


def decode(words, n_words, stream, offset, errors, mhz, crc_init, rules=MODEL):
    """The two records btbbx_le_coded_decode_hits_device writes for a hit at `offset`: dicts keyed like LE_PKT_DTYPE (without pad) and
    LE_CODED_INFO_DTYPE (without reserved)."""
    chan = _le.channel_index(mhz) & 0x3F
    wh = _le.whitening_bits(chan, 37 + 8 * 260)
    wh1, wh2 = (wh[:37], wh[37:]) if rules.whiten_block1 else (np.zeros(37, np.uint8), wh)

    def symbols(first, n):
        return _le.stream_bits(words, n_words, first, n)

    # rule 3
    t1 = Trellis(8, rules)
    for t in range(37):
        t1.step(symbols(offset + 80 + 8 * t, 8))
    b1 = np.array(t1.trace(0), np.uint8) ^ wh1
    aa = _le.bits_value(b1[:32])
    ci = int(b1[32]) * 2 + int(b1[33]) if rules.ci_msb_first else int(b1[32]) + 2 * int(b1[33])
    metric1 = t1.metrics[0]
    s = FORMAT["s_of_ci"].get(ci, 0)                # rule 4
    if s == 0:
        raw = int(aa).to_bytes(4, "little") + bytes(_le.MAX_BYTES - 4)
        rec = dict(offset=offset, stream=stream, aa_errors=errors, crc_ok=0, crc_rx=0, crc_calc=0, pdu_bytes=0, truncated=0, bytes=raw)
        rec.update(_le.lell_fields(raw, mhz))
        return rec, dict(symbols=376, metric2=0, metric1=metric1, ci=ci, s=0, header_moved=0)
    # rule 5
    step = 8 if rules.s2_reads_8 else s
    base = offset + FORMAT["block2"]
    t2 = Trellis(step, rules)
    for t in range(16 + LAG):
        t2.step(symbols(base + step * t, step))
    lag_header = t2.trace(0 if rules.lag_from_state0 else t2.best())[:16]
    L = _le.bits_value(np.array(lag_header[8:16], np.uint8) ^ wh2[8:16])
    n = 8 * (L + 5) + 3
    # rule 6
    for t in range(16 + LAG, n):
        t2.step(symbols(base + step * t, step))
    end_state = t2.best() if rules.final_from_best else 0
    path = t2.trace(end_state)
    metric2 = t2.metrics[end_state]
    moved = int(path[:16] != lag_header)
    # rule 7
    if rules.revise_l:
        L = _le.bits_value(np.array(path[8:16], np.uint8) ^ wh2[8:16])
    pdu_n = 2 + L
    body = np.zeros(8 * (pdu_n + 3), np.uint8)
    keep = min(len(body), n - 3)
    body[:keep] = path[:keep]
    body ^= wh2[:len(body)]
    pdu_b, crc_b = body[:8 * pdu_n], body[8 * pdu_n:]
    crc_calc = _le.bits_value(_le.crc24_tx_bits(pdu_b, crc_init & 0xFFFFFF))
    crc_rx = _le.bits_value(crc_b)
    n_symbols = 376 + s * n
    end = offset + n_symbols
    truncated = end >= n_words * 64 if rules.truncated_ge else end > n_words * 64
    raw = (int(aa).to_bytes(4, "little") + _le.bits_octets(body))[:_le.MAX_BYTES]
    raw = raw + bytes(_le.MAX_BYTES - len(raw))
    rec = dict(offset=offset, stream=stream, aa_errors=errors, crc_ok=int(not truncated and crc_calc == crc_rx), crc_rx=crc_rx,
               crc_calc=crc_calc, pdu_bytes=pdu_n, truncated=int(truncated), bytes=raw)
    rec.update(_le.lell_fields(raw, mhz))
    return rec, dict(symbols=n_symbols, metric2=metric2, metric1=metric1, ci=ci, s=s, header_moved=moved)


# ---- the same for many hits at once ----------------------------------------------------------------------------------
def _forward_many(sym, starts, s, steps):
    """Rule 2 for len(starts) hits in step: sym = one symbol array with zeros behind it, starts = the first symbol of each hit's block,
    steps[i] = that hit's number of steps.  Returns metrics after steps[i] steps (n, 8), the decisions (max steps, n, 8) and, for
    rule 5, the metrics after step 16 + LAG."""
    n, top = len(starts), int(max(steps))
    expect = np.array([[branch((nxt >> 1) | (x << 2), nxt & 1, s) for x in (0, 1)] for nxt in range(8)], np.uint8)   # (8, 2, s)
    metrics = np.full((n, 8), INF, np.int64)
    metrics[:, 0] = 0
    final = metrics.copy()
    at_lag = None
    dec = np.zeros((top, n, 8), np.uint8)
    pred = np.array([[(nxt >> 1) | (x << 2) for x in (0, 1)] for nxt in range(8)])
    idx = np.arange(s)
    for t in range(top):
        r = sym[(starts + s * t)[:, None] + idx]                                    # (n, s)
        bm = (r[:, None, None, :] != expect[None]).sum(axis=3)                      # (n, 8, 2)
        sums = metrics[:, pred] + bm                                                # (n, 8, 2)
        x = (sums[:, :, 1] < sums[:, :, 0]).astype(np.uint8)
        metrics = np.minimum(np.where(x == 1, sums[:, :, 1], sums[:, :, 0]), INF + 100000)
        dec[t] = x
        if t + 1 == 16 + LAG:
            at_lag = metrics.copy()
        done = steps == t + 1
        final[done] = metrics[done]
    return final, dec, at_lag


def _trace_many(dec, steps, states):
    """The paths that end in states[i] after steps[i] steps -> (n, max steps) bits, zero behind a path's end."""
    n = len(steps)
    out = np.zeros((n, dec.shape[0]), np.uint8)
    state = np.array(states, np.int64)
    rows = np.arange(n)
    for t in range(dec.shape[0] - 1, -1, -1):
        live = steps > t
        out[live, t] = state[live] & 1
        x = dec[t, rows, state]
        state = np.where(live, (state >> 1) | (x.astype(np.int64) << 2), state)
    return out


def decode_many(words, n_words, stream, offsets, errors, mhz, crc_init):
    """decode() for many hits of one stream, MODEL rules: a list of (pkt, info) in the order of `offsets`."""
    offsets = np.asarray(offsets, np.int64)
    n = len(offsets)
    if n == 0:
        return []
    sym = np.zeros(n_words * 64 + 376 + 8 * 2100, np.uint8)
    sym[:n_words * 64] = np.unpackbits(np.asarray(words[:n_words], np.uint64).view(np.uint8), bitorder="little")
    wh = _le.whitening_bits(_le.channel_index(mhz) & 0x3F, 8 * 260)
    m1, d1, _ = _forward_many(sym, offsets + 80, 8, np.full(n, 37))
    b1 = _trace_many(d1, np.full(n, 37), np.zeros(n, np.int64))
    out = [None] * n
    ci = b1[:, 32].astype(int) + 2 * b1[:, 33].astype(int)
    for s in (0, 8, 2):
        sel = np.nonzero(np.array([FORMAT["s_of_ci"].get(int(c), 0) == s for c in ci]))[0]
        if len(sel) == 0:
            continue
        if s:
            base = offsets[sel] + FORMAT["block2"]
            lag_steps = np.full(len(sel), 16 + LAG)
            mlag, dlag, _ = _forward_many(sym, base, s, lag_steps)
            best = np.array([min(range(8), key=lambda q: (mlag[i, q], q)) for i in range(len(sel))])
            lag_header = _trace_many(dlag, lag_steps, best)[:, :16]
            Ls = np.array([_le.bits_value(h[8:16] ^ wh[8:16]) for h in lag_header])
            steps = 8 * (Ls + 5) + 3
            m2, d2, _ = _forward_many(sym, base, s, steps)
            paths = _trace_many(d2, steps, np.zeros(len(sel), np.int64))
        for j, i in enumerate(sel):
            aa = _le.bits_value(b1[i, :32])
            o = int(offsets[i])
            if s == 0:
                raw = int(aa).to_bytes(4, "little") + bytes(_le.MAX_BYTES - 4)
                rec = dict(offset=o, stream=stream, aa_errors=int(errors[i]), crc_ok=0, crc_rx=0, crc_calc=0, pdu_bytes=0, truncated=0, bytes=raw)
                info = dict(symbols=376, metric2=0, metric1=int(m1[i, 0]), ci=int(ci[i]), s=0, header_moved=0)
            else:
                L, nb = int(Ls[j]), int(steps[j])
                body = paths[j, :nb - 3] ^ wh[:nb - 3]
                pdu_b, crc_b = body[:8 * (2 + L)], body[8 * (2 + L):]
                crc_calc, crc_rx = _le.bits_value(_le.crc24_tx_bits(pdu_b, crc_init & 0xFFFFFF)), _le.bits_value(crc_b)
                truncated = o + 376 + s * nb > n_words * 64
                raw = (int(aa).to_bytes(4, "little") + _le.bits_octets(body))[:_le.MAX_BYTES]
                raw = raw + bytes(_le.MAX_BYTES - len(raw))
                rec = dict(offset=o, stream=stream, aa_errors=int(errors[i]), crc_ok=int(not truncated and crc_calc == crc_rx), crc_rx=crc_rx,
                           crc_calc=crc_calc, pdu_bytes=2 + L, truncated=int(truncated), bytes=raw)
                info = dict(symbols=376 + s * nb, metric2=int(m2[j, 0]), metric1=int(m1[i, 0]), ci=int(ci[i]), s=s,
                            header_moved=int((paths[j, :16] != lag_header[j]).any()))
            rec.update(_le.lell_fields(raw, mhz))
            out[i] = (rec, info)
    return out


INFO_FIELDS = ("symbols", "metric2", "metric1", "ci", "s", "header_moved")


def info_dict(r):
    return {k: int(r[k]) for k in INFO_FIELDS}


# ---- shared inputs ---------------------------------------------------------------------------------------------------
def pdu_of(rng, length, adv=True):
    return _le.make_pdu(int(rng.integers(0, 256)) & (0xCF if adv else 0x1F), rng.integers(0, 256, length, dtype=np.uint8).tobytes())


def flip(sym, positions):
    sym = sym.copy()
    sym[np.asarray(positions, np.int64)] ^= 1
    return sym


def tie_received():
    """Three symbol errors at S = 2 that leave two paths at the same distance from the received word: the code's free distance is 6,
    reached by the message 1 + x (G0 (1 + x) = 1 + x^4, G1 (1 + x) = 1 + x + x^2 + x^4), so flipping three of the six symbols in
    which its code word differs from zero's puts the received word halfway.  Returns (message bits, received S = 2 symbols) for a
    43-bit message ending in three zeros."""
    msg = [0] * 43
    other = list(msg)
    other[10] = other[11] = 1
    a, b = np.array(encode(msg), np.uint8), np.array(encode(other), np.uint8)
    diff = np.nonzero(a != b)[0]
    assert len(diff) == 6
    return msg, flip(a, diff[:3])


def decode_cases(seed=20):
    """The GPU decode test's inputs: a list of dicts(words, n_words, hits=[(offset, errors)], mhz, crc_init, note), one stream each.
    Lengths x S x channel kinds, 64 bit phases, RFU CIs, error counts at the guaranteed-correctable limit, a built tie, 10 % errors,
    a header hit (header_moved = 1, another L), L = 255 decoded from noise behind a short stream, and streams that end around the
    packet's end, inside block 1 and at the lag step."""
    rng = np.random.default_rng(seed)
    cases = []

    def stream_of(pieces, total=None, noise=True):
        """pieces: [(offset, symbols)] -> (words, n_words); total symbols (default: just behind the last piece, rounded up to words)"""
        end = max(o + len(s) for o, s in pieces)
        total = end if total is None else total
        n_words = (total + 63) // 64
        line = rng.integers(0, 2, n_words * 64, dtype=np.uint8) if noise else np.zeros(n_words * 64, np.uint8)
        for o, s in pieces:
            k = min(len(s), len(line) - o)
            if k > 0:
                line[o:o + k] = s[:k]
        line[total:] = 0
        return _le.pack(line), n_words

    # lengths x S x channel kind, clean, at odd offsets
    for mhz, crc_init, aa in ((2402, _le.ADV_CRC_INIT, _le.ADV_AA), (2440, 0x1A2B3C, 0x5A3C96E1)):
        chan = _le.channel_index(mhz)
        for s in (2, 8):
            pieces, hits, at = [], [], 37
            for L in (0, 1, 37, 38, 254, 255):
                sym = coded_symbols(aa, chan, pdu_of(rng, L, mhz == 2402), crc_init, s)
                pieces.append((at, sym))
                hits.append((at, 0))
                at += len(sym) + int(rng.integers(1, 90))
            w, nw = stream_of(pieces)
            cases.append(dict(words=w, n_words=nw, hits=hits, mhz=mhz, crc_init=crc_init, note="lengths S=%d %d MHz" % (s, mhz)))
    # 64 consecutive bit phases, S = 2 and S = 8 alternating, L = 3
    pieces, hits, at = [], [], 0
    for phase in range(64):
        s = (2, 8)[phase & 1]
        sym = coded_symbols(_le.ADV_AA, 38, pdu_of(rng, 3), _le.ADV_CRC_INIT, s)
        at = (at + 63) // 64 * 64 + phase
        pieces.append((at, sym))
        hits.append((at, phase))
        at += len(sym)
    w, nw = stream_of(pieces)
    cases.append(dict(words=w, n_words=nw, hits=hits, mhz=2426, crc_init=_le.ADV_CRC_INIT, note="phases"))
    # RFU CIs; correctable error counts (2 per block at S = 2, 11 per block at S = 8); the tie; 10 % errors; a header hit
    pieces, hits, at = [], [], 11
    for ci in (2, 3):
        sym = coded_symbols(_le.ADV_AA, 37, pdu_of(rng, 5), _le.ADV_CRC_INIT, 8, ci=ci)
        pieces.append((at, sym))
        hits.append((at, 1))
        at += len(sym) + 3
    for s, k in ((2, 2), (8, 11)):
        for rep in range(3):
            sym = coded_symbols(_le.ADV_AA, 37, pdu_of(rng, 9), _le.ADV_CRC_INIT, s)
            sym = flip(sym, 80 + rng.choice(296, 11, replace=False))
            sym = flip(sym, 376 + rng.choice(len(sym) - 376, k, replace=False))
            pieces.append((at, sym))
            hits.append((at, 2))
            at += len(sym) + 5
    msg, rx = tie_received()
    head = coded_symbols(_le.ADV_AA, 37, pdu_of(rng, 0), _le.ADV_CRC_INIT, 2)[:376]
    pieces.append((at, np.concatenate([head, rx])))
    hits.append((at, 0))
    at += 376 + len(rx) + 2
    for s in (2, 8):
        sym = coded_symbols(_le.ADV_AA, 37, pdu_of(rng, 30), _le.ADV_CRC_INIT, s)
        noisy = sym.copy()
        noisy[80:] ^= (rng.random(len(sym) - 80) < 0.10).astype(np.uint8)
        pieces.append((at, noisy))
        hits.append((at, 3))
        at += len(sym) + 4 * 260 * s                    # (room for whatever L the noise decodes)
    w, nw = stream_of(pieces, noise=False)
    cases.append(dict(words=w, n_words=nw, hits=hits, mhz=2402, crc_init=_le.ADV_CRC_INIT, note="rfu, errors, tie, noise"))
    cases.append(header_hit_case(rng))
    # L = 255 decoded from noise behind a short stream: only block 1 and a few steps are there
    chan = 37
    sym = coded_symbols(_le.ADV_AA, chan, _le.make_pdu(0x42, bytes(255)), _le.ADV_CRC_INIT, 2)
    w, nw = stream_of([(5, sym)], total=5 + 376 + 2 * 44)
    cases.append(dict(words=w, n_words=nw, hits=[(5, 0)], mhz=2402, crc_init=_le.ADV_CRC_INIT, note="L 255 behind a short stream"))
    # streams ending around the packet's end, inside block 1, at the lag step
    for s in (2, 8):
        sym = coded_symbols(_le.ADV_AA, 39, pdu_of(rng, 2), _le.ADV_CRC_INIT, s)
        ends = [len(sym) + d for d in (0, 1, -1, s - 1, -(s - 1), s, -s, s + 1, -(s + 1))] + [200, 376 + s * 40, 376 + s * 40 - 1, 376 + s * 40 + 1]
        for e in ends:
            off = (64 - (e % 64)) % 64                  # the stream's last word ends exactly where the packet (or its cut) does
            w, nw = stream_of([(off, sym[:e] if e <= len(sym) else sym)], total=off + e)
            assert nw * 64 == off + e
            cases.append(dict(words=w, n_words=nw, hits=[(off, 0)], mhz=2480, crc_init=_le.ADV_CRC_INIT, note="end %+d S=%d" % (e - len(sym), s)))
    return cases


def header_hit_case(rng):
    """Errors such that the lag decision's header differs from the final path's, length octet included.  A second message differs
    from the sent one at bits 12, 15, 18 .. 45: its path leaves the sent one inside the header and stays apart past the lag step.
    Of the symbols in which the two code words differ, more than half of those in front of step 40 are flipped (the wrong path leads
    at the lag step) but fewer than half of all (the sent path wins in the end).  Which ones: the first choice the model accepts."""
    for attempt in range(400):
        sym = coded_symbols(_le.ADV_AA, 37, pdu_of(rng, 12), _le.ADV_CRC_INIT, 2)
        sent = sym[376:]
        diff = np.zeros(len(sent) // 2, np.uint8)
        diff[12:46:3] = 1
        apart = np.nonzero(np.array(encode(diff), np.uint8))[0]     # (the code is linear: the code words differ where diff's is 1)
        early = apart[apart < 80]
        k = len(early) // 2 + 1
        assert 2 * k < len(apart)
        bad = flip(sym, 376 + rng.choice(early, k, replace=False))
        line = np.zeros(64 * 80, np.uint8)
        line[9:9 + len(bad)] = bad
        w = _le.pack(line)
        rec, info = decode(w, len(w), 0, 9, 0, 2402, _le.ADV_CRC_INIT)
        alt, _ = decode(w, len(w), 0, 9, 0, 2402, _le.ADV_CRC_INIT, Rules(revise_l=True))
        if info["header_moved"] and alt["pdu_bytes"] != rec["pdu_bytes"]:
            return dict(words=w, n_words=len(w), hits=[(9, 0)], mhz=2402, crc_init=_le.ADV_CRC_INIT, note="header hit")
    raise AssertionError("no header hit found")
