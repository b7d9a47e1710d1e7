"""A deterministic lattice for the Bluetooth LE path (libbtbb_amd/csrc/le.hip), built from fixed seeds.

Seeded random captures (tests/test_gpu_le.py) meet the branch points of the LE kernels rarely or never; here every case is
laid on purpose, so that a kernel whose boundary, mask or table entry is off by one disagrees with the model (tests/_le.py)
on a named hit.  Two builders, both byte-identical from one build to the next:

* decode_lattice(): packed streams plus a hand-built HIT_DTYPE list for btbbx_le_decode_hits_device -- no scan is needed to
  decode a list that carries any access address at any offset.  One axis after the other, not their product:
  - header octet 1 = 0..255 on a data and on an advertising channel (`length` masks 0x1f / 0x3f, pdu_bytes all eight bits,
    the dword packing of `bytes` around its 64-byte cap); one in eight has one bit flipped in header octet 0, the last
    payload octet, the first or the last CRC bit;
  - offset mod 64 = 0..63 for a packet of at most 8 octets and for one with 100 payload octets or more;
  - packets at the end of their stream: END_LENGTHS x both channel kinds x the end distances of end_distances();
  - access addresses on data channels (L = 0): the advertising AA and its neighbours, four equal octets, runs, more than 24
    transitions, every 12-bit low and high window, each of the 38 windows the reference's case list omits at each of the six
    nibble-aligned positions with the window's one-bit neighbours, a random thousand; on an advertising channel the
    advertising AA, its neighbours and 200 others;
  - one stream per MHz value 2400..2483 (packets are whitened with channel_index(mhz) & 0x3f: a valid CRC proves the seed);
  - ac_errors 0..4 spread over the list; stream 0 and the last stream both carry hits.
  Every packet is laid into its stream as preamble, AA, whitened PDU and CRC, so the model reads the AA the hit carries.
  loose: random non-zero words between n_words and pitch_words; tight: pitch_words == n_words, so what lies behind a
  stream's end is the next stream, which like every stream starts with a packet at offset 0.

* scan_lattice(): access addresses for the generic scan kernel (le_scan_kernel<-1, L>: every AA but the advertising one),
  each with two streams of two full tiles and a ragged one: noise, planted 40-bit patterns with exactly 0..6 mismatches
  drawn from the three zones the filter and the exact check treat differently, patterns across the lane, wave and tile
  seams and at the last searched offset, true advertising packets for the neighbours of the advertising AA, and for four
  AAs a stream of the pattern back to back (a hit every 40 bits: the per-wave hit ring wraps).
"""
import functools
from collections import namedtuple

import numpy as np

import _le
import _libs
import libbtbb_amd as bt

CONN_AA = 0x50654C3B
MAIN_CRC_INIT = _le.ADV_CRC_INIT
END_LENGTHS = (0, 1, 6, 37, 60, 255)
FLIPS = ("h0", "last_payload", "crc_first", "crc_last")
ZONES = ((0, 8), (8, 32), (32, 40))                 # window bits: preamble, AA bits 0..23, AA top octet
DATA_MHZ = tuple(m for m in range(2400, 2484) if _le.channel_index(m) < 37)

# axis: lengths / phase / end / aa / aa_adv / head; kind: "data" or "adv"; L: header octet 1; detail: per axis (lengths: None;
# phase: (phase, "short" | "long"); end: the end distance; aa / aa_adv: (family, ...)); flip: None or one of FLIPS; dist: end of
# the packet minus end of the stream (> 0: truncated)
Tag = namedtuple("Tag", "axis kind L detail flip dist")
DecodeLattice = namedtuple("DecodeLattice", "words n_streams n_words pitch_words mhz hits tags crc_init")
Planted = namedtuple("Planted", "stream offset errors zones what")
ScanCase = namedtuple("ScanCase", "aa words n_words search_bits mhz planted adv_packets dense_stream")


def end_distances(L):
    """end - 64 * n_words for the packets at a stream's end: exact, the bits and octets around the CRC, then the header
    16 bits inside, 8 bits inside, and wholly outside (offset + 40 == 64 * n_words)."""
    return (0, 1, 7, 8, 9, 23, 24, 25, 8 * (L + 3), 8 * (L + 4), 8 * (L + 5))


def run_aas():
    """Runs of 6, 7, 8 and 12 equal bits at every position (the list of test_le_model.test_lell_fields_special_aas)."""
    out = []
    for run in (6, 7, 8, 12):
        for start in range(0, 33 - run):
            base = 0x5555AAAA if start & 1 else 0xAAAA5555
            ones = ((1 << run) - 1) << start
            out += [(base | ones) & 0xFFFFFFFF, base & ~ones & 0xFFFFFFFF]
    return out


TRANSITION_AAS = (0xAAAAAAAA, 0x55555555, 0xAAAAAAAB, 0x2AAAAAAA, 0xD5555555, 0x5555AAAA)


def omitted_window_aas():
    """(aa, window, shift, flipped window bit or None): each omitted window at each aligned position in an alternating AA."""
    out = []
    for v in sorted(_le.OMITTED_WINDOWS):
        for shift in range(0, 21, 4):
            for flip in (None,) + tuple(range(12)):
                w = v if flip is None else v ^ (1 << flip)
                out.append(((0x55555555 & ~(0xFFF << shift) | (w << shift)) & 0xFFFFFFFF, v, shift, flip))
    return out


def packet_bits(aa, mhz, h0, payload, crc_init, flip=None, rng=None):
    """One packet on air; `flip` turns one bit over after the CRC was formed."""
    pdu = _le.make_pdu(h0, payload)
    bits = _le.tx_bits(aa, _le.channel_index(mhz) & 0x3F, pdu, crc_init & 0xFFFFFF).copy()
    n = len(bits)
    if flip == "h0":
        bits[40 + int(rng.integers(0, 8))] ^= 1
    elif flip == "last_payload":
        assert len(payload)
        bits[n - 24 - 8 + int(rng.integers(0, 8))] ^= 1
    elif flip == "crc_first":
        bits[n - 24] ^= 1
    elif flip == "crc_last":
        bits[n - 1] ^= 1
    else:
        assert flip is None
    return bits


def _items(rng, full):
    """The packets of the lattice before they are given a stream: dicts of kind, aa, L, flip, tag parts, phase."""
    items = []

    def add(axis, kind, L, detail=None, flip=None, aa=None, phase=None):
        if aa is None:
            aa = _le.ADV_AA if kind == "adv" else int(rng.integers(0, 1 << 32))
        items.append(dict(axis=axis, kind=kind, L=L, detail=detail, flip=flip, aa=aa, phase=phase))

    for kind in ("data", "adv"):
        for L in range(0, 256, 1 if full else 5):
            add("lengths", kind, L, flip=FLIPS[(L >> 3) & 3] if L & 7 == 3 else None)
    for phase in range(0, 64, 1 if full else 7):
        for size in ("short", "long"):
            L = int(rng.integers(0, 4)) if size == "short" else int(rng.integers(100, 141))
            add("phase", ("data", "adv")[(phase + (size == "long")) & 1], L, detail=(phase, size), phase=phase)
    data_aas = [("adv_aa", _le.ADV_AA)] + [("adv_neighbour", _le.ADV_AA ^ (1 << i)) for i in range(32)]
    adv_aas = list(data_aas)
    if full:
        data_aas += [("equal_octets", b * 0x01010101) for b in range(256)]
        data_aas += [("run", a) for a in run_aas()] + [("transitions", a) for a in TRANSITION_AAS]
        data_aas += [("low_window", v) for v in range(4096)] + [("high_window", v << 20) for v in range(4096)]
        data_aas += [(("omitted", v, shift, flip), a) for a, v, shift, flip in omitted_window_aas()]
        data_aas += [("random", int(a)) for a in rng.integers(0, 1 << 32, 1000, dtype=np.uint64)]
        adv_aas += [("random", int(a)) for a in rng.integers(0, 1 << 32, 200, dtype=np.uint64)]
    else:
        data_aas += [("random", int(a)) for a in rng.integers(0, 1 << 32, 40, dtype=np.uint64)]
        adv_aas += [("random", int(a)) for a in rng.integers(0, 1 << 32, 20, dtype=np.uint64)]
    for family, aa in data_aas:
        add("aa", "data", 0, detail=family, aa=aa)
    for family, aa in adv_aas:
        add("aa_adv", "adv", 0, detail=family, aa=aa)
    return items


@functools.lru_cache(maxsize=None)
def decode_lattice(tight=False, crc_init=MAIN_CRC_INIT, full=True):
    """The decoder's lattice (module docstring).  full=False: a thinned copy of a few hundred hits, for further CRCInit
    values.  The packets' CRCs are formed with crc_init & 0xffffff."""
    rng = np.random.default_rng(_libs.seed(7400))
    ends = [(kind, L, d) for L in END_LENGTHS for kind in ("data", "adv") for d in dict.fromkeys(end_distances(L))]
    mhz = list(range(2400, 2484))
    for i, (kind, L, d) in enumerate(ends):
        mhz.append(DATA_MHZ[(7 * i + 3) % len(DATA_MHZ)] if kind == "data" else _le.ADV_MHZ[i % 3])
    n_streams = len(mhz)
    kind_of = ["data" if _le.channel_index(m) < 37 else "adv" for m in mhz]
    parts = [[] for _ in range(n_streams)]              # (offset, bits) per stream
    cursor = [0] * n_streams
    hits, tags = [], []

    def lay(s, it, offset=None, dist=None):
        payload = rng.integers(0, 256, it["L"], dtype=np.uint8).tobytes()
        bits = packet_bits(it["aa"], mhz[s], int(rng.integers(0, 256)), payload, crc_init, it["flip"], rng)
        if offset is None:
            offset = cursor[s] + (int(rng.integers(0, 17)) if cursor[s] else 0)
            if it["phase"] is not None:
                offset += (it["phase"] - offset) % 64
        assert offset >= cursor[s]
        parts[s].append((offset, bits))
        cursor[s] = offset + len(bits)
        hits.append((s, offset, it["aa"]))
        tags.append(Tag(it["axis"], it["kind"], it["L"], it["detail"], it["flip"], dist))

    for s in range(n_streams):                          # every stream starts with a packet: its seed, and the tight variant
        lay(s, dict(axis="head", kind=kind_of[s], L=2, detail=mhz[s], flip=None, phase=None,
                    aa=_le.ADV_AA if kind_of[s] == "adv" else int(rng.integers(0, 1 << 32))))
    by_kind = {k: [s for s in range(n_streams) if kind_of[s] == k] for k in ("data", "adv")}
    for it in _items(rng, full):
        lay(min(by_kind[it["kind"]], key=lambda s: cursor[s]), it)
    n_words = (max(cursor) + 8 * 260 + 40 + 64 + 63) // 64
    for i, (kind, L, d) in enumerate(ends):
        s = 84 + i
        assert kind_of[s] == kind
        offset = 64 * n_words + d - 40 - 8 * (L + 5)
        lay(s, dict(axis="end", kind=kind, L=L, detail=d, flip=None, phase=None,
                    aa=_le.ADV_AA if kind == "adv" else int(rng.integers(0, 1 << 32))), offset=offset, dist=d)
    pitch = n_words if tight else n_words + 3
    words = np.zeros((n_streams, pitch), np.uint64)
    for s in range(n_streams):
        sym = rng.integers(0, 2, 64 * n_words, dtype=np.uint8)
        for offset, bits in parts[s]:
            keep = min(len(bits), 64 * n_words - offset)
            sym[offset:offset + keep] = bits[:keep]
        words[s, :n_words] = _le.pack(sym)
    tail = rng.integers(1, 1 << 63, (n_streams, 3), dtype=np.uint64) | np.uint64(1 << 63)
    if not tight:
        words[:, n_words:] = tail
    h = np.zeros(len(hits), bt.HIT_DTYPE)
    h["stream"] = [x[0] for x in hits]
    h["offset"] = [x[1] for x in hits]
    h["lap"] = [x[2] for x in hits]
    h["ac_errors"] = np.arange(len(hits)) % 5
    assert (h["offset"] + 40 <= 64 * n_words).all()
    words.flags.writeable = False
    h.flags.writeable = False
    return DecodeLattice(words, n_streams, n_words, pitch, np.array(mhz, np.uint16), h, tuple(tags), crc_init)


def model_record(lat, i, rules=_le.MODEL, crc_init=None):
    """The model's record of hit i.  The row handed to the model runs on to the end of the capture, as the memory does."""
    h = lat.hits[i]
    s = int(h["stream"])
    row = lat.words.reshape(-1)[s * lat.pitch_words:]
    return _le.decode(row, lat.n_words, s, int(h["offset"]), int(h["ac_errors"]), int(lat.mhz[s]),
                      lat.crc_init if crc_init is None else crc_init, rules)


@functools.lru_cache(maxsize=None)
def expected(tight=False, crc_init=MAIN_CRC_INIT, full=True):
    """The model's records of the whole lattice, computed once per process."""
    lat = decode_lattice(tight, crc_init, full)
    return tuple(model_record(lat, i) for i in range(len(lat.hits)))


def records_array(recs):
    """Model records -> LE_PKT_DTYPE (zero tail padding), to compare records as bytes."""
    out = np.zeros(len(recs), bt.LE_PKT_DTYPE)
    for i, r in enumerate(recs):
        for k in _le.FIELDS:
            out[k][i] = r[k]
        out["bytes"][i] = np.frombuffer(r["bytes"], np.uint8)
    return out


# ---- the scan lattice --------------------------------------------------------------------------------------------------
TOP_OCTETS = (0x00, 0xFF, 0x55, 0xAA, 0x8E, 0x71, 0x01, 0x80)
SCAN_N_WORDS = 2 * 512 + 3
DENSE_AAS = 4


def scan_aas():
    rng = np.random.default_rng(_libs.seed(7410))
    out = []
    for top in TOP_OCTETS:
        for bit0 in (0, 1):
            out.append((top << 24) | (int(rng.integers(0, 1 << 23)) << 1) | bit0)
    out += [_le.ADV_AA ^ 1, _le.ADV_AA ^ (1 << 8), _le.ADV_AA ^ (1 << 31), CONN_AA]
    assert len(set(out)) == len(out) and _le.ADV_AA not in out
    return out


def _error_sets(rng):
    """(mismatch positions, zones) of the planted patterns: for every count 0..6 the three zones alone, in pairs and all
    three, at least six per count up to five."""
    out = []
    for e in range(7):
        if e == 0:
            out += [((), ())] * 7
            continue
        mixes = [(0,), (1,), (2,)] * (2 if e == 1 else 1)
        if e >= 2:
            mixes += [(0, 1), (1, 2), (0, 2)]
        if e >= 3:
            mixes += [(0, 1, 2)]
        if e == 6:
            mixes = [(0,), (1,), (2,), (0, 1, 2)]
        for zones in mixes:
            split = [1] * len(zones)
            for _ in range(e - len(zones)):
                split[int(rng.integers(0, len(zones)))] += 1
            pos = []
            for z, k in zip(zones, split):
                lo, hi = ZONES[z]
                pos += list(lo + rng.choice(hi - lo, k, replace=False))
            out.append((tuple(sorted(int(p) for p in pos)), zones))
    return out


def _best_dense_mhz(aa):
    """The data MHz at which the back-to-back stream's hits all decode to the shortest PDU (header octet 1 is AA octet 0
    XOR the whitening's second octet: one value for the whole stream)."""
    best = None
    for m in range(2404, 2480, 2):
        if m == 2426:
            continue
        wh = _le.bits_value(_le.whitening_bits(_le.channel_index(m) & 0x3F, 16)[8:])
        L = (aa & 0xFF) ^ wh
        if best is None or L < best[0]:
            best = (L, m)
    return best[1]


@functools.lru_cache(maxsize=None)
def scan_lattice():
    """One ScanCase per access address of scan_aas() (module docstring)."""
    aas = scan_aas()
    dense_for = {aas[0], aas[5], aas[10], CONN_AA}
    assert len(dense_for) == DENSE_AAS and {a & 1 for a in dense_for} == {0, 1}
    cases = []
    n_words = SCAN_N_WORDS
    n_bits = 64 * n_words
    search_bits = n_bits - 39 - 5
    data = [m for m in range(2404, 2480, 2) if m != 2426]
    for i, aa in enumerate(aas):
        rng = np.random.default_rng(_libs.seed(7420 + i))
        pat = _le.pattern_bits(aa)
        mhz = [data[(5 * i + 1) % len(data)], 2402 if i % 2 == 0 else data[(3 * i + 7) % len(data)]]
        crc_init = scan_crc_init(aa)
        syms = [rng.integers(0, 2, n_bits, dtype=np.uint8) for _ in range(2)]
        planted, taken = [], [[], []]

        def plant(s, offset, pos, zones, what, max_payload=8):
            assert all(offset + 40 + 8 <= lo or offset >= hi + 8 for lo, hi in taken[s]), (s, offset, what)
            payload = rng.integers(0, 256, int(rng.integers(0, max_payload + 1)), dtype=np.uint8).tobytes()
            b = packet_bits(aa, mhz[s], int(rng.integers(0, 256)), payload, crc_init)
            b[list(pos)] ^= 1
            keep = min(len(b), n_bits - offset)
            syms[s][offset:offset + keep] = b[:keep]
            taken[s].append((offset, offset + keep))
            planted.append(Planted(s, offset, len(pos), zones, what))

        # seams: lane (128 bits), wave (8192), tile (32768; the second one starts the ragged tile) and the last searched
        # offset, with one pattern just behind it; 0..2 mismatches at the seams
        sets = _error_sets(rng)
        few = [x for x in sets if len(x[0]) <= 2]
        k = 0
        for s in range(2):
            spots = [(128 * (9 + 6 * j + 3 * s) + d, "lane") for j, d in enumerate((-39, -20, -1, 0))]
            spots += [(8192 * w + d, "wave") for w, d in zip((1, 2, 3, 5, 6, 7), (-39, -1, 0, -20, -8, -32))]
            spots += [(32768 + (-39, -1)[s], "tile"), (65536 + (0, -20)[s], "tile")]
            for offset, what in spots:
                pos, zones = few[k % len(few)]
                plant(s, offset, pos, zones, what, max_payload=0 if offset > 65000 else 8)
                k += 1
            plant(s, search_bits - 1 + s, (), (), "last offset" if s == 0 else "behind the last offset")
        # the error sets, laid where nothing else lies
        cur = [300, 300]
        for j, (pos, zones) in enumerate(sets):
            s = j & 1
            while True:
                offset = cur[s] + int(rng.integers(150, 600))
                cur[s] = offset + 200
                if all(offset + 200 <= lo or offset >= hi + 8 for lo, hi in taken[s]):
                    break
            assert offset + 200 < search_bits
            plant(s, offset, pos, zones, "planted")
        adv_packets = []
        if bin(aa ^ _le.ADV_AA).count("1") == 1:        # true advertising packets in the stream of a neighbour AA
            for s in range(2):
                for _ in range(4):
                    while True:
                        offset = cur[s] + int(rng.integers(150, 600))
                        cur[s] = offset + 400
                        if all(offset + 400 <= lo or offset >= hi + 8 for lo, hi in taken[s]):
                            break
                    b = packet_bits(_le.ADV_AA, mhz[s], int(rng.integers(0, 256)), rng.integers(0, 256, 6, dtype=np.uint8).tobytes(),
                                    crc_init)
                    syms[s][offset:offset + len(b)] = b
                    taken[s].append((offset, offset + len(b)))
                    adv_packets.append((s, offset))
        dense = None
        if aa in dense_for:
            dense = 2
            syms.append(np.tile(pat, n_bits // 40 + 1)[:n_bits])
            mhz.append(_best_dense_mhz(aa))
        words = np.stack([_le.pack(x) for x in syms])
        words.flags.writeable = False
        cases.append(ScanCase(aa, words, n_words, search_bits, np.array(mhz, np.uint16), tuple(planted), tuple(adv_packets), dense))
    return tuple(cases)


def scan_crc_init(aa):
    return (aa * 0x9E3779B1 >> 7) & 0xFFFFFF


def window_errors(words_row, offset, aa):
    """The 40 bits at `offset` against preamble + AA: the mismatch count and the zones the mismatches lie in."""
    diff = _le.stream_bits(words_row, len(words_row), offset, 40) ^ _le.pattern_bits(aa)
    return int(diff.sum()), tuple(z for z, (lo, hi) in enumerate(ZONES) if diff[lo:hi].any())


def scan_model(case, max_errors, cache, only=None):
    """match_all filtered by the limit, then decode: the records bt.le_scan returns for the case, in (stream, offset) order
    (only = s: for stream s scanned alone, as stream 0)."""
    out = []
    crc_init = scan_crc_init(case.aa)
    for s in (range(len(case.words)) if only is None else (only,)):
        if ("match", s) not in cache:
            cache[("match", s)] = _le.match_all(case.words[s], case.n_words, case.search_bits, case.aa, 4)
        off, err, _ = cache[("match", s)]
        as_stream = s if only is None else 0
        for o, e in zip(off, err):
            if e > max_errors:
                continue
            key = (s, as_stream, int(o))
            if key not in cache:
                cache[key] = _le.decode(case.words[s], case.n_words, as_stream, int(o), int(e), int(case.mhz[s]), crc_init)
            out.append(cache[key])
    return out
