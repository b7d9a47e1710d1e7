"""Captures and expectations for the frames of the LE Coded kernels (no test in here): what libbtbb_amd/csrc/le_coded.h and
le_cfind.h do when a workgroup works more than one tile, when a wave holds more hits than its ring, when the cfind decoder strides
over its pre-records, when the host wrapper's first guess is short, and beyond bit 2^32 of a stream and byte 2^32 of a capture.
tests/test_le_coded_frames_model.py (CPU) shows what the captures hold; tests/test_gpu_le_coded_frames.py runs the kernels on them.

Every expectation is one of the existing models': _le_coded.mismatch_counts / match_all / decode_many, _le_cfind.StreamModel /
pre_records / candidates, _le_ctrack.symbols.  Nothing here is taken from a kernel; the constants below restate the frames'
geometry (tile_scan.h, le_coded.h, le_cfind.h) only to say which inputs reach which branch.

* walk(n_words, cus): thousands of short streams dealt from K distinct contents -- more tiles than workgroups
* dense_*: streams that repeat the preamble's eight symbols -- 1024 hits per wave and tile, 16 pre-records per lane
* far(): two streams of a little more than 2^29 words, zero except for copies of a short capture
* the wrong variants of the expectations: first_trip_only, drop_129th, offsets_32bit, Far.read(byte_bits=32)
"""
import collections
import functools

import numpy as np

import _le
import _le_cfind as f
import _le_coded as c
import _le_ctrack as ct
import _le_discover as d

# ---- the frames' geometry (tile_scan.h tile_grid, le_coded.h, le_cfind.h) ----------------------------------------------
TILE_WORDS = 512
TILE = 64 * TILE_WORDS                     # offsets per tile
WAVE = 8192                                # offsets per wave and tile: 64 lanes of 128
LANE = 128
RING = 128                                 # entries of a wave's ring
FLUSH = 64
SCAN_WGS_PER_CU = 8
DECODE_WGS_PER_CU = 32
DECODE_RECS = 8                            # pre-records per decoder workgroup and trip

PERIOD = np.array(c.FORMAT["preamble"][:8], np.uint8)      # 0 0 1 1 1 1 0 0
DENSE_AA = 0xFFFFFFFF                      # its pattern is 12 mismatches from the periodic stream at every eighth offset
ADV_MHZ = _le.ADV_MHZ
MAX_ERRORS = 16
_rng0 = np.random.default_rng(4242)
AA_A, AA_B = d.good_aa(_rng0), d.good_aa(_rng0)            # two data-channel addresses without offense
INIT_A, INIT_B = 0x2B5C91, 0x00F00D
FLIPS = (0, 0, 3, 16, 0, 17, 9, 0, 2, 20)                  # mismatches planted into a pattern, by the plant's index


def scan_grid(cus, n_tiles):
    return min(n_tiles, SCAN_WGS_PER_CU * cus)


def tiles_per_stream(search_bits):
    return ((search_bits + 63) // 64 + TILE_WORDS - 1) // TILE_WORDS


def decode_grid(cus, pre_cap):
    return min((pre_cap + DECODE_RECS - 1) // DECODE_RECS, DECODE_WGS_PER_CU * cus)


def packet_symbols(s, length):
    return f.BLOCK2 + s * (8 * (length + 5) + 3)


# ---- 1. more tiles than workgroups -------------------------------------------------------------------------------------
# (offset, "packet" or "bare"): a whole coded data packet where one fits the stream behind the offset, the bare 336 symbols where
# only they do.  Dealt to the contents in turn: place i goes to content i mod K.
_PLACES = {
    12: [(o, "packet") for o in (0, 1, 63, 64, 65, 127, 128, 129, 190, 200, 255, 256, 300, 306, 37)] + [(432, "bare"), (432, "bare")],
    1030: [(LANE * 14, "packet"), (LANE * 21 - 336, "packet"), (LANE * 30 - 1, "packet"), (LANE * 40 + 1, "packet"), (LANE * 50 - 100, "packet"),
           (WAVE, "packet"), (WAVE * 2 - 1, "packet"), (WAVE * 3 + 1, "packet"), (WAVE * 5 - 335, "packet"), (WAVE * 6 - 336, "packet"),
           (WAVE - 200, "packet"), (TILE, "packet"), (TILE - 1, "packet"), (TILE + 1, "packet"), (TILE - 335, "packet"), (TILE - 336, "packet"),
           (TILE - 170, "packet"), (2 * TILE - 336, "packet"), (2 * TILE - 335, "packet"),
           (2 * TILE, "bare"), (64 * 1030 - 336, "bare"), (64 * 1030 - 336, "bare"), (2 * TILE + 1, "bare"), (2 * TILE - 170, "bare"),
           (2 * TILE - 1, "bare")],
}
_K = {12: 17, 1030: 19}
PITCH_EXTRA = 7


def content_mhz(k):
    return 2404 + 2 * (k % 11)                                      # data channel index k mod 11


@functools.lru_cache(maxsize=None)
def walk_contents(n_words):
    """K distinct stream contents of n_words words: seeded noise with the places above and, in the long form, two more packets in
    each full tile.  Returns (words (K, n_words), planted)."""
    K = _K[n_words]
    total = 64 * n_words
    mhz = [content_mhz(k) for k in range(K)]
    b = f._Builder(K, n_words, mhz, 9100 + n_words)
    rng = np.random.default_rng(9200 + n_words)
    for i, (o, kind) in enumerate(_PLACES[n_words]):
        k = i % K
        aa, init = ((AA_A, INIT_A), (AA_B, INIT_B))[i & 1]
        flips = rng.choice(c.PATTERN, (0, 3, 16)[i % 3] if kind == "bare" else FLIPS[i % len(FLIPS)], replace=False)
        if kind == "bare":
            b.plant(k, o, aa, init, 2, 1, 0, "bare pattern", flips=flips, symbols=c.pattern_symbols(aa))
            continue
        s, length = ((2, 0), (8, 0), (2, 5), (8, 5), (2, 27), (8, 27))[i % 6] if n_words > 12 else (2, 0)
        if o + packet_symbols(s, length) > total:
            s, length = 2, 0
        assert o + packet_symbols(s, length) <= total, (o, kind)
        b.plant(k, o, aa, init, s, (1, 2, 3, 0x1D, 0x0A)[i % 5], length, "place %d" % o, flips=flips)
    if n_words > 12:
        for k in range(K):
            for tile in (0, 0, 1, 1):
                aa, init = ((AA_A, INIT_A), (AA_B, INIT_B))[int(rng.integers(0, 2))]
                s, length = (2, 8)[int(rng.integers(0, 2))], int(rng.integers(0, 12))
                while True:
                    o = tile * TILE + int(rng.integers(400, TILE - 2000))
                    if b.free(k, o - 8, packet_symbols(s, length) + 16):
                        break
                b.plant(k, o, aa, init, s, 1 + int(rng.integers(0, 3)), length, "fill")
    words = b.words(n_words)
    words.flags.writeable = False
    return words, tuple(b.planted)


@functools.lru_cache(maxsize=None)
def walk_content_models(n_words):
    """Per content, computed once: the mismatch counts of both addresses at every searchable offset, the pre-records and the
    candidates (stream 0, the content's own data channel)."""
    words, _ = walk_contents(n_words)
    search_bits = 64 * n_words - (c.PATTERN - 1)
    out = []
    for k in range(len(words)):
        sym = np.unpackbits(words[k].view(np.uint8), bitorder="little")
        counts = {aa: c.mismatch_counts(sym, aa, search_bits) for aa in (AA_A, AA_B)}
        sm = f.StreamModel(words[k], n_words, content_mhz(k), 0)
        out.append((counts, tuple(f.pre_records(sm, search_bits, MAX_ERRORS)), tuple(f.candidates(sm, search_bits, 255, MAX_ERRORS))))
    return tuple(out)


class Walk:
    """One geometry: n_streams streams of n_words words, pitch above n_words, every stream one of the K contents (a seeded
    permutation of the streams, taken mod K) on the content's data channel or, three times in ten, on an advertising channel."""

    def __init__(self, n_words, cus):
        self.n_words, self.pitch_words, self.cus = n_words, n_words + PITCH_EXTRA, cus
        self.search_bits = 64 * n_words - (c.PATTERN - 1)
        self.tps = tiles_per_stream(self.search_bits)
        full = SCAN_WGS_PER_CU * cus
        self.n_streams = 2 * full + 37 if n_words == 12 else 2 * full // self.tps + 5
        self.n_tiles = self.tps * self.n_streams
        self.grid = scan_grid(cus, self.n_tiles)
        self.K = _K[n_words]
        rng = np.random.default_rng(77 + n_words)
        self.content_of = rng.permutation(self.n_streams) % self.K
        adv = rng.random(self.n_streams) < 0.3
        adv_mhz = np.array(ADV_MHZ)[rng.integers(0, 3, self.n_streams)]
        self.mhz = np.where(adv, adv_mhz, np.array([content_mhz(k) for k in range(self.K)])[self.content_of]).astype(np.uint16)
        self.is_adv = adv

    def words(self):
        contents, _ = walk_contents(self.n_words)
        out = np.random.default_rng(5).integers(0, 1 << 63, (self.n_streams, self.pitch_words), dtype=np.uint64)    # (noise behind every stream)
        out[:, :self.n_words] = contents[self.content_of]
        return out

    def streams_of(self, k):
        return np.nonzero(self.content_of == k)[0]

    def coded_hits(self, aa, limit):
        """sorted (stream, offset, aa, mismatches) of the whole capture"""
        out = []
        for k, (counts, _, _) in enumerate(walk_content_models(self.n_words)):
            offs = np.nonzero(counts[aa] <= limit)[0]
            out += [(int(s), int(o), aa, int(counts[aa][o])) for s in self.streams_of(k) for o in offs]
        return sorted(out)

    def cfind(self):
        """(sorted [(Cand, Info)], sorted pre-records (offset, stream, bound)) of the whole capture"""
        cands, pre = [], []
        for k, (_, p, cd) in enumerate(walk_content_models(self.n_words)):
            for s in self.streams_of(k):
                if not self.is_adv[s]:
                    cands += [(x._replace(stream=int(s)), i) for x, i in cd]
                    pre += [(o, int(s), bound) for o, bound in p]
        return sorted(cands, key=lambda t: (t[0].stream, t[0].offset)), sorted(pre)

    def tile_of(self, stream, offset):
        """the tile's number in the order the workgroups stride over"""
        return stream * self.tps + offset // TILE

    def geometry(self):
        """What the workgroups walk, from grid and tiles_per_stream alone: a dict of the facts the tests assert."""
        g = np.arange(self.n_tiles)
        trips = np.bincount(g % self.grid, minlength=self.grid)             # tiles per workgroup
        nxt = g[g + self.grid < self.n_tiles]                               # tiles that have a successor in their workgroup
        s0, s1 = nxt // self.tps, (nxt + self.grid) // self.tps
        t0, t1 = nxt % self.tps, (nxt + self.grid) % self.tps
        return dict(min_trips=int(trips.min()), max_trips=int(trips.max()), cursor_steps=int((s1 - s0).min()),
                    streams_differ=bool((s1 != s0).all()), tiles_differ=bool((t1 != t0).all()),
                    # (behind its last tile every workgroup's cursor leaves the capture: the fetch with fstream >= n_streams)
                    prefetch_past_the_end=bool((trips >= 1).all()))

    def skip_and_work(self):
        """(workgroups that work an advertising tile and then a data tile that holds a candidate, workgroups the other way round)"""
        cands, _ = self.cfind()
        holds = np.zeros(self.n_tiles, bool)
        for x, _ in cands:
            holds[self.tile_of(x.stream, x.offset)] = True
        g = np.arange(self.n_tiles - self.grid)
        adv = self.is_adv[np.arange(self.n_tiles) // self.tps]
        a = adv[g] & holds[g + self.grid]
        b = holds[g] & adv[g + self.grid]
        return len(set((g[a] % self.grid).tolist())), len(set((g[b] % self.grid).tolist()))


@functools.lru_cache(maxsize=None)
def walk(n_words, cus):
    return Walk(n_words, cus)


def first_trip_only(records, tile_of, grid):
    """Wrong variant: a cursor that stays in its first stream.  Behind its first tile the workgroup asks for tile t + grid of that
    stream, which no stream has (tile_grid keeps grid + tiles_per_stream tiles apart), reads zeros and finds nothing: what is left
    are the records of every workgroup's first tile.  records: tuples (stream, offset, ...)."""
    return [r for r in records if tile_of(r[0], r[1]) < grid]


# ---- 2. dense rings ----------------------------------------------------------------------------------------------------
DENSE_WORDS = 1100
DENSE_SPARSE = ((5003, 0), (2 * WAVE - 100, 0), (TILE - 170, 0), (50001, 3), (64 * DENSE_WORDS - 336, 1))  # AA_B patterns: (offset, flips)
FLIP_P = 0.01


def periodic(n_words, flipped, seed=5):
    sym = np.tile(PERIOD, 8 * n_words)
    if flipped:
        sym ^= (np.random.default_rng(seed).random(len(sym)) < FLIP_P).astype(np.uint8)
    return sym


@functools.lru_cache(maxsize=None)
def dense_stream(flipped):
    """(words, mismatch counts by address) of one stream of DENSE_WORDS words: the periodic content, clean or with every symbol
    flipped with probability 0.01, and a few ordinary patterns of AA_B."""
    sym = periodic(DENSE_WORDS, flipped)
    rng = np.random.default_rng(6)
    for o, k in DENSE_SPARSE:
        sym[o:o + c.PATTERN] = c.flip(c.pattern_symbols(AA_B), rng.choice(c.PATTERN, k, replace=False))
    n = 64 * DENSE_WORDS - (c.PATTERN - 1)
    words = _le.pack(sym)
    words.flags.writeable = False
    return words, {aa: c.mismatch_counts(sym, aa, n) for aa in (DENSE_AA, AA_B)}


def dense_hits(flipped, aa, limit):
    counts = dense_stream(flipped)[1][aa]
    return [(0, int(o), aa, int(counts[o])) for o in np.nonzero(counts <= limit)[0]]


def wave_tile_counts(offsets):
    """hits per wave and tile: a wave works the 8192 offsets of a quarter tile"""
    return np.bincount(np.asarray(offsets, np.int64) // WAVE)


def ring_trace(ballots):
    """The ring's bookkeeping for one wave and tile as le_coded.h states it, given the sizes of the non-empty ballots in order:
    (flushes inside stage, flushes of the drain behind the tile, the largest free-running tail, entries left)."""
    head = tail = in_stage = drain = 0
    for n in ballots:
        assert 0 < n <= 64
        if tail - head + FLUSH > RING:
            head += FLUSH
            in_stage += 1
        tail += n
    top = tail
    while tail - head >= FLUSH:
        head += FLUSH
        drain += 1
    return in_stage, drain, top, tail - head


def lanes_alike(sym, wave_tile):
    """Whether all 64 lanes of a wave read the same symbols (their 128 offsets and the 335 behind them): every ballot of that wave
    is then full or empty, whatever the pre-filter lets through."""
    base = wave_tile * WAVE
    runs = np.stack([sym[base + LANE * k:base + LANE * k + LANE + c.PATTERN - 1] for k in range(64)])
    return bool((runs == runs[0]).all())


def drop_129th(hits):
    """Wrong variant: a ring that drops its 129th entry -- of every wave and tile, in offset order."""
    out, seen = [], collections.Counter()
    for h in sorted(hits):
        key = (h[0], h[1] // WAVE)
        seen[key] += 1
        if seen[key] != RING + 1:
            out.append(h)
    return out


def possible_bases(wave_tiles, cap):
    """Whether `cap` can be the base of a flush under SOME order of the atomics: flushes move 64 records, and a wave's last one what
    is left of its count.  False: cap lies strictly inside a 64-record flush, whatever the order."""
    rest = [int(n) % FLUSH for n in wave_tiles if n % FLUSH]
    full = sum(int(n) // FLUSH for n in wave_tiles)
    sums = {0}
    for r in rest:
        sums |= {s + r for s in sums}
    return any(s <= cap and (cap - s) % FLUSH == 0 and (cap - s) // FLUSH <= full for s in sums)


Dense = collections.namedtuple("Dense", "words n_words pitch_words search_bits mhz model planted")
DENSE_MHZ = 2440
DENSE_CFIND = (2200, 35)                   # (n_words, n_packets) of the capture whose caps fall inside a flush


@functools.lru_cache(maxsize=None)
def dense_cfind(n_words, n_packets):
    """One data-channel stream of the flipped periodic content with n_packets whole coded packets spread evenly over it: both S,
    L in 0, 5, 27, addresses without offense, every one of them a candidate by its making."""
    sym = periodic(n_words, True, seed=8)
    rng = np.random.default_rng(1000 + n_packets)
    total = 64 * n_words
    ch = _le.channel_index(DENSE_MHZ)
    planted = []
    room = packet_symbols(8, 27) + 64
    for i in range(n_packets):
        s, length = (2, 8)[i & 1], (0, 5, 27)[i % 3]
        o = 500 + (total - 500 - room) * i // n_packets + int(rng.integers(0, 64))
        aa, init = d.good_aa(rng, i & 3), int(rng.integers(0, 1 << 24))
        payload = rng.integers(0, 256, length, dtype=np.uint8).tobytes()
        p = c.coded_symbols(aa, ch, bytes([(1, 2, 3)[i % 3], length]) + payload, init, s)
        assert not planted or o > planted[-1][0] + room
        sym[o:o + len(p)] = p
        planted.append((o, aa, init, s, length))
    pitch = n_words + 5
    words = np.full(pitch, np.uint64(0xFFFFFFFFFFFFFFFF))
    words[:n_words] = _le.pack(sym)
    words.flags.writeable = False
    return Dense(words, n_words, pitch, total - (c.PATTERN - 1), DENSE_MHZ, f.StreamModel(words, n_words, DENSE_MHZ, 0), tuple(planted))


@functools.lru_cache(maxsize=None)
def dense_cfind_model(n_words, n_packets):
    """(sorted [(Cand, Info)], sorted pre-records (offset, stream, bound)) at MAX_ERRORS, max_len 255"""
    cap = dense_cfind(n_words, n_packets)
    pre = [(o, 0, b) for o, b in f.pre_records(cap.model, cap.search_bits, MAX_ERRORS)]
    return tuple(f.candidates(cap.model, cap.search_bits, 255, MAX_ERRORS)), tuple(pre)


def stride_words(cus):
    return 2 * DECODE_WGS_PER_CU * cus + 300


# the host wrapper's second pass: 640 words of the flipped content at limit 63.  On the clean stream block 1 decodes an RFU CI at
# every hit (the model says so), and such a hit has no block 2.  The flips turn the CI of a few dozen hits into 0 or 1, and those
# decode a body that the same eight symbols dictate: its second octet, dewhitened, is L, so L depends on the channel alone, and
# decode_many walks 8 (L + 5) + 3 trellis steps for all of them.  SECOND_PASS_MHZ is the channel of the 40 (_le.mhz_of's) on which
# that L is smallest: 2434 MHz, index 14, L = 0 (tests/test_le_coded_frames_model.py derives it).
SECOND_PASS_WORDS = 640
SECOND_PASS_MHZ = 2434


def second_pass_hits():
    w = second_pass_stream()
    return c.match_all(w, len(w), 64 * len(w) - (c.PATTERN - 1), DENSE_AA, c.MAX_ERRORS)


def second_pass_lengths():
    """channel MHz -> the L that most of the hits with a block 2 decode on that channel: one decode on 2402 MHz gives the octet as
    it was sent, each channel's whitening the rest"""
    w = second_pass_stream()
    offs, errs = second_pass_hits()
    res = c.decode_many(w, len(w), 0, offs, errs, 2402, _le.ADV_CRC_INIT)
    common = collections.Counter(pkt["pdu_bytes"] - 2 for pkt, info in res if info["s"]).most_common(1)[0][0]

    def wh(mhz):
        return _le.bits_value(_le.whitening_bits(_le.channel_index(int(mhz)) & 0x3F, 16)[8:16])
    return {int(mhz): common ^ wh(2402) ^ wh(mhz) for mhz in _le.mhz_of(40)}


@functools.lru_cache(maxsize=None)
def second_pass_stream():
    words = _le.pack(periodic(SECOND_PASS_WORDS, True, seed=9))
    words.flags.writeable = False
    return words


# ---- 3. far offsets ----------------------------------------------------------------------------------------------------
PAD_FRONT, PAD_BEHIND = 64, 300            # zero words around R in the short references
BIT32_WORD = 1 << 26                       # bit 2^32 of a stream = word 2^26
BYTE32_WORD = 1 << 29                      # bit 2^35 = byte 2^32 = word 2^29
R_WORDS = 3000
R_BITS = 64 * R_WORDS
FAR_N_WORDS = BYTE32_WORD + 1000
FAR_PITCH = FAR_N_WORDS + 37
FAR_MHZ = (2440, 2404)                     # two data channels
FAR_AAS = (AA_A, DENSE_AA)
CROSS_BIT32 = 64 * 470                     # the bit of R on which bit 2^32 falls in copy B
CROSS_BYTE32 = 64 * (R_WORDS - 1000)       # the bit of R on which bit 2^35 falls in the copies C
Copy = collections.namedtuple("Copy", "name stream base ends")        # base in words; ends: R ends the stream there
COPIES = (Copy("A", 0, PAD_FRONT, False), Copy("B", 1, BIT32_WORD - CROSS_BIT32 // 64, False),
          Copy("C0", 0, FAR_N_WORDS - R_WORDS, True), Copy("C1", 1, FAR_N_WORDS - R_WORDS, True))
FarPlant = collections.namedtuple("FarPlant", "stream offset aa s length flips note")


@functools.lru_cache(maxsize=None)
def far_short():
    """R of both streams (words (2, R_WORDS)) and what was planted: noise with whole coded packets of both S, L in 0, 5, 27, 255, a
    few symbol errors, a burst of the periodic content on either side of bit 2^35, and at the crossings what must cross them."""
    b = f._Builder(2, R_WORDS, FAR_MHZ, 7700)
    rng = np.random.default_rng(7701)
    notes = []

    def put(stream, o, aa, s, length, flips=0, note="", over=False):
        init = INIT_A if aa == AA_A else INIT_B
        fl = rng.choice(packet_symbols(s, length), flips, replace=False)
        if over:                                        # laid over a longer packet's body: the builder would refuse the place
            ch = _le.channel_index(FAR_MHZ[stream])
            p = c.flip(c.coded_symbols(aa, ch, bytes([1, length]) + bytes(length), init, s), fl) if s else c.pattern_symbols(aa)
            b.sym[stream, o:o + len(p)] = p
        else:
            b.plant(stream, o, aa, init, s, (1, 2, 3)[len(notes) % 3], length, note, flips=fl)
        notes.append(FarPlant(stream, o, aa, s, length, flips, note))

    def burst(stream, o, n=704):
        assert o % 8 == 0 and b.free(stream, o, n)
        b.sym[stream, o:o + n] = np.tile(PERIOD, n // 8)
        b.used[stream].append((o, o + n))

    # stream 0
    put(0, 100, AA_A, 2, 0)
    put(0, 3000, AA_A, 8, 27, 3)
    put(0, 8000, AA_B, 2, 255)
    put(0, 20000, AA_A, 8, 255)
    put(0, 40000, AA_A, 2, 27, 5)
    burst(0, 60000)
    put(0, CROSS_BYTE32 - 1000, AA_A, 8, 27, note="across bit 2^35")
    put(0, 131000, AA_A, 2, 0)
    put(0, 133000, AA_B, 8, 0)
    put(0, 136000, AA_A, 2, 27, 2)
    put(0, 140000, AA_A, 2, 255)
    burst(0, 150000)
    put(0, R_BITS - 1500, AA_A, 8, 27, note="the stream ends inside its block 2")
    # stream 1
    put(1, 50, AA_B, 8, 0)
    put(1, 2000, AA_A, 2, 5, 4)
    put(1, 20000, AA_A, 8, 255, note="block 2 across bit 2^32")
    put(1, CROSS_BIT32 - 170, AA_A, 2, 0, note="pattern across bit 2^32", over=True)
    put(1, 45000, AA_A, 2, 27)
    put(1, CROSS_BYTE32 - 100, AA_A, 2, 27, note="across bit 2^35")
    put(1, 130000, AA_A, 8, 5)
    put(1, 133000, AA_B, 2, 0, 1)
    put(1, 137000, AA_A, 2, 255)
    burst(1, 150000)
    put(1, R_BITS - packet_symbols(8, 255), AA_A, 8, 255, note="ends on the stream's last symbol")
    put(1, R_BITS - c.PATTERN, AA_A, 0, 0, note="the last searchable offset", over=True)
    words = b.words(R_WORDS)
    words.flags.writeable = False
    return words, tuple(notes)


class Far:
    """The far capture as the models read it: zero except for the copies.  ref(stream, ends) are the short references; read() is
    the capture itself, sparse."""

    def __init__(self):
        self.R, self.plants = far_short()
        self.n_words, self.pitch_words, self.copies, self.mhz = FAR_N_WORDS, FAR_PITCH, COPIES, np.array(FAR_MHZ, np.uint16)
        self.search_bits = 64 * FAR_N_WORDS - (c.PATTERN - 1)

    def ref(self, stream, ends, front=PAD_FRONT, behind=PAD_BEHIND):
        return np.concatenate([np.zeros(front, np.uint64), self.R[stream], np.zeros(0 if ends else behind, np.uint64)])

    def copies_of(self, stream):
        return [cp for cp in self.copies if cp.stream == stream]

    def read(self, stream, w0, w1, byte_bits=None):
        """Words [w0, w1) of a stream (any w1: what lies behind the stream is part of the buffer).  byte_bits = 32: wrong variant, the
        byte address of every word kept in 32 bits."""
        flat = stream * self.pitch_words + np.arange(w0, w1, dtype=np.int64)
        if byte_bits is not None:
            flat &= (1 << (byte_bits - 3)) - 1
        out = np.zeros(len(flat), np.uint64)
        for cp in self.copies:
            at = cp.stream * self.pitch_words + cp.base
            inside = (flat >= at) & (flat < at + R_WORDS)
            out[inside] = self.R[cp.stream][flat[inside] - at]
        return out

    def __getitem__(self, key):                                              # as _le_ctrack.symbols indexes a capture
        s, sl = key
        return self.read(s, sl.start, sl.stop)

    def moved(self, ref_offset, cp):
        return ref_offset - 64 * PAD_FRONT + 64 * cp.base

    def union(self, model):
        """model(stream, ends) -> tuples that begin with an offset of the short reference.  -> (stream, moved offset, rest...) over
        every copy, in (stream, offset) order."""
        out = []
        for s in (0, 1):
            res = {ends: model(s, ends) for ends in (False, True)}
            for cp in self.copies_of(s):
                out += [(s, self.moved(t[0], cp)) + tuple(t[1:]) for t in res[cp.ends]]
        return sorted(out)


@functools.lru_cache(maxsize=None)
def far():
    return Far()


def ref_coded_hits(words, aa, limit=MAX_ERRORS):
    """[(offset, aa, mismatches)] of one short reference, every searchable offset"""
    offs, errs = c.match_all(words, len(words), 64 * len(words) - (c.PATTERN - 1), aa, limit)
    return [(int(o), aa, int(e)) for o, e in zip(offs, errs)]


@functools.lru_cache(maxsize=None)
def far_coded_hits(aa):
    fr = far()
    return tuple(fr.union(lambda s, ends: ref_coded_hits(fr.ref(s, ends), aa)))


def ref_decode(words, stream, hits, mhz, crc_init=INIT_A):
    """decode_many over [(offset, aa, mismatches)] of one short reference -> [(offset, pkt, info)]"""
    pairs = c.decode_many(words, len(words), stream, [h[0] for h in hits], [h[2] for h in hits], mhz, crc_init)
    return [(h[0], pkt, info) for h, (pkt, info) in zip(hits, pairs)]


@functools.lru_cache(maxsize=None)
def far_decoded():
    """[(stream, offset, pkt, info)] of the far capture's hits of both addresses in (stream, offset) order, pkt["offset"] moved"""
    fr = far()

    def model(s, ends):
        w = fr.ref(s, ends)
        hits = sorted(h for aa in FAR_AAS for h in ref_coded_hits(w, aa))
        return ref_decode(w, s, hits, FAR_MHZ[s])
    out = []
    for s, o, pkt, info in fr.union(model):
        out.append((s, o, dict(pkt, offset=o), info))
    return tuple(out)


def ref_cfind(words, stream, mhz):
    """([(offset, Cand, Info)], [(offset, bound)]) of one short reference"""
    sm = f.StreamModel(words, len(words), mhz, stream)
    n = 64 * len(words) - (c.PATTERN - 1)
    return [(x.offset, x, i) for x, i in f.candidates(sm, n, 255, MAX_ERRORS)], f.pre_records(sm, n, MAX_ERRORS)


@functools.lru_cache(maxsize=None)
def far_cfind():
    """([(Cand, Info)] with moved offsets, [(offset, stream, bound)]) of the far capture, both sorted by (stream, offset)"""
    fr = far()
    res = {(s, ends): ref_cfind(fr.ref(s, ends), s, FAR_MHZ[s]) for s in (0, 1) for ends in (False, True)}
    cands = [(x._replace(offset=o), i) for s, o, x, i in fr.union(lambda s, ends: res[s, ends][0])]
    pre = [(o, s, b) for s, o, b in fr.union(lambda s, ends: res[s, ends][1])]
    return tuple(cands), tuple(pre)


def far_durations(cands):
    fr = far()
    return ct.symbols(fr, fr.n_words, cands, 2)


def offsets_32bit(records, field=1):
    """Wrong variant: a stream offset kept in 32 bits."""
    return sorted(r[:field] + (r[field] & 0xFFFFFFFF,) + r[field + 1:] for r in records)


def far_crossings():
    """name -> True / False for every crossing condition, from the placement table and what was planted."""
    fr = far()
    by = {p.note: p for p in fr.plants if p.note}
    b, c0, c1 = fr.copies[1], fr.copies[2], fr.copies[3]
    x32 = 64 * (BIT32_WORD - b.base)                            # bit 2^32 of stream 1, as a bit of R
    out = {}
    p = by["pattern across bit 2^32"]
    out["B: a packet's 336-symbol pattern straddles bit 2^32"] = p.stream == b.stream and p.offset < x32 < p.offset + c.PATTERN
    p = by["block 2 across bit 2^32"]
    out["B: another packet's block 2 straddles bit 2^32"] = p.stream == b.stream and p.offset + f.BLOCK2 < x32 < p.offset + packet_symbols(p.s, p.length)
    for cp in (c0, c1):
        x35 = 64 * (BYTE32_WORD - cp.base)
        out[cp.name + ": ends the stream across word 2^29"] = cp.ends and cp.base + R_WORDS == fr.n_words and 0 < x35 < R_BITS
        out[cp.name + ": a packet lies across bit 2^35"] = any(q.stream == cp.stream and q.s and q.offset < x35 < q.offset + packet_symbols(q.s, q.length)
                                                             for q in fr.plants)
    p = by["the stream ends inside its block 2"]
    out["C0: the stream ends inside block 2 of an S = 8 packet"] = (p.stream, p.s) == (0, 8) and p.offset + f.BLOCK2 < R_BITS < p.offset + packet_symbols(8, p.length)
    p = by["ends on the stream's last symbol"]
    out["C1: the stream ends on the last symbol of a packet"] = p.stream == 1 and p.offset + packet_symbols(p.s, p.length) == R_BITS
    p = by["the last searchable offset"]
    out["C1: the last searchable offset holds a pattern"] = p.stream == 1 and p.offset == R_BITS - c.PATTERN
    gaps = sorted((cp.stream, cp.base) for cp in fr.copies)
    out["copies lie at least 364 zero words apart"] = all(b2 - (b1 + R_WORDS) >= PAD_FRONT + PAD_BEHIND for (s1, b1), (s2, b2) in zip(gaps, gaps[1:]) if s1 == s2) \
        and all(cp.base >= PAD_FRONT for cp in fr.copies)
    return out
