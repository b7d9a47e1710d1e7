"""GPU: the candidate events of the headline scan (scan_slide_kernel, one-level form).  A pass notes a lane's candidate in a
register and the trip appends the notes to the wave's ring once; a second candidate of a lane that already holds a note, and
candidates the ring has no room for, take the older paths.  Every case plants sync words where one of those paths is taken and
compares the hit lists record for record with the oracle's all-matches loop: the appended list after sorting, the list of
btbbx_scan_ordered_device as it comes, for LSB-first words and for BTBBX_FMT_PACKED_MSB.

Streams are two and three tiles long (a tile is 12 waves x 63 words = 756 words) plus five words, so the last tile is ragged.
A launch that small gives every workgroup ONE tile, so the second tile of a trip stays empty in the numbered cases; the last
test makes more tiles than workgroups out of many short streams and has both tiles of a trip carry candidates.

Sync words that overlap (two in one 64-bit word) are found by solving the overlap over GF(2): a sync word is an affine function
of its LAP's bits."""
import functools

import numpy as np
import pytest

import _libs
import libbtbb_amd as bt
from libbtbb_amd import synth

pytestmark = pytest.mark.gpu

TILE, WAVE_WORDS = 756, 63
LENGTHS = (2 * TILE + 5, 3 * TILE + 5)
FMT_LSB, FMT_MSB = 0, 2


@pytest.fixture(scope="module", autouse=True)
def ready():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    bt.lib().btbbx_shutdown()
    bt.init(2)
    orc = _libs.oracle()
    orc.orc_reset_syndrome_map()
    orc.orc_init(2)
    yield
    bt.lib().btbbx_shutdown()


# ---- overlapping sync words ----------------------------------------------------------------------------------------------

def _affine(msb):
    """syncword(msb << 23 | x) = base ^ XOR of cols[j] over the set bits j of x (x < 2^23)."""
    base = synth.syncword(msb << 23)
    return base, [synth.syncword((msb << 23) | (1 << j)) ^ base for j in range(23)]


def _parity(v):
    return bin(v).count("1") & 1


def _solve(rows, nvar, rng):
    """rows: (mask over the unknowns, right-hand side) of a consistent system over GF(2).  Returns an assignment, its free unknowns
    drawn from rng."""
    pivots = []                                       # (pivot bit, mask, rhs), fully reduced against each other
    for mask, rhs in rows:
        for pb, pm, pr in pivots:
            if mask >> pb & 1:
                mask, rhs = mask ^ pm, rhs ^ pr
        if not mask:
            assert not rhs
            continue
        pb = mask.bit_length() - 1
        pivots = [(b, m ^ mask, r ^ rhs) if m >> pb & 1 else (b, m, r) for b, m, r in pivots] + [(pb, mask, rhs)]
    x = (int(rng.integers(0, 1 << 62)) | (int(rng.integers(0, 1 << 62)) << 62)) & ((1 << nvar) - 1)
    for pb, pm, pr in pivots:
        x &= ~(1 << pb)
    for pb, pm, pr in pivots:
        if _parity(pm & x) ^ pr:
            x |= 1 << pb
    return x


def _fewest_violations(rows, limit=4):
    """Sets of at most `limit` equations (as bit masks over the rows) whose right-hand sides, flipped, make the system consistent,
    fewest first.  The sync word code is cyclic, so the overlap equations of two shifted words have rank 30 however many they
    are: most right-hand sides are contradictory, and which equations to give up is a small decoding problem -- solved by the
    syndromes of the left null space, pairs of equations met in the middle."""
    m = len(rows)
    null, pivots = [], []
    for e, (mask, _) in enumerate(rows):
        combo = 1 << e
        for pb, pm, pc in pivots:
            if mask >> pb & 1:
                mask, combo = mask ^ pm, combo ^ pc
        if mask:
            pivots.append((mask.bit_length() - 1, mask, combo))
        else:
            null.append(combo)
    rhs = sum(r << e for e, (_, r) in enumerate(rows))

    def syn(v):
        return sum(_parity(n & v) << t for t, n in enumerate(null))

    one = [syn(1 << e) for e in range(m)]
    target = syn(rhs)
    upto2 = {0: 0}
    for a in range(m):
        upto2.setdefault(one[a], 1 << a)
    for a in range(m):
        for b in range(a + 1, m):
            upto2.setdefault(one[a] ^ one[b], (1 << a) | (1 << b))
    found = set()
    halves = [0] + [1 << a for a in range(m)] + [(1 << a) | (1 << b) for a in range(m) for b in range(a + 1, m)]
    for h in halves:
        other = upto2.get(target ^ syn(h))
        if other is not None and bin(h ^ other).count("1") <= limit:
            found.add(h ^ other)
    return sorted(found, key=lambda v: bin(v).count("1"))


@functools.lru_cache(maxsize=None)
def overlapped(offsets, seed):
    """Sync words at the given bit offsets (ascending, each overlapping the next, none the one after it) that agree where they
    overlap except for at most two symbols of each, none of them a barker bit.  Returns (laps, symbols from offsets[0] on)."""
    rng = np.random.default_rng(_libs.seed(seed))
    k = len(offsets)
    for msb_all in rng.permutation(1 << k):
        msb = [int(msb_all) >> i & 1 for i in range(k)]
        aff = [_affine(b) for b in msb]
        rows, where = [], []
        for i in range(k - 1):
            delta = offsets[i + 1] - offsets[i]
            assert 0 < delta < 64 and (i + 2 >= k or offsets[i + 2] - offsets[i] >= 64)
            for p in range(64 - delta):               # bit delta + p of word i = bit p of word i + 1
                mask = 0
                for j in range(23):
                    mask |= (aff[i][1][j] >> (delta + p) & 1) << (23 * i + j)
                    mask |= (aff[i + 1][1][j] >> p & 1) << (23 * (i + 1) + j)
                rows.append((mask, (aff[i][0] >> (delta + p) & 1) ^ (aff[i + 1][0] >> p & 1)))
                where.append((i, delta + p, p))
        for given_up in _fewest_violations(rows):
            # a symbol two words disagree on is an error of one of them: of the later word while it has fewer than two
            errors = [0] * k
            later_wins = set()
            ok = True
            for e in range(len(rows)):
                if given_up >> e & 1:
                    i, p_early, p_late = where[e]
                    if errors[i + 1] < 2 and p_late < 57:
                        errors[i + 1] += 1
                    elif errors[i] < 2 and p_early < 57:
                        errors[i] += 1
                        later_wins.add(offsets[i + 1] - offsets[0] + p_late)
                    else:
                        ok = False
            if not ok:
                continue
            x = _solve([(mk, r ^ (given_up >> e & 1)) for e, (mk, r) in enumerate(rows)], 23 * k, rng)
            laps = [(msb[i] << 23) | (x >> (23 * i) & ((1 << 23) - 1)) for i in range(k)]
            span = offsets[-1] - offsets[0] + 64
            sym = np.zeros(span, np.uint8)
            done = np.zeros(span, bool)
            for i in range(k):
                bits = synth.bits_lsb(synth.syncword(laps[i]), 64)
                at = offsets[i] - offsets[0]
                for q in range(64):
                    if not done[at + q] or at + q in later_wins:
                        sym[at + q] = bits[q]
                done[at:at + 64] = True
            for i in range(k):                        # (what the choice above promises)
                at = offsets[i] - offsets[0]
                errs = np.flatnonzero(sym[at:at + 64] != synth.bits_lsb(synth.syncword(laps[i]), 64))
                assert len(errs) <= 2 and (len(errs) == 0 or errs.max() < 57), (offsets, i, errs)
            return tuple(laps), sym
    raise AssertionError("no pair of sync words overlaps at %r with two errors each" % (offsets,))


# ---- the cases -------------------------------------------------------------------------------------------------------------

def _word(tile, wave, lane):
    return tile * TILE + wave * WAVE_WORDS + lane


class Case:
    def __init__(self, nwords, seed):
        self.nwords = nwords
        self.sym = np.ascontiguousarray(synth.unpack_bits(synth.noise_words(_libs.seed(seed), 0, nwords)))
        self.planted = []

    def plant(self, word, offsets, seed):
        """sync words at the given offsets of one word (offsets >= 64: of the words behind it)"""
        if len(offsets) > 1:
            laps, bits = overlapped(tuple(offsets), seed)
        else:
            laps = ((seed * 7919 + 0x4A1B3) & 0xFFFFFF,)
            bits = synth.bits_lsb(synth.syncword(laps[0]), 64)
        at = word * 64 + offsets[0]
        self.sym[at:at + len(bits)] = bits
        self.planted += [(word * 64 + o, lap) for o, lap in zip(offsets, laps)]

    def finish(self):
        self.nbits = self.nwords * 64 - 63
        self.words = synth.pack_bits(self.sym)
        assert len(self.words) == self.nwords
        self.want = _libs.orc_find_all(self.sym, self.nbits, _libs.LAP_ANY, 2, cap=1 << 12)
        assert self.want == sorted(self.want)
        found = {(o, lap) for (o, lap, e) in self.want}
        missing = [p for p in self.planted if p not in found]
        assert not missing, ("planted sync words the oracle does not find", missing)
        return self


@functools.lru_cache(maxsize=None)
def case(name, nwords):
    c = Case(nwords, 700 + len(name) + nwords)
    last_tile = (nwords - 1) // TILE
    if name == "two_chains_of_a_lane":                # (1) offsets 0 and 40 of one word: both halves, two chains of one lane in one trip
        c.plant(_word(1, 3, 17), (0, 40), 11)
    elif name == "one_chain_twice":                   # (2) offsets 3 and 20: one chain in two passes, the second meets the lane's note
        c.plant(_word(1, 5, 9), (3, 20), 12)
        c.plant(_word(0, 7, 44), (35, 59), 13)        # ... and the same in the upper half
    elif name == "four_chains_of_a_lane":             # (3) the same lane of two tiles, both halves of each
        for t in range(last_tile):
            c.plant(_word(t, 2, 30), (0, 40), 14 + t)
    elif name == "wave_and_tile_edges":               # (4) lanes 0 and 62, the word lane 63 shadows, the last word of a tile, the ragged end
        c.plant(_word(0, 0, 0), (7,), 21)
        c.plant(_word(0, 0, 62), (33,), 22)           # (its check bits come from lane 63 = the next wave's first word)
        c.plant(_word(0, 1, 0), (35,), 23)
        c.plant(_word(0, 11, 62), (50,), 24)          # (... from the next tile's first word)
        c.plant(_word(1, 0, 0), (60,), 25)
        c.plant(_word(last_tile, 0, 1), (12, 52), 26)
        c.plant(nwords - 1, (0,), 27)                 # the only offset of the stream's last word that is searched
    elif name == "more_candidates_than_ring":         # (5) every lane's word of one wave, four lanes twice: 67 candidates, a ring of 64
        first = _word(1, 4, 0)
        twice = (5, 20, 33, 50)
        for lane in range(WAVE_WORDS):
            if lane in twice:
                c.plant(first + lane, (0, 40, 64), 30 + lane)
            elif lane - 1 not in twice:
                c.plant(first + lane, (0,), 100 + lane)
    else:
        raise KeyError(name)
    return c.finish()


CASES = ("two_chains_of_a_lane", "one_chain_twice", "four_chains_of_a_lane", "wave_and_tile_edges", "more_candidates_than_ring")


def _tuples(hits):
    return [(int(h["stream"]), int(h["offset"]), int(h["lap"]), int(h["ac_errors"])) for h in hits]


def run_both(rows_lsb, syms, nwords, pitch, nbits, fmt, want):
    """rows: the streams' LSB-first words.  The appended list (sorted) and the ordered list (as it comes) against `want`."""
    lib = bt.lib()
    n_streams = len(rows_lsb)
    if fmt == FMT_MSB:
        rows = [np.packbits(s, bitorder="big").view(np.uint64) for s in syms]
        assert all(len(r) == nwords for r in rows) and not np.array_equal(rows[0], rows_lsb[0])
    else:
        rows = rows_lsb
    buf = np.zeros(n_streams * pitch, np.uint64)
    for ch, r in enumerate(rows):
        buf[ch * pitch:ch * pitch + nwords] = r
    cap = len(want) + 4096
    d_w = bt.DeviceBuffer(buf.nbytes).upload(buf)
    d_h = bt.DeviceBuffer(cap * 16).zero()
    d_c = bt.DeviceBuffer(16).zero()
    sb = lib.btbbx_scan_ordered_scratch_bytes(nbits, n_streams, bt.LAP_ANY, cap)
    assert sb > lib.btbbx_order_hits_scratch_bytes(cap)       # (with the segment slots: the scan kernel's ordered form)
    d_s = bt.DeviceBuffer(sb)
    try:
        bt.check(lib.btbbx_scan_device_fmt(d_w.ptr, nwords, pitch, n_streams, nbits, bt.LAP_ANY, 2, fmt, d_h.ptr, cap, d_c.ptr, None), "scan_fmt")
        bt.check(lib.btbbx_sync(None))
        cnt = int(d_c.download(np.uint32, 4)[0])
        assert cnt == len(want)
        assert sorted(_tuples(d_h.download(bt.HIT_DTYPE, cap)[:cnt])) == want
        d_h.zero()
        bt.check(lib.btbbx_scan_ordered_device_fmt(d_w.ptr, nwords, pitch, n_streams, nbits, bt.LAP_ANY, 2, fmt, d_h.ptr, cap, d_c.ptr,
                                                   d_s.ptr, sb, None), "scan_ordered_fmt")
        bt.check(lib.btbbx_sync(None))
        cnt = int(d_c.download(np.uint32, 4)[0])
        assert cnt == len(want)
        assert _tuples(d_h.download(bt.HIT_DTYPE, cap)[:cnt]) == want
    finally:
        for b in (d_w, d_h, d_c, d_s):
            b.free()


@pytest.mark.parametrize("fmt", [FMT_LSB, FMT_MSB])
@pytest.mark.parametrize("nwords", LENGTHS)
@pytest.mark.parametrize("name", CASES)
def test_candidate_events(name, nwords, fmt):
    c = case(name, nwords)
    if name == "more_candidates_than_ring":
        assert len(c.planted) == 67
    run_both([c.words], [c.sym], nwords, nwords, c.nbits, fmt, [(0,) + h for h in c.want])


@functools.lru_cache(maxsize=None)
def many_short_streams():
    n_streams, nwords = 1040, 70                      # one ragged tile per stream: more tiles than twice the workgroups that are resident
    rows, syms, want = [], [], []
    for ch in range(n_streams):
        c = Case(nwords, 9000 + ch)
        c.plant(10, (0, 40), 40 + ch % 3)             # every tile: lane 10 of wave 0, both halves
        if ch % 5 == 0:
            c.plant(20, (3, 20), 12)                  # ... and a lane whose second candidate meets its note
        c.finish()
        rows.append(c.words)
        syms.append(c.sym)
        want += [(ch,) + h for h in c.want]
    return rows, syms, nwords, want


@pytest.mark.parametrize("fmt", [FMT_LSB, FMT_MSB])
def test_both_tiles_of_a_trip(fmt):
    """More tiles than workgroups: a workgroup then works two tiles per trip, and with the same lane of every tile carrying a sync
    word in both halves, all four chains of that lane hold a candidate in one trip -- one note, three events of the older kind."""
    rows, syms, nwords, want = many_short_streams()
    run_both(rows, syms, nwords, nwords + 2, nwords * 64 - 63, fmt, want)
