"""GPU: the ring drains of the headline scan (scan_slide_kernel, one-level form): record read and window cut, the exact rule in its
form for tables of two errors or fewer, the pending-hit queue and its flush inside a drain, and the paths a lane's second and
third candidate take.  Every case is compared hit for hit (stream, offset, lap, ac_errors) with the oracle's all-matches loop:
the appended list after sorting, the list of btbbx_scan_ordered_device as it comes, for LSB-first words and BTBBX_FMT_PACKED_MSB.

Geometry.  A launch of one short stream gives every workgroup a single tile, so the second tile of a trip stays empty and the
ring is only ever drained behind the last trip.  Here a launch is MANY COPIES of one stream of 761 words -- a full tile (12 waves
x 63 words) and a ragged one of five words -- at a pitch larger than the length: more tiles than four times the workgroups a
device of 256 CUs keeps resident, every one of a workgroup's tiles of the same kind (its tiles are an even number apart), so both
tiles of a trip carry the planted words, and a wave with thirty or more candidates per tile reaches the drain threshold (60
ring entries) at the end of its first trip.  The oracle runs once per distinct stream; a copy's hits are the same with its
stream number.

Three sync words that start in one 64-bit word exist only far apart (two errors each leave about 2^(last - first - 6) solutions);
the solver below finds them for offsets about thirty apart, which puts two of them in one half of the word."""
import functools
import inspect

import numpy as np
import pytest

import _libs
import libbtbb_amd as bt
from libbtbb_amd import synth
import test_gpu_scan_events as ev
from test_gpu_scan_events import FMT_LSB, FMT_MSB, TILE, WAVE_WORDS, Case, _tuples, _word, run_both

pytestmark = pytest.mark.gpu

NWORDS = TILE + 5                  # tile 0 full (its two halo words are in range), tile 1 ragged: five words
N_STREAMS = 1040                   # 2080 tiles: four per workgroup at 2 x 256 resident workgroups
PITCH = NWORDS + 3
NBITS = NWORDS * 64 - 63


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


# ---- three sync words that all overlap ---------------------------------------------------------------------------------------

def _overlapped_any():
    """test_gpu_scan_events.overlapped without its rule that word i + 2 starts behind word i: a choice of given-up equations whose
    symbols do not come out within two errors of every word is passed over instead of being asserted."""
    src = inspect.getsource(ev.overlapped.__wrapped__)
    for old, new in (
            ("def overlapped(", "def overlapped_any("),
            ("assert 0 < delta < 64 and (i + 2 >= k or offsets[i + 2] - offsets[i] >= 64)", "assert 0 < delta < 64"),
            ("            for i in range(k):                        # (what the choice above promises)",
             "            bad = False\n            for i in range(k):"),
            ("assert len(errs) <= 2 and (len(errs) == 0 or errs.max() < 57), (offsets, i, errs)",
             "bad = bad or not (len(errs) <= 2 and (len(errs) == 0 or errs.max() < 57))"),
            ("            return tuple(laps), sym", "            if bad:\n                continue\n            return tuple(laps), sym")):
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    ns = dict(vars(ev))
    exec(src, ns)
    return functools.lru_cache(maxsize=None)(ns["overlapped_any"])


overlapped_any = _overlapped_any()


def plant_many(c, word, offsets, seed):
    """sync words at the given offsets of one word, all of them overlapping"""
    laps, bits = overlapped_any(tuple(offsets), seed)
    at = word * 64 + offsets[0]
    c.sym[at:at + len(bits)] = bits
    c.planted += [(word * 64 + o, lap) for o, lap in zip(offsets, laps)]


def plant_flipped(c, word, offset, lap, flips):
    """the sync word of `lap` with the symbols `flips` (positions in the word, LSB = first symbol) inverted"""
    bits = np.array(synth.bits_lsb(synth.syncword(lap), 64), np.uint8)
    for f in flips:
        bits[f] ^= 1
    at = word * 64 + offset
    c.sym[at:at + 64] = bits
    return at


# ---- the streams -------------------------------------------------------------------------------------------------------------

LAP_CLASS0, LAP_CLASS1 = 0x1E8B33, 0x9E8B33            # bit 23 picks the barker code of the sync word's last seven symbols


def _fill_wave(c, wave, used, offset, total, seed):
    """single sync words at one offset (so that they do not overlap) in lanes of `wave` away from the `used` ones, until the wave
    has `total` planted candidates per tile: about thirty make sixty ring entries per trip -- the drain threshold at the end of
    a trip; the set's false positives in the noise (two per wave and tile) put some trips a little beyond the ring's 64 as well"""
    have = sum(1 for (o, lap) in c.planted if (o // 64) // WAVE_WORDS == wave)
    lane = 2
    while have < total:
        assert lane < WAVE_WORDS - 2
        if all(abs(lane - u) > 1 for u in used):
            c.plant(_word(0, wave, lane), (offset,), seed + lane)
            have += 1
        lane += 1


@functools.lru_cache(maxsize=None)
def stream(name):
    c = Case(NWORDS, 8100 + len(name))
    c.expect_errors, c.absent = {}, []
    if name == "pairs":                       # two sync words that start in one word: lanes 0, 31, 62 and the word lane 63 shadows
        c.plant(_word(0, 2, 0), (3, 20), 12)              # one half, the lower one: the second meets the lane's note in a later pass
        c.plant(_word(0, 2, 31), (35, 59), 13)            # one half, the upper one
        c.plant(_word(0, 3, 0), (5, 45), 14)              # both halves; wave 2's lane 63 works on this word too and owns none of its offsets
        c.plant(_word(0, 4, 62), (0, 40), 11)             # both halves (its check bits behind offset 31 come from lane 63)
        _fill_wave(c, 2, (0, 31), 17, 30, 300)
        _fill_wave(c, 3, (0,), 40, 30, 400)
        _fill_wave(c, 4, (62,), 5, 31, 500)
    elif name == "triples":                   # three: the second note, the third candidate's fall-back, the order of a lane's records
        plant_many(c, _word(0, 2, 0), (0, 29, 60), 5)     # lower, lower, upper half
        plant_many(c, _word(0, 2, 31), (2, 33, 62), 5)    # lower, upper, upper
        plant_many(c, _word(0, 3, 0), (3, 34, 63), 5)     # the shadowed word
        plant_many(c, _word(0, 4, 62), (1, 31, 63), 5)    # lane 62
        _fill_wave(c, 2, (0, 31), 17, 30, 600)
        _fill_wave(c, 3, (0,), 40, 30, 700)
        _fill_wave(c, 4, (62,), 5, 31, 800)
    elif name == "errors":                    # 0, 1 and 2 errors, in the barker symbols, in symbol 0; three errors are no hit
        for k, lap in enumerate((LAP_CLASS0, LAP_CLASS1)):
            lane = 1
            for flips in ((), (0,), (33,), (56,), (0, 56), (10, 47), (0, 1), (34, 35)):
                at = plant_flipped(c, _word(0, 5 + 2 * k, lane), (lane * 11) % 64, lap, flips)
                c.planted.append((at, lap))
                c.expect_errors[at] = len(flips)
                lane += 2
            for flips in ((58,), (60,), (63,), (57,), (61, 62), (59, 20), (63, 0, 30)):        # symbols 57 .. 63: LAP bit 23 and the barker code
                plant_flipped(c, _word(0, 5 + 2 * k, lane), (lane * 11) % 64, lap, flips)      # (the oracle says what these are)
                lane += 2
            assert lane == 31
            for j in range(15):                                                                # thirty per tile: a drain at the trip's end
                c.plant(_word(0, 5 + 2 * k, 33 + j), (17,), 900 + 20 * k + j)
            lane = 1
            for flips in ((0, 1, 2), (5, 30, 56), (12, 33, 34)):
                c.absent.append(plant_flipped(c, _word(0, 6 + 2 * k, lane), (lane * 11) % 64, lap, flips))
                lane += 2
    elif name == "back_to_back":              # 2^14 symbols of sync words: four waves whose every lane holds a candidate in both tiles of a
        for w in range(256):                  # trip -- 126 notes for a ring of 64 -- and more than 128 hits per wave: flushes inside drains
            c.plant(w, (0,), w)
    elif name == "ragged_end":                # the last offset that is searched holds a hit; a sync word the stream's end cuts is none
        c.plant(NWORDS - 1, (0,), 27)
        c.plant(TILE - 1, (50,), 24)                       # (the full tile's last word: its window ends in the ragged tile)
        c.plant(TILE + 1, (12, 52), 26)                    # the ragged tile
    else:
        raise KeyError(name)
    c.finish()
    assert c.nbits == NBITS
    found = {o: e for (o, lap, e) in c.want}
    for at, n in c.expect_errors.items():
        assert found[at] == n, (at, n, found[at])
    for at in c.absent:
        assert at not in found, at
    return c


STREAMS = ("pairs", "triples", "errors", "back_to_back", "ragged_end")


@functools.lru_cache(maxsize=None)
def wanted(name):
    c = stream(name)
    return [(ch,) + h for ch in range(N_STREAMS) for h in c.want]


@pytest.mark.parametrize("fmt", [FMT_LSB, FMT_MSB])
@pytest.mark.parametrize("name", STREAMS)
def test_drains(name, fmt):
    c = stream(name)
    if name == "back_to_back":
        assert len(c.want) >= 256
    if name == "triples":
        assert len(c.planted) >= 12 + 60
    run_both([c.words] * N_STREAMS, [c.sym] * N_STREAMS, NWORDS, PITCH, NBITS, fmt, wanted(name))


@pytest.mark.parametrize("fmt", [FMT_LSB, FMT_MSB])
def test_cut_sync_word(fmt):
    """A sync word whose last symbol lies behind the stream's end -- and is a zero, as the padding behind the stream is: the 63
    symbols that are there and the padding make a whole sync word at an offset that is not searched."""
    for lap in (LAP_CLASS0, LAP_CLASS1):
        bits = synth.bits_lsb(synth.syncword(lap), 64)
        if bits[63] == 0:
            break
    else:
        raise AssertionError("no sync word ends in a zero")
    c = Case(NWORDS, 8200)
    at = (NWORDS - 1) * 64 + 1
    c.sym[at:] = bits[:63]
    c.plant(NWORDS - 1 - 4, (9,), 31)
    c.finish()
    assert all(o < NBITS for (o, lap, e) in c.want)
    whole = np.concatenate([c.sym, np.zeros(64, np.uint8)])
    assert (at, lap) in {(o, lp) for (o, lp, e) in _libs.orc_find_all(whole, NBITS + 64, _libs.LAP_ANY, 2, cap=1 << 12)}
    n = 64
    run_both([c.words] * n, [c.sym] * n, NWORDS, PITCH, NBITS, fmt, [(ch,) + h for ch in range(n) for h in c.want])


@pytest.mark.parametrize("fmt", [FMT_LSB, FMT_MSB])
def test_hit_buffer_smaller_than_count(fmt):
    """Waves with more than 128 hits flush their pending records inside drains; with a buffer of `cap` records the count is still
    exact and exactly `cap` records are written, every one a hit of the list and none twice."""
    lib = bt.lib()
    c = stream("back_to_back")
    want = set(wanted("back_to_back"))
    row = c.words if fmt == FMT_LSB else np.packbits(c.sym, bitorder="big").view(np.uint64)
    buf = np.zeros(N_STREAMS * PITCH, np.uint64)
    for ch in range(N_STREAMS):
        buf[ch * PITCH:ch * PITCH + NWORDS] = row
    cap = 100003
    assert cap < len(want)
    d_w = bt.DeviceBuffer(buf.nbytes).upload(buf)
    d_h = bt.DeviceBuffer((cap + 64) * 16).zero()
    d_c = bt.DeviceBuffer(16).zero()
    try:
        bt.check(lib.btbbx_scan_device_fmt(d_w.ptr, NWORDS, PITCH, N_STREAMS, NBITS, bt.LAP_ANY, 2, fmt, d_h.ptr, cap, d_c.ptr, None), "scan_fmt")
        bt.check(lib.btbbx_sync(None))
        assert int(d_c.download(np.uint32, 4)[0]) == len(want)
        recs = d_h.download(bt.HIT_DTYPE, cap + 64)
        got = _tuples(recs[:cap])
        assert len(set(got)) == cap and set(got) <= want
        assert not recs[cap:].view(np.uint8).any()             # nothing behind the buffer's end
    finally:
        for b in (d_w, d_h, d_c):
            b.free()
