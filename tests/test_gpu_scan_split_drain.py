"""GPU: the split ring drain of the headline scan (scan_slide_kernel, one-level form).  A trip end that drains the ring only
SENDS the batch's pattern look-ups (drain_issue: slots h and h + 1 of every lane); the trip behind it reads the answers, decodes and pushes the hits
(the drain's second half); a batch still pending when a wave leaves its trip loop is finished by the epilogue, in front of what is left
in the ring.  Every case is compared hit for hit (stream, offset, lap, ac_errors) with the oracle's all-matches loop: the
appended list after sorting, the list of btbbx_scan_ordered_device as it comes, for LSB-first words and BTBBX_FMT_PACKED_MSB.

Geometry: that of test_gpu_scan_drain.py.  A launch is many copies of streams of 761 words (one full tile, one ragged tile of
five words) at a pitch of 764; a workgroup's tiles are all of one kind, and with 512 resident workgroups the number of copies
says how many trips a workgroup makes: 520 copies one, 1040 two, 1560 three (a few workgroups one more).  A wave with thirty or
more planted sync words per tile has sixty ring entries at the end of every trip and sends a batch there."""
import functools
import itertools

import numpy as np
import pytest

import _libs
import libbtbb_amd as bt
from test_gpu_scan_events import FMT_LSB, FMT_MSB, WAVE_WORDS, Case, _word, run_both
from test_gpu_scan_drain import NBITS, NWORDS, PITCH, plant_flipped, plant_many

pytestmark = pytest.mark.gpu

PER_WAVE = 31                      # planted per loaded wave and tile: 62 notes per trip, the drain threshold is 60 (ordered form: 40)


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


def _wave_of(offset):
    return (offset // 64) // WAVE_WORDS


def _load_wave(c, wave, offset, seed, total=PER_WAVE, first_lane=2):
    """single sync words at one offset in consecutive lanes of `wave` (they do not overlap) until it has `total` planted"""
    have = sum(1 for (o, lap) in c.planted if _wave_of(o) == wave)
    lane = first_lane
    while have < total:
        assert lane < WAVE_WORDS - 2
        c.plant(_word(0, wave, lane), (offset,), seed + lane)
        have += 1
        lane += 1


def _silence(c, wave):
    """the words of `wave` as zeros: no window of zeros is within one symbol of a barker code, so nothing there is a candidate"""
    c.sym[_word(0, wave, 0) * 64:(_word(0, wave + 1, 0) + 1) * 64] = 0


IDLE_WAVE = 10


@functools.lru_cache(maxsize=None)
def loaded_stream():
    """Waves 2, 3, 5 and 8 send a batch at every trip end (wave 3 with three sync words that overlap in the word lane 63 of wave 2
    shadows); wave 10 has ONE candidate per tile, so its only batch is the epilogue's; the other waves have the noise's few."""
    c = Case(NWORDS, 16001)
    _silence(c, IDLE_WAVE)
    plant_many(c, _word(0, 3, 0), (3, 34, 63), 5)
    _load_wave(c, 2, 17, 1600)
    _load_wave(c, 3, 40, 1700)
    _load_wave(c, 5, 5, 1800)
    _load_wave(c, 8, 61, 1900)
    c.plant(_word(0, IDLE_WAVE, 20), (9,), 77)
    c.finish()
    assert c.nbits == NBITS
    return c


def _wanted(streams, copies):
    return [(ch,) + h for ch in range(copies) for h in streams[ch % len(streams)].want]


def _run(streams, copies, fmt):
    rows = [streams[ch % len(streams)].words for ch in range(copies)]
    syms = [streams[ch % len(streams)].sym for ch in range(copies)]
    run_both(rows, syms, NWORDS, PITCH, NBITS, fmt, _wanted(streams, copies))


@pytest.mark.parametrize("fmt", [FMT_LSB, FMT_MSB])
@pytest.mark.parametrize("copies", [1040, 520, 1560])
def test_batches_across_trips(copies, fmt):
    """1040 copies, two trips: a batch sent at the end of trip 1 is finished in trip 2, the one sent there by the epilogue; a
    loaded wave has 4 x 31 = 124 hits, so the pending-hit queue flushes inside a drain's second half.  520 copies, one trip: the batch
    is sent at the wave's last trip end and is pending when the loop ends -- the epilogue finishes it, then the ring's rest.
    1560 copies, three trips: the second trip finishes a batch and sends the next one."""
    c = loaded_stream()
    per_wave = {w: sum(1 for (o, lap, e) in c.want if _wave_of(o) == w) for w in (2, 3, 5, 8)}
    assert min(per_wave.values()) >= 30 and 2 * min(per_wave.values()) * (copies // 520) >= 60, per_wave
    if copies == 1040:
        assert 4 * min(per_wave.values()) > 64
    _run([loaded_stream()], copies, fmt)


@pytest.mark.parametrize("fmt", [FMT_LSB, FMT_MSB])
def test_idle_wave_beside_loaded_waves(fmt):
    """A wave with exactly one candidate per tile beside loaded waves never reaches the threshold: no batch of its is pending
    at any trip, which must not be read as a batch of zero entries; its two or four records leave through the epilogue."""
    c = loaded_stream()
    at = _word(0, IDLE_WAVE, 20) * 64 + 9
    assert [(o, e) for (o, lap, e) in c.want if _wave_of(o) == IDLE_WAVE] == [(at, 0)]
    assert not c.sym[_word(0, IDLE_WAVE, 0) * 64:at].any() and not c.sym[at + 64:_word(0, IDLE_WAVE + 1, 0) * 64].any()
    _run([c], 1040, fmt)


# ---- every error pattern class the slots hold ----------------------------------------------------------------------------------

N_ZERO, N_PAIRS = 23, 640          # with the 57 single positions: 720 = 2 streams x 12 waves x 30


@functools.lru_cache(maxsize=None)
def pattern_streams():
    rng = np.random.default_rng(1609)
    all_pairs = list(itertools.combinations(range(57), 2))
    pairs = [(0, 1), (0, 56), (55, 56), (33, 34), (31, 32)]
    for i in rng.permutation(len(all_pairs)):
        if len(pairs) == N_PAIRS:
            break
        if all_pairs[i] not in pairs:
            pairs.append(all_pairs[i])
    flips = [()] * N_ZERO + [(p,) for p in range(57)] + pairs
    assert len(flips) == 720 and len(set(pairs)) == N_PAIRS
    flips = [flips[i] for i in rng.permutation(len(flips))]        # every wave gets all three kinds
    out = []
    for s in range(2):
        c = Case(NWORDS, 16100 + s)
        expect = {}
        for wave in range(12):
            for lane in range(1, 31):
                f = flips.pop()
                lap = int(rng.integers(0, 1 << 24))
                at = plant_flipped(c, _word(0, wave, lane), (wave * 5 + 3) % 64, lap, f)
                c.planted.append((at, lap))
                expect[at] = len(f)
        c.finish()
        found = {o: e for (o, lap, e) in c.want}
        for at, n in expect.items():
            assert found[at] == n, (at, n, found[at])
        out.append(c)
    assert not flips
    return out


@pytest.mark.parametrize("fmt", [FMT_LSB, FMT_MSB])
def test_every_pattern_class(fmt):
    """Thirty planted sync words per wave and tile in all twelve waves of two streams (520 copies each, two trips): all 57
    single-error positions 0 .. 56, 640 distinct pairs of them and 23 words without an error (syndrome zero: no look-up is read).

    The displaced first slot.  The pattern table for two errors has 2^15 slots for 58 + 1653 = 1711 patterns (load 0.052).  A
    pattern does not sit in its first slot when that slot was taken as it was stored: for the k-th pattern stored about
    (k - 1) / 32768, 0.026 on average (clusters only raise it).  That none of the 697 distinct patterns planted here is displaced,
    so that the second half never has to look at its second slot, has a probability of about exp(-697 x 0.026) = 1e-8.  The
    probe that goes on behind the second slot, waiting, needs both slots taken: 0.003 per false candidate, about 0.001 per
    stored pattern -- even odds here; the noise streams of test_gpu_scan.py, with thousands of false candidates, take it."""
    _run(pattern_streams(), 1040, fmt)
