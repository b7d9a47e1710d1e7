"""CPU: what tests/test_gpu_far_offsets.py rests on.  All-zero words are quiet for every model used there; the far capture of
tests/_far.py puts what must cross bit 2^32 and bit 2^35 across them; and the models themselves are translation invariant --
S at two different small bases gives the same result moved, so they may serve as the yardstick at a base of 2^26 or 2^29 words."""
import numpy as np
import pytest

import _far
import _follow as fw
import _le
import _le_discover as ld
import _libs
import _survey
import libbtbb_amd as bt
from libbtbb_amd import synth

ZERO_WORDS = 1024


@pytest.fixture(scope="module")
def orc():
    o = _libs.oracle()
    o.orc_reset_syndrome_map()
    o.orc_init(2)
    yield o
    o.orc_reset_syndrome_map()
    o.orc_init(2)


@pytest.mark.parametrize("n_init", [2, 3, 5])
def test_zeros_hold_no_access_code(orc, n_init):
    sym = np.zeros(64 * ZERO_WORDS, np.uint8)
    n = len(sym) - 63
    try:
        orc.orc_reset_syndrome_map()
        assert orc.orc_init(n_init) == 0
        for me in range(0, 7):
            assert _libs.orc_find_all(sym, n, _libs.LAP_ANY, me) == [], (n_init, me)
        for lap in (0x9E8B33, 0x1E8B33, 0x000000, 0xFFFFFF):
            ones = bin(synth.syncword(lap)).count("1")
            assert 20 <= ones <= 44, (hex(lap), ones)
            for me in range(0, 10):
                assert _libs.orc_find_all(sym, n, lap, me) == [], (n_init, hex(lap), me)
    finally:
        orc.orc_reset_syndrome_map()
        orc.orc_init(2)


def test_zeros_hold_no_le_packet():
    w = np.zeros(ZERO_WORDS, np.uint64)
    assert ld.candidates(w, len(w), 64 * len(w) - 39, 2440, 255) == []
    off, err, aa = _le.match_all(w, len(w), 64 * len(w) - 39, _le.ADV_AA, 4)
    assert len(off) == 0


def test_byte_wise_bit_reversal_is_its_own_inverse():
    """btbbx_msb_to_lsb_device reverses the bits of every byte: applied twice it restores the capture, so the far capture can be
    turned round in place for the MSB-first scans and turned back."""
    sym = _far.far().S[0][:64 * 200]
    lsb = np.packbits(sym, bitorder="little")
    msb = np.packbits(sym, bitorder="big")
    rev = np.array([int("{:08b}".format(b)[::-1], 2) for b in range(256)], np.uint8)
    assert np.array_equal(rev[lsb], msb) and np.array_equal(rev[msb], lsb) and np.array_equal(rev[rev], np.arange(256))


def test_placement():
    f = _far.far()
    assert f.n_words > _far.BYTE32_WORD and f.pitch_words > f.n_words and (f.pitch_words - f.n_words) % 2 == 1
    assert not np.array_equal(f.words[0][:1000], f.words[1][:1000])
    for s in (0, 1):
        cs = sorted(_far.copies_of(s), key=lambda c: c.base)
        W = len(f.words[s])
        assert [c.ends for c in cs] == [False] * (len(cs) - 1) + [True]
        for a, b in zip(cs, cs[1:]):
            assert a.base + W + 64 <= b.base
        assert cs[-1].base + W == f.n_words
        for c in cs:
            assert c.base >= 64 and (c.name == "A0" or c.base % _far.SLOT == 0)
        b, c = [x for x in cs if x.name[0] == "B"][0], cs[-1]
        assert b.base < _far.BIT32_WORD < b.base + W and c.base < _far.BYTE32_WORD < c.base + W
    bases = [c.base % (1 << 20) for c in f.copies]
    assert len(set(bases)) == len(bases)


def test_crossing_conditions(orc):
    got = _far.crossings()
    assert len(got) == 13 and all(got.values()), [k for k, v in got.items() if not v]


def test_short_capture_holds_what_the_issue_lists(orc):
    f = _far.far()
    kinds = [[p.kind for p in pl] for pl in f.plants]
    le = [p for p in f.plants[0] if p.kind == "le"]
    assert {p.meta["length"] for p in le} >= {0, 27, 255} and len({p.offset % 64 for p in le}) >= 16
    assert all(sum(p.meta["conn"] == c for p in le) >= 3 for c in (0, 1))
    assert kinds[1].count("le_adv") >= 6 and kinds[1].count("survey") == 1 and kinds[0].count("survey") == 0
    names = {f.lat.tags[i][0] for _, i in _far.br_hits(0)}
    assert len(names) == 17
    for s in (0, 1):                                     # ... and packets whose capture the end of S cuts
        total = len(f.S[s])
        assert sum(o + synth.MAX_SYMBOLS > total for o, _ in _far.br_hits(s)) >= 2
        assert kinds[s].count("sync") >= 40
        for lap in (synth.LAP_ANY,) + _far.KNOWN_LAPS:
            errs = {e for _, _, e in _far.find_all(s, False, lap, 2)}
            assert errs == {0, 1, 2}, (s, hex(lap), errs)


def _at(stream, base):
    w = _far.far().words[stream]
    return np.concatenate([np.zeros(base, np.uint64), w, np.zeros(64, np.uint64)])


BASES = (64, 64 + 625 + 38)


@pytest.mark.parametrize("stream", [0, 1])
def test_models_are_translation_invariant(orc, stream):
    """S at two small bases (38 words more: another word phase of every tile and wave; 625 more: another slot)."""
    res = []
    for base in BASES:
        w = _at(stream, base)
        sym = np.ascontiguousarray(synth.unpack_bits(w))
        finds = tuple(tuple((o - 64 * base, lap_, e) for o, lap_, e in _libs.orc_find_all(sym, len(sym) - 63, lap, 2))
                      for lap in (_libs.LAP_ANY,) + _far.KNOWN_LAPS)
        cands = [c._replace(offset=c.offset - 64 * base) for c in ld.candidates(w, len(w), 64 * len(w) - 39, _far.MHZ[stream], 255, stream)]
        off, err, aa = _le.match_all(w, len(w), 64 * len(w) - 39, _le.ADV_AA, _far.LE_SCAN_ERRORS)
        decoded = [_le.decode(w, len(w), stream, int(o), int(e), _far.MHZ[stream], _le.ADV_CRC_INIT) for o, e in zip(off, err)]
        for d in decoded:
            d["offset"] -= 64 * base
        res.append((finds, cands, ld.group(cands, 2), (off - np.uint64(64 * base)).tolist(), err.tolist(), aa.tolist(), decoded))
    assert res[0] == res[1]
    assert len(res[0][0][0]) > 40 and (len(res[0][1]) > 20) == (stream == 0) and (len(res[0][3]) >= 8) == (stream == 1)
    # the short references are S at base 64
    assert tuple((o + 64 * 64, l, e) for o, l, e in res[0][0][0]) == _far.find_all(stream, False, synth.LAP_ANY, 2)


def survey_expected(base, clkn_far, clk_phase):
    """_survey.expected on S1 at `base` words, for the hits of capture_single moved to it; the clock of the first bit of the
    stream is clkn_far.  Returns (records with first_offset relative to S, candidates)."""
    cap, _ = _survey.capture_single()
    sp = _far.survey_plant()
    w = _at(1, base)

    class Line:
        sym = [np.ascontiguousarray(synth.unpack_bits(w))]
        channels, clk_div = None, 625
    hits = cap.hits().copy()
    hits["offset"] += 64 * base + sp.offset
    recs, cands = _survey.expected(_survey.OracleEngine(), Line, hits, clkn_far, clk_phase)
    # the follow's model over these records, no clock job stored: stages 0 and 1, every packet's clock from its offset
    none = np.zeros(0, np.uint32)
    pin, fol, _ = fw.model(hits, recs, none, np.zeros(0, bt.CLOCK_RESULT_DTYPE), np.zeros(0, bt.CLOCK_JOB_DTYPE), None, 1,
                           _survey.entry_state(clkn_far), 625, clk_phase, None)
    recs["first_offset"] -= 64 * base
    return recs, cands, pin, fol


def test_survey_and_follow_models_are_translation_invariant(orc):
    """The survey's clock is clkn + (offset + phase) / 625: moving the capture by a whole number of slots (625 words = 64 slots
    ... of 625 symbols: 64 * 625 bits) and the clock back by as many leaves every record as it was."""
    a, ca, pin_a, fol_a = survey_expected(625, *_far.survey_clock(625))
    b, cb, pin_b, fol_b = survey_expected(2 * 625, *_far.survey_clock(2 * 625))
    assert _far.survey_clock(625)[1] == _far.survey_clock(2 * 625)[1] != 0
    _survey.assert_records_equal(a, ca, b, cb)
    assert (a["settled_by"] == 2).sum() >= 3 and (a["settled_by"] == 1).sum() >= 1
    assert pin_a["clkn"].tolist() == pin_b["clkn"].tolist() and pin_a.tobytes() == pin_b.tobytes() and fol_a.tobytes() == fol_b.tobytes()
    assert (fol_a["stage"] == 1).sum() >= 20 and (fol_a["stage"] == 0).sum() >= 20
