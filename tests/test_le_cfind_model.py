"""The model of the promiscuous LE Coded connection discovery (tests/_le_cfind.py) against the transmitter, against itself in
its slow every-offset form, and against deliberately wrong variants on the captures tests/test_gpu_le_cfind.py runs."""
import numpy as np
import pytest

import _le
import _le_coded as c
import _le_discover as d
import _le_cfind as f

# the GPU test's (tight, max_len, max_errors) cases on which the variants are looked for, cheapest first
CASES = ((False, 255, 16), (False, 255, 1), (False, 27, 16), (False, 255, 0))


def test_every_transmitted_packet_is_a_candidate_with_the_sent_address_and_crcinit():
    rng = np.random.default_rng(5)
    mhz = 2440
    ch = _le.channel_index(mhz)
    line, sent, at = [], [], 41
    for s in (2, 8):
        for length in (0, 1, 27, 255):
            aa, init = d.good_aa(rng), int(rng.integers(0, 1 << 24))
            sym = c.coded_symbols(aa, ch, _le.make_pdu(0x02, rng.integers(0, 256, length, dtype=np.uint8).tobytes()), init, s)
            gap = rng.integers(0, 2, at - sum(len(x) for x in line), dtype=np.uint8)
            line += [gap, sym]
            sent.append((at, aa, init, s, length, len(sym)))
            at += len(sym) + int(rng.integers(1, 99))
    sym = np.concatenate(line)
    sym = np.concatenate([sym, np.zeros(-len(sym) % 64, np.uint8)])
    words = _le.pack(sym)
    sm = f.StreamModel(words, len(words), mhz)
    for limit in (0, 16):
        got = {cand.offset: (cand, info) for cand, info in f.candidates(sm, 64 * len(words) - 335, 255, limit)}
        for o, aa, init, s, length, n in sent:
            cand, info = got[o]
            assert (cand.access_address, cand.crc_init, cand.header0, cand.length, cand.channel) == (aa, init, 0x02, length, ch)
            assert info == f.Info(n, 0, 0, 0, {8: 0, 2: 1}[s], s)
    short = {cand.offset for cand, _ in f.candidates(sm, 64 * len(words) - 335, 26, 0)}                    # max_len 26: lengths 0 and 1 only
    assert short & {o for o, *_ in sent} == {o for o, _, _, _, length, _ in sent if length <= 26}
    assert not f.candidates(f.StreamModel(words, len(words), 2402), 64 * len(words) - 335, 255, 16)         # an advertising channel


def test_backward_crc_agrees_with_the_forward_crc_for_every_length():
    rng = np.random.default_rng(6)
    for length in range(256):
        bits = _le.octet_bits(_le.make_pdu(int(rng.integers(0, 256)), rng.integers(0, 256, length, dtype=np.uint8).tobytes()))
        init = int(rng.integers(0, 1 << 24)) if length else 0xABCDEF
        assert d.crc24_backward(bits, _le.crc24_tx_bits(bits, init)) == init, length


def test_the_scans_second_condition_never_exceeds_rule_4s_count():
    """On planted windows (clean and with errors) and on random ones: whatever address block 1 decodes to.  And the pre-record
    list holds every offset that rule 4 passes."""
    cap = f.lattice(False)
    rng = np.random.default_rng(8)
    for s in f.DATA_STREAMS:
        sm = cap.model(s)
        offs = sorted({p.offset for p in cap.planted if p.stream == s and p.offset < cap.search_bits} |
                      set(rng.integers(0, cap.search_bits, 300).tolist()))
        b1 = sm.block1(offs)
        tight = 0
        for o in offs:
            bound = f.second_condition(sm.sym, o)
            assert bound <= b1[o][3], (s, o)
            tight += bound == b1[o][3]
        assert tight > 10                                                               # (a clean packet: both are what the preamble and the pairs show)
        for limit in (16, 63):
            pre = dict(f.pre_records(sm, cap.search_bits, limit))
            assert all(pre[o] == f.second_condition(sm.sym, o) for o in list(pre)[:50])
            assert {cand.offset for cand, _ in f.candidates(sm, cap.search_bits, 255, limit)} <= set(pre)


def test_the_model_equals_the_one_that_decodes_every_offset():
    """One stream of 64 words, planted packets and noise: the preamble bound skips nothing that the every-offset model keeps, and the
    table-driven block 1 and count equal _le_coded's decoder and a literal comparison with pattern_symbols(AA')."""
    rng = np.random.default_rng(9)
    mhz = 2478
    ch = _le.channel_index(mhz)
    sym = rng.integers(0, 2, 64 * 64, dtype=np.uint8)
    sent = []
    for o, s, length, flips in ((30, 2, 0, ()), (600, 8, 1, (3, 90, 200, 335)), (1500, 2, 27, (70, 71, 72, 100, 333)), (2500, 8, 3, ()),
                                (3700, 2, 0, ())):
        aa, init = d.good_aa(rng), int(rng.integers(0, 1 << 24))
        p = c.flip(c.coded_symbols(aa, ch, _le.make_pdu(0x01, bytes(length)), init, s), flips)
        k = min(len(p), len(sym) - o)
        sym[o:o + k] = p[:k]
        sent.append((o, aa, init))
    words = _le.pack(sym)
    sm = f.StreamModel(words, 64, mhz)
    search_bits = 64 * 64 - 335
    for max_len, limit in ((255, 63), (27, 16), (255, 4)):
        fast = f.candidates(sm, search_bits, max_len, limit)
        slow = f.candidates(f.StreamModel(words, 64, mhz), search_bits, max_len, limit, every_offset=True)
        assert fast == slow and len(fast) >= 3
    found = {cand.offset: cand for cand, _ in f.candidates(sm, search_bits, 255, 16)}
    for o, aa, init in sent[:4]:
        assert (found[o].access_address, found[o].crc_init) == (aa, init)
    assert 3700 not in found                                                            # it ends past the stream


def test_the_lattice_holds_what_it_was_built_for():
    cap = f.lattice(False)
    got = {(cand.stream, cand.offset): (cand, info) for cand, info in f.lattice_model(False, 255, 16)}
    notes = {p.note: p for p in cap.planted}
    for p in cap.planted:
        if not p.flips and p.note != "header hit":
            hit = got.get((p.stream, p.offset))
            assert (hit is not None) == f.plant_expected(cap, p, 255, 16), p
            if hit is not None:
                assert (hit[0].access_address, hit[0].crc_init, hit[0].header0, hit[0].length, hit[1].s) == (p.aa, p.crc_init, p.header0, p.length, p.s), p
    for note in ("header hit", "ends one symbol past the stream", "at search_bits", "advertising channel", "ci 2", "ci 3", "LLID 0", "RFU bit 5",
                 "one offense: run_window", "64 errors: preamble"):
        assert note in notes and (notes[note].stream, notes[note].offset) not in got, note
    last = next(p for p in f.lattice(True).planted if p.note == "ends on the last symbol")               # (below search_bits in the tight form only)
    assert last.offset + f.BLOCK2 + 2 * 51 == 64 * f.N_WORDS and (last.stream, last.offset) in {(x.stream, x.offset) for x, _ in f.lattice_model(True, 255, 16)}
    for note in ("at search_bits - 1", "every allowed bit", "S 8 length 255", "S 2 length 255", "16 errors: preamble",
                 "16 errors: one of a pair", "16 errors: both of a pair"):
        assert (notes[note].stream, notes[note].offset) in got, note
    assert {p.offset % 64 for p in cap.planted if p.stream == 0} == set(range(64))
    # errors that make block 1 decode another address than the one sent: the model keeps some as candidates of that other address
    other = [p for p in cap.planted if p.flips and (p.stream, p.offset) in got and got[(p.stream, p.offset)][0].access_address != p.aa]
    assert other
    # every limit is met from both sides with the address sent
    planted = {(p.stream, p.offset): p for p in cap.planted}
    by_errors = {info.errors for cand, info in f.lattice_model(False, 255, 63)
                 if (cand.stream, cand.offset) in planted and planted[(cand.stream, cand.offset)].aa == cand.access_address}
    assert {0, 1, 2, 15, 16, 17, 62, 63} <= by_errors and max(by_errors) == 63


@pytest.mark.parametrize("name", sorted(f.VARIANTS))
def test_every_wrong_variant_differs_from_the_model_on_the_gpu_tests_inputs(name):
    kw = f.VARIANTS[name]
    if name == "given_aa":
        kw = dict(given_aa=f.lattice(False).planted[0].aa)
    rules = f.Rules(**kw)
    for tight, max_len, limit in CASES:
        if list(f.lattice(tight).candidates(max_len, limit, rules)) != list(f.lattice_model(tight, max_len, limit)):
            return
    raise AssertionError("the captures do not tell %s from the model" % name)
