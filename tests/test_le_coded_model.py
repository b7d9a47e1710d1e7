"""The LE Coded PHY model (tests/_le_coded.py) against what can be known without it: the encoder two ways, the code's free
distance, the trellis decoder against brute force, the guaranteed error correction, the side lobes behind rule 1's cap of 63, the
vectorised decoder against the literal one, and -- on the GPU test's own inputs -- every wrong variant told from the model."""
import itertools

import numpy as np
import pytest

import _le
import _le_coded as m


def _poly_mul(msg, g):
    """Message polynomial times generator over GF(2): coefficient k of the product, k < len(msg)."""
    out = [0] * (len(msg) + len(g) - 1)
    for i, b in enumerate(msg):
        for j, c in enumerate(g):
            out[i + j] ^= b & c
    return out[:len(msg)]


def test_encoder_two_ways():
    rng = np.random.default_rng(3)
    for n in (1, 2, 5, 37, 43, 200):
        msg = [int(b) for b in rng.integers(0, 2, n)]
        coded = m.encode(msg)
        assert coded[0::2] == _poly_mul(msg, m.FORMAT["g0"]) and coded[1::2] == _poly_mul(msg, m.FORMAT["g1"])
    assert m.encode([1, 0, 0, 0]) == [1, 1, 1, 0, 1, 1, 1, 1]        # the impulse response: G0 = 1111, G1 = 1011, a0 first
    assert m.map_symbols([0, 1], 8) == [0, 0, 1, 1, 1, 1, 0, 0] and m.map_symbols([0, 1], 2) == [0, 1]
    pat = m.pattern_symbols(_le.ADV_AA)
    assert len(pat) == m.PATTERN == 336 and list(pat[:80]) == [0, 0, 1, 1, 1, 1, 0, 0] * 10
    sym = m.coded_symbols(_le.ADV_AA, 37, _le.make_pdu(0x42, bytes(255)), _le.ADV_CRC_INIT, 8)
    assert len(sym) == 17040 and (sym[:336] == pat).all()
    # every group of four pattern symbols is 0011 or 1100, whatever the address: what the scan's pre-filter rests on
    for aa in (_le.ADV_AA, 0, 0xFFFFFFFF, 0x5A3C96E1):
        groups = m.pattern_symbols(aa).reshape(84, 4)
        assert ((groups[:, 0] == groups[:, 1]) & (groups[:, 2] == groups[:, 3]) & (groups[:, 0] != groups[:, 2])).all()


def test_free_distance_is_six():
    """Every message of up to 10 bits that starts with a one, zero-terminated: the smallest code word weight."""
    best = min(sum(m.encode([1] + list(tail) + [0, 0, 0])) for n in range(10) for tail in itertools.product((0, 1), repeat=n))
    assert best == 6
    assert sum(m.encode([1, 1, 0, 0, 0])) == 6


def _viterbi(received, s, n_bits):
    t = m.Trellis(s)
    for k in range(n_bits):
        t.step(received[s * k:s * (k + 1)])
    return t.trace(0), t.metrics[0]


@pytest.mark.parametrize("s", [2, 8])
def test_decoder_equals_brute_force(s):
    """All 2^7 messages of 7 + 3 termination bits against random received words: the trellis finds the smallest metric and, among
    equals, the smallest integer with bit i weighted 2^i (rule 2's tie rule: x = 0 is the older zero)."""
    rng = np.random.default_rng(5 + s)
    words = [np.array(m.map_symbols(m.encode(m.int_bits(v, 7) + [0, 0, 0]), s), np.uint8) for v in range(128)]
    for trial in range(300):
        rx = rng.integers(0, 2, 10 * s, dtype=np.uint8)
        if trial % 2:                                   # half of the words near a code word, where ties are likelier than in noise
            rx = m.flip(words[int(rng.integers(0, 128))], rng.choice(10 * s, 3 if s == 2 else 12, replace=False))
        want = min(range(128), key=lambda v: (int((words[v] != rx).sum()), v))
        bits, metric = _viterbi(rx, s, 10)
        assert _le.bits_value(bits[:7]) == want and bits[7:] == [0, 0, 0] and metric == int((words[want] != rx).sum())


@pytest.mark.parametrize("s,k", [(2, 2), (8, 11)])
def test_guaranteed_correction(s, k):
    rng = np.random.default_rng(7)
    for trial in range(400):
        msg = [int(b) for b in rng.integers(0, 2, 40)] + [0, 0, 0]
        tx = np.array(m.map_symbols(m.encode(msg), s), np.uint8)
        bits, metric = _viterbi(m.flip(tx, rng.choice(len(tx), k, replace=False)), s, 43)
        assert bits == msg and metric == k


def test_three_errors_at_s2_may_tie():
    msg, rx = m.tie_received()
    t0, t1 = m.Trellis(2), m.Trellis(2, m.Rules(tie_x=1))
    for k in range(43):
        t0.step(rx[2 * k:2 * k + 2])
        t1.step(rx[2 * k:2 * k + 2])
    assert t0.metrics[0] == t1.metrics[0] == 3 and t0.trace(0) != t1.trace(0)
    assert sorted([t0.trace(0), t1.trace(0)])[0] == msg              # one of the two is the zero message


def test_side_lobes_stay_above_the_cap():
    """Rule 1: the smallest mismatch count at any wrong offset within +-400 symbols of a planted packet."""
    rng = np.random.default_rng(11)

    def lobe(aa):
        sym = m.coded_symbols(aa, 37, m.pdu_of(rng, 40), _le.ADV_CRC_INIT, 8)
        line = np.concatenate([rng.integers(0, 2, 400, dtype=np.uint8), sym])
        err = m.mismatch_counts(line, aa, 801)
        assert err[400] == 0
        err[400] = 999
        return int(err.min())

    assert lobe(_le.ADV_AA) > m.MAX_ERRORS
    assert min(lobe(int(a)) for a in rng.integers(0, 1 << 32, 200, dtype=np.uint64)) > m.MAX_ERRORS


@pytest.fixture(scope="module")
def cases():
    return m.decode_cases()


@pytest.fixture(scope="module")
def literal(cases):
    """The literal decoder's records for every hit of every case, computed once."""
    return [[m.decode(c["words"], c["n_words"], 0, o, e, c["mhz"], c["crc_init"]) for o, e in c["hits"]] for c in cases]


def test_vectorised_decoder_equals_the_literal_one(cases, literal):
    for c, lit in zip(cases, literal):
        offs, errs = [o for o, _ in c["hits"]], [e for _, e in c["hits"]]
        assert m.decode_many(c["words"], c["n_words"], 0, offs, errs, c["mhz"], c["crc_init"]) == lit, c["note"]


@pytest.mark.parametrize("name", sorted(m.WRONG))
def test_the_gpu_inputs_tell_every_wrong_variant_from_the_model(cases, literal, name):
    """(cases in reverse, stopping at the first hit that tells the variant: the long packets of the first cases are not needed for any)"""
    rules = m.Rules(**{name: m.WRONG[name]})
    for c, lit in reversed(list(zip(cases, literal))):
        for (o, e), want in zip(c["hits"], lit):
            if m.decode(c["words"], c["n_words"], 0, o, e, c["mhz"], c["crc_init"], rules) != want:
                return
    raise AssertionError("no input tells %s from the model" % name)
