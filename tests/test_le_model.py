"""CPU checks of the Bluetooth LE model (tests/_le.py) and of the argument checks of the btbbx_le_* entry points.

The model's registers are written from the spec's figures; the lell fields it derives are held against the compiled
reference's lell_allocate_and_decode (oracle/_ref/libbtbb_ref.so; skipped when it is not built)."""
import ctypes as C

import numpy as np
import pytest

import _le
import _libs
import libbtbb_amd as bt


def test_whitening_is_an_involution_with_period_127():
    rng = np.random.default_rng(_libs.seed(1))
    for chan in range(40):
        w = _le.whitening_bits(chan, 127 * 3)
        assert (w[:127] == w[127:254]).all() and (w[:127] == w[254:]).all()
        assert all((w[:127] != np.roll(w[:127], -p)).any() for p in range(1, 127))          # no shorter period
        assert w[:127].sum() == 64                                                           # a maximal-length sequence
        data = rng.integers(0, 2, 300, dtype=np.uint8)
        once = data ^ _le.whitening_bits(chan, 300)
        assert (once != data).any()
        assert (once ^ _le.whitening_bits(chan, 300) == data).all()


def test_whitening_seed_layout():
    # channel 0: position 0 = 1, positions 1..6 = 0 -> the register puts out six zeros, then the one that reached position 6
    w = _le.whitening_bits(0, 7)
    assert list(w) == [0, 0, 0, 0, 0, 0, 1]
    # channel 1 (LSB in position 6): the first output is that bit
    assert _le.whitening_bits(1, 1)[0] == 1


@pytest.mark.parametrize("crc_init", [_le.ADV_CRC_INIT, 0x000000, 0xFFFFFF, 0x1A2B3C])
def test_crc_residue_zero_and_single_bit_errors(crc_init):
    rng = np.random.default_rng(_libs.seed(2) + crc_init)
    for L in (0, 1, 6, 37, 255):
        pdu = _le.make_pdu(int(rng.integers(0, 256)), rng.integers(0, 256, L, dtype=np.uint8).tobytes())
        bits = _le.octet_bits(pdu)
        crc = _le.crc24_tx_bits(bits, crc_init)
        both = np.concatenate([bits, crc])
        assert not any(_le.crc24_register(both, crc_init))
        for i in range(0, len(both), max(1, len(both) // 97)):
            bad = both.copy()
            bad[i] ^= 1
            assert any(_le.crc24_register(bad, crc_init)), (L, i)


def _reflected_tables():
    crc_tab = []
    for i in range(256):
        s = i
        for _ in range(8):
            s = (s >> 1) ^ (0xDA6000 if s & 1 else 0)
        crc_tab.append(s)
    wh = []
    for st in range(128):
        s, o = st, 0
        for k in range(8):
            o |= (s & 1) << k
            if s & 1:
                s ^= 0x88
            s >>= 1
        wh.append((o, s))
    return crc_tab, wh


def test_reflected_byte_forms_agree_with_the_spec_registers():
    """The kernels' form (le.hip: byte-wise CRC table of the reflected register, whitening eight bits per step from the
    state chan | 0x40) against the bit-serial position form of the spec's figures."""
    crc_tab, wh = _reflected_tables()
    rng = np.random.default_rng(_libs.seed(3))
    for chan in range(40):
        s, out = (chan & 0x3F) | 0x40, []
        for _ in range(40):
            o, s = wh[s]
            out.append(o)
        assert bytes(out) == _le.bits_octets(_le.whitening_bits(chan, 320))
    for crc_init in (_le.ADV_CRC_INIT, int(rng.integers(0, 1 << 24))):
        data = rng.integers(0, 256, 77, dtype=np.uint8).tobytes()
        s = int("{:024b}".format(crc_init)[::-1], 2)
        for b in data:
            s = (s >> 8) ^ crc_tab[(s ^ b) & 0xFF]
        assert s == _le.bits_value(_le.crc24_tx_bits(_le.octet_bits(data), crc_init))


def test_channel_mapping():
    assert [_le.channel_index(m) for m in (2402, 2426, 2480)] == [37, 38, 39]
    assert [_le.channel_index(2404 + 2 * k) for k in range(11)] == list(range(11))
    assert [_le.channel_index(2428 + 2 * k) for k in range(26)] == list(range(11, 37))
    assert _le.channel_k(2402) == 0 and _le.channel_k(2480) == 39


@pytest.fixture(scope="module")
def ref():
    r = _libs.ref()
    if r is None:
        pytest.skip("oracle/_ref/libbtbb_ref.so not built")
    return r


def _check_lell(ref, aa, mhz, h0=0x40, h1=0x25):
    b = int(aa).to_bytes(4, "little") + bytes([h0, h1]) + bytes(58)
    assert _le.lell_fields(b, mhz) == _le.ref_lell_fields(ref, b, mhz), (hex(aa), mhz, h0, h1)


def test_lell_fields_random_aas(ref):
    rng = np.random.default_rng(_libs.seed(4))
    aas = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64)
    for i, aa in enumerate(aas):
        _check_lell(ref, int(aa), 2404 + 2 * (i % 11) if i & 1 else (2402, 2426, 2480)[i % 3], h0=i & 0xFF, h1=(i * 37) & 0xFF)


def test_lell_fields_special_aas(ref):
    special = [_le.ADV_AA] + [_le.ADV_AA ^ (1 << i) for i in range(32)]
    special += [b * 0x01010101 for b in range(256)]                                     # all four octets equal
    for run in (6, 7, 8, 12):
        for start in range(0, 33 - run):
            base = 0x5555AAAA if start & 1 else 0xAAAA5555
            ones = ((1 << run) - 1) << start
            special += [base | ones, base & ~ones & 0xFFFFFFFF]                         # runs of ones / zeros
    special += [0xAAAAAAAA, 0x55555555, 0xAAAAAAAB, 0x2AAAAAAA, 0xD5555555, 0x5555AAAA]     # > 24 transitions
    special += list(range(4096))                                                         # every 12-bit low window
    special += [v << 20 for v in range(4096)]                                            # every 12-bit high window
    for aa in special:
        for mhz in (2404, 2426, 2478):
            _check_lell(ref, aa & 0xFFFFFFFF, mhz)


def test_lell_fields_every_mhz(ref):
    for mhz in range(2400, 2484):
        for h0 in (0x00, 0x46, 0xC5, 0x3F):
            _check_lell(ref, _le.ADV_AA, mhz, h0=h0, h1=0xFF)
            _check_lell(ref, 0x50654C3B, mhz, h0=h0, h1=0x9C)


def test_le_entry_points_reject_bad_arguments_without_a_gpu():
    lib = bt.lib()
    words = np.zeros(64, np.uint64)
    phys = np.full(65536, 2402, np.uint16)
    hits = np.zeros(4, bt.HIT_DTYPE)
    cnt = np.zeros(4, np.uint32)
    pk = np.zeros(1, bt.LE_PKT_DTYPE)
    wp, pp, hp, cp, kp = (a.ctypes.data_as(C.c_void_p) for a in (words, phys, hits, cnt, pk))
    ok_bits = 64 * 64 - 39
    cases = [
        (5, ok_bits, 1),              # max_errors 5
        (-1, ok_bits, 1),
        (2, ok_bits + 1, 1),          # search_bits + 39 > 64 n_words
        (2, 64, 65536),               # n_streams = 65536
        (2, 64, 0),
    ]
    for err, sb, ns in cases:
        assert lib.btbbx_le_scan_host(wp, 64, 64, ns, sb, pp, _le.ADV_AA, _le.ADV_CRC_INIT, err, kp, 1) == -3, (err, sb, ns)
        assert lib.btbbx_le_scan_device(wp, 64, 64, ns, sb, _le.ADV_AA, err, hp, 4, cp, None) == -3, (err, sb, ns)
    assert b"max_errors" in lib.btbbx_last_error() or b"n_streams" in lib.btbbx_last_error()


def test_le_pkt_dtype_matches_the_library():
    assert bt.LE_PKT_DTYPE.itemsize == 104
    names = [n for n in bt.LE_PKT_DTYPE.names if n != "pad"]
    assert names[:len(_le.FIELDS) + 1] == list(_le.FIELDS) + ["bytes"]


def test_tx_chain_layout():
    pdu = _le.make_pdu(0x42, bytes(range(6)))
    bits = _le.tx_bits(_le.ADV_AA, 37, pdu, _le.ADV_CRC_INIT)
    assert len(bits) == 8 + 32 + 8 * (len(pdu) + 3)
    assert _le.bits_octets(bits[:40]) == bytes([0xAA, 0xD6, 0xBE, 0x89, 0x8E])          # the 40 bits on air of the advertising AA
    sym = np.zeros(512, np.uint8)
    sym[100:100 + len(bits)] = bits
    words = np.packbits(sym, bitorder="little").view(np.uint64)
    off, err, aa = _le.match_all(words, len(words), 512 - 39, _le.ADV_AA, 0)
    assert list(off) == [100] and list(aa) == [_le.ADV_AA]
    rec = _le.decode(words, len(words), 0, 100, 0, 2402, _le.ADV_CRC_INIT)
    assert rec["crc_ok"] == 1 and rec["pdu_bytes"] == len(pdu) and rec["bytes"][4:4 + len(pdu)] == pdu
    assert rec["adv_type"] == 2 and rec["adv_tx_add"] == 1 and rec["length"] == 6
