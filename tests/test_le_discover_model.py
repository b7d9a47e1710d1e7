"""The model of the LE connection discovery (tests/_le_discover.py) against code that is independent of it, its grouping on
hand-made lists, the lattice of the GPU tests against deliberately wrong variants of the model, and -- without a device -- the
public layouts and the loud failure of the entry points that compute (btbbx_le_discover_scratch_bytes is arithmetic).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import _le
import _le_discover as ld


def test_backward_walk_against_the_forward_register():
    """crc24_tx_bits(pdu, found CRCInit) == the received bits: forward through code the backward walk shares nothing with."""
    rng = np.random.default_rng(1)
    for n in range(256):
        pdu = _le.octet_bits(bytes([int(rng.integers(0, 256)), n]) + rng.integers(0, 256, n, dtype=np.uint8).tobytes())
        preset = int(rng.integers(0, 1 << 24)) if n else (0, 0xFFFFFF, 0x555555, 1, 0x800000)[n % 5]
        rx = _le.crc24_tx_bits(pdu, preset)
        found = ld.crc24_backward(pdu, rx)
        assert found == preset, (n, hex(preset), hex(found))
        assert (_le.crc24_tx_bits(pdu, found) == rx).all()
    for preset in (0, 0xFFFFFF, 0x555555, 1, 0x800000):
        pdu = _le.octet_bits(b"\x01\x00")
        assert ld.crc24_backward(pdu, _le.crc24_tx_bits(pdu, preset)) == preset


def test_every_transmitted_data_packet_is_a_candidate():
    rng = np.random.default_rng(2)
    for k in range(40):
        mhz = int(rng.choice([m for m in range(2404, 2480, 2) if m != 2426]))
        ch = _le.channel_index(mhz)
        aa, ci = ld.good_aa(rng, k & 3), int(rng.integers(0, 1 << 24))
        n = (0, 1, 27, 255)[k & 3] if k < 8 else int(rng.integers(0, 28))
        h0 = (1, 2, 3, 0x1F)[k % 4]
        pdu = bytes([h0, n]) + rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        sym = _le.tx_bits(aa, ch, pdu, ci)
        lead = int(rng.integers(0, 130))
        line = np.concatenate([rng.integers(0, 2, lead, dtype=np.uint8), sym])
        words = _le.pack(line)
        got = ld.candidates(words, len(words), lead + 1, mhz, 255, stream=3)
        assert ld.Cand(lead, aa, ci, 3, h0, n, ch) in got, (k, got)
        if 64 * len(words) == len(line):                         # it ends at the stream's last bit: one word less and it is no candidate
            assert lead not in [c.offset for c in ld.candidates(words, len(words) - 1, lead + 1, mhz, 255)]
        # no candidates on an advertising channel
        assert ld.candidates(words, len(words), lead + 1, 2402, 255) == []


def test_grouping_model_on_hand_made_lists():
    c = ld.Cand
    lst = [c(900, 0xA0000001, 0x000002, 1, 1, 0, 5), c(100, 0xA0000001, 0x000002, 1, 2, 3, 5), c(50, 0xA0000001, 0x000002, 0, 1, 0, 36),
           c(7, 0xA0000001, 0x000003, 0, 1, 0, 1), c(8, 0x20000001, 0x000002, 0, 1, 9, 2), c(9, 0x20000001, 0x000002, 2, 1, 9, 0)]
    conns, out = ld.group(lst, 2)
    assert conns == [ld.Conn(0x20000001, 2, 2, 0, 0b101, 0), ld.Conn(0xA0000001, 2, 3, 2, (1 << 36) | (1 << 5), 2)]
    assert [(o.offset, o.stream, o.channel) for o in out] == [(8, 0, 0), (9, 2, 0), (50, 0, 1), (100, 1, 1), (900, 1, 1), (7, 0, ld.NO_CONN)]
    conns1, out1 = ld.group(lst, 1)
    assert [k.n_packets for k in conns1] == [2, 3, 1] and [k.first for k in conns1] == [0, 2, 5] and out1[5].channel == 2
    assert ld.group(lst, 4) == ([], [o._replace(channel=ld.NO_CONN) for o in out])
    assert ld.group([], 2) == ([], [])


@pytest.mark.parametrize("max_len", [0, 27, 255])
@pytest.mark.parametrize("tight", [False, True])
def test_lattice_holds_what_it_was_built_to_hold(max_len, tight):
    cap = ld.scan_lattice(max_len, tight)
    found = {(c.stream, c.offset): c for c in ld.lattice_model(max_len, tight)}
    notes = set()
    for p in cap.planted:
        want = ld.plant_expected(cap, p)
        got = found.get((p.stream, p.offset))
        assert (got is not None) == want, p
        if want:
            assert (got.access_address, got.crc_init, got.header0, got.length) == (p.aa, p.crc_init, p.header0, p.length), p
        if p.note == "ends one bit past the stream" and (tight or max_len >= 16):
            assert p.offset < cap.search_bits and p.offset + 80 + 8 * p.length == 64 * cap.n_words + 1     # rule 5 alone keeps it out
        notes.add((p.note.split(",")[0].split(":")[0].rstrip(" 0123456789-"), want))
    # both outcomes of every rule are planted
    for note, want in (("phase", True), ("seam", True), ("back to back", True),
                       ("ends one bit past the stream", False), ("LLID", False), ("RFU bit", False), ("every allowed bit", True),
                       ("one offense", False), ("AA low bits", True), ("advertising channel", False)):
        assert (note, want) in notes, (note, want, sorted(notes))
    if max_len < 255:                                            # (a length of max_len + 1 does not exist at 255)
        assert ("back to back", False) in notes and ("length", False) in notes, sorted(notes)
    if tight:
        assert ("ends at the last bit", True) in notes, sorted(notes)
    else:
        assert ("at search_bits", True) in notes and ("at search_bits", False) in notes, sorted(notes)
    assert len(ld.one_offense_aas()) == len(ld.OFFENSE_KINDS)
    assert {p.offset & 63 for p in cap.planted if p.note.startswith("phase")} == set(range(64))


@pytest.mark.parametrize("variant", sorted(ld.VARIANTS))
def test_lattice_tells_the_model_from_wrong_variants(variant):
    """Each wrong variant of the model yields another candidate set on the lattice, so a kernel that made the same mistake
    would fail the GPU comparison."""
    told = 0                                                     # (the GPU tests run both forms of the lattice; rule 5's packet lies inside
    for tight in (False, True):                                  # search_bits only in the tight one)
        cap = ld.scan_lattice(27, tight)
        wrong = set(ld.capture_candidates(cap, 27, ld.Rules(**ld.VARIANTS[variant])))
        told += wrong != set(ld.lattice_model(27, tight))
    assert told >= 1 and (told == 2 or variant == "end_strict"), variant


@pytest.mark.parametrize("max_len", [0, 27, 255])
@pytest.mark.parametrize("variant", ["end_permissive", "end_absent"])
def test_rule_five_is_exercised_at_every_max_len(max_len, variant):
    """A packet that starts below search_bits and ends one bit past the stream is planted at every max_len: a model whose rule 5
    is off by one on the permissive side, or that has none, reports it, and the model does not."""
    cap = ld.scan_lattice(max_len, True)
    plant = [p for p in cap.planted if p.note == "ends one bit past the stream"]
    assert len(plant) == 1
    key = (plant[0].stream, plant[0].offset)
    wrong = {(c.stream, c.offset) for c in ld.capture_candidates(cap, max_len, ld.Rules(**ld.VARIANTS[variant]))}
    right = {(c.stream, c.offset) for c in ld.lattice_model(max_len, True)}
    assert key in wrong and key not in right and right < wrong


def test_layouts_and_loud_failure_without_a_device():
    import libbtbb_amd as bt
    assert bt.LE_CAND_DTYPE.itemsize == 24 and bt.LE_CONN_DTYPE.itemsize == 32
    assert [bt.LE_CAND_DTYPE.fields[k][1] for k in ("offset", "access_address", "crc_init", "stream", "header0", "length", "conn")] == \
        [0, 8, 12, 16, 18, 19, 20]
    assert [bt.LE_CONN_DTYPE.fields[k][1] for k in ("access_address", "crc_init", "n_packets", "n_empty", "channel_mask", "first")] == \
        [0, 4, 8, 12, 16, 24]
    lib = bt.lib()
    assert lib.btbbx_le_discover_scratch_bytes(1000) >= 1000 * 60
    import torch
    if torch.cuda.is_available():
        return                                                   # (with a device they work: tests/test_gpu_le_discover.py)
    words = np.zeros(64, np.uint64)
    phys = np.array([2404], np.uint16)
    buf = np.zeros(4096, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                  # noqa: E731
    assert lib.btbbx_le_discover_scan_device(vp(words), 64, 64, 1, 1000, vp(phys), 27, vp(buf), 8, vp(buf[2048:]), None) < 0
    assert lib.btbbx_last_error()
    assert lib.btbbx_le_discover_group_device(vp(buf), vp(buf[2048:]), 0, 2, vp(buf), 8, vp(buf[2048:]), vp(buf), 4096, None) < 0
    assert lib.btbbx_le_discover_host(vp(words), 64, 64, 1, 1000, vp(phys), 27, 2, vp(buf), 8, vp(buf[1024:]), 8, None) < 0
    with pytest.raises(bt.BtbbError):
        bt.le_discover(words, 1000, [2404])
