"""The model of LE following from CONNECT_IND (tests/_le_follow.py) without a GPU: its CONNECT_IND parse against what the compiled
reference prints (oracle/_ref/libbtbb_ref.so: lell_allocate_and_decode + lell_print in a child process whose stdout is parsed;
skipped when it is not built), the planted connections -- which hop by the forward selections -- against its predictions, and
that the lattice tells every deliberately wrong variant from it."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _le
import _le_follow as lf
import _le_track as lt
import _libs
import libbtbb_amd as bt

CHILD = r"""
import ctypes as C, sys
lib = C.CDLL(sys.argv[1])
libc = C.CDLL(None)
dec, show, unref = lib.lell_allocate_and_decode, lib.lell_print, lib.lell_packet_unref
dec.restype, dec.argtypes = None, [C.c_char_p, C.c_uint16, C.c_uint32, C.POINTER(C.c_void_p)]
show.restype, show.argtypes = None, [C.c_void_p]
unref.restype, unref.argtypes = None, [C.c_void_p]
for line in sys.stdin.read().split():
    p = C.c_void_p()
    dec(bytes.fromhex(line), 2402, 0, C.byref(p))
    sys.stdout.write("==== %s\n" % line)
    sys.stdout.flush()
    show(p)
    libc.fflush(None)
    unref(p)
"""


@pytest.fixture(scope="module", autouse=True)
def _the_model_numbers_things_as_the_package_does():
    assert (lf.SEEDED, lf.COUNTED, lf.STOPPED, lf.TERMINATED, lf.ENCRYPTED) == (
        bt.LE_FOLLOW_SEEDED, bt.LE_FOLLOW_COUNTED, bt.LE_FOLLOW_STOPPED, bt.LE_FOLLOW_TERMINATED, bt.LE_FOLLOW_ENCRYPTED)
    assert (lf.ST_COUNTED, lf.ST_BEFORE, lf.ST_BEYOND) == (bt.LE_STATE_COUNTED, bt.LE_STATE_BEFORE, bt.LE_STATE_BEYOND)
    assert (lf.DATA, lf.CONTROL, lf.MAP_UPDATE, lf.PARAM_UPDATE, lf.TERMINATE, lf.ENC_START, lf.OPAQUE) == (
        bt.LE_PDU_DATA, bt.LE_PDU_CONTROL, bt.LE_PDU_MAP_UPDATE, bt.LE_PDU_PARAM_UPDATE, bt.LE_PDU_TERMINATE, bt.LE_PDU_ENC_START,
        bt.LE_PDU_OPAQUE)
    assert lf.seed_array(lf.lattice_model()[0], bt.LE_SEED_DTYPE).dtype.itemsize == 56


def test_the_lattice_tells_every_variant_from_the_model():
    b = lf.lattice()
    want = lf.lattice_model()
    assert lf.model(b, lf.Rules()) == want
    for name, kw in lf.VARIANTS.items():
        got = lf.model(b, lf.Rules(**kw))
        differ = [n for n, s, s2, f, f2 in zip(b.names, want[0], got[0], want[1], got[1]) if s != s2 or f != f2]
        differ += [b.names[c.channel] for c, p, p2 in zip(b.cands, want[2], got[2]) if p != p2]
        assert differ, name
        print("%-18s %s" % (name, sorted(set(differ))[:3]))
    assert len(lf.VARIANTS) == 15


def test_the_lattice_holds_what_it_names():
    b = lf.lattice()
    seeds, follows, fpkts = lf.lattice_model()
    by = dict(zip(b.names, zip(seeds, follows)))
    for name in ("hop 4", "hop 17", "interval 5", "interval 3201", "win_size 0 of interval 6", "win_size 9 of interval 12",
                 "win_size 6 of interval 6", "win_offset = interval + 1", "map of one channel", "crc_ok 0", "length 33", "length 35",
                 "type 5 on a data-channel stream", "adv type 4", "equal AA with another CRCInit", "R = first_anchor + 1", "no request"):
        assert by[name][0] is None and by[name][1] is None, name
    for name in ("hop 5", "hop 16", "interval 6", "interval 3200", "win_size 1 of interval 6", "win_size 8 of interval 12",
                 "win_size 5 of interval 6", "win_offset = interval", "R = first_anchor"):
        assert by[name][0] is not None, name
    assert by["planted: map bit 0 and bit 36, top bits set"][0].map == (1 << 0) | (1 << 20) | (1 << 36)
    # the first event around t0: one bit decides between BEFORE and counter 0, and between counters 0 and 1
    assert (by["A_f = t0 - jitter"][1].n_before, by["A_f = t0 - jitter - 1"][1].n_before) == (0, 1)
    assert (by["A_f = t0 + P - jitter - 1"][1].counter_first, by["A_f = t0 + P - jitter"][1].counter_first) == (0, 1)
    assert by["A_f = t0 + win_size"][1].counter_first == 0 and by["A_f = t0"][1].n_off == 0
    assert by["planted: counters beyond 2^32"][1].n_on == 6 and by["planted: counters beyond 2^32, #1"][1].n_on == 6
    assert [by["planted: delta %d" % d][1].n_map_updates for d in (6, 32766, 32767, 32768)] == [1, 1, 0, 0]
    assert by["planted: two with equal I"][1].map == lf.FIVE and by["planted: two updates out of order"][1].map == lf.FIVE
    assert by["planted: a retransmitted update"][1].n_map_updates == 3
    assert by["planted: map update PDU in a BEYOND event"][1].n_map_updates == 1 and by["planted: map update PDU in a BEYOND event"][1].stop == 6
    assert by["update in a BEFORE event"][1].n_map_updates == 0 and not by["update in a BEFORE event"][1].flags & lf.STOPPED
    assert by["unseeded with control PDUs"][1] is None
    kinds = sorted(p.kind for c, p in zip(b.cands, fpkts) if p is not None and b.names[c.channel] == "unseeded with control PDUs")
    assert kinds == [lf.DATA] * 4 + [lf.CONTROL, lf.ENC_START, lf.OPAQUE, lf.OPAQUE]
    for r in (0, 1, 63):
        g = b.names.index("planted: control PDU at offset %d mod 64" % r)
        at = [c.offset % 64 for c, p in zip(b.cands, fpkts) if c.channel == g and p.kind == lf.MAP_UPDATE]
        assert at == [r], (r, at)
    g = b.names.index("planted: last bit is the stream's last bit")
    assert [c.offset + 80 + 8 * c.length for c, p in zip(b.cands, fpkts) if c.channel == g and p.kind == lf.MAP_UPDATE] == [64 * lf.N_WORDS]
    assert {c.stream for c, p in zip(b.cands, fpkts) if p is not None and p.kind == lf.MAP_UPDATE} >= {0, 36}
    assert any(c.stream >= lt.N_STREAMS for c in b.cands) and sum(c.channel >= len(b.conns) for c in b.cands) >= 40


def test_the_model_predicts_the_planted_channels():
    b = lf.lattice()
    assert lf.check_planted(b, *lf.lattice_model()) > 600
    s = lf.seam_world()
    want = lf.seam_model()
    assert lf.check_planted(s, *want) > 7000
    big = want[1][s.names.index("planted: large")]
    assert (big.n_on, big.n_off, big.n_map_updates) == (5000, 0, 40)
    w = lf.wrap_world()                                                    # update PDUs next to counter 65 536, inside the streams
    assert lf.check_planted(w, *lf.wrap_model()) == sum(len(i.counters) for i in w.info) == 42
    assert all(t.n_events == len(i.counters) for t, i in zip(w.tracks, sorted(w.info, key=lambda i: (i.aa, i.crc_init))))


def test_the_chain_capture_is_followed_where_the_tracking_loses_the_hop():
    cap, planted = lf.chain_capture()
    conns, cands, tracks, pkts, adv, seeds, follows, fpkts = lf.chain_model()
    assert len(adv) == 2 and all(lf.is_request(r) for r in adv)
    by = {(c.access_address, c.crc_init): g for g, c in enumerate(conns)}
    for p in planted:
        g = by[(p.aa, p.crc_init)]
        if not p.seeded:
            assert seeds[g] is None and follows[g] is None
            continue
        before_stop = len([c for c in p.counters if p.stop is None or c < p.stop])
        f = follows[g]
        assert (f.n_on, f.n_off, f.n_before, f.n_beyond, f.algorithm) == (before_stop, 0, 0, len(p.counters) - before_stop, p.alg), (p, f)
        mine = [i for i, c in enumerate(cands) if c.channel == g]
        assert len([i for i in mine if fpkts[i].state == lf.ST_COUNTED]) == 2 * before_stop
        late = [i for i in mine if fpkts[i].state == lf.ST_COUNTED and fpkts[i].counter >= p.first_update]
        assert tracks[g].n_off_hop > 0 and not all(pkts[i].on_hop for i in late)


def test_the_request_parse_equals_what_the_reference_prints():
    ref = _libs.ref()
    if ref is None:
        pytest.skip("oracle/_ref/libbtbb_ref.so not built")
    b = lf.lattice()
    reqs = [r["bytes"] for r in b.adv] + [lf.connect_ind(0xDEADBEEF, 0xABCDEF, (1 << 37) - 1, 31, 0xFFFF, 255, 0xFFFE, 0x1234, 0x8765, sca=7,
                                                         chsel=1, tx_add=1, rx_add=0, top_bits=5)]
    reqs = [r for r in reqs if (r[4] & 0xF) == 5]
    path = os.path.join(_libs.ORACLE_DIR, "_ref", "libbtbb_ref.so")
    out = subprocess.run([sys.executable, "-c", CHILD, path], input="\n".join(r.hex() for r in reqs), capture_output=True, text=True,
                         check=True).stdout
    blocks = out.split("==== ")[1:]
    assert len(blocks) == len(reqs) > 60
    for block, raw in zip(blocks, reqs):
        lines = block.splitlines()
        assert lines[0] == raw.hex()
        got = {}
        for line in lines[1:]:
            key, _, rest = line.strip().partition(":")
            if key in ("InitA", "AdvA", "AA", "CRCInit", "WinSize", "WinOffset", "Interval", "Latency", "Timeout", "ChM", "Hop", "SCA"):
                got[key] = rest.strip()
        f = lf.parse_request(raw)
        addr = lambda a, random: ":".join("%02x" % x for x in a[::-1]) + (" (random)" if random else " (public)")   # noqa: E731
        assert got["InitA"] == addr(f["init_a"], f["tx_add"]) and got["AdvA"] == addr(f["adv_a"], f["rx_add"]), (got, f)
        assert int(got["AA"], 16) == f["aa"] and int(got["CRCInit"], 16) == f["crc_init"], (got, f)
        for key, name in (("WinSize", "win_size"), ("WinOffset", "win_offset"), ("Interval", "interval"), ("Latency", "latency"),
                          ("Timeout", "timeout")):
            assert int(got[key].split()[0], 16) == f[name] and got[key].split()[1] == "(%d)" % f[name], (key, got, f)
        assert int.from_bytes(bytes(int(x, 16) for x in got["ChM"].split()), "little") & lf.MAP37 == f["map"], (got, f)
        assert int(got["Hop"]) == f["hop"] and int(got["SCA"].split(",")[0]) == f["sca"], (got, f)
        assert _le.ref_lell_fields(ref, raw, 2402)["adv_type"] == 5
    assert np.all([len(r) == 64 for r in reqs])
