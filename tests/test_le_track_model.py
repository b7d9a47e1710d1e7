"""The model of the LE connection tracking (tests/_le_track.py): its hand-built lattice against deliberately wrong variants of
the model, the recovery of planted connections (made by the forward channel selection, which shares nothing with the model's
inverse) over a sweep of sizes, maps and losses, the planted maps of the chain capture, and -- without a device -- the public
layouts and the loud failure of the entry points that compute.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import _le_discover as ld
import _le_track as lt


def test_forward_channel_selection_by_hand():
    full = (1 << 37) - 1
    assert [lt.csa1(0, 7, n, full) for n in range(1, 7)] == [7, 14, 21, 28, 35, 5]         # the spec's unmappedChannel sequence
    assert lt.csa1(36, 16, 1, full) == 15 and lt.csa1(11, 5, 0, full) == 11
    chmap = (1 << 4) | (1 << 17) | (1 << 30)
    assert lt.csa1(4, 5, 0, chmap) == 4 and lt.csa1(5, 5, 0, chmap) == 30 and lt.csa1(0, 9, 1, chmap) == 4 and lt.csa1(0, 10, 1, chmap) == 17


def test_model_by_hand():
    """Three events of interval 8 on channels 3, 16, 29: hop 13 from 3, every figure worked out by hand."""
    c = ld.Cand
    cands = [c(1000 + 8 * 1250 * n + d, 1, 2, ch, 1, 0, 0) for n, (ch, d) in enumerate(((3, 0), (16, 7), (29, -7)))]
    cands.insert(2, c(1000 + 8 * 1250 + 7 + 80 + 200, 1, 2, 16, 1, 0, 0))                   # second packet of event 1, at exactly ifs
    cands.append(c(5, 9, 9, 0, 1, 0, ld.NO_CONN))
    tracks, pkts = lt.track(cands, 1, lt.LATTICE_MHZ, lt.N_STREAMS, 1250, 200, 50, 0)
    assert tracks == [lt.Track(1000, (1 << 3) | (1 << 16) | (1 << 29), 3, 2, 8, 3, 0, 1, 13, 3, 3, lt.TIMED | lt.HOPPING)]
    assert pkts == [lt.Pkt(0, 0, 0, 3, 3, 3, 1), lt.Pkt(1, 1, 1, 16, 16, 16, 1), lt.Pkt(2, 1, 1, 16, 16, 16, 1), lt.Pkt(3, 2, 2, 29, 29, 29, 1), None]


@pytest.mark.parametrize("variant", sorted(lt.VARIANTS))
def test_lattice_tells_the_model_from_wrong_variants(variant):
    """Each wrong variant of the model gives other records on the lattice (with or without REMAP), so a kernel that made the same
    mistake would fail the GPU comparison."""
    told = []
    for flags in (0, lt.REMAP):
        names, right, right_pkts = lt.lattice_tracks(flags)
        _, wrong, wrong_pkts = lt.lattice_tracks(flags, lt.Rules(**lt.VARIANTS[variant]))
        told += [n for n, a, b in zip(names, right, wrong) if a != b]
        told += ["packets"] if right_pkts != wrong_pkts else []
    print(variant, sorted(set(t for t in told if t)))
    assert told, variant
    # the two variants that one case each was built for: that case, and no other connection, tells them
    if variant == "tie_unstable":
        assert set(told) == set(lt.TIE_CASES) | {"packets"}, told
    if variant == "hop_from_truncated_counter":
        assert set(told) == {"counter beyond 2^32", "packets"}, told


def test_lattice_holds_what_it_was_built_to_hold():
    names, tracks, pkts = lt.lattice_tracks(lt.REMAP)
    by = dict(zip(names, tracks))
    assert len(by) == len(names) - names.count(None) + (1 if None in names else 0)
    assert by["one event, three packets"].n_events == 1 and by["gap of ifs + 1: two events"].n_events == 2
    assert by["gap of ifs behind a long packet"].n_events == 2 and by["same channel, far apart"].n_events == 3
    assert by["channel change inside ifs"].n_events == 4 and by["two channels at one offset"].n_events == 4
    assert by["two streams at one MHz"].n_events == 3
    assert by["remainder +jitter"].n_fit == 3 and by["remainder +jitter+1"].n_fit == 2
    assert by["remainder -jitter"].n_fit == 3 and by["remainder -jitter-1"].n_fit == 2
    assert by["no fitting pair"].interval == 0 and by["no fitting pair"].flags == 0
    assert by["min is not the gcd"].interval == 6
    assert [bool(by["interval %d" % iv].flags & lt.TIMED) for iv in (5, 6, 3200, 3201)] == [False, True, True, False]
    for k in (2, 36, 37, 38):
        t = by["missed events, k = %d" % k]
        assert t.flags == lt.TIMED | lt.HOPPING and (t.interval, t.hop_increment, t.first_unmapped, t.n_off_hop) == (7, 13, 21, 0), (k, t)
    for h in range(5, 17):
        t = by["increment %d" % h]
        assert t.flags == lt.TIMED | lt.HOPPING and (t.interval, t.hop_increment, t.first_unmapped) == (6 + h, h, (3 * h) % 37), t
    assert [by["map of %d" % n].n_used for n in (37, 36, 3, 2, 1)] == [37, 36, 3, 2, 1]
    assert by["tie between two u"].flags == lt.TIMED and by["tie between two h"].flags == lt.TIMED
    assert by["events off the hop"].n_off_hop == 2
    assert by["offsets near 2^46"].first_anchor > (1 << 45) and by["offsets near 2^46"].flags == lt.TIMED | lt.HOPPING
    assert by["foreign streams among the members"].n_events == 7 and by["only foreign streams"] == lt.Track(*([0] * 12))
    assert sum(p is None for p in pkts) >= 40 + 6
    assert [by[n].n_events for n in lt.TIE_CASES] == [2, 1]                                   # the tie goes by list order
    t = by["counter beyond 2^32"]
    assert (t.interval, t.n_events, t.n_fit, t.flags, t.n_off_hop) == (6, 8, 7, lt.TIMED | lt.HOPPING, 0)
    conns, cands, _ = lt.lattice_list(2)
    g = names.index("counter beyond 2^32")
    assert max(c.offset for c in cands if c.channel == g) < 1 << 45
    assert sorted((p.event, p.counter) for c, p in zip(cands, pkts) if c.channel == g)[4:] == [(4, 5), (5, 6), (6, 7), (7, 9)]
    _, plain, _ = lt.lattice_tracks(0)
    assert dict(zip(names, plain))["map of 3"].n_on_hop < by["map of 3"].n_on_hop            # without REMAP most predictions are unknown


SWEEP = [(40, 20, 0.0), (60, 5, 0.0), (60, 2, 0.0), (30, 3, 0.0), (150, 37, 0.0), (120, 37, 0.1), (40, 9, 0.2)]
DRAWS = 400


def _draw(rng, n_events, n_used, loss):
    interval, h, u0 = int(rng.integers(6, 40)), int(rng.integers(5, 17)), int(rng.integers(0, 37))
    chmap = lt.random_map(rng, n_used)
    cands, seen = lt.synth(rng, n_events, chmap, interval, h, u0, loss=loss, jitter=20)
    return interval, h, u0, chmap, cands, seen


@pytest.mark.parametrize("n_events,n_used,loss", SWEEP)
def test_recovery_of_planted_connections(n_events, n_used, loss):
    """Every draw whose observed map is the planted one and that has two consecutive events comes out with the planted interval,
    increment and first unmapped channel (shifted to the first event seen), HOPPING set and no event off the hop."""
    rng = np.random.default_rng(1000 * n_events + 10 * n_used + int(10 * loss))
    qualified, wrong = 0, []
    for d in range(DRAWS):
        interval, h, u0, chmap, cands, seen = _draw(rng, n_events, n_used, loss)
        if not cands:
            continue
        (t,), _ = lt.track(cands, 1, lt.LATTICE_MHZ, lt.N_STREAMS, 1250, 200, 50, lt.REMAP)
        if t.map_mask != chmap or not any(b - a == 1 for a, b in zip(seen, seen[1:])):
            continue
        qualified += 1
        if (t.interval, t.hop_increment, t.first_unmapped, t.flags, t.n_off_hop) != (interval, h, (u0 + h * seen[0]) % 37,
                                                                                     lt.TIMED | lt.HOPPING, 0):
            wrong.append((d, interval, h, u0, hex(chmap), t))
    print("E %d, n_used %d, p %.1f: %d of %d draws qualify, %d wrong" % (n_events, n_used, loss, qualified, DRAWS, len(wrong)))
    assert qualified >= 0.95 * DRAWS, qualified
    assert not wrong, wrong[:3]


@pytest.mark.parametrize("n_events,loss,draws", [(12, 0.0, 400), (24, 0.3, 300)])
@pytest.mark.parametrize("flags", [0, lt.REMAP])
def test_recovery_with_an_incomplete_map(n_events, loss, draws, flags):
    """Every channel used, so few events that the observed map stays incomplete: every draw must still come out right."""
    rng = np.random.default_rng(77 + n_events)
    wrong = []
    for d in range(draws):
        interval, h, u0, chmap, cands, seen = _draw(rng, n_events, 37, loss)
        (t,), _ = lt.track(cands, 1, lt.LATTICE_MHZ, lt.N_STREAMS, 1250, 200, 50, flags) if cands else ((None,), None)
        if t is None or (t.interval, t.hop_increment, t.first_unmapped, t.flags, t.n_off_hop) != (
                interval, h, (u0 + h * seen[0]) % 37, lt.TIMED | lt.HOPPING, 0):
            wrong.append((d, interval, h, u0, seen, t))
    print("E %d, p %.1f, flags %d: %d of %d draws wrong" % (n_events, loss, flags, len(wrong), draws))
    assert not wrong, wrong[:3]


def test_chain_capture_holds_the_planted_connections():
    """The planted maps come out complete from the discovery's and the tracking's models; the fourth connection, seen at two
    events two intervals apart, comes out with the doubled interval (the documented limit)."""
    cap, planted = lt.chain_capture()
    conns, cands = lt.chain_model()
    tracks, pkts = lt.track(cands, len(conns), cap.mhz, len(cap.mhz), 1250, 200, 50, lt.REMAP)
    by = {(c.access_address, c.crc_init): t for c, t in zip(conns, tracks)}
    for k, p in enumerate(planted):
        t = by[(p.aa, p.crc_init)]
        if k < 3:
            assert (t.interval, t.hop_increment, t.first_unmapped, t.map_mask, t.flags, t.n_off_hop, t.n_events) == (
                p.interval, p.hop, (p.u0 + p.hop * p.counters[0]) % 37, p.chmap, lt.TIMED | lt.HOPPING, 0, len(p.counters)), (k, t)
        else:
            assert t.interval == 2 * p.interval and t.n_events == 2 and not t.flags & lt.HOPPING, t
    assert sum(p is not None for p in pkts) == sum(c.n_packets for c in conns)
    # the second connection's shifted alias on channel 3: a group of its own, on one channel, which the hop check does not pass
    aliases = [(c, t) for c, t in zip(conns, tracks) if c.access_address not in {p.aa for p in planted}]
    assert len(aliases) >= 1
    for c, t in aliases:
        assert c.access_address == (planted[1].aa >> 2) | (1 << 31) and c.channel_mask == 1 << 3 and c.n_packets >= 2
        assert not t.flags & lt.HOPPING, t


def test_packet_records_as_bytes():
    """pkt_array builds the records field by field with numpy: the same bytes as one record after the other, 0xFF for no member."""
    import libbtbb_amd as bt
    dtype = bt.LE_TRACK_PKT_DTYPE
    _, _, pkts = lt.lattice_tracks(lt.REMAP)
    pkts = [None] + pkts + [lt.Pkt(0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFF, 36, 0xFF, 0xFF, 0), None]
    assert sum(p is None for p in pkts) >= 3 and any(p is not None and p.counter > 1 << 31 for p in pkts)
    want = b"".join(b"\xff" * dtype.itemsize if p is None else np.array([tuple(p)], dtype).tobytes() for p in pkts)
    assert lt.pkt_array(pkts, dtype).tobytes() == want and lt.pkt_array([], dtype).tobytes() == b""
    assert lt.pkt_array([None], dtype).tobytes() == b"\xff" * 16


def test_layouts_and_loud_failure_without_a_device():
    import libbtbb_amd as bt
    assert bt.LE_TRACK_DTYPE.itemsize == 48 and bt.LE_TRACK_PKT_DTYPE.itemsize == 16
    assert [bt.LE_TRACK_DTYPE.fields[k][1] for k in lt.Track._fields + ("reserved",)] == [0, 8, 16, 20, 24, 28, 32, 36, 40, 41, 42, 43, 44]
    assert [bt.LE_TRACK_PKT_DTYPE.fields[k][1] for k in lt.Pkt._fields] == [0, 4, 8, 12, 13, 14, 15]
    assert (bt.LE_TRACK_REMAP, bt.LE_TRACK_TIMED, bt.LE_TRACK_HOPPING) == (lt.REMAP, lt.TIMED, lt.HOPPING)
    lib = bt.lib()
    assert lib.btbbx_le_track_scratch_bytes(1000, 10) >= 1000 * 40 + 10 * 444 * 4
    import torch
    if torch.cuda.is_available():
        return                                                   # (with a device they work: tests/test_gpu_le_track.py)
    words = np.zeros(64, np.uint64)
    phys = np.array([2404], np.uint16)
    buf = np.zeros(1 << 16, np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)                  # noqa: E731
    assert lib.btbbx_le_track_device(vp(buf), vp(buf[2048:]), 4, vp(buf[4096:]), vp(buf[2056:]), 4, vp(phys), 1, 1250, 200, 50, 0,
                                     vp(buf[8192:]), vp(buf[12288:]), vp(buf[16384:]), (1 << 16) - 16384, None) < 0
    assert lib.btbbx_last_error()
    assert lib.btbbx_le_track_host(vp(words), 64, 64, 1, 1000, vp(phys), 27, 2, vp(buf), 8, vp(buf[1024:]), 8, None,
                                   1250, 200, 50, 0, vp(buf[2048:]), vp(buf[4096:])) < 0
    with pytest.raises(bt.BtbbError):
        bt.le_track(words, 1000, [2404])
