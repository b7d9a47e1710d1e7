"""The LE connection tracking (libbtbb_amd/csrc/le_track.h) on the GPU: btbbx_le_track_device on the hand-built lattice of
tests/_le_track.py -- one connection per branch point of the seven rules --, on lists that cross the kernels' seams (a sort
tile, many waves, more connections than one workgroup's worth), and the chain discover -> track on a capture with four planted
connections, once through the host wrapper and once device-resident.  Every expectation is the model's (tests/_le_track.py),
byte for byte.  Output buffers start as 0xA5 and are one record longer than their caps, so a byte a kernel leaves unwritten, or
writes where it should not, shows.

The runs of tests/_le_track_paths.py (RUNS) pin the decomposition: lists whose connections begin and end on, one before and one
behind every boundary of a wave, a workgroup, a score tile and a scan tile, with values in them that a mistake in the wave-wide
tally, the merge of the waves' gcd, the 64-bit sums or the tile prefix would change.  tests/test_le_track_paths_model.py shows on
the CPU that each run carries its tags and that the runs carry all of them.  Two paths are left out on purpose: a fourth radix
pass over the connection index needs conn_cap >= 2^24, about 30 GB of scratch; a second round of the 64-bit tile prefix with
steps in it needs more than 524 288 EVENTS, too many for the plain model (the second round of the 32-bit prefix runs on the long
trains, that of the 64-bit prefix with zeros only)."""
import functools

import numpy as np
import pytest

import _le_discover as ld
import _le_track as lt
import _le_track_paths as lp
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu

CAND, CONN, TRACK, PKT = bt.LE_CAND_DTYPE, bt.LE_CONN_DTYPE, bt.LE_TRACK_DTYPE, bt.LE_TRACK_PKT_DTYPE
E_ARG = -3


@pytest.fixture(scope="module", autouse=True)
def _init():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    bt.init(2)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    pad = (-a.nbytes) % 8
    raw = np.frombuffer(a.tobytes() + bytes(pad), np.int64).copy() if a.nbytes else np.zeros(1, np.int64)
    return torch.from_numpy(raw).cuda()


def _filled(nbytes):
    import torch
    return torch.full(((nbytes + 7) // 8 * 8 + 8,), 0xA5, dtype=torch.uint8, device="cuda")


def _track_device(cand_arr, conn_arr, mhz, n_streams, flags, unit=lt.UNIT, ifs=lt.IFS, jitter=lt.JITTER, conn_cap=None, count=None,
                  cand_cap=None, conn_count=None):
    """btbbx_le_track_device over a grouped list -> (tracks buffer, pkts buffer), whole, one record longer than their caps."""
    import torch
    lib = bt.lib()
    n, k = len(cand_arr), len(conn_arr)
    count = n if count is None else count
    cand_cap = n if cand_cap is None else cand_cap
    conn_count = k if conn_count is None else conn_count
    conn_cap = k if conn_cap is None else conn_cap
    d_cands, d_conns, d_phys = _dev(cand_arr), _dev(conn_arr), _dev(np.asarray(mhz, np.uint16))
    d_tracks, d_pkts = _filled((conn_cap + 1) * TRACK.itemsize), _filled((cand_cap + 1) * PKT.itemsize)
    d_cnt = torch.from_numpy(np.array([count, conn_count], np.int64).astype(np.uint32).view(np.int32)).cuda()
    scratch = lib.btbbx_le_track_scratch_bytes(cand_cap, conn_cap)
    d_scr = _filled(scratch)
    bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), d_cnt.data_ptr(), cand_cap, d_conns.data_ptr(), d_cnt.data_ptr() + 4, conn_cap,
                                       d_phys.data_ptr(), n_streams, unit, ifs, jitter, flags, d_tracks.data_ptr(), d_pkts.data_ptr(),
                                       d_scr.data_ptr(), scratch, None), "btbbx_le_track_device")
    torch.cuda.synchronize()
    return (d_tracks.cpu().numpy()[:(conn_cap + 1) * TRACK.itemsize].view(TRACK), d_pkts.cpu().numpy()[:(cand_cap + 1) * PKT.itemsize].view(PKT))


def _check(conns, cands, mhz, n_streams, flags, want=None, cand_arr=None, **kw):
    """The device against the model (want: the model's (tracks, pkts), cand_arr: the candidates' records, when the caller has
    them already)."""
    n, k = len(cands), len(conns)
    work = min(kw.get("count", n) if kw.get("count") is not None else n, kw.get("cand_cap", n) if kw.get("cand_cap") is not None else n)
    kept = min(kw.get("conn_count", k) if kw.get("conn_count") is not None else k,
               kw.get("conn_cap", k) if kw.get("conn_cap") is not None else k)
    if want is None:
        want = lt.track(cands[:work], kept, mhz, n_streams, kw.get("unit", lt.UNIT), kw.get("ifs", lt.IFS), kw.get("jitter", lt.JITTER), flags)
    tracks, pkts = _track_device(ld.cand_array(cands, CAND) if cand_arr is None else cand_arr, ld.conn_array(conns, CONN), mhz, n_streams,
                                 flags, **kw)
    if kw.get("conn_cap") == 0 or kw.get("cand_cap") == 0:
        work = kept = 0
    want_t, want_p = lt.track_array(want[0][:kept], TRACK), lt.pkt_array(want[1][:work], PKT)
    if tracks[:kept].tobytes() != want_t.tobytes():
        bad = [g for g in range(kept) if tracks[g].tobytes() != want_t[g].tobytes()]
        raise AssertionError("connection %d: %s, model %s (%d differ)" % (bad[0], tracks[bad[0]], want_t[bad[0]], len(bad)))
    assert tracks[kept:].tobytes() == b"\xa5" * (TRACK.itemsize * (len(tracks) - kept))
    if pkts[:work].tobytes() != want_p.tobytes():
        bad = [i for i in range(work) if pkts[i].tobytes() != want_p[i].tobytes()]
        raise AssertionError("candidate %d %s: %s, model %s (%d differ)" % (bad[0], cands[bad[0]], pkts[bad[0]], want_p[bad[0]], len(bad)))
    assert pkts[work:].tobytes() == b"\xa5" * (PKT.itemsize * (len(pkts) - work))
    return want


# ---- hand-built lists ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _lattice(flags):
    conns, cands, names = lt.lattice_list(2)
    return conns, cands, names, lt.track(cands, len(conns), lt.LATTICE_MHZ, lt.N_STREAMS, lt.UNIT, lt.IFS, lt.JITTER, flags)


@pytest.mark.parametrize("flags", [0, lt.REMAP])
def test_track_on_the_lattice(flags):
    conns, cands, names, want = _lattice(flags)
    assert len(conns) >= 50 and sum(c.channel == ld.NO_CONN for c in cands) >= 40          # non-members lie between the groups
    _check(conns, cands, lt.LATTICE_MHZ, lt.N_STREAMS, flags, want=want)
    by = dict(zip(names, want[0]))
    print("lattice, flags %d: %d connections, %d candidates, %d TIMED, %d HOPPING" % (
        flags, len(conns), len(cands), sum(t.flags & 1 for t in want[0]), sum(t.flags >> 1 for t in want[0])))
    assert by["increment 16"].hop_increment == 16 and by["interval 3200"].flags & lt.TIMED and not by["interval 3201"].flags


@pytest.mark.parametrize("flags", [0, lt.REMAP])
def test_caps_and_counts_on_the_lattice(flags):
    conns, cands, _, _ = _lattice(flags)
    n, k = len(cands), len(conns)
    a = (conns, cands, lt.LATTICE_MHZ, lt.N_STREAMS, flags)
    _check(*a, conn_cap=k - 5)                                         # the connections cut off: their candidates are no members
    _check(*a, conn_cap=1)
    _check(*a, conn_cap=k + 300)                                       # more than eight bits of connection index
    _check(*a, conn_count=k - 11)
    _check(*a, conn_count=k + 1000)
    _check(*a, count=n - 7)
    _check(*a, count=n + 1000)                                         # a counter beyond the cap: the cap's worth is worked on
    _check(*a, cand_cap=n - 9)
    _check(*a, count=0)
    _check(*a, conn_count=0)
    _check(*a, conn_cap=0)                                             # nothing is written
    _check(*a, cand_cap=0)


def test_other_units_and_gaps():
    """The same list read with another unit, inter-frame gap and jitter: other events, other intervals."""
    conns, cands, _, _ = _lattice(0)
    _check(conns, cands, lt.LATTICE_MHZ, lt.N_STREAMS, lt.REMAP, unit=625, ifs=0, jitter=311)
    _check(conns, cands, lt.LATTICE_MHZ, lt.N_STREAMS, lt.REMAP, unit=2, ifs=100000, jitter=0)
    _check(conns, cands, lt.LATTICE_MHZ, 5, 0)                            # five streams: most members fall away


def test_bad_arguments_are_refused_before_any_launch():
    import torch
    lib = bt.lib()
    buf = _filled(1 << 16)
    p = buf.data_ptr()
    scratch = lib.btbbx_le_track_scratch_bytes(8, 4)
    assert scratch <= (1 << 16) - 8192

    def call(cands=p, cnt=p + 1024, conns=p + 2048, ccnt=p + 1028, phys=p + 3072, n_streams=1, unit=1250, jitter=50, tracks=p + 4096,
             pkts=p + 6144, scr=p + 8192, scr_bytes=scratch):
        return lib.btbbx_le_track_device(cands, cnt, 8, conns, ccnt, 4, phys, n_streams, unit, 200, jitter, 0, tracks, pkts, scr, scr_bytes, None)

    for kw in (dict(cands=None), dict(cnt=None), dict(conns=None), dict(ccnt=None), dict(phys=None), dict(tracks=None), dict(pkts=None),
               dict(scr=None), dict(cands=p + 4), dict(conns=p + 2052), dict(tracks=p + 4100), dict(pkts=p + 6148), dict(scr=p + 8196),
               dict(cnt=p + 1026), dict(n_streams=0), dict(unit=1), dict(unit=100, jitter=50), dict(scr_bytes=scratch - 1)):
        assert call(**kw) == E_ARG, kw
        assert lib.btbbx_last_error()
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == b"\xa5" * len(buf)
    assert call(unit=100, jitter=49) == 0                               # (counts of 0xa5a5a5a5: the caps' worth of 0xa5 records is read)
    torch.cuda.synchronize()


# ---- sizes that cross the kernels' seams ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seam_model():
    conns, cands = lt.seam_list()
    return lt.track(cands, len(conns), lt.LATTICE_MHZ, lt.N_STREAMS, lt.UNIT, lt.IFS, lt.JITTER, lt.REMAP)


def test_beyond_one_sort_tile_and_one_workgroup():
    """One connection of 5 000 events with two packets each (10 000 members: three sort tiles, five flag tiles, 157 waves) beside
    3 000 connections of 2 to 4 events."""
    conns, cands = lt.seam_list()
    assert len(conns) == 3001 and 15000 <= len(cands) <= 25000 and max(c.n_packets for c in conns) == 10000
    want = _check(conns, cands, lt.LATTICE_MHZ, lt.N_STREAMS, lt.REMAP, want=_seam_model())
    big = want[0][[c.n_packets for c in conns].index(10000)]
    assert (big.n_events, big.interval, big.hop_increment, big.first_unmapped, big.flags, big.n_off_hop) == (5000, 6, 11, 8, 3, 0), big


def test_seam_list_cut_by_the_caps():
    conns, cands = lt.seam_list()
    _check(conns, cands, lt.LATTICE_MHZ, lt.N_STREAMS, lt.REMAP, conn_cap=2000, cand_cap=len(cands) - 4097)


# ---- the waves, workgroups and tiles a connection begins and ends on ------------------------------------------------------
@pytest.mark.parametrize("run", [r for r in lp.RUNS if r.build == "align_list"], ids=lambda r: r.name)
def test_track_on_the_alignment_lists(run):
    """Connections of 63 to 3 071 events back to back, each group from a multiple of its unit; counters beyond 2^32 in front of
    all others; a gcd that needs the merge of three waves, and one that needs the pair at lane 63 / at thread 255; events planted
    off the hop in waves of one connection and in shared ones.  Once more with three radix passes over the connection index, with
    a capacity of more than 256 scan tiles, and with a count that ends mid-wave inside the connection with the planted events."""
    conns, cands, names = lp.run_list(run)
    assert set(run.tags) <= lp.run_tags(run)
    want = _check(conns, cands, lt.LATTICE_MHZ, lt.N_STREAMS, run.flags, want=lp.run_model(run), **lp.run_kw(run))
    off = want[0][names.index("off hop")]
    print("%s: %d connections, %d candidates, %d events, %d planted off the hop" % (
        run.name, len(conns), len(cands), sum(t.n_events for t in want[0]), off.n_off_hop))
    assert off.n_off_hop >= 1


def test_more_connections_than_sixteen_bits_number():
    """65 544 connections: 65 540, most of one event, and four that hop behind them, at indices that differ from those of
    connections 4 to 7 in the third byte alone, and at the same time as these."""
    (run,) = [r for r in lp.RUNS if r.build == "crowd_list"]
    conns, cands, names = lp.run_list(run)
    assert len(conns) == lt.CROWD + 4 and names[-4:] == ["behind a", "behind b", "behind c", "behind d"] and set(run.tags) <= lp.run_tags(run)
    want = _check(conns, cands, lt.LATTICE_MHZ, lt.N_STREAMS, run.flags, want=lp.run_model(run))
    assert [(t.n_events, t.interval) for t in want[0][-4:]] == [(12, 6), (9, 6), (6, 6), (70, 6)]


def test_more_slots_than_one_round_of_the_tile_prefix():
    """Forty events of 13 300 packets each -- 532 000 slots, 260 scan tiles, most of which open no event -- and three small
    connections whose slots and events lie behind tile 256."""
    (run,) = [r for r in lp.RUNS if r.build == "long_event_list"]
    conns, cands, names, fields = lt.long_event_list()
    assert len(cands) > lp.PREFIX_ROUND * lp.LT_TILE and set(run.tags) <= lp.run_tags(run)
    arr = np.zeros(len(cands), CAND)
    for k, name in enumerate(("offset", "access_address", "crc_init", "stream", "header0", "length", "conn")):
        arr[name] = fields[:, k]
    assert arr[:50].tobytes() == ld.cand_array(cands[:50], CAND).tobytes() and arr[-50:].tobytes() == ld.cand_array(cands[-50:], CAND).tobytes()
    for name, field in (("offset", "offset"), ("stream", "stream"), ("length", "length"), ("conn", "channel")):       # every record
        assert np.array_equal(arr[name].astype(np.int64), np.fromiter((getattr(c, field) for c in cands), np.int64, len(cands))), name
    want = _check(conns, cands, lt.LATTICE_MHZ, lt.N_STREAMS, run.flags, want=lp.run_model(run), cand_arr=arr)
    assert [t.n_events for t in want[0]] == [40, 30, 5, 5] and want[0][0].interval == 3200


# ---- the chain ----------------------------------------------------------------------------------------------------------
def test_chain_discover_then_track():
    import torch
    lib = bt.lib()
    cap, planted = lt.chain_capture()
    want_conns, want_cands = lt.chain_model()
    want_tracks, want_pkts = lt.track(want_cands, len(want_conns), cap.mhz, len(cap.mhz), 1250, 200, 50, lt.REMAP)
    n_cands, n_conns = len(want_cands), len(want_conns)
    # from Python, through the host wrapper
    conns, cands, tracks, pkts = bt.le_track(cap.words, cap.search_bits, cap.mhz, max_len=27, min_count=2, n_streams=len(cap.mhz),
                                             pitch_words=cap.pitch_words, n_words=cap.n_words, unit_bits=1250, ifs_bits=200, jitter_bits=50,
                                             flags=bt.LE_TRACK_REMAP)
    assert conns.tobytes() == ld.conn_array(want_conns, CONN).tobytes() and cands.tobytes() == ld.cand_array(want_cands, CAND).tobytes()
    assert tracks.tobytes() == lt.track_array(want_tracks, TRACK).tobytes()
    assert pkts.tobytes() == lt.pkt_array(want_pkts, PKT).tobytes()
    # the device chain, nothing read back between the stages
    cand_cap, conn_cap = n_cands + 100, 64
    d_words, d_phys = _dev(cap.words.reshape(-1)), _dev(cap.mhz.astype(np.uint16))
    d_cands, d_conns = _filled(cand_cap * CAND.itemsize), _filled(conn_cap * CONN.itemsize)
    d_tracks, d_pkts = _filled((conn_cap + 1) * TRACK.itemsize), _filled((cand_cap + 1) * PKT.itemsize)
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    scratch, tscratch = lib.btbbx_le_discover_scratch_bytes(cand_cap), lib.btbbx_le_track_scratch_bytes(cand_cap, conn_cap)
    d_scr, d_tscr = torch.zeros(scratch // 8 + 2, dtype=torch.int64, device="cuda"), _filled(tscratch)
    bt.check(lib.btbbx_le_discover_scan_device(d_words.data_ptr(), cap.n_words, cap.pitch_words, len(cap.mhz), cap.search_bits,
                                               d_phys.data_ptr(), 27, d_cands.data_ptr(), cand_cap, d_cnt.data_ptr(), None))
    bt.check(lib.btbbx_le_discover_group_device(d_cands.data_ptr(), d_cnt.data_ptr(), cand_cap, 2, d_conns.data_ptr(), conn_cap,
                                                d_cnt.data_ptr() + 4, d_scr.data_ptr(), scratch, None))
    bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), d_cnt.data_ptr(), cand_cap, d_conns.data_ptr(), d_cnt.data_ptr() + 4, conn_cap,
                                       d_phys.data_ptr(), len(cap.mhz), 1250, 200, 50, lt.REMAP, d_tracks.data_ptr(), d_pkts.data_ptr(),
                                       d_tscr.data_ptr(), tscratch, None))
    torch.cuda.synchronize()
    assert (int(d_cnt[0].item()), int(d_cnt[1].item())) == (n_cands, n_conns) and n_conns <= conn_cap
    got_t = d_tracks.cpu().numpy()[:(conn_cap + 1) * TRACK.itemsize]
    got_p = d_pkts.cpu().numpy()[:(cand_cap + 1) * PKT.itemsize]
    assert got_t[:n_conns * TRACK.itemsize].tobytes() == tracks.tobytes() and set(got_t[n_conns * TRACK.itemsize:].tolist()) == {0xA5}
    assert got_p[:n_cands * PKT.itemsize].tobytes() == pkts.tobytes() and set(got_p[n_cands * PKT.itemsize:].tolist()) == {0xA5}
    # the planted connections: interval, increment and map as planted; the fourth with the doubled interval the rules give
    by_key = {(int(k["access_address"]), int(k["crc_init"])): g for g, k in enumerate(conns)}
    own = {}
    for i, p in enumerate(planted):
        t = tracks[by_key[(p.aa, p.crc_init)]]
        own[p.aa] = int(t["n_on_hop"])
        if i < 3:
            assert (int(t["interval"]), int(t["hop_increment"]), int(t["first_unmapped"]), int(t["map_mask"]), int(t["flags"]),
                    int(t["n_off_hop"]), int(t["n_events"])) == (p.interval, p.hop, (p.u0 + p.hop * p.counters[0]) % 37, p.chmap,
                                                                 lt.TIMED | lt.HOPPING, 0, len(p.counters)), (i, t)
        else:
            assert int(t["interval"]) == 2 * p.interval and int(t["n_events"]) == 2 and not int(t["flags"]) & lt.HOPPING, t
    # every other group is an alias of a planted connection: not TIMED, or not HOPPING, or fewer events on the hop than its source
    spans = {}
    for p in cap.planted:
        spans.setdefault(p.stream, []).append(p)
    aliases = 0
    for (aa, ci), g in by_key.items():
        if aa in own:
            continue
        c = cands[int(conns[g]["first"])]
        near = [p for p in spans.get(int(c["stream"]), []) if p.offset - 8 <= int(c["offset"]) < p.offset + 80 + 8 * p.length]
        assert len(near) == 1, (hex(aa), c)
        t = tracks[g]
        aliases += 1
        assert int(t["flags"]) != lt.TIMED | lt.HOPPING or int(t["n_on_hop"]) < own[near[0].aa], (hex(aa), t, own[near[0].aa])
    print("chain: %d candidates, %d connections, %d of them aliases" % (n_cands, n_conns, aliases))
