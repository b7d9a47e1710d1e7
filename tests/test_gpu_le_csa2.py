"""The LE channel selection #2 stage (libbtbb_amd/csrc/le_csa2.h) on the GPU: hand-built candidate lists run through
btbbx_le_track_device and then btbbx_le_csa2_device, as tests/test_gpu_le_track.py runs the tracking -- the lattice of
tests/_le_csa2.py, the runs of tests/_le_csa2_paths.py that put winners and runners-up where the kernels split the work, lists that
cross the kernels' seams (several LDS tiles of events per work item, more connections than sixteen
bits number), and the chain discover -> track -> select on a capture, once through the host wrapper and once device-resident.
Every expectation is the model's (tests/_le_csa2.py on top of tests/_le_track.py's model of the tracking), byte for byte.  Output
buffers start as 0xA5 and are one record longer than their caps, so a byte a kernel leaves unwritten, or writes where it should
not, shows."""
import functools

import numpy as np
import pytest

import _le_csa2 as lc
import _le_csa2_paths as lp
import _le_discover as ld
import _le_track as lt
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu

CAND, CONN, TRACK, PKT, SEL, SEL_PKT = (bt.LE_CAND_DTYPE, bt.LE_CONN_DTYPE, bt.LE_TRACK_DTYPE, bt.LE_TRACK_PKT_DTYPE, bt.LE_CSA2_DTYPE,
                                        bt.LE_CSA2_PKT_DTYPE)
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


def _select_device(cand_arr, conn_arr, flags, conn_cap=None, count=None, cand_cap=None, conn_count=None):
    """btbbx_le_track_device, then btbbx_le_csa2_device on what it left -> (sel buffer, sel_pkts buffer), whole, one record longer
    than their caps."""
    import torch
    lib = bt.lib()
    n, k = len(cand_arr), len(conn_arr)
    count = n if count is None else count
    cand_cap = n if cand_cap is None else cand_cap
    conn_count = k if conn_count is None else conn_count
    conn_cap = k if conn_cap is None else conn_cap
    d_cands, d_conns, d_phys = _dev(cand_arr), _dev(conn_arr), _dev(np.asarray(lt.LATTICE_MHZ, np.uint16))
    d_tracks, d_pkts = _filled((conn_cap + 1) * TRACK.itemsize), _filled((cand_cap + 1) * PKT.itemsize)
    d_sel, d_sel_pkts = _filled((conn_cap + 1) * SEL.itemsize), _filled((cand_cap + 1) * SEL_PKT.itemsize)
    d_cnt = torch.from_numpy(np.array([count, conn_count], np.int64).astype(np.uint32).view(np.int32)).cuda()
    tscratch, scratch = lib.btbbx_le_track_scratch_bytes(cand_cap, conn_cap), lib.btbbx_le_csa2_scratch_bytes(cand_cap, conn_cap)
    d_tscr, d_scr = _filled(tscratch), _filled(scratch)
    bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), d_cnt.data_ptr(), cand_cap, d_conns.data_ptr(), d_cnt.data_ptr() + 4, conn_cap,
                                       d_phys.data_ptr(), lt.N_STREAMS, lt.UNIT, lt.IFS, lt.JITTER, flags, d_tracks.data_ptr(),
                                       d_pkts.data_ptr(), d_tscr.data_ptr(), tscratch, None), "btbbx_le_track_device")
    # (flags + 6: only bit 0 is read)
    bt.check(lib.btbbx_le_csa2_device(d_cands.data_ptr(), d_cnt.data_ptr(), cand_cap, d_conns.data_ptr(), d_cnt.data_ptr() + 4, conn_cap,
                                      d_tracks.data_ptr(), d_pkts.data_ptr(), flags + 6, d_sel.data_ptr(), d_sel_pkts.data_ptr(),
                                      d_scr.data_ptr(), scratch, None), "btbbx_le_csa2_device")
    torch.cuda.synchronize()
    return (d_sel.cpu().numpy()[:(conn_cap + 1) * SEL.itemsize].view(SEL), d_sel_pkts.cpu().numpy()[:(cand_cap + 1) * SEL_PKT.itemsize].view(SEL_PKT))


def _check(conns, cands, flags, want=None, **kw):
    """The device against the model (want: the model's (sels, sel_pkts), when the caller has them already)."""
    n, k = len(cands), len(conns)
    get = lambda name, default: default if kw.get(name) is None else kw[name]          # noqa: E731
    work, kept = min(get("count", n), get("cand_cap", n)), min(get("conn_count", k), get("conn_cap", k))
    if want is None:
        tracks, pkts = lc.tracked(conns, cands, flags, work, kept)
        want = lc.select(conns[:kept], cands[:work], tracks, pkts, flags)
    sel, sel_pkts = _select_device(ld.cand_array(cands, CAND), ld.conn_array(conns, CONN), flags, **kw)
    if kw.get("conn_cap") == 0 or kw.get("cand_cap") == 0:
        work = kept = 0
    want_s, want_p = lc.sel_array(want[0][:kept], SEL), lc.sel_pkt_array(want[1][:work], SEL_PKT)
    if sel[:kept].tobytes() != want_s.tobytes():
        bad = [g for g in range(kept) if sel[g].tobytes() != want_s[g].tobytes()]
        raise AssertionError("connection %d: %s, model %s (%d differ)" % (bad[0], sel[bad[0]], want_s[bad[0]], len(bad)))
    assert sel[kept:].tobytes() == b"\xa5" * (SEL.itemsize * (len(sel) - kept))
    if sel_pkts[:work].tobytes() != want_p.tobytes():
        bad = [i for i in range(work) if sel_pkts[i].tobytes() != want_p[i].tobytes()]
        raise AssertionError("candidate %d %s: %s, model %s (%d differ)" % (bad[0], cands[bad[0]], sel_pkts[bad[0]], want_p[bad[0]], len(bad)))
    assert sel_pkts[work:].tobytes() == b"\xa5" * (SEL_PKT.itemsize * (len(sel_pkts) - work))
    return want


# ---- hand-built lists ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, lc.REMAP])
def test_select_on_the_lattice(flags):
    conns, cands, names = lc.lattice_list()
    assert sum(c.channel == ld.NO_CONN for c in cands) >= 40                               # non-members lie between the groups
    tracks, _, want = lc.lattice_model(flags)
    _check(conns, cands, flags, want=want)
    by = dict(zip(names, want[0]))
    print("lattice, flags %d: %d connections, %d candidates, %d EVALUATED, %d UNIQUE, %d PREFERRED" % (
        flags, len(conns), len(cands), sum(s.flags & 1 for s in want[0]), sum(s.flags >> 1 & 1 for s in want[0]), sum(s.flags >> 2 for s in want[0])))
    assert (by["wrap inside"].counter0, by["wrap inside"].n_on) == (65530, 12) and by["n_e beyond 2^32"].flags == 7
    assert by["no members"].flags == 0 and by["not TIMED: interval 5"].flags == 0 and not by["algorithm #1"].flags & lc.PREFERRED
    if flags:                                                              # the forced ties: the smaller counter wins, the other is the runner-up
        for name, tie in (("tie across two blocks", lc.TIE_ACROSS), ("tie inside one block", lc.TIE_INSIDE)):
            assert (by[name].counter0, by[name].n_on, by[name].n_second, by[name].flags) == (tie[1], 6, 6, lc.EVALUATED), (name, by[name])


@pytest.mark.parametrize("flags", [0, lc.REMAP])
def test_caps_and_counts_on_the_lattice(flags):
    conns, cands, _ = lc.lattice_list()
    n, k = len(cands), len(conns)
    a = (conns, cands, flags)
    _check(*a, conn_cap=k - 5)                                         # the connections cut off: their candidates are no members
    _check(*a, conn_cap=1)
    _check(*a, conn_cap=k + 300)
    _check(*a, conn_count=k - 11)
    _check(*a, conn_count=k + 1000)
    _check(*a, count=n - 7)
    _check(*a, count=n + 1000)                                         # a counter beyond the cap: the cap's worth is worked on
    _check(*a, cand_cap=n - 9)
    _check(*a, count=0)
    _check(*a, conn_count=0)
    _check(*a, conn_cap=0)                                             # nothing is written
    _check(*a, cand_cap=0)


def test_bad_arguments_are_refused_before_any_launch():
    import torch
    lib = bt.lib()
    buf = _filled(1 << 16)
    p = buf.data_ptr()
    scratch = lib.btbbx_le_csa2_scratch_bytes(8, 4)
    assert scratch <= (1 << 16) - 12288

    def call(cands=p, cnt=p + 1024, conns=p + 2048, ccnt=p + 1028, tracks=p + 4096, pkts=p + 6144, sel=p + 8192, sel_pkts=p + 10240,
             scr=p + 12288, scr_bytes=scratch):
        return lib.btbbx_le_csa2_device(cands, cnt, 8, conns, ccnt, 4, tracks, pkts, 1, sel, sel_pkts, scr, scr_bytes, None)

    for kw in (dict(cands=None), dict(cnt=None), dict(conns=None), dict(ccnt=None), dict(tracks=None), dict(pkts=None), dict(sel=None),
               dict(sel_pkts=None), dict(scr=None), dict(cands=p + 4), dict(conns=p + 2052), dict(tracks=p + 4100), dict(pkts=p + 6148),
               dict(sel=p + 8196), dict(sel_pkts=p + 10244), dict(scr=p + 12292), dict(cnt=p + 1026), dict(ccnt=p + 1030),
               dict(scr_bytes=scratch - 1)):
        assert call(**kw) == E_ARG, kw
        assert lib.btbbx_last_error()
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == b"\xa5" * len(buf)
    assert call() == 0                               # (counts of 0xa5a5a5a5: the caps' worth of 0xa5 records is read, every event base cut at 8)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert got[10240:10240 + 64].tobytes() == b"\xff" * 64 and got[10240 + 64:12288].tobytes() == b"\xa5" * (2048 - 64)
    assert got[8192 + 96:10240].tobytes() == b"\xa5" * (2048 - 96) and got[:8192].tobytes() == b"\xa5" * 8192


# ---- where the kernels split the work: the runs of tests/_le_csa2_paths.py -----------------------------------------------------
def _run(name):
    """One run of lp.RUNS on the device against the models; a cut run with conn_cap one below the connections, which drops the last
    one: other event bases, another grid.  Returns (names, sels)."""
    run = [r for r in lp.RUNS if r.name == name][0]
    conns, cands, names = lp.run_list(run)
    want = lp.run_model(run)[2]
    if run.cut:
        _check(conns, cands, run.flags, want=lc.without_last_connection(conns, cands, want), conn_cap=len(conns) - 1)
    else:
        _check(conns, cands, run.flags, want=want)
    return names, want[0]


@pytest.mark.parametrize("flags", [0, lc.REMAP])
def test_pairs_of_planted_hypotheses(flags):
    """37 connections of 32 events on one chId, 18 on hypothesis A and 14 on B, or 16 and 16: winner and runner-up in one lane, in
    one wave, at threads 63 | 64, in two waves, in two blocks (0 and 63, adjacent ones at j = 1023 | 0), each UNIQUE in both orders
    and as an exact tie."""
    names, sels = _run("pairs, REMAP" if flags else "pairs")
    by = dict(zip(names, sels))
    for name, (a, b, tie) in lc.PAIRS.items():
        assert (by[name].counter0, by[name].n_on, by[name].n_second, by[name].flags & 3) == ((min(a, b), 16, 16, 1) if tie else (a, 18, 14, 3)), (name, by[name])


def test_winners_at_the_ends_of_wide_windows():
    """Gaps that widen the window to 1 024 + 1 711 and to the cut, winners at j = 1023 and j = 0; d_last at the cut - 1, the cut,
    the cut + 1; far events that decide; a tile over more than 2^16 counters; n_e wrapping inside the second tile; block 63."""
    names, sels = _run("windows, REMAP")
    by = dict(zip(names, sels))
    assert [(by[w.name].counter0, by[w.name].flags) for w in lc.WINDOWS] == [(w.counter0, 7) for w in lc.WINDOWS]
    assert (by["tile spans 2^16"].n_on, by["n_e wraps in tile two"].n_on, by["d_last cut + 1"].n_on) == (600, 722, 32)


@pytest.mark.parametrize("flags", [0, lc.REMAP])
def test_tile_counts_and_events_off_the_prediction_behind_event_63(flags):
    """511, 512, 513, 1 024 and 1 025 events; events off the prediction at 63, 64, 511, 512, 513 and at the end; a map of 20
    channels, whose unknown predictions count on neither side without REMAP; a runner-up that the second tile alone makes."""
    names, sels = _run("counts, REMAP" if flags else "counts")
    by = dict(zip(names, sels))
    assert (by["1025 events"].n_on, by["1025 events"].n_off, by["1025 events"].counter0) == (1019, 6, 1023)
    assert by["map of 20, last event off"].n_off == 3 and (by["map of 20, last event off"].n_on == 600) == bool(flags)
    assert (by["second only in tile two"].n_on, by["second only in tile two"].n_second >= 60) == (543, True)


@pytest.mark.parametrize("group", ["windows", "counts"])
def test_wide_connections_with_the_last_one_cut_off(group):
    _run("%s, REMAP, cut" % group)


# ---- sizes that cross the kernels' seams ------------------------------------------------------------------------------
def test_many_tiles_of_events_beside_many_small_connections():
    """One connection of 5 000 events with two packets each (ten LDS tiles in each of its 64 work items, one with a gap inside the
    window and one with a gap beyond it) beside 1 000 connections of 2 to 4 events: 64 064 work items for a grid of a few thousand
    workgroups."""
    conns, cands, names = lc.seam_list()
    assert len(conns) == 1001 and max(c.n_packets for c in conns) == 10000
    want = _check(conns, cands, lc.REMAP)
    big = want[0][names.index("large")]
    assert (big.n_on, big.n_off, big.counter0, big.flags) == (5000, 0, 60000, 7), big
    print("seams: %d connections, %d UNIQUE" % (len(conns), sum(s.flags >> 1 & 1 for s in want[0])))


@functools.lru_cache(maxsize=None)
def _crowd_model():
    conns, cands, names = lc.crowd_list()
    tracks, pkts = lc.tracked(conns, cands, lc.REMAP)
    return tracks, pkts, lc.select(conns, cands, tracks, pkts, lc.REMAP)


def test_more_connections_than_sixteen_bits_number():
    """65 544 connections, most of one event (not TIMED: the scoring pass strides over their 4.2 million work items without
    working on them), sixteen of ten events among them and four behind connection 65 539."""
    conns, cands, names = lc.crowd_list()
    assert len(conns) == lc.CROWD + 4 and names[-4:] == ["behind"] * 4 and names.count("ten events") == 16
    want = _crowd_model()[2]
    _check(conns, cands, lc.REMAP, want=want)
    assert [s.n_on for s in want[0][-4:]] == [12, 9, 30, 70] and all(s.flags == 7 for s in want[0][-2:])


def test_the_crowd_through_a_small_conn_cap():
    conns, cands, _ = lc.crowd_list()
    _check(conns, cands, lc.REMAP, conn_cap=9000)


# ---- the chain ----------------------------------------------------------------------------------------------------------
def test_chain_discover_track_select():
    import torch
    lib = bt.lib()
    cap, planted = lc.chain_capture()
    want_conns, want_cands = lc.chain_model()
    want_tracks, want_pkts = lt.track(want_cands, len(want_conns), cap.mhz, len(cap.mhz), 1250, 200, 50, lc.REMAP)
    want_sel, want_sel_pkts = lc.select(want_conns, want_cands, want_tracks, want_pkts, lc.REMAP)
    n_cands, n_conns = len(want_cands), len(want_conns)
    # from Python, through the host wrapper
    conns, cands, tracks, pkts, sel, sel_pkts = bt.le_csa2(cap.words, cap.search_bits, cap.mhz, max_len=27, min_count=2, n_streams=len(cap.mhz),
                                                           pitch_words=cap.pitch_words, n_words=cap.n_words, unit_bits=1250, ifs_bits=200,
                                                           jitter_bits=50, flags=bt.LE_CSA2_REMAP)
    assert conns.tobytes() == ld.conn_array(want_conns, CONN).tobytes() and cands.tobytes() == ld.cand_array(want_cands, CAND).tobytes()
    assert tracks.tobytes() == lt.track_array(want_tracks, TRACK).tobytes() and pkts.tobytes() == lt.pkt_array(want_pkts, PKT).tobytes()
    assert sel.tobytes() == lc.sel_array(want_sel, SEL).tobytes()
    assert sel_pkts.tobytes() == lc.sel_pkt_array(want_sel_pkts, SEL_PKT).tobytes()
    # the device chain, nothing read back between the stages
    cand_cap, conn_cap = n_cands + 100, 64
    d_words, d_phys = _dev(cap.words.reshape(-1)), _dev(cap.mhz.astype(np.uint16))
    d_cands, d_conns = _filled(cand_cap * CAND.itemsize), _filled(conn_cap * CONN.itemsize)
    d_tracks, d_pkts = _filled((conn_cap + 1) * TRACK.itemsize), _filled((cand_cap + 1) * PKT.itemsize)
    d_sel, d_sel_pkts = _filled((conn_cap + 1) * SEL.itemsize), _filled((cand_cap + 1) * SEL_PKT.itemsize)
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    scratch, tscratch = lib.btbbx_le_discover_scratch_bytes(cand_cap), lib.btbbx_le_track_scratch_bytes(cand_cap, conn_cap)
    sscratch = lib.btbbx_le_csa2_scratch_bytes(cand_cap, conn_cap)
    d_scr, d_tscr, d_sscr = torch.zeros(scratch // 8 + 2, dtype=torch.int64, device="cuda"), _filled(tscratch), _filled(sscratch)
    bt.check(lib.btbbx_le_discover_scan_device(d_words.data_ptr(), cap.n_words, cap.pitch_words, len(cap.mhz), cap.search_bits,
                                               d_phys.data_ptr(), 27, d_cands.data_ptr(), cand_cap, d_cnt.data_ptr(), None))
    bt.check(lib.btbbx_le_discover_group_device(d_cands.data_ptr(), d_cnt.data_ptr(), cand_cap, 2, d_conns.data_ptr(), conn_cap,
                                                d_cnt.data_ptr() + 4, d_scr.data_ptr(), scratch, None))
    bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), d_cnt.data_ptr(), cand_cap, d_conns.data_ptr(), d_cnt.data_ptr() + 4, conn_cap,
                                       d_phys.data_ptr(), len(cap.mhz), 1250, 200, 50, lc.REMAP, d_tracks.data_ptr(), d_pkts.data_ptr(),
                                       d_tscr.data_ptr(), tscratch, None))
    bt.check(lib.btbbx_le_csa2_device(d_cands.data_ptr(), d_cnt.data_ptr(), cand_cap, d_conns.data_ptr(), d_cnt.data_ptr() + 4, conn_cap,
                                      d_tracks.data_ptr(), d_pkts.data_ptr(), lc.REMAP, d_sel.data_ptr(), d_sel_pkts.data_ptr(),
                                      d_sscr.data_ptr(), sscratch, None))
    torch.cuda.synchronize()
    assert (int(d_cnt[0].item()), int(d_cnt[1].item())) == (n_cands, n_conns) and n_conns <= conn_cap
    got_s = d_sel.cpu().numpy()[:(conn_cap + 1) * SEL.itemsize]
    got_p = d_sel_pkts.cpu().numpy()[:(cand_cap + 1) * SEL_PKT.itemsize]
    assert got_s[:n_conns * SEL.itemsize].tobytes() == sel.tobytes() and set(got_s[n_conns * SEL.itemsize:].tolist()) == {0xA5}
    assert got_p[:n_cands * SEL_PKT.itemsize].tobytes() == sel_pkts.tobytes() and set(got_p[n_cands * SEL_PKT.itemsize:].tolist()) == {0xA5}
    assert d_tracks.cpu().numpy()[:n_conns * TRACK.itemsize].tobytes() == tracks.tobytes()     # (the tracking's records are only read)
    # the planted connections: those of algorithm #2 PREFERRED with their planted counters and every event on the prediction; the
    # one of algorithm #1 HOPPING and not PREFERRED
    by_key = {(int(c["access_address"]), int(c["crc_init"])): g for g, c in enumerate(conns)}
    own = set()
    for p in planted:
        g = by_key[(p.aa, p.crc_init)]
        own.add(p.aa)
        s, t = sel[g], tracks[g]
        if p.algorithm == 2:
            assert (int(s["flags"]), int(s["counter0"]), int(s["n_on"]), int(s["n_off"])) == (7, (p.counter0 + p.counters[0]) % 65536,
                                                                                              len(p.counters), 0), (p, s)
            assert int(t["map_mask"]) & ~p.chmap == 0 and int(t["n_on_hop"]) < int(s["n_on"]), (p, t)
            assert int(t["map_mask"]) == p.chmap or p.chmap == lc.FULL_MAP             # (42 events do not show all 37 channels)
            mine = np.flatnonzero(cands["conn"] == g)
            assert len(mine) and sel_pkts["on_hop"][mine].all()
            assert np.array_equal(sel_pkts["counter"][mine], (p.counter0 + pkts["counter"][mine]) % 65536)
        else:
            assert int(t["flags"]) == lt.TIMED | lt.HOPPING and not int(s["flags"]) & lc.PREFERRED, (p, s, t)
    aliases = [g for (aa, _), g in by_key.items() if aa not in own]
    assert aliases and not any(int(sel[g]["flags"]) & lc.PREFERRED for g in aliases), sel[aliases]
    print("chain: %d candidates, %d connections, %d of them aliases, %d of those EVALUATED" % (
        n_cands, n_conns, len(aliases), sum(int(sel[g]["flags"]) & 1 for g in aliases)))
