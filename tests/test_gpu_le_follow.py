"""LE following from CONNECT_IND (libbtbb_amd/csrc/le_follow.h) on the GPU: the planted worlds of tests/_le_follow.py run through
btbbx_le_track_device, btbbx_le_seed_device and btbbx_le_epoch_device -- the lattice, caps and counts on it, the refusals, the
list that crosses the kernels' seams -- and the chain scan -> discover -> track -> seed -> follow on a capture, once through the host
wrapper and once device-resident.  Every expectation is the model's (tests/_le_follow.py on top of tests/_le_track.py's model of
the tracking), byte for byte.  Output buffers start as 0xA5 and are one record longer than their caps, so a byte a kernel leaves
unwritten, or writes where it should not, shows.

The worlds of tests/_le_follow_paths.py drive the kernels' decomposition -- tile prefix, rounds, radix passes over more than one tile
and over the connection's second byte, the searches' ends, the per-wave runs --; which tag each carries is asserted on the CPU
(tests/test_le_follow_paths_model.py) and once more here, in front of the run."""
import numpy as np
import pytest

import _le_discover as ld
import _le_follow as lf
import _le_follow_paths as lp
import _le_track as lt
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu

CAND, CONN, TRACK, PKT, ADV = bt.LE_CAND_DTYPE, bt.LE_CONN_DTYPE, bt.LE_TRACK_DTYPE, bt.LE_TRACK_PKT_DTYPE, bt.LE_PKT_DTYPE
SEED, FOLLOW, FPKT = bt.LE_SEED_DTYPE, bt.LE_FOLLOW_DTYPE, bt.LE_FOLLOW_PKT_DTYPE
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
    return torch.full(((nbytes + 15) // 16 * 16 + 16,), 0xA5, dtype=torch.uint8, device="cuda")


def _records(buf, n, dtype):
    return buf.cpu().numpy()[:n * dtype.itemsize].view(dtype)


def _follow_device(b, conn_cap=None, count=None, cand_cap=None, conn_count=None, adv_cap=None, adv_count=None, pad_words=0, records=None):
    """Tracking, seed and follow on the device -> (seeds, follows, fpkts), each whole, one record longer than its cap.
    pad_words: the rows of the streams that many words apart, the words between them all ones; records: (conns, tracks, pkts)
    as arrays -- the tracking is not run, the seed and follow stages get these in its place."""
    import torch
    lib = bt.lib()
    n, k, m = len(b.cands), len(b.conns), len(b.adv)
    count, cand_cap = n if count is None else count, n if cand_cap is None else cand_cap
    conn_count, conn_cap = k if conn_count is None else conn_count, k if conn_cap is None else conn_cap
    adv_count, adv_cap = m if adv_count is None else adv_count, m if adv_cap is None else adv_cap
    d_cands, d_conns = _dev(ld.cand_array(b.cands, CAND)), _dev(ld.conn_array(b.conns, CONN))
    words = b.words
    if pad_words:
        words = np.full((len(b.words), b.n_words + pad_words), ~np.uint64(0), np.uint64)
        words[:, :b.n_words] = b.words
    d_phys, d_words, d_adv = _dev(np.asarray(lt.LATTICE_MHZ, np.uint16)), _dev(words.reshape(-1)), _dev(lf.adv_array(b.adv, ADV))
    d_tracks, d_pkts = _filled((conn_cap + 1) * TRACK.itemsize), _filled((cand_cap + 1) * PKT.itemsize)
    d_seeds, d_follows = _filled((conn_cap + 1) * SEED.itemsize), _filled((conn_cap + 1) * FOLLOW.itemsize)
    d_fpkts = _filled((cand_cap + 1) * FPKT.itemsize)
    d_cnt = torch.from_numpy(np.array([count, conn_count, adv_count], np.int64).astype(np.uint32).view(np.int32)).cuda()
    tscratch, scratch = lib.btbbx_le_track_scratch_bytes(cand_cap, conn_cap), lib.btbbx_le_epoch_scratch_bytes(cand_cap, conn_cap)
    d_tscr, d_scr = _filled(tscratch), _filled(scratch)
    p = d_cnt.data_ptr()
    if records is None:
        bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), p, cand_cap, d_conns.data_ptr(), p + 4, conn_cap, d_phys.data_ptr(), lt.N_STREAMS,
                                           b.unit, b.ifs, b.jitter, lt.REMAP, d_tracks.data_ptr(), d_pkts.data_ptr(), d_tscr.data_ptr(), tscratch,
                                           None), "btbbx_le_track_device")
    else:
        assert (len(records[0]), len(records[1]), len(records[2])) == (k, k, n) and (conn_cap, cand_cap) == (k, n)
        d_conns, d_tracks, d_pkts = (_dev(r) for r in records)
    bt.check(lib.btbbx_le_seed_device(d_adv.data_ptr(), p + 8, adv_cap, d_conns.data_ptr(), p + 4, conn_cap, d_tracks.data_ptr(), b.unit,
                                      d_seeds.data_ptr(), None), "btbbx_le_seed_device")
    bt.check(lib.btbbx_le_epoch_device(d_words.data_ptr(), b.n_words, b.n_words + pad_words, lt.N_STREAMS, d_phys.data_ptr(), d_cands.data_ptr(), p,
                                        cand_cap, d_conns.data_ptr(), p + 4, conn_cap, d_tracks.data_ptr(), d_pkts.data_ptr(),
                                        d_seeds.data_ptr(), b.unit, b.jitter, d_follows.data_ptr(), d_fpkts.data_ptr(), d_scr.data_ptr(),
                                        scratch, None), "btbbx_le_epoch_device")
    torch.cuda.synchronize()
    return _records(d_seeds, conn_cap + 1, SEED), _records(d_follows, conn_cap + 1, FOLLOW), _records(d_fpkts, cand_cap + 1, FPKT)


def _same(got, want, kept, what, names=None):
    if got[:kept].tobytes() != want.tobytes():
        bad = [g for g in range(kept) if got[g].tobytes() != want[g].tobytes()]
        raise AssertionError("%s %d (%s): %s, model %s (%d differ)" % (what, bad[0], names[bad[0]] if names else "", got[bad[0]], want[bad[0]],
                                                                       len(bad)))
    assert got[kept:].tobytes() == b"\xa5" * (got.dtype.itemsize * (len(got) - kept)), what


def _check(b, want=None, **kw):
    """The device against the model (want: the model's (seeds, follows, fpkts), when the caller has them already)."""
    n, k, m = len(b.cands), len(b.conns), len(b.adv)
    get = lambda name, default: default if kw.get(name) is None else kw[name]          # noqa: E731
    work, kept = min(get("count", n), get("cand_cap", n)), min(get("conn_count", k), get("conn_cap", k))
    if want is None:
        want = lf.model_cut(b, work, kept, min(get("adv_count", m), get("adv_cap", m)))[2:]
    seeds, follows, fpkts = _follow_device(b, **kw)
    if kw.get("conn_cap") == 0 or kw.get("cand_cap") == 0:
        work = kept = 0
    if kw.get("cand_cap") != 0:                                            # (cand_cap 0: the tracking wrote no record for the seed stage to read)
        _same(seeds, lf.seed_array(want[0][:kept], SEED), kept, "seed", b.names)
    _same(follows, lf.follow_array(want[1][:kept], FOLLOW), kept, "connection", b.names)
    _same(fpkts, lf.fpkt_array(want[2][:work], FPKT), work, "candidate")
    return want


def test_follow_on_the_lattice():
    b = lf.lattice()
    assert sum(c.channel == ld.NO_CONN for c in b.cands) >= 40                  # non-members lie between the groups
    want = lf.lattice_model()
    _check(b, want=want)
    by = dict(zip(b.names, zip(*want[:2])))
    assert by["hop 4"][0] is None and by["hop 17"][0] is None and by["interval 3201"][0] is None and by["R = first_anchor + 1"][0] is None
    assert by["R = first_anchor"][0] is not None and by["planted: two requests, the later wins"][0].hop == 9
    assert by["every event BEFORE"][1].flags == lf.SEEDED and by["every event BEFORE"][1].n_before == 2
    assert by["planted: delta 32766"][1].n_map_updates == 1 and by["planted: delta 32767"][1].n_map_updates == 0
    assert by["an exact tie"][1].algorithm == 2 and (by["an exact tie"][1].n_on, by["an exact tie"][1].n_off) == (1, 1)
    assert by["planted: ChSel 1 with #1"][1].algorithm == 1 and by["ChSel 0 on a connection that #2 explains"][1].n_off >= 15
    assert by["planted: parameter update"][1].flags == lf.SEEDED | lf.COUNTED | lf.STOPPED and by["planted: parameter update"][1].n_beyond == 7
    assert by["planted: an update behind ENC START"][1].flags & lf.ENCRYPTED and not by["planted: an update behind ENC START"][1].flags & lf.TERMINATED
    assert by["planted: TERMINATE"][1].flags & lf.TERMINATED and not by["planted: TERMINATE of length 3"][1].flags & lf.TERMINATED
    assert by["planted: last bit is the stream's last bit"][1].n_map_updates == 1
    n = lf.check_planted(b, *want)
    print("lattice: %d connections, %d candidates, %d seeded, %d packets of planted connections on the prediction" % (
        len(b.conns), len(b.cands), sum(s is not None for s in want[0]), n))


def test_caps_and_counts_on_the_lattice():
    b = lf.lattice()
    n, k, m = len(b.cands), len(b.conns), len(b.adv)
    _check(b, conn_cap=k - 5)                                              # the connections cut off: their candidates are no members
    _check(b, conn_cap=1)
    _check(b, conn_cap=k + 300)
    _check(b, conn_count=k - 11)
    _check(b, conn_count=k + 1000)
    _check(b, count=n - 7)
    _check(b, count=n + 1000)                                              # a counter beyond the cap: the cap's worth is worked on
    _check(b, cand_cap=n - 9)
    _check(b, cand_cap=n + 64)
    _check(b, adv_cap=m - 30)
    _check(b, adv_cap=m + 5)
    _check(b, adv_count=m - 17)
    _check(b, adv_count=m + 1000)
    _check(b, adv_count=0)
    _check(b, adv_cap=0)
    _check(b, count=0)
    _check(b, conn_count=0)
    _check(b, conn_cap=0)                                                  # nothing is written
    _check(b, cand_cap=0)                                                  # the follow stage writes nothing


def test_bad_arguments_are_refused_before_any_launch():
    import torch
    lib = bt.lib()
    buf = _filled(1 << 17)
    p = buf.data_ptr()
    scratch = lib.btbbx_le_epoch_scratch_bytes(8, 4)
    assert scratch <= (1 << 17) - 32768

    def follow(words=p, phys=p + 512, cands=p + 1024, cnt=p + 2048, conns=p + 3072, ccnt=p + 2052, tracks=p + 4096, pkts=p + 6144,
               seeds=p + 8192, follows=p + 10240, fpkts=p + 12288, scr=p + 32768, scr_bytes=scratch, n_words=8, pitch=8, n_streams=2,
               unit=1250, jitter=50):
        return lib.btbbx_le_epoch_device(words, n_words, pitch, n_streams, phys, cands, cnt, 8, conns, ccnt, 4, tracks, pkts, seeds, unit,
                                          jitter, follows, fpkts, scr, scr_bytes, None)

    def seed(adv=p, acnt=p + 2056, conns=p + 3072, ccnt=p + 2052, tracks=p + 4096, seeds=p + 8192, unit=1250):
        return lib.btbbx_le_seed_device(adv, acnt, 2, conns, ccnt, 4, tracks, unit, seeds, None)

    for kw in (dict(words=None), dict(phys=None), dict(cands=None), dict(cnt=None), dict(conns=None), dict(ccnt=None), dict(tracks=None),
               dict(pkts=None), dict(seeds=None), dict(follows=None), dict(fpkts=None), dict(scr=None), dict(words=p + 4), dict(phys=p + 513),
               dict(cands=p + 1028), dict(conns=p + 3076), dict(tracks=p + 4100), dict(pkts=p + 6148), dict(seeds=p + 8196),
               dict(follows=p + 10244), dict(fpkts=p + 12290), dict(scr=p + 32776), dict(cnt=p + 2050), dict(ccnt=p + 2054),
               dict(scr_bytes=scratch - 1), dict(n_words=0), dict(pitch=7), dict(n_streams=0), dict(unit=1), dict(jitter=625)):
        assert follow(**kw) == E_ARG, kw
        assert lib.btbbx_last_error()
    for kw in (dict(adv=None), dict(acnt=None), dict(conns=None), dict(ccnt=None), dict(tracks=None), dict(seeds=None), dict(adv=p + 4),
               dict(conns=p + 3076), dict(tracks=p + 4100), dict(seeds=p + 8196), dict(acnt=p + 2058), dict(ccnt=p + 2054), dict(unit=1)):
        assert seed(**kw) == E_ARG, kw
        assert lib.btbbx_last_error()
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == b"\xa5" * len(buf)
    # (counts of 0xa5a5a5a5: the caps' worth of 0xa5 records is read; no candidate is a member and no record a request)
    assert seed() == 0 and follow() == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert got[12288:12288 + 96].tobytes() == b"\xff" * 96 and got[12288 + 96:32768].tobytes() == b"\xa5" * (32768 - 12288 - 96)
    assert got[10240 + 192:12288].tobytes() == b"\xa5" * (2048 - 192) and got[8192 + 224:10240].tobytes() == b"\xa5" * (2048 - 224)
    assert got[:8192].tobytes() == b"\xa5" * 8192 and got[32768 + scratch:].tobytes() == b"\xa5" * (len(got) - 32768 - scratch)
    assert got[8192:8192 + 224].tobytes() == bytes(224)                          # (no 0xa5 record is a request: every seed is zero)


def test_update_pdus_next_to_counter_65536_inside_the_streams():
    """unit_bits 2, jitter_bits 0: counters around 2^16 whose control PDUs the streams hold; an instant across 65535 -> 0."""
    b = lf.wrap_world()
    want = lf.wrap_model()
    _check(b, want=want)
    by = dict(zip(b.names, want[1]))
    for name in ("planted: instant across 65535 -> 0", "planted: instant 65536", "planted: instant 0x10003, #2", "planted: counters from 0"):
        assert (by[name].n_map_updates, by[name].n_off, by[name].n_before) == (1, 0, 0), (name, by[name])
    assert by["planted: instant across 65535 -> 0"].counter_first == 65527 and by["planted: instant 0x10003, #2"].map == lf.NINE
    assert lf.check_planted(b, *want) == sum(len(i.counters) for i in b.info)


# ---- sizes that cross the kernels' seams ------------------------------------------------------------------------------
def test_a_long_connection_with_forty_updates_beside_a_thousand_small_ones():
    """One connection of 5 000 events with 40 map updates beside 1 000 connections of 2 to 4 events, two thirds of them seeded:
    more slots than three scan tiles hold, a segment of 40 entries in the sorted update list, and 1 001 connections -- more than one
    workgroup of the per-connection kernels (4 per workgroup in the seed stage, 256 in the verdict)."""
    b = lf.seam_world()
    assert len(b.conns) == 1001 and max(c.n_packets for c in b.conns) > 6000
    want = lf.seam_model()
    _check(b, want=want)
    big = want[1][b.names.index("planted: large")]
    assert (big.n_on, big.n_off, big.n_map_updates, big.algorithm) == (5000, 0, 40, 2), big
    assert lf.check_planted(b, *want) > 7000
    print("seams: %d connections, %d seeded" % (len(b.conns), sum(s is not None for s in want[0])))


# ---- the path lattice (tests/_le_follow_paths.py) -----------------------------------------------------------------------
@pytest.mark.parametrize("run", [r for r in lp.RUNS if r.cut is None], ids=[r.name for r in lp.RUNS if r.cut is None])
def test_worlds_of_the_path_lattice(run):
    """crowd_world: 4 436 listed updates over nine scan tiles, one of them empty, 1 450 connections; byte_world: instants that only
    the passes over bytes 1 and 2 order; tally_world: the runs of le_epoch_predict_kernel lane by lane."""
    b, full = lp.world(run.world)
    assert set(run.tags) <= lp.run_tags(run)
    _check(b, want=full[:3])
    assert lf.check_planted(b, *full[:3]) > 0


def test_cuts_of_the_crowd():
    """conn_cap one short; cand_cap cut inside the last connection; a count that is no multiple of 256 and leaves an update in the
    last slot."""
    b, full = lp.world("crowd")
    n, k, ragged = len(b.cands), len(b.conns), lp.ragged_count(b, full)
    assert b.conns[-1].first < n - 5 and ragged % 256 and "update_in_the_last_slot_of_a_ragged_list" in lp.run_tags(lp.RUNS[1])
    for kw, cut in ((dict(conn_cap=k - 1), dict(kept=k - 1)), (dict(cand_cap=n - 5), dict(work=n - 5)), (dict(count=ragged), dict(work=ragged))):
        _, seeds, follows, fpkts, _ = lf.cut_model(b, full, full[3], **cut)
        _check(b, want=(seeds, follows, fpkts), **kw)


@pytest.mark.parametrize("conn_cap, passes", [(255, 1), (256, 2), (65535, 2), (65536, 3)])
def test_lattice_at_the_capacities_that_add_a_connection_pass(conn_cap, passes):
    """One radix pass per byte of conn_cap over the connection: the list comes out the same however many there are."""
    assert passes == max(1, (conn_cap.bit_length() + 7) // 8)
    _check(lf.lattice(), want=lf.lattice_model(), conn_cap=conn_cap)


@pytest.mark.parametrize("name", ["lattice", "tally"])
def test_rows_two_words_apart_from_their_ends(name):
    """pitch_words = n_words + 2, the padding all ones: a payload read that stops at the pitch instead of n_words turns the zeros
    behind a stream's end into ones.  The lattice's packets at the streams' end ("one bit beyond the stream's end") have their
    payload inside the streams or more than two words behind them, so no byte of the lattice shows that; tally_world's last
    connection has an LL_CHANNEL_MAP_IND whose instant lies half inside: with ones behind the end it becomes a valid update."""
    b, want = (lf.lattice(), lf.lattice_model()) if name == "lattice" else (lf.tally_world(), lf.tally_model()[:3])
    end = 64 * b.n_words
    across = [c for c in b.cands if (c.header0 & 3) == 3 and c.length and c.offset + 56 < end < c.offset + 56 + 8 * min(c.length, 12) < end + 128]
    assert len(across) == (1 if name == "tally" else 0)
    assert name == "tally" or end + 1 in [c.offset + 80 + 8 * c.length for c in b.cands]
    _check(b, want=want, pad_words=2)


def _refused(b, tracks, pkts, none):
    """The model's records with the candidates `none` made no members."""
    pkts = [None if i in none else p for i, p in enumerate(pkts)]
    seeds = lf.seed(b.adv, b.conns, tracks, b.unit)
    return (seeds,) + lf.follow(b.conns, b.cands, tracks, pkts, seeds, b.words, b.n_words, b.unit, b.jitter)


@pytest.mark.parametrize("case", ["rank", "event", "first = N", "first >= 2^32"])
def test_a_list_that_breaks_the_grouping_promise_in_one_place(case):
    """include/btbbx.h: a member whose first + rank or first + event lies beyond N is treated as no member; so is every candidate of
    a connection whose `first` lies beyond N.  The tracking's records come from the model here, broken in exactly one place: the
    last-ranked member of a connection, alone in its event (so the ranks and events that remain have no gap), gets rank or event
    N - first; or conns[g].first becomes N, or gets bit 32 set.  Expected: the model's records with those candidates no members;
    everything else byte for byte as before."""
    b = lf.lattice()
    n = len(b.cands)
    g = b.names.index("planted: two updates in order" if case in ("rank", "event") else "planted: two updates out of order")
    first, mine = b.conns[g].first, [i for i, c in enumerate(b.cands) if c.channel == g]
    conns, tracks, pkts = ld.conn_array(b.conns, CONN), lt.track_array(b.tracks, TRACK), lt.pkt_array(b.pkts, PKT)
    if case in ("rank", "event"):
        last = max(mine, key=lambda i: b.pkts[i].rank)
        assert sum(b.pkts[i].event == b.pkts[last].event for i in mine) == 1 and b.pkts[last].rank == len(mine) - 1
        pkts[last][case] = n - first
        none = {last}
    else:
        conns[g]["first"] = n if case == "first = N" else first | (1 << 32)
        none = set(mine)
    want = _refused(b, b.tracks, b.pkts, none)
    whole = lf.lattice_model()
    assert want[1][g] != whole[1][g] and [x for x in range(len(b.conns)) if want[1][x] != whole[1][x]] == [g]
    assert all(want[2][i] is None for i in none) and sum(p is None for p in want[2]) == sum(p is None for p in whole[2]) + len(none)
    _check(b, want=want, records=(conns, tracks, pkts))


# ---- the chain ----------------------------------------------------------------------------------------------------------
def test_chain_scan_discover_track_seed_follow():
    import torch
    lib = bt.lib()
    cap, planted = lf.chain_capture()
    w_conns, w_cands, w_tracks, w_pkts, w_adv, w_seeds, w_follows, w_fpkts = lf.chain_model()
    n_cands, n_conns, n_streams = len(w_cands), len(w_conns), len(cap.mhz)
    # from Python, through the host wrapper
    conns, cands, tracks, pkts, seeds, follows, fpkts = bt.le_follow(cap.words, cap.search_bits, cap.mhz, max_len=27, min_count=2,
                                                                     n_streams=n_streams, pitch_words=cap.pitch_words, n_words=cap.n_words,
                                                                     unit_bits=1250, ifs_bits=200, jitter_bits=50)
    assert conns.tobytes() == ld.conn_array(w_conns, CONN).tobytes() and cands.tobytes() == ld.cand_array(w_cands, CAND).tobytes()
    assert tracks.tobytes() == lt.track_array(w_tracks, TRACK).tobytes() and pkts.tobytes() == lt.pkt_array(w_pkts, PKT).tobytes()
    assert seeds.tobytes() == lf.seed_array(w_seeds, SEED).tobytes()
    assert follows.tobytes() == lf.follow_array(w_follows, FOLLOW).tobytes()
    assert fpkts.tobytes() == lf.fpkt_array(w_fpkts, FPKT).tobytes()
    # the device chain, nothing read back between the stages
    cand_cap, conn_cap, adv_cap = n_cands + 100, 64, 16
    d_words, d_phys = _dev(cap.words.reshape(-1)), _dev(cap.mhz.astype(np.uint16))
    d_cands, d_conns = _filled(cand_cap * CAND.itemsize), _filled(conn_cap * CONN.itemsize)
    d_tracks, d_pkts = _filled((conn_cap + 1) * TRACK.itemsize), _filled((cand_cap + 1) * PKT.itemsize)
    d_seeds, d_follows = _filled((conn_cap + 1) * SEED.itemsize), _filled((conn_cap + 1) * FOLLOW.itemsize)
    d_fpkts = _filled((cand_cap + 1) * FPKT.itemsize)
    d_hits, d_adv = _filled(adv_cap * 16), _filled(adv_cap * ADV.itemsize)
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    scratch, tscratch = lib.btbbx_le_discover_scratch_bytes(cand_cap), lib.btbbx_le_track_scratch_bytes(cand_cap, conn_cap)
    fscratch, oscratch = lib.btbbx_le_epoch_scratch_bytes(cand_cap, conn_cap), lib.btbbx_order_hits_scratch_bytes(adv_cap)
    d_scr, d_tscr = torch.zeros(scratch // 8 + 2, dtype=torch.int64, device="cuda"), _filled(tscratch)
    d_fscr, d_oscr = _filled(fscratch), torch.zeros(oscratch // 8 + 2, dtype=torch.int64, device="cuda")
    p = d_cnt.data_ptr()
    geometry = (d_words.data_ptr(), cap.n_words, cap.pitch_words, n_streams)
    bt.check(lib.btbbx_le_scan_device(*geometry, cap.search_bits, bt.LE_ADV_AA, 0, d_hits.data_ptr(), adv_cap, p + 8, None))
    bt.check(lib.btbbx_order_hits_device(d_hits.data_ptr(), p + 8, adv_cap, d_oscr.data_ptr(), oscratch, None))
    bt.check(lib.btbbx_le_decode_hits_device(d_words.data_ptr(), cap.n_words, cap.pitch_words, d_hits.data_ptr(), p + 8, adv_cap,
                                             d_phys.data_ptr(), bt.LE_ADV_CRC_INIT, d_adv.data_ptr(), None))
    bt.check(lib.btbbx_le_discover_scan_device(*geometry, cap.search_bits, d_phys.data_ptr(), 27, d_cands.data_ptr(), cand_cap, p, None))
    bt.check(lib.btbbx_le_discover_group_device(d_cands.data_ptr(), p, cand_cap, 2, d_conns.data_ptr(), conn_cap, p + 4, d_scr.data_ptr(),
                                                scratch, None))
    bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), p, cand_cap, d_conns.data_ptr(), p + 4, conn_cap, d_phys.data_ptr(), n_streams,
                                       1250, 200, 50, lt.REMAP, d_tracks.data_ptr(), d_pkts.data_ptr(), d_tscr.data_ptr(), tscratch, None))
    bt.check(lib.btbbx_le_seed_device(d_adv.data_ptr(), p + 8, adv_cap, d_conns.data_ptr(), p + 4, conn_cap, d_tracks.data_ptr(), 1250,
                                      d_seeds.data_ptr(), None))
    bt.check(lib.btbbx_le_epoch_device(*geometry, d_phys.data_ptr(), d_cands.data_ptr(), p, cand_cap, d_conns.data_ptr(), p + 4, conn_cap,
                                        d_tracks.data_ptr(), d_pkts.data_ptr(), d_seeds.data_ptr(), 1250, 50, d_follows.data_ptr(),
                                        d_fpkts.data_ptr(), d_fscr.data_ptr(), fscratch, None))
    torch.cuda.synchronize()
    assert [int(v) for v in d_cnt[:3].cpu()] == [n_cands, n_conns, len(w_adv)] and n_conns <= conn_cap and len(w_adv) <= adv_cap
    for buf, host, dtype, kept, cap_n in ((d_seeds, seeds, SEED, n_conns, conn_cap), (d_follows, follows, FOLLOW, n_conns, conn_cap),
                                          (d_fpkts, fpkts, FPKT, n_cands, cand_cap)):
        got = buf.cpu().numpy()[:(cap_n + 1) * dtype.itemsize]
        assert got[:kept * dtype.itemsize].tobytes() == host.tobytes() and set(got[kept * dtype.itemsize:].tolist()) == {0xA5}, dtype
    assert d_tracks.cpu().numpy()[:n_conns * TRACK.itemsize].tobytes() == tracks.tobytes()     # (the tracking's records are only read)
    assert _records(d_adv, len(w_adv), ADV).tobytes() == lf.adv_array(w_adv, ADV).tobytes()
    # the planted connections: every event before `stop` on the prediction, where the tracking alone shows events off the hop
    by_key = {(int(c["access_address"]), int(c["crc_init"])): g for g, c in enumerate(conns)}
    for pl in planted:
        g = by_key[(pl.aa, pl.crc_init)]
        f, t, s = follows[g], tracks[g], seeds[g]
        if not pl.seeded:
            assert int(s["flags"]) == 0 and follows[g].tobytes() == bytes(FOLLOW.itemsize), pl
            continue
        before_stop = len([c for c in pl.counters if pl.stop is None or c < pl.stop])
        assert int(s["flags"]) == lf.SEEDED and int(f["algorithm"]) == pl.alg, (pl, f)
        assert (int(f["n_on"]), int(f["n_off"]), int(f["n_before"]), int(f["n_beyond"])) == (before_stop, 0, 0, len(pl.counters) - before_stop), (pl, f)
        assert bool(int(f["flags"]) & lf.STOPPED) == (pl.stop is not None) and int(f["counter_first"]) == 0
        mine = np.flatnonzero(cands["conn"] == g)
        counted = mine[fpkts["state"][mine] == lf.ST_COUNTED]
        assert len(counted) == 2 * before_stop and fpkts["on_hop"][counted].all()
        # the gap this closes: behind the first update the tracking, which takes the observed map for the connection's, is off the hop
        late = mine[(fpkts["counter"][mine] >= pl.first_update) & (fpkts["state"][mine] == lf.ST_COUNTED)]
        assert int(t["n_off_hop"]) > 0 and not pkts["on_hop"][late].all(), (pl, t)
    print("chain: %d candidates, %d connections, %d advertising records" % (n_cands, n_conns, len(w_adv)))


def test_more_advertising_matches_than_the_wrapper_first_has_room_for():
    """The host wrapper repeats the advertising scan into a second block when the first was too small; the records it seeds from
    are the same, in (stream, offset) order."""
    cap = lf.crowded_adv_capture()
    w_conns, w_cands, w_tracks, w_pkts, w_adv, w_seeds, w_follows, w_fpkts = lf.capture_model(cap)
    assert len(w_adv) > 4096 + cap.search_bits // 16384 * len(cap.mhz)
    conns, cands, tracks, pkts, seeds, follows, fpkts = bt.le_follow(cap.words, cap.search_bits, cap.mhz, max_len=27, min_count=2,
                                                                     n_streams=len(cap.mhz), pitch_words=cap.pitch_words, n_words=cap.n_words)
    assert conns.tobytes() == ld.conn_array(w_conns, CONN).tobytes() and cands.tobytes() == ld.cand_array(w_cands, CAND).tobytes()
    assert tracks.tobytes() == lt.track_array(w_tracks, TRACK).tobytes() and pkts.tobytes() == lt.pkt_array(w_pkts, PKT).tobytes()
    assert seeds.tobytes() == lf.seed_array(w_seeds, SEED).tobytes() and follows.tobytes() == lf.follow_array(w_follows, FOLLOW).tobytes()
    assert fpkts.tobytes() == lf.fpkt_array(w_fpkts, FPKT).tobytes()
    seeded = [s for s in w_seeds if s is not None]
    assert len(seeded) == 1 and seeded[0].request == [r["offset"] for r in w_adv if r["stream"] == 1].index(200)


def _device_chain(cap, cand_cap, conn_cap, adv_cap, adv_errors=0):
    """Advertising scan, order, decode, discovery, grouping, tracking, seed and follow, device-resident, nothing read back between
    the stages -> (counts, seeds, follows, fpkts), the records whole, one longer than their caps."""
    import torch
    lib = bt.lib()
    n_streams = len(cap.mhz)
    d_words, d_phys = _dev(cap.words.reshape(-1)), _dev(cap.mhz.astype(np.uint16))
    d_cands, d_conns = _filled(cand_cap * CAND.itemsize), _filled(conn_cap * CONN.itemsize)
    d_tracks, d_pkts = _filled((conn_cap + 1) * TRACK.itemsize), _filled((cand_cap + 1) * PKT.itemsize)
    d_seeds, d_follows = _filled((conn_cap + 1) * SEED.itemsize), _filled((conn_cap + 1) * FOLLOW.itemsize)
    d_fpkts = _filled((cand_cap + 1) * FPKT.itemsize)
    d_hits, d_adv = _filled(adv_cap * 16), _filled(adv_cap * ADV.itemsize)
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    scratch, tscratch = lib.btbbx_le_discover_scratch_bytes(cand_cap), lib.btbbx_le_track_scratch_bytes(cand_cap, conn_cap)
    fscratch, oscratch = lib.btbbx_le_epoch_scratch_bytes(cand_cap, conn_cap), lib.btbbx_order_hits_scratch_bytes(adv_cap)
    d_scr, d_tscr = torch.zeros(scratch // 8 + 2, dtype=torch.int64, device="cuda"), _filled(tscratch)
    d_fscr, d_oscr = _filled(fscratch), torch.zeros(oscratch // 8 + 2, dtype=torch.int64, device="cuda")
    p = d_cnt.data_ptr()
    geometry = (d_words.data_ptr(), cap.n_words, cap.pitch_words, n_streams)
    bt.check(lib.btbbx_le_scan_device(*geometry, cap.search_bits, bt.LE_ADV_AA, adv_errors, d_hits.data_ptr(), adv_cap, p + 8, None))
    bt.check(lib.btbbx_order_hits_device(d_hits.data_ptr(), p + 8, adv_cap, d_oscr.data_ptr(), oscratch, None))
    bt.check(lib.btbbx_le_decode_hits_device(d_words.data_ptr(), cap.n_words, cap.pitch_words, d_hits.data_ptr(), p + 8, adv_cap,
                                             d_phys.data_ptr(), bt.LE_ADV_CRC_INIT, d_adv.data_ptr(), None))
    bt.check(lib.btbbx_le_discover_scan_device(*geometry, cap.search_bits, d_phys.data_ptr(), 27, d_cands.data_ptr(), cand_cap, p, None))
    bt.check(lib.btbbx_le_discover_group_device(d_cands.data_ptr(), p, cand_cap, 2, d_conns.data_ptr(), conn_cap, p + 4, d_scr.data_ptr(),
                                                scratch, None))
    bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), p, cand_cap, d_conns.data_ptr(), p + 4, conn_cap, d_phys.data_ptr(), n_streams,
                                       1250, 200, 50, lt.REMAP, d_tracks.data_ptr(), d_pkts.data_ptr(), d_tscr.data_ptr(), tscratch, None))
    bt.check(lib.btbbx_le_seed_device(d_adv.data_ptr(), p + 8, adv_cap, d_conns.data_ptr(), p + 4, conn_cap, d_tracks.data_ptr(), 1250,
                                      d_seeds.data_ptr(), None))
    bt.check(lib.btbbx_le_epoch_device(*geometry, d_phys.data_ptr(), d_cands.data_ptr(), p, cand_cap, d_conns.data_ptr(), p + 4, conn_cap,
                                       d_tracks.data_ptr(), d_pkts.data_ptr(), d_seeds.data_ptr(), 1250, 50, d_follows.data_ptr(),
                                       d_fpkts.data_ptr(), d_fscr.data_ptr(), fscratch, None))
    torch.cuda.synchronize()
    return ([int(v) for v in d_cnt[:3].cpu()], _records(d_seeds, conn_cap + 1, SEED), _records(d_follows, conn_cap + 1, FOLLOW),
            _records(d_fpkts, cand_cap + 1, FPKT))


def test_payload_read_on_a_small_capture():
    """Control PDUs on channels 0 and 36, at stream offsets 0, 1 and 63 modulo 64, and one whose last bit is the stream's last bit,
    on a capture built with tests/_le_discover._Builder, through the device entries.  (A stream index >= n_streams cannot come out
    of a scan: the lattice holds that case.)"""
    cap = lf.payload_capture()
    conns, cands, tracks, pkts, adv, seeds, follows, fpkts = lf.capture_model(cap)
    updates = [c for c, p in zip(cands, fpkts) if p is not None and p.kind == lf.MAP_UPDATE]
    assert {c.offset % 64 for c in updates} >= {0, 1, 63} and {c.stream for c in updates} == {0, 1}
    assert max(c.offset + 80 + 8 * c.length for c in updates) == 64 * cap.n_words
    assert len(conns) == 1 and follows[0].n_map_updates == len(updates) >= 10 and max(p.epoch for p in fpkts if p is not None) >= 8
    cand_cap, conn_cap = len(cands) + 7, 5
    counts, got_s, got_f, got_p = _device_chain(cap, cand_cap, conn_cap, 8)
    assert counts == [len(cands), 1, len(adv)]
    _same(got_s, lf.seed_array(seeds, SEED), 1, "seed")
    _same(got_f, lf.follow_array(follows, FOLLOW), 1, "connection")
    _same(got_p, lf.fpkt_array(fpkts, FPKT), len(cands), "candidate")


def test_adv_errors_in_the_host_wrapper():
    """A CONNECT_IND received with one wrong bit in its access address: not seen without errors allowed, seeded with one; values
    outside 0..4 are refused."""
    cap, aa = lf.errors_capture()
    kw = dict(max_len=27, min_count=2, n_streams=len(cap.mhz), pitch_words=cap.pitch_words, n_words=cap.n_words)
    for adv_errors, seeded in ((0, False), (1, True), (4, True)):
        want = lf.capture_model(cap, adv_errors)
        g = [c.access_address for c in want[0]].index(aa)
        assert (want[5][g] is not None) == seeded and (want[6][g] is not None) == seeded
        conns, cands, tracks, pkts, seeds, follows, fpkts = bt.le_follow(cap.words, cap.search_bits, cap.mhz, adv_errors=adv_errors, **kw)
        assert conns.tobytes() == ld.conn_array(want[0], CONN).tobytes() and cands.tobytes() == ld.cand_array(want[1], CAND).tobytes()
        assert seeds.tobytes() == lf.seed_array(want[5], SEED).tobytes() and follows.tobytes() == lf.follow_array(want[6], FOLLOW).tobytes()
        assert fpkts.tobytes() == lf.fpkt_array(want[7], FPKT).tobytes()
        if seeded:
            assert (int(follows[g]["n_on"]), int(follows[g]["n_off"])) == (10, 0)
    for bad in (-1, 5):
        with pytest.raises(bt.BtbbError):
            bt.le_follow(cap.words, cap.search_bits, cap.mhz, adv_errors=bad, **kw)
        assert b"max_errors must be 0..4" in bt.lib().btbbx_last_error()
