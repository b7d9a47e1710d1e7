"""LE following through connection parameter updates (libbtbb_amd/csrc/le_span.h) on the GPU: the planted worlds of tests/_le_span.py
run through btbbx_le_track_device, btbbx_le_seed_device and btbbx_le_span_device and held against the model, every byte of the
three outputs; the equivalences with btbbx_le_epoch_device, device against device; and the host wrapper on a capture.  Output
buffers start as 0xA5 and are one record (one connection's span records) longer than their caps, so a byte a kernel leaves
unwritten, or writes where it should not, shows."""
import numpy as np
import pytest

import _le_discover as ld
import _le_follow as lf
import _le_span as ls
import _le_track as lt
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu

CAND, CONN, TRACK, PKT, ADV = bt.LE_CAND_DTYPE, bt.LE_CONN_DTYPE, bt.LE_TRACK_DTYPE, bt.LE_TRACK_PKT_DTYPE, bt.LE_PKT_DTYPE
SEED, FOLLOW, FPKT = bt.LE_SEED_DTYPE, bt.LE_FOLLOW_DTYPE, bt.LE_FOLLOW_PKT_DTYPE
SPAN, SPKT, REC = bt.LE_SPAN_DTYPE, bt.LE_SPAN_PKT_DTYPE, bt.LE_SPAN_REC_DTYPE
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


def _span_device(b, max_updates, conn_cap=None, count=None, cand_cap=None, conn_count=None, pad_words=0, records=None, epoch=False):
    """Tracking, seed and span stage on the device -> (seeds, spans, spkts, recs[, follows, fpkts]), each whole, one record (recs:
    max_updates + 1 records) longer than its cap.  epoch: the follow stage over the same records in the same run."""
    import torch
    lib = bt.lib()
    n, k, m = len(b.cands), len(b.conns), len(b.adv)
    count, cand_cap = n if count is None else count, n if cand_cap is None else cand_cap
    conn_count, conn_cap = k if conn_count is None else conn_count, k if conn_cap is None else conn_cap
    per = max_updates + 1
    d_cands, d_conns = _dev(ld.cand_array(b.cands, CAND)), _dev(ld.conn_array(b.conns, CONN))
    words = b.words
    if pad_words:
        words = np.full((len(b.words), b.n_words + pad_words), ~np.uint64(0), np.uint64)
        words[:, :b.n_words] = b.words
    d_phys, d_words, d_adv = _dev(np.asarray(lt.LATTICE_MHZ, np.uint16)), _dev(words.reshape(-1)), _dev(lf.adv_array(b.adv, ADV))
    d_tracks, d_pkts = _filled((conn_cap + 1) * TRACK.itemsize), _filled((cand_cap + 1) * PKT.itemsize)
    d_seeds, d_spans = _filled((conn_cap + 1) * SEED.itemsize), _filled((conn_cap + 1) * SPAN.itemsize)
    d_spkts, d_recs = _filled((cand_cap + 1) * SPKT.itemsize), _filled((conn_cap + 1) * per * REC.itemsize)
    d_follows, d_fpkts = _filled((conn_cap + 1) * FOLLOW.itemsize), _filled((cand_cap + 1) * FPKT.itemsize)
    d_cnt = torch.from_numpy(np.array([count, conn_count, m], np.int64).astype(np.uint32).view(np.int32)).cuda()
    tscratch, scratch = lib.btbbx_le_track_scratch_bytes(cand_cap, conn_cap), lib.btbbx_le_span_scratch_bytes(cand_cap, conn_cap, max_updates)
    d_tscr, d_scr = _filled(tscratch), _filled(scratch)
    p = d_cnt.data_ptr()
    if records is None:
        bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), p, cand_cap, d_conns.data_ptr(), p + 4, conn_cap, d_phys.data_ptr(), lt.N_STREAMS,
                                           b.unit, b.ifs, b.jitter, lt.REMAP, d_tracks.data_ptr(), d_pkts.data_ptr(), d_tscr.data_ptr(), tscratch,
                                           None), "btbbx_le_track_device")
    else:
        assert (len(records[0]), len(records[1]), len(records[2])) == (k, k, n) and (conn_cap, cand_cap) == (k, n)
        d_conns, d_tracks, d_pkts = (_dev(r) for r in records)
    bt.check(lib.btbbx_le_seed_device(d_adv.data_ptr(), p + 8, m, d_conns.data_ptr(), p + 4, conn_cap, d_tracks.data_ptr(), b.unit,
                                      d_seeds.data_ptr(), None), "btbbx_le_seed_device")
    front = (d_words.data_ptr(), b.n_words, b.n_words + pad_words, lt.N_STREAMS, d_phys.data_ptr(), d_cands.data_ptr(), p, cand_cap,
             d_conns.data_ptr(), p + 4, conn_cap, d_tracks.data_ptr(), d_pkts.data_ptr(), d_seeds.data_ptr(), b.unit, b.jitter)
    bt.check(lib.btbbx_le_span_device(*front, max_updates, d_spans.data_ptr(), d_spkts.data_ptr(), d_recs.data_ptr(), d_scr.data_ptr(), scratch,
                                      None), "btbbx_le_span_device")
    out = ()
    if epoch:
        escratch = lib.btbbx_le_epoch_scratch_bytes(cand_cap, conn_cap)
        d_escr = _filled(escratch)
        bt.check(lib.btbbx_le_epoch_device(*front, d_follows.data_ptr(), d_fpkts.data_ptr(), d_escr.data_ptr(), escratch, None),
                 "btbbx_le_epoch_device")
    torch.cuda.synchronize()
    if epoch:
        out = (_records(d_follows, conn_cap + 1, FOLLOW), _records(d_fpkts, cand_cap + 1, FPKT))
    assert set(d_scr.cpu().numpy()[scratch:].tolist()) == {0xA5}                # nothing behind the scratch
    return (_records(d_seeds, conn_cap + 1, SEED), _records(d_spans, conn_cap + 1, SPAN), _records(d_spkts, cand_cap + 1, SPKT),
            _records(d_recs, (conn_cap + 1) * per, REC)) + out


def _same(got, want, kept, what, names=None, per=1):
    want = want.reshape(-1)
    if got[:kept].tobytes() != want.tobytes():
        bad = [g for g in range(kept) if got[g].tobytes() != want[g].tobytes()]
        raise AssertionError("%s %d (%s): %s, model %s (%d differ)" % (what, bad[0], names[bad[0] // per] if names else "", got[bad[0]],
                                                                       want[bad[0]], len(bad)))
    assert got[kept:].tobytes() == b"\xa5" * (got.dtype.itemsize * (len(got) - kept)), what


def _cut_model(b, max_updates, work, kept):
    """The models on the first `work` candidates and `kept` connections: what the device entries see through caps and counts."""
    n, k = min(work, len(b.cands)), min(kept, len(b.conns))
    tracks, pkts = lt.track(b.cands[:n], k, lt.LATTICE_MHZ, lt.N_STREAMS, b.unit, b.ifs, b.jitter, lt.REMAP)
    seeds = lf.seed(b.adv, b.conns[:k], tracks, b.unit)
    return (seeds,) + ls.span_follow(b.conns[:k], b.cands[:n], tracks, pkts, seeds, b.words, b.n_words, b.unit, b.jitter, max_updates)


def _check(b, max_updates, want=None, **kw):
    """The device against the model (want: the model's (seeds, spans, spkts, recs), when the caller has them already)."""
    n, k = len(b.cands), len(b.conns)
    get = lambda name, default: default if kw.get(name) is None else kw[name]          # noqa: E731
    work, kept = min(get("count", n), get("cand_cap", n)), min(get("conn_count", k), get("conn_cap", k))
    if want is None:
        want = _cut_model(b, max_updates, work, kept)
    seeds, spans, spkts, recs = _span_device(b, max_updates, **kw)[:4]
    per = max_updates + 1
    if kw.get("conn_cap") == 0 or kw.get("cand_cap") == 0:
        work = kept = 0                                                        # nothing is written
    if kw.get("cand_cap") != 0:                                            # (cand_cap 0: the tracking wrote no record for the seed stage to read)
        _same(seeds, lf.seed_array(want[0][:kept], SEED), kept, "seed", b.names)
    _same(spans, ls.span_array(want[1][:kept], SPAN), kept, "connection", b.names)
    _same(spkts, ls.spkt_array(want[2][:work], SPKT), work, "candidate")
    _same(recs, ls.rec_array(want[3][:kept], REC, max_updates), kept * per, "span record", b.names, per)
    return want


@pytest.mark.parametrize("max_updates", [0, 1, 4])
def test_span_following_on_the_lattice(max_updates):
    b = ls.lattice()
    assert sum(c.channel == ld.NO_CONN for c in b.cands) >= 40                  # non-members lie between the groups
    want = _check(b, max_updates, want=ls.world_model("lattice", max_updates))
    by = dict(zip(b.names, want[1]))
    if max_updates:
        assert by["planted: a stray event between L and T"].n_gap == 1 and by["planted: refused, interval 5"].flags & ls.REFUSED
        assert by["planted: two updates"].n_spans == min(max_updates, 2) + 1
        assert by["planted: ENC START in front of the update"].n_spans == 1 and by["planted: delta 0 in the span's first event"].flags & ls.REFUSED
    else:
        assert all(s is None or s.n_spans == 1 for s in want[1]) and by["planted: two updates"].flags & ls.CAPPED
    print("lattice, max_updates %d: %d connections, %d candidates, %d packets of planted connections on the prediction" % (
        max_updates, len(b.conns), len(b.cands), ls.check_planted(b, *want)))


def _equal_to_epoch(b, max_updates):
    """Device against device: the span stage and the follow stage over the same records in the same run."""
    n, k = len(b.cands), len(b.conns)
    seeds, spans, spkts, recs, follows, fpkts = _span_device(b, max_updates, epoch=True)
    spans, spkts, follows, fpkts = spans[:k], spkts[:n], follows[:k], fpkts[:n]
    member = fpkts["state"] != 0xFF
    assert (member == (spkts["state"] != 0xFF)).all()
    if max_updates == 0:
        for f in ("map", "counter_first", "stop", "n_before", "n_on", "n_off", "n_beyond", "n_control", "n_map_updates", "algorithm"):
            assert (spans[f] == follows[f]).all(), f
        assert ((spans["flags"] & ~np.uint8(ls.CAPPED | ls.REFUSED)) == follows["flags"]).all()
        assert ((spans["n_gap"] == 0) & (spans["n_spans"] == (follows["flags"] & 1))).all()
        for f in ("counter", "epoch", "kind", "opcode", "expected", "on_hop", "state"):
            assert (spkts[f] == fpkts[f]).all(), f
        assert not spkts["span"][member].any() and not spkts["applied"][member].any()
    # every event of span 0 that the follow stage leaves COUNTED carries the same values
    same = member & (fpkts["state"] == lf.ST_COUNTED) & (follows["flags"][np.minimum(ld.cand_array(b.cands, CAND)["conn"], k - 1)] & 1).astype(bool)
    assert same.sum() > 0 and not spkts["span"][same].any()
    for f in ("counter", "epoch", "state"):
        assert (spkts[f][same] == fpkts[f][same]).all(), f
    # (kind: a PDU the follow stage calls PARAM_UPDATE is one here; expected and on_hop follow the algorithm, which is chosen over
    # all spans: equal where the choice is)
    alg_same = same & (spans["algorithm"] == follows["algorithm"])[np.minimum(ld.cand_array(b.cands, CAND)["conn"], k - 1)]
    for f in ("kind", "opcode"):
        assert (spkts[f][same] == fpkts[f][same]).all(), f
    for f in ("expected", "on_hop"):
        assert (spkts[f][alg_same] == fpkts[f][alg_same]).all(), f
    return int(same.sum())


@pytest.mark.parametrize("world", ["follow lattice", "follow wrap", "lattice", "chain"])
@pytest.mark.parametrize("max_updates", [0, 4])
def test_equivalence_with_the_follow_stage(world, max_updates):
    b = {"follow lattice": lf.lattice, "follow wrap": lf.wrap_world, "lattice": ls.lattice, "chain": ls.chain_world}[world]()
    assert _equal_to_epoch(b, max_updates) > 20


@pytest.mark.parametrize("max_updates", ls.MAX_UPDATES)
def test_chains_of_updates(max_updates):
    b = ls.chain_world()
    want = _check(b, max_updates, want=ls.world_model("chain", max_updates))
    by = dict(zip(b.names, want[1]))
    for n in (1, 2, 3):
        s = by["planted: chain of %d, #2" % n]
        assert s.n_spans == min(n, max_updates) + 1 and bool(s.flags & ls.CAPPED) == (max_updates < n) and s.algorithm == 2, (n, s)
        if max_updates >= n:
            assert (s.n_on, s.n_off, s.n_beyond, s.n_map_updates) == (30, 0, 0, 1), (n, s)
    assert ls.check_planted(b, *want) > 0


def test_update_pdus_next_to_counter_65536():
    b = ls.wrap_world()
    want = _check(b, 4, want=ls.world_model("wrap", 4))
    for name, s in zip(b.names, want[1]):
        if name is not None and name.startswith("planted"):
            assert (s.n_spans, s.n_off, s.n_beyond, s.n_gap) == (2, 0, 0, 0), (name, s)
    assert ls.check_planted(b, *want) == sum(len(i.counters) for i in b.info)


def test_caps_and_counts_on_the_lattice():
    b = ls.lattice()
    n, k = len(b.cands), len(b.conns)
    inside = b.conns[k // 2].first + 3                                     # a count that cuts a connection
    for kw in (dict(conn_cap=k - 1), dict(conn_cap=1), dict(conn_cap=k + 300), dict(conn_count=k - 11), dict(conn_count=k + 1000),
               dict(count=inside), dict(count=n + 1000), dict(cand_cap=n - 9), dict(cand_cap=inside + 2), dict(count=0), dict(conn_count=0), dict(conn_cap=0), dict(cand_cap=0)):
        _check(b, 2, **kw)


@pytest.mark.parametrize("conn_cap", [255, 256, 65536])
def test_lattice_at_the_capacities_that_add_a_connection_pass(conn_cap):
    _check(ls.lattice(), 4, want=ls.world_model("lattice", 4), conn_cap=conn_cap)


def test_a_crowd_across_the_tile_seams():
    b = ls.crowd_world()
    want = _check(b, 2, want=ls.world_model("crowd", 2))
    trace = {}
    ls.model(b, 2, trace=trace)
    tile, across, split, hole = ls.CROWD_TILE, 0, 0, 0
    for g, c in enumerate(b.conns):
        events = max(b.pkts[i].event for i in range(c.first, c.first + c.n_packets)) + 1
        for seam in range(tile, len(b.cands), tile):
            if c.first < seam < c.first + events:
                across += 1
                rec = want[3][g]
                if rec[0] is not None and rec[1] is not None:
                    last, f1 = rec[0].first_event + rec[0].n_events - 1, rec[1].first_event
                    split += c.first + last == seam - 1 and c.first + f1 == seam
                    hole += g in trace and trace[g]["state"].get(seam - c.first) == ls.ST_GAP
    assert across >= len(b.cands) // tile - 1 and split >= 1 and hole >= 1, (across, split, hole)
    assert ls.check_planted(b, *want) > 10000


def test_a_long_connection_with_eight_updates_beside_a_thousand_small_ones():
    b = ls.seam_world()
    want = _check(b, 8, want=ls.world_model("seam", 8))
    big = want[1][b.names.index("planted: large")]
    assert (big.n_spans, big.n_on, big.n_off, big.n_map_updates, big.n_param_updates, big.algorithm) == (9, 5000, 0, 2, 8, 2), big
    assert ls.check_planted(b, *want) > 9000


def test_rows_two_words_apart_from_their_ends():
    """pitch_words = n_words + 2, the padding all ones: an update PDU across the streams' end is read with zeros behind the end."""
    b = ls.end_world()
    end = 64 * b.n_words
    across = [c for c in b.cands if (c.header0 & 3) == 3 and c.length == 12 and c.offset + 56 < end < c.offset + 56 + 96]
    assert len(across) == 1
    _check(b, 4, want=ls.world_model("end", 4), pad_words=2)
    _check(ls.lattice(), 4, want=ls.world_model("lattice", 4), pad_words=2)


@pytest.mark.parametrize("case", ["rank", "event", "first = N", "first >= 2^32"])
def test_a_list_that_breaks_the_grouping_promise_in_one_place(case):
    """As tests/test_gpu_le_follow.py: the tracking's records from the model, broken in exactly one place; the candidates concerned
    are no members, everything else is as before."""
    b = ls.lattice()
    n = len(b.cands)
    g = b.names.index("planted: two updates")
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
    mpkts = [None if i in none else p for i, p in enumerate(b.pkts)]
    seeds = lf.seed(b.adv, b.conns, b.tracks, b.unit)
    want = (seeds,) + ls.span_follow(b.conns, b.cands, b.tracks, mpkts, seeds, b.words, b.n_words, b.unit, b.jitter, 4)
    whole = ls.world_model("lattice", 4)
    assert [x for x in range(len(b.conns)) if want[1][x] != whole[1][x]] == [g]
    _check(b, 4, want=want, records=(conns, tracks, pkts))


def test_bad_arguments_are_refused_before_any_launch():
    import torch
    lib = bt.lib()
    buf = _filled(1 << 17)
    p = buf.data_ptr()
    scratch = lib.btbbx_le_span_scratch_bytes(8, 4, 2)
    assert scratch <= (1 << 17) - 32768

    def span(words=p, phys=p + 512, cands=p + 1024, cnt=p + 2048, conns=p + 3072, ccnt=p + 2052, tracks=p + 4096, pkts=p + 6144,
             seeds=p + 8192, spans=p + 10240, spkts=p + 12288, recs=p + 14336, scr=p + 32768, scr_bytes=scratch, n_words=8, pitch=8,
             n_streams=2, unit=1250, jitter=50, max_updates=2):
        return lib.btbbx_le_span_device(words, n_words, pitch, n_streams, phys, cands, cnt, 8, conns, ccnt, 4, tracks, pkts, seeds, unit,
                                        jitter, max_updates, spans, spkts, recs, scr, scr_bytes, None)

    for kw in (dict(words=None), dict(phys=None), dict(cands=None), dict(cnt=None), dict(conns=None), dict(ccnt=None), dict(tracks=None),
               dict(pkts=None), dict(seeds=None), dict(spans=None), dict(spkts=None), dict(recs=None), dict(scr=None), dict(words=p + 4),
               dict(phys=p + 513), dict(cands=p + 1028), dict(conns=p + 3076), dict(tracks=p + 4100), dict(pkts=p + 6148),
               dict(seeds=p + 8196), dict(spans=p + 10244), dict(spkts=p + 12292), dict(recs=p + 14340), dict(scr=p + 32776),
               dict(cnt=p + 2050), dict(ccnt=p + 2054), dict(scr_bytes=scratch - 1), dict(n_words=0), dict(pitch=7), dict(n_streams=0),
               dict(unit=1), dict(jitter=625), dict(max_updates=17)):
        assert span(**kw) == E_ARG, kw
        assert lib.btbbx_last_error()
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == b"\xa5" * len(buf)
    # (counts of 0xa5a5a5a5: the caps' worth of 0xa5 records is read; no candidate is a member, and a 0xa5 seed counts as seeded)
    assert span() == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert got[12288:12288 + 128].tobytes() == b"\xff" * 128 and got[12288 + 128:14336].tobytes() == b"\xa5" * (2048 - 128)
    assert got[:10240].tobytes() == b"\xa5" * 10240 and got[10240 + 224:12288].tobytes() == b"\xa5" * (2048 - 224)
    assert got[14336 + 480:32768].tobytes() == b"\xa5" * (32768 - 14336 - 480)
    assert got[32768 + scratch:].tobytes() == b"\xa5" * (len(got) - 32768 - scratch)


def test_le_span_on_a_capture_through_the_host_wrapper():
    cap, planted = ls.span_capture()
    w_conns, w_cands, w_tracks, w_pkts, w_adv, w_seeds, w_follows, w_fpkts, w_spans, w_spkts, w_recs = ls.capture_model(4)
    kw = dict(max_len=27, min_count=2, n_streams=len(cap.mhz), pitch_words=cap.pitch_words, n_words=cap.n_words, unit_bits=1250, ifs_bits=200,
              jitter_bits=50)
    conns, cands, tracks, pkts, seeds, spans, spkts, recs = bt.le_span(cap.words, cap.search_bits, cap.mhz, max_updates=4, **kw)
    assert conns.tobytes() == ld.conn_array(w_conns, CONN).tobytes() and cands.tobytes() == ld.cand_array(w_cands, CAND).tobytes()
    assert tracks.tobytes() == lt.track_array(w_tracks, TRACK).tobytes() and pkts.tobytes() == lt.pkt_array(w_pkts, PKT).tobytes()
    assert seeds.tobytes() == lf.seed_array(w_seeds, SEED).tobytes()
    assert spans.tobytes() == ls.span_array(w_spans, SPAN).tobytes()
    assert spkts.tobytes() == ls.spkt_array(w_spkts, SPKT).tobytes()
    assert recs.shape == (len(w_conns), 5) and recs.tobytes() == ls.rec_array(w_recs, REC, 4).tobytes()
    # against bt.le_follow: the shared fields in front of stop
    f_conns, f_cands, f_tracks, f_pkts, f_seeds, follows, fpkts = bt.le_follow(cap.words, cap.search_bits, cap.mhz, **kw)
    assert f_conns.tobytes() == conns.tobytes() and f_cands.tobytes() == cands.tobytes() and f_seeds.tobytes() == seeds.tobytes()
    assert f_tracks.tobytes() == tracks.tobytes() and f_pkts.tobytes() == pkts.tobytes()
    front = (fpkts["state"] == lf.ST_COUNTED) & (fpkts["kind"] != 0xFF)
    for f in ("counter", "epoch", "kind", "opcode", "expected", "on_hop", "state"):
        assert (spkts[f][front] == fpkts[f][front]).all(), f
    by_key = {(int(c["access_address"]), int(c["crc_init"])): g for g, c in enumerate(conns)}
    for aa, ci, alg, anchors in planted:
        g = by_key[(aa, ci)]
        s, f = spans[g], follows[g]
        assert (int(s["n_spans"]), int(s["n_off"]), int(s["n_beyond"]), int(s["n_gap"]), int(s["algorithm"])) == (2, 0, 0, 0, alg), s
        assert int(s["n_on"]) == len(anchors) and int(f["n_beyond"]) > 0 and int(f["n_on"]) + int(f["n_beyond"]) == len(anchors)
        assert int(s["flags"]) == lf.SEEDED | lf.COUNTED and int(s["n_param_updates"]) == 1
        mine = np.flatnonzero(cands["conn"] == g)
        for i in mine:
            if int(cands["offset"][i]) in anchors:
                assert int(spkts["counter"][i]) == anchors[int(cands["offset"][i])] and int(spkts["on_hop"][i]) == 1
    with pytest.raises(bt.BtbbError):
        bt.le_span(cap.words, cap.search_bits, cap.mhz, max_updates=17, **kw)
    assert b"max_updates must be 0..16" in bt.lib().btbbx_last_error()
