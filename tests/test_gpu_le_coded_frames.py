"""The frames of the LE Coded kernels (libbtbb_amd/csrc/le_coded.h, le_cfind.h, le_ctrack.h) on the captures of
tests/_le_coded_frames.py: more tiles than workgroups (the stride step, the cursor's walk across streams, the prefetch past the
last stream, cfind's skipped advertising tile), rings that fill, flush inside stage, drain and wrap, caps inside a flush, the cfind
decoder's stride, the host wrapper's second pass, and offsets beyond bit 2^32 of a stream and byte 2^32 of a capture.  Every
expectation is the models' (tests/test_le_coded_frames_model.py shows on the CPU what the captures hold and that the simplest
wrong variants give other lists); everything is compared for equality.  Output buffers start as 0xA5, are longer than their caps
and are checked byte for byte behind the count.  The grids come from the device's CU count; each geometry condition is asserted
from it before the kernel runs."""
import numpy as np
import pytest

import _le
import _le_coded as c
import _le_coded_frames as fr
import libbtbb_amd as bt
from test_gpu_le_cfind import _records
from test_gpu_le_coded import _arrays
from test_gpu_le_ctrack import _symbols_device

pytestmark = pytest.mark.gpu

HIT, CAND, INFO, PKT, CINFO = (bt.HIT_DTYPE.itemsize, bt.LE_CAND_DTYPE.itemsize, bt.LE_CODED_CAND_INFO_DTYPE.itemsize, bt.LE_PKT_DTYPE.itemsize,
                               bt.LE_CODED_INFO_DTYPE.itemsize)
SLACK = 9                                                  # records behind every cap


@pytest.fixture(scope="module", autouse=True)
def _init():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    bt.init(2)


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


_FAULT = []


@pytest.fixture(autouse=True)
def nothing_is_launched_after_a_gpu_fault():
    """a HIP error is sticky: once a test has met one, the others fail here instead of launching more work on that device"""
    import torch
    assert not _FAULT, _FAULT
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        _FAULT.append(str(e))
        raise


def _dev(a):
    import torch
    raw = np.ascontiguousarray(a).tobytes()
    raw += bytes((-len(raw)) % 8 + 8)
    return torch.from_numpy(np.frombuffer(raw, np.int64).copy()).cuda()


def _filled(nbytes):
    import torch
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")


def _tuples(hits):
    return [(int(h["stream"]), int(h["offset"]), int(h["lap"]), int(h["ac_errors"])) for h in hits]


def _coded_scan(ptr, n_words, pitch, n_streams, search_bits, aa, limit, hit_cap):
    """btbbx_le_coded_scan_device -> (count, the whole hit buffer: hit_cap + SLACK records that were 0xA5)"""
    import torch
    d_hits = _filled((hit_cap + SLACK) * HIT)
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    bt.check(bt.lib().btbbx_le_coded_scan_device(ptr, n_words, pitch, n_streams, search_bits, aa, limit, d_hits.data_ptr(), hit_cap, d_cnt.data_ptr(),
                                                 None), "btbbx_le_coded_scan_device")
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy().view(np.uint32)
    assert not cnt[1:].any()
    return int(cnt[0]), d_hits.cpu().numpy().view(bt.HIT_DTYPE)


def _check_coded_scan(ptr, n_words, pitch, n_streams, search_bits, aa, limit, want, ctx):
    """the sorted hit tuples and the count equal the model's, and the 0xA5 tail is intact"""
    count, hits = _coded_scan(ptr, n_words, pitch, n_streams, search_bits, aa, limit, len(want) + 1)
    print("%s: %d hits (model %d)" % (ctx, count, len(want)))
    assert count == len(want), (ctx, count, len(want))
    got = sorted(_tuples(hits[:count]))
    if got != want:
        g, w = set(got), set(want)
        raise AssertionError((ctx, "missing", sorted(w - g)[:6], "extra", sorted(g - w)[:6]))
    assert not hits["reserved"][:count].any() and hits[count:].tobytes() == b"\xa5" * HIT * (len(hits) - count), ctx


def _cfind_scan(ptr, n_words, pitch, n_streams, search_bits, d_phys, cand_cap, pre_cap, max_len=255, max_errors=fr.MAX_ERRORS):
    """btbbx_le_cfind_scan_device -> (candidate count, pre-record count, candidates, info, pre-records); each buffer SLACK records
    longer than its cap, all 0xA5 before"""
    import torch
    d_cands, d_info, d_pre = _filled((cand_cap + SLACK) * CAND), _filled((cand_cap + SLACK) * INFO), _filled((pre_cap + SLACK) * 16)
    d_cnt = torch.zeros(8, dtype=torch.int32, device="cuda")
    d_cnt[4] = 77                                           # (the pre-record counter is cleared by the call)
    bt.check(bt.lib().btbbx_le_cfind_scan_device(ptr, n_words, pitch, n_streams, search_bits, d_phys.data_ptr(), max_len, max_errors, d_cands.data_ptr(),
                                                 d_info.data_ptr(), cand_cap, d_cnt.data_ptr(), d_cnt.data_ptr() + 16, d_pre.data_ptr(), 16 * pre_cap, None),
             "btbbx_le_cfind_scan_device")
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy().view(np.uint32)
    assert not cnt[[1, 2, 3, 5, 6, 7]].any()
    return (int(cnt[0]), int(cnt[4]), d_cands.cpu().numpy().view(bt.LE_CAND_DTYPE), d_info.cpu().numpy().view(bt.LE_CODED_CAND_INFO_DTYPE),
            d_pre.cpu().numpy().view(np.uint32).reshape(-1, 4))


def _pre_tuples(pre_recs):
    return [(int(r[0]) | int(r[1]) << 32, int(r[2]), int(r[3])) for r in pre_recs]


def _check_cfind(ptr, n_words, pitch, n_streams, search_bits, d_phys, model, pre, ctx):
    """candidate and info records as a sorted set, the pre-record set and both counts equal the model's; 0xA5 behind both counts.
    Returns the pre-records in the order the scan left them."""
    want_c, want_i = _records(model)
    count, pre_count, cands, info, pre_recs = _cfind_scan(ptr, n_words, pitch, n_streams, search_bits, d_phys, len(model) + 2, len(pre) + 2)
    print("%s: candidates %d (model %d), pre-records %d (model %d)" % (ctx, count, len(model), pre_count, len(pre)))
    assert (count, pre_count) == (len(model), len(pre)), (ctx, count, len(model), pre_count, len(pre))
    got = sorted(cands[i].tobytes() + info[i].tobytes() for i in range(count))
    assert got == sorted(want_c[i].tobytes() + want_i[i].tobytes() for i in range(count)), ctx
    assert cands[count:].tobytes() == b"\xa5" * CAND * (len(cands) - count) and info[count:].tobytes() == b"\xa5" * INFO * (len(info) - count), ctx
    got_pre = _pre_tuples(pre_recs[:pre_count])
    assert sorted(got_pre) == sorted(pre) and pre_recs[pre_count:].tobytes() == b"\xa5" * 16 * (len(pre_recs) - pre_count), ctx
    return got_pre, cands[:count]


# ---- 1. more tiles than workgroups -------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[12, 1030])
def walk(request, cus):
    """(capture, its words in HBM, its channels in HBM), after the geometry conditions: with one ragged tile per stream every
    workgroup works two tiles and 37 work three, and the cursor walks `grid` streams per step; with three tiles per stream a
    workgroup's successive tiles lie in different streams at different tile indices; behind its last tile every workgroup fetches
    with a stream index past the capture."""
    w = fr.walk(request.param, cus)
    g = w.geometry()
    assert w.grid == fr.SCAN_WGS_PER_CU * cus and w.pitch_words > w.n_words and w.n_tiles > 2 * w.grid and g["min_trips"] >= 2 and g["prefetch_past_the_end"]
    if request.param == 12:
        assert w.tps == 1 and w.n_streams == 2 * w.grid + 37 and g["max_trips"] == 3 and g["cursor_steps"] == w.grid
    else:
        assert w.tps == 3 and w.grid % 3 != 0 and g["streams_differ"] and g["tiles_differ"]
    return w, _dev(w.words()), _dev(w.mhz)


@pytest.mark.parametrize("limit", [0, 16])
@pytest.mark.parametrize("aa", [fr.AA_A, fr.AA_B])
def test_coded_scan_walks_every_tile(walk, aa, limit):
    w, d_words, _ = walk
    want = w.coded_hits(aa, limit)
    assert len(want) > 100 and fr.first_trip_only(want, w.tile_of, w.grid) != want
    _check_coded_scan(d_words.data_ptr(), w.n_words, w.pitch_words, w.n_streams, w.search_bits, aa, limit, want, (w.n_words, hex(aa), limit))


def test_cfind_scan_walks_every_tile_and_skips_advertising_tiles(walk):
    w, d_words, d_phys = walk
    model, pre = w.cfind()
    skip_work, work_skip = w.skip_and_work()
    assert skip_work >= 50 and work_skip >= 50, (skip_work, work_skip)
    assert len(model) > 100 and not any(w.is_adv[x.stream] for x, _ in model)
    _, cands = _check_cfind(d_words.data_ptr(), w.n_words, w.pitch_words, w.n_streams, w.search_bits, d_phys, model, pre, w.n_words)
    assert not w.is_adv[cands["stream"]].any()


# ---- 2. dense rings ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flipped", [False, True])
def test_coded_scan_on_a_dense_stream(flipped):
    """One stream of the periodic content: 1024 hits per wave and tile on the clean one (every ballot full, the ring flushed inside
    stage, drained behind the tile and wrapped), 650 to 900 on the flipped one (partial ballots onto tails that are no multiple of
    64); one mismatch below the content's twelve nothing is found; a sparse search of the same stream is not disturbed."""
    words, _ = fr.dense_stream(flipped)
    d_words = _dev(np.concatenate([words, np.full(5, np.uint64(0xFFFFFFFFFFFFFFFF))]))
    n, search_bits = fr.DENSE_WORDS, 64 * fr.DENSE_WORDS - (c.PATTERN - 1)
    for limit in (12, 16, 63) + (() if flipped else (11,)):
        want = fr.dense_hits(flipped, fr.DENSE_AA, limit)
        per = fr.wave_tile_counts([h[1] for h in want]) if want else np.zeros(1, int)
        if limit == 11:
            assert not want
        elif flipped:
            assert (per % fr.FLUSH != 0).any() and (limit == 12 or per.max() > 2 * fr.RING)
        else:
            in_stage, drain, top, _ = fr.ring_trace([64] * 16)
            assert per.max() == 1024 > 2 * fr.RING and in_stage and drain and top > fr.RING
        _check_coded_scan(d_words.data_ptr(), n, n + 5, 1, search_bits, fr.DENSE_AA, limit, want, (flipped, limit))
    want = fr.dense_hits(flipped, fr.AA_B, 16)
    assert [(h[1], h[3]) for h in want] == sorted(fr.DENSE_SPARSE)
    _check_coded_scan(d_words.data_ptr(), n, n + 5, 1, search_bits, fr.AA_B, 16, want, (flipped, "sparse"))


def test_hit_cap_inside_a_flush():
    """hit_cap = count // 2 + 13 and hit_cap = 1 on the flipped stream: the count is the whole number, hit_cap distinct records of the
    model's are written and nothing behind them.  Flushes move 64 records (a wave's last: two at least), so hit_cap = 1 lies inside
    the flush whose base is 0 and the other inside or on the end of one that begins below it."""
    words, _ = fr.dense_stream(True)
    d_words = _dev(np.concatenate([words, np.full(5, np.uint64(0xFFFFFFFFFFFFFFFF))]))
    full = fr.dense_hits(True, fr.DENSE_AA, 16)
    per = fr.wave_tile_counts([h[1] for h in full])
    assert not fr.possible_bases(per, 1) and (per % fr.FLUSH != 1).all()
    for cap in (len(full) // 2 + 13, 1):
        assert 0 < cap < len(full) - fr.FLUSH
        count, hits = _coded_scan(d_words.data_ptr(), fr.DENSE_WORDS, fr.DENSE_WORDS + 5, 1, 64 * fr.DENSE_WORDS - 335, fr.DENSE_AA, 16, cap)
        got = _tuples(hits[:cap])
        assert count == len(full) and len(set(got)) == cap and set(got) <= set(full), cap
        assert hits[cap:].tobytes() == b"\xa5" * HIT * SLACK, cap


def test_pre_cap_and_cand_cap_inside_a_flush():
    """The same for btbbx_le_cfind_scan_device on a data-channel stream of the flipped content with whole packets in it: pre_cap and
    cand_cap at count // 2 + 13 and at 1."""
    cap = fr.dense_cfind(*fr.DENSE_CFIND)
    model, pre = (list(x) for x in fr.dense_cfind_model(*fr.DENSE_CFIND))
    want_c, want_i = _records(model)
    full = {want_c[i].tobytes(): want_i[i].tobytes() for i in range(len(model))}
    per = fr.wave_tile_counts([p[0] for p in pre])
    assert per.max() > 2 * fr.RING and not fr.possible_bases(per, 1) and len(model) // 2 + 13 < len(model)
    d_words, d_phys = _dev(cap.words), _dev(np.array([cap.mhz], np.uint16))
    args = (d_words.data_ptr(), cap.n_words, cap.pitch_words, 1, cap.search_bits, d_phys)
    _check_cfind(*args, model, pre, "whole")
    for k in (len(model) // 2 + 13, 1):                     # cand_cap below the count
        count, pre_count, cands, info, _ = _cfind_scan(*args, k, len(pre))
        assert (count, pre_count) == (len(model), len(pre))
        got = [cands[i].tobytes() for i in range(k)]
        assert len(set(got)) == k and all(full.get(x) == info[i].tobytes() for i, x in enumerate(got)), k
        assert cands[k:].tobytes() == b"\xa5" * CAND * SLACK and info[k:].tobytes() == b"\xa5" * INFO * SLACK, k
    for k in (len(pre) // 2 + 13, 1):                       # pre_cap below its count: what was decoded of the pre-records kept is true
        count, pre_count, cands, info, pre_recs = _cfind_scan(*args, len(model), k)
        assert pre_count == len(pre) and count <= len(model) and (count > 0 or k == 1), k
        kept = _pre_tuples(pre_recs[:k])
        assert len(set(kept)) == k and set(kept) <= set(pre) and pre_recs[k:].tobytes() == b"\xa5" * 16 * SLACK, k
        got = [cands[i].tobytes() for i in range(count)]
        assert len(set(got)) == count and all(full.get(x) == info[i].tobytes() for i, x in enumerate(got)), k
        assert {int(x["offset"]) for x in cands[:count]} == {x.offset for x, _ in model} & {p[0] for p in kept}, k
        assert cands[count:].tobytes() == b"\xa5" * CAND * (len(cands) - count), k


def test_cfind_decoder_strides_over_the_pre_records(cus):
    """2 * 32 * CUs + 300 words of the flipped content with 40 whole packets: pre_cap above the count makes the decoder's grid
    32 * CUs, and the pre-records outnumber one trip of that grid (8 per workgroup), so the stride runs: more than half of the
    workgroups take a second trip (7788 of 8192 at 256 CUs).  All of them would need 16 * 32 * CUs pre-records; the stream has
    8 * (2 * 32 * CUs + 300) offsets that are 0 mod 8, 2400 to spare, and the 40 packets take more than that.  At least 5 candidates come from pre-records that the scan left at index
    8 * 32 * CUs or beyond."""
    n_words = fr.stride_words(cus)
    cap = fr.dense_cfind(n_words, 40)
    model, pre = (list(x) for x in fr.dense_cfind_model(n_words, 40))
    grid = fr.DECODE_WGS_PER_CU * cus
    one_trip = fr.DECODE_RECS * grid
    assert cap.n_words == 2 * grid + 300 and fr.decode_grid(cus, len(pre) + 2) == grid
    second = (len(pre) - one_trip + fr.DECODE_RECS - 1) // fr.DECODE_RECS   # workgroups with a second trip
    assert len(pre) > one_trip and 2 * second > grid, (len(pre), one_trip)
    assert {x.offset for x, _ in model} >= {p[0] for p in cap.planted} and len(cap.planted) == 40
    d_words, d_phys = _dev(cap.words), _dev(np.array([cap.mhz], np.uint16))
    got_pre, _ = _check_cfind(d_words.data_ptr(), cap.n_words, cap.pitch_words, 1, cap.search_bits, d_phys, model, pre, "stride")
    offsets = {x.offset for x, _ in model}
    beyond = sum(p[0] in offsets for p in got_pre[one_trip:])
    print("%d pre-records, %d candidates, %d of them from index %d or beyond" % (len(pre), len(model), beyond, one_trip))
    assert beyond >= 5


def test_host_wrapper_takes_its_second_pass():
    """le_coded_scan on 640 words of the flipped content at limit 63: more hits than the wrapper's first guess has room for, so it
    scans again with room.  Records and info are match_all + decode_many in (stream, offset) order."""
    words = fr.second_pass_stream()
    search_bits = 64 * len(words) - (c.PATTERN - 1)
    offs, errs = fr.second_pass_hits()
    assert len(offs) > search_bits // 1024 * 1 + 4096
    # (fr.SECOND_PASS_MHZ: the channel on which the hits that decode a block 2 at all decode the shortest one)
    want_pk, want_info = _arrays(c.decode_many(words, len(words), 0, offs, errs, fr.SECOND_PASS_MHZ, _le.ADV_CRC_INIT))
    assert set(want_info["s"]) == {0, 2, 8}
    pk, info = bt.le_coded_scan(words, search_bits, [fr.SECOND_PASS_MHZ], aa=fr.DENSE_AA, max_errors=63)
    assert len(pk) == len(offs) and pk.tobytes() == want_pk.tobytes() and info.tobytes() == want_info.tobytes()


# ---- 3. far offsets ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def far():
    """The far capture: about 8 GiB of zeros on the device, the copies of R written by slice assignment; freed at the module's end."""
    import torch
    F = fr.far()
    t = torch.zeros(2 * F.pitch_words, dtype=torch.int64, device="cuda")
    for cp in F.copies:
        at = cp.stream * F.pitch_words + cp.base
        t[at:at + fr.R_WORDS] = _dev(F.R[cp.stream])[:fr.R_WORDS]
    torch.cuda.synchronize()
    yield F, t, _dev(F.mhz)
    del t
    torch.cuda.empty_cache()


def _refs(F):
    return [(s, ends, F.ref(s, ends)) for s in (0, 1) for ends in (False, True)]


@pytest.mark.parametrize("aa", fr.FAR_AAS)
def test_far_coded_scan(far, aa):
    """Both streams at full search_bits: the model's hits on the short references, moved; stream 1's last searchable offset among
    them; and the short references themselves give the unmoved lists."""
    F, t, _ = far
    want = list(fr.far_coded_hits(aa))
    assert sum(h[1] >= 1 << 32 for h in want) >= 8 and sum(h[1] >= 1 << 35 for h in want) >= 4 and fr.offsets_32bit(want) != want
    assert aa != fr.AA_A or (1, F.search_bits - 1, aa, 0) in want
    _check_coded_scan(t.data_ptr(), F.n_words, F.pitch_words, 2, F.search_bits, aa, fr.MAX_ERRORS, want, ("far", hex(aa)))
    for s, ends, w in _refs(F):
        short = [(0,) + h for h in fr.ref_coded_hits(w, aa)]
        d_w = _dev(w)
        _check_coded_scan(d_w.data_ptr(), len(w), len(w), 1, 64 * len(w) - 335, aa, fr.MAX_ERRORS, short, ("short", s, ends, hex(aa)))


def test_far_coded_scan_with_search_bits_inside_the_last_copy(far):
    """search_bits ends one past a hit above bit 2^35 with another hit within two words behind it: the ragged tile's mask is formed
    from search_bits - first_off beyond 2^35."""
    F, t, _ = far
    everything = list(fr.far_coded_hits(fr.DENSE_AA))
    above = [h for h in everything if h[1] >= 1 << 35]
    pivot = [a for a, b in zip(above, above[1:]) if b[0] == a[0] and b[1] - a[1] <= 128 and (a[1] + 1) % 32][-1]
    bits = pivot[1] + 1
    want = [h for h in everything if h[1] < bits]
    assert pivot in want and any(h[0] == pivot[0] and bits <= h[1] < bits + 128 for h in everything) and bits % 32 and len(want) < len(everything)
    _check_coded_scan(t.data_ptr(), F.n_words, F.pitch_words, 2, bits, fr.DENSE_AA, fr.MAX_ERRORS, want, ("far cut", bits))


def _decode(ptr, n_words, pitch, rows, d_phys, crc_init=fr.INIT_A):
    """btbbx_le_coded_decode_hits_device over rows [(stream, offset, pkt, info)] -> both record arrays, two records longer than the list"""
    import torch
    n = len(rows)
    hits = np.zeros(n + 1, bt.HIT_DTYPE)
    for i, (s, o, pkt, _) in enumerate(rows):
        hits[i] = (o, 0xDEADBEEF, pkt["aa_errors"], 0, s)
    d_hits = _dev(hits)
    d_cnt = torch.from_numpy(np.array([n, 0, 0, 0], np.uint32).view(np.int32)).cuda()
    d_out, d_info = _filled((n + 2) * PKT), _filled((n + 2) * CINFO)
    bt.check(bt.lib().btbbx_le_coded_decode_hits_device(ptr, n_words, pitch, d_hits.data_ptr(), d_cnt.data_ptr(), n, d_phys.data_ptr(), crc_init,
                                                        d_out.data_ptr(), d_info.data_ptr(), None, 0, None), "btbbx_le_coded_decode_hits_device")
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(bt.LE_PKT_DTYPE), d_info.cpu().numpy().view(bt.LE_CODED_INFO_DTYPE)


def _check_decode(ptr, n_words, pitch, rows, d_phys, ctx):
    want_pk, want_info = _arrays([(pkt, info) for _, _, pkt, info in rows])
    pk, info = _decode(ptr, n_words, pitch, rows, d_phys)
    n = len(rows)
    bad = [i for i in range(n) if pk[i].tobytes() != want_pk[i].tobytes() or info[i].tobytes() != want_info[i].tobytes()]
    assert not bad, (ctx, len(bad), [(rows[i][:2], pk[i], want_pk[i], info[i], want_info[i]) for i in bad[:2]])
    assert pk[n:].tobytes() == b"\xa5" * PKT * 2 and info[n:].tobytes() == b"\xa5" * CINFO * 2, ctx


def test_far_decode_hits(far):
    """The ordered far hit list of both addresses: every byte of both record arrays."""
    F, t, d_phys = far
    rows = list(fr.far_decoded())
    assert rows == sorted(rows, key=lambda r: r[:2]) and len(rows) > 100
    assert any(o >= 1 << 35 and p["crc_ok"] for _, o, p, _ in rows) and any(o >= 1 << 35 and p["truncated"] for _, o, p, _ in rows)
    _check_decode(t.data_ptr(), F.n_words, F.pitch_words, rows, d_phys, "far")
    for s, ends, w in _refs(F):
        hits = sorted(h for aa in fr.FAR_AAS for h in fr.ref_coded_hits(w, aa))
        short = [(0, o, pkt, info) for o, pkt, info in fr.ref_decode(w, 0, hits, fr.FAR_MHZ[s])]
        d_w = _dev(w)
        _check_decode(d_w.data_ptr(), len(w), len(w), short, _dev(np.array([fr.FAR_MHZ[s]], np.uint16)), ("short", s, ends))


def test_far_cfind_scan_and_durations(far):
    """btbbx_le_cfind_scan_device over both streams, then btbbx_le_ctrack_symbols_device on that candidate list: the run that reads
    beyond byte 2^32 of the buffer -- all of stream 1 lies there."""
    F, t, d_phys = far
    model, pre = (list(x) for x in fr.far_cfind())
    assert sum(x.offset >= 1 << 32 for x, _ in model) >= 8 and sum(x.offset >= 1 << 35 for x, _ in model) >= 4
    assert 8 * F.pitch_words > 1 << 32 and any(x.stream == 1 for x, _ in model)
    _check_cfind(t.data_ptr(), F.n_words, F.pitch_words, 2, F.search_bits, d_phys, model, pre, "far")
    cands = [x for x, _ in model]
    want = fr.far_durations(cands)
    assert want == [i.symbols for _, i in model]
    got = _symbols_device(t, F.n_words, F.pitch_words, 2, cands)
    assert got[:len(cands)].tolist() == want and (got[len(cands):] == 0xA5A5A5A5).all()
    for s, ends, w in _refs(F):
        cd, pr = fr.ref_cfind(w, 0, fr.FAR_MHZ[s])
        short = [(x, i) for _, x, i in cd]
        d_w = _dev(w)
        _check_cfind(d_w.data_ptr(), len(w), len(w), 1, 64 * len(w) - 335, _dev(np.array([fr.FAR_MHZ[s]], np.uint16)), short,
                     [(o, 0, b) for o, b in pr], ("short", s, ends))
        got = _symbols_device(d_w, len(w), len(w), 1, [x for x, _ in short])
        assert got[:len(short)].tolist() == [i.symbols for _, i in short]
