"""GPU: the hit ordering and the segment-slot compaction (libbtbb_amd/csrc/sort.hip) on the branch lattice of
tests/_order_model.py -- every named list through every entry, compared record for record with a plain lexsort; the scan-counted
general path, order_single_kernel and the compaction on streams built for their branches, compared with the oracle.  The model
says which branch tags a call takes; tests/test_order_model.py checks on the CPU that the lattice covers them all.
Run with `-m gpu` on an MI355X."""
import functools

import numpy as np
import pytest

import _libs
import _order_model as om
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu

KEY_FIELDS = ("stream", "offset", "lap", "ac_errors")


@pytest.fixture(scope="module", autouse=True)
def ready():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    bt.lib().btbbx_shutdown()
    bt.init(2)
    orc = _libs.oracle()
    orc.orc_reset_syndrome_map()
    orc.orc_init(2)
    yield
    bt.lib().btbbx_shutdown()


def patterned(nbytes, byte):
    """Device memory that holds a non-zero byte pattern: nothing may rely on fresh memory being zero."""
    b = bt.DeviceBuffer(nbytes)
    bt.check(bt.lib().btbbx_memset(b.ptr, byte, b.nbytes), "memset")
    return b


# ---- a. caller-supplied lists ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def lattice_list(name):
    case = next(c for c in om.LATTICE if c.name == name)
    hits = case.build()
    hits.setflags(write=False)
    return case, hits


def lattice_runs():
    """(case, run) pairs: every case through the three entries that read the count from HBM, and through btbbx_sort_hits_device
    where count == cap == the length (that entry has one number for all three)."""
    out = []
    for c in om.LATTICE:
        cap, count = om.case_numbers(c, lattice_list(c.name)[1])
        out += [(c.name, run) for run in ("extent", "exact", "loose")]
        if cap == count == len(lattice_list(c.name)[1]):
            out.append((c.name, "sort"))
    return out


@pytest.mark.parametrize("name,run", lattice_runs(), ids=lambda v: v)
def test_lattice_list_through_every_entry(name, run):
    """extent: btbbx_order_hits_device; exact / loose: btbbx_order_scan_hits_device with the list's own extent / with wider
    bounds (fine, non-power-of-two bucket counts); sort: btbbx_sort_hits_device.  The first min(count, cap) records come back in (stream, offset) order, the records behind them are
    untouched; hit buffer and scratch are pre-filled with a byte pattern."""
    lib = bt.lib()
    case, hits = lattice_list(name)
    cap, count = om.case_numbers(case, hits)
    tags = om.run_tags(case, hits, run)
    if run == ("loose" if case.form == "bounds" else case.form):
        assert case.tags <= tags
    n = min(count, cap)
    keep = cap if cap <= 1 << 19 else n + 4096             # (the two cases with millions of empty records: only what matters comes back)
    room = np.frombuffer(b"\xa5" * (16 * keep), dtype=bt.HIT_DTYPE).copy()
    room[:min(len(hits), keep)] = hits[:keep]
    d = patterned(cap * 16, 0xA5).upload(hits[:cap])
    bufs = [d]
    try:
        if run == "sort":
            bt.check(lib.btbbx_sort_hits_device(d.ptr, cap, None), "btbbx_sort_hits_device")
        else:
            c = bt.DeviceBuffer(16).upload(np.array([count, 0x5A5A5A5A, 0x5A5A5A5A, 0x5A5A5A5A], np.uint32))
            sb = lib.btbbx_order_hits_scratch_bytes(cap)
            s = patterned(sb, 0x5A)
            bufs += [c, s]
            if run == "extent":
                bt.check(lib.btbbx_order_hits_device(d.ptr, c.ptr, cap, s.ptr, sb, None), "btbbx_order_hits_device")
            else:
                ns, bits = om.case_bounds(case, hits, run == "loose")
                bt.check(lib.btbbx_order_scan_hits_device(d.ptr, c.ptr, cap, ns, bits, s.ptr, sb, None), "btbbx_order_scan_hits_device")
        bt.check(lib.btbbx_sync(None), "sync")
        got = d.download(bt.HIT_DTYPE, keep)
        if run != "sort":
            assert int(c.download(np.uint32, 4)[0]) == count
    finally:
        for b in bufs:
            b.free()
    want = om.expected(hits, count, cap)
    unique = not om.has_repeats(hits, count, cap)
    if not om.same_list(got[:n], want, unique):
        keys = lambda a: (a["stream"].astype(np.uint64) << np.uint64(48)) | a["offset"]
        bad = np.flatnonzero(keys(got[:n]) != keys(want))
        first = int(bad[0]) if len(bad) else -1
        raise AssertionError("%s / %s %s: %d of %d keys out of place, the first at %d (got %s, want %s)" % (
            name, run, sorted(tags), len(bad), n, first, got[first] if first >= 0 else "-", want[first] if first >= 0 else "records differ"))
    assert got[n:].tobytes() == room[n:].tobytes(), "records behind min(count, cap) were touched"


def scan_ordered(words, n_words, pitch, n_streams, bits, lap, cap, slots):
    """btbbx_scan_ordered_device on pattern-filled buffers -> (count, list, SlotHeader or None)."""
    lib = bt.lib()
    d_w = bt.DeviceBuffer(words.nbytes).upload(words)
    d_h = patterned(cap * 16, 0xA5)
    d_c = bt.DeviceBuffer(16).upload(np.array([0x5A5A5A5A] * 4, np.uint32))       # stale: the call owns the counter
    front = lib.btbbx_order_hits_scratch_bytes(cap)
    sb = lib.btbbx_scan_ordered_scratch_bytes(bits, n_streams, lap, cap) if slots else front
    assert (sb > front) == slots
    d_s = patterned(sb, 0x5A)
    try:
        bt.check(lib.btbbx_scan_ordered_device(d_w.ptr, n_words, pitch, n_streams, bits, lap, 2, d_h.ptr, cap, d_c.ptr, d_s.ptr, sb, None),
                 "btbbx_scan_ordered_device")
        bt.check(lib.btbbx_sync(None), "sync")
        cnt = int(d_c.download(np.uint32, 4)[0])
        got = d_h.download(bt.HIT_DTYPE, cap)
        header = None
        if slots:
            at = om.slot_header_offset(front)
            header = om.slot_header(d_s.download(np.uint32, at // 4 + 4)[at // 4:])
    finally:
        for b in (d_w, d_h, d_c, d_s):
            b.free()
    tup = [tuple(int(h[f]) for f in KEY_FIELDS) for h in got[:min(cnt, cap)]]
    assert (got["reserved"][:min(cnt, cap)] == 0).all()
    return cnt, tup, header, got


@pytest.mark.parametrize("cap,tag", om.BURST_CASES)
@pytest.mark.parametrize("lap", om.STREAM_LAPS)
def test_scan_counted_general_path_with_shared_and_crowded_buckets(lap, cap, tag):
    """b. btbbx_scan_ordered_device with the scratch of btbbx_order_hits_scratch_bytes only: the scan kernels count every record in
    its bucket, then scan of the counts, order_scatter_kernel with `final` and `work`, order_rank_list_kernel, order_crowded_kernel.
    The burst puts 32 or more records into buckets of 2048 keys (cap 600: order_rank_list_kernel ranks them) and 64 or more into
    buckets of 4096 (cap 300: all pairs); the model, fed the oracle's list, says so."""
    words, bits, want = om.burst_stream(lap)
    assert 260 <= len(want) <= 300
    tags = om.classify(om.as_records(want), len(want), cap, "scan", 1, bits)
    assert {tag, "alone", "count_lt_cap"} <= tags and ("pairs" in tags) == (tag == "pairs")
    cnt, got, _, raw = scan_ordered(words, om.BURST_WORDS, om.BURST_WORDS, 1, bits, lap, cap, slots=False)
    assert cnt == len(want) and got == want
    assert raw[cnt:].tobytes() == b"\xa5" * (16 * (cap - cnt))


@pytest.mark.parametrize("cap,tag", om.BURST_CASES)
@pytest.mark.parametrize("lap", om.STREAM_LAPS)
def test_order_single_kernel_ranks_shared_and_crowded_buckets(lap, cap, tag):
    """c. The same streams with the full slot scratch: the slots refuse the burst, the gated re-scan parks the list and
    order_single_kernel orders it in one workgroup -- its own copy of the shared-bucket ranking (cap 600) and its call of
    order_crowded_body(..., 0, 1) for buckets of more than 48 (cap 300: all pairs).  The SlotHeader, read from the caller's
    scratch, proves the path: irregular == 1 and redo_count == *d_count.
    Not reached: the presence bitmap inside order_single_kernel.  It needs more than 4096 hits in one bucket, at least 32 offsets
    apart, while the bucket count is at least twice the capacity -- a stream of 2^31 offsets or more; it is the same
    order_crowded_body that test_lattice_list_through_every_entry covers through order_crowded_kernel."""
    words, bits, want = om.burst_stream(lap)
    tags = om.classify(om.as_records(want), len(want), cap, "scan", 1, bits)
    assert {tag, "alone"} <= tags and ("pairs" in tags) == (tag == "pairs")
    cnt, got, header, raw = scan_ordered(words, om.BURST_WORDS, om.BURST_WORDS, 1, bits, lap, cap, slots=True)
    print("SlotHeader", header)
    assert header.irregular == 1 and header.redo_count == cnt
    assert cnt == len(want) and got == want
    assert raw[cnt:].tobytes() == b"\xa5" * (16 * (cap - cnt))


# ---- d. compaction -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("lap", om.STREAM_LAPS)
def test_compaction_over_two_workgroups_with_every_segment_population(lap):
    """d. slot_sums_kernel / slot_place_kernel / slot_overflow_kernel: more than 8192 segments (two workgroups of slot_place_kernel:
    `before`), a ragged segment count (LAP_ANY), segments of 0, 1, 2, 3 and 20 hits, hits on the first and last offset of a segment
    and on both sides of a stream's end.  cap >= count: the oracle's list.  cap < count with room in the overflow list: exactly
    the cap smallest records -- the cut once between a segment's two slots, once inside its overflow records -- and the full
    count.  cap < count with the overflow list full: the general path redoes the call; ordered, a subset, the full count.
    The oracle runs on the whole of every stream (about a second per stream on the host)."""
    words, n_words, pitch, bits, want, oracle_s = om.slot_stream(lap)
    print("oracle: %.2f s for %d hits" % (oracle_s, len(want)))
    keys = [(s, o) for (s, o, _, _) in want]
    count = len(want)
    assert 500 <= count <= 2000
    tags = om.slot_tags(keys, bits, 3, lap, count + 50)
    need = set(om.SLOT_NEED)
    if lap == bt.LAP_ANY:
        need.add("n_segs_ragged")
    assert need <= tags, sorted(need - tags)
    cnt, got, header, raw = scan_ordered(words, n_words, pitch, 3, bits, lap, count + 50, slots=True)
    assert header.irregular == 0 and header.total == count and header.redo_count == 0
    assert cnt == count and got == want
    assert raw[count:].tobytes() == b"\xa5" * (16 * 50)
    caps = om.slot_caps(want, bits, lap)
    for tag in ("cut_between_slots", "cut_in_overflow"):
        cap = caps[tag]
        assert {tag, "overflow_fits"} <= om.slot_tags(keys, bits, 3, lap, cap), (cap, tag)
        cnt, got, header, _ = scan_ordered(words, n_words, pitch, 3, bits, lap, cap, slots=True)
        assert header.irregular == 0 and header.total == count, (tag, header)
        assert cnt == count and got == want[:cap], tag
    cap = caps["overflow_full"]
    assert "overflow_full" in om.slot_tags(keys, bits, 3, lap, cap)
    cnt, got, header, _ = scan_ordered(words, n_words, pitch, 3, bits, lap, cap, slots=True)
    assert header.irregular == 1 and header.redo_count == count
    assert cnt == count and len(got) == cap and got == sorted(got) and set(got) <= set(want)
