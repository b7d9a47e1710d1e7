"""btbbx_survey_hits_device / btbbx_survey_host on the GPU against the survey loop over the oracle port (tests/_survey.py;
tests/test_survey_model.py pins that loop on the compiled reference).  Integer logic: every field of every record and all 64
candidates must be equal."""
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np
import pytest

import _libs
import _survey as sv
import libbtbb_amd as bt
from libbtbb_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def engine():
    bt.init(2)
    return sv.OracleEngine()


def _run(capture, hits, kw, engine, ctx, **opts):
    taken = min(len(hits) if opts.get("count") is None else opts["count"], opts.get("cap", len(hits)))
    want, want_cand = sv.expected(engine, capture, hits[:taken], kw["clkn0"], kw.get("clk_phase", 0), kw.get("max_length", bt.MAX_SYMBOLS))
    n, recs, cand = bt.run_survey_hits(capture.words(), hits, sv.entry_state(kw["clkn0"]), channels=capture.channels, clk_div=capture.clk_div,
                                       clk_phase=kw.get("clk_phase", 0), max_length=kw.get("max_length", bt.MAX_SYMBOLS),
                                       n_words=capture.n_words, **opts)
    assert n == len(want), (ctx, n, len(want))
    k = len(recs)
    sv.assert_records_equal(recs, cand, want[:k], want_cand[:k], ctx)
    return n, recs, cand, want, want_cand


@pytest.mark.parametrize("name", ["single", "multi", "oops"])
def test_fixture_captures(engine, name):
    cap, kw = sv.FIXTURES[name]()
    hits = cap.hits()
    _run(cap, hits, kw, engine, name)
    _run(cap, hits, kw, engine, name + " counted", count=len(hits))


@pytest.mark.parametrize("clk_phase", [0, 1, 624])
def test_79_streams_pitch_channels_phase_and_clock_wrap(engine, clk_phase):
    channels = (np.arange(79) * 40 + 11) % 79
    cap = sv.Capture(21 + clk_phase, 79, 64 * 512, pitch_extra=5, channels=channels)
    clkn0 = (1 << 27) - 20
    sv.populate(cap, clkn0, clk_phase=clk_phase, n_id=30, n_twins=3)
    hits = cap.hits()
    _run(cap, hits, dict(clkn0=clkn0, clk_phase=clk_phase), engine, "79 streams phase %d" % clk_phase)
    cap.channels = None                                                   # the stream index is the channel
    _run(cap, hits, dict(clkn0=0xFFFFFFF0, clk_phase=clk_phase), engine, "79 streams, identity, uint32 wrap")


def test_list_order_does_not_matter(engine):
    cap, kw = sv.capture_multi()
    hits = cap.hits()
    n, recs, cand, want, want_cand = _run(cap, hits, kw, engine, "ordered")
    perm = np.random.default_rng(5).permutation(len(hits))
    _run(cap, hits[perm], kw, engine, "permuted")
    # ... and the list as btbbx_scan_device leaves it (unordered), through the library's own scan
    lib = bt.lib()
    words = cap.words()
    d_w = bt.DeviceBuffer(words.nbytes + 16).upload(words)
    d_h = bt.DeviceBuffer(16 * 4096)
    d_c = bt.DeviceBuffer(8).zero()
    bt.check(lib.btbbx_scan_device(d_w.ptr, cap.n_words, cap.pitch_words, cap.n_streams, cap.search_bits, bt.LAP_ANY, 2, d_h.ptr, 4096,
                                   d_c.ptr, None))
    bt.check(lib.btbbx_sync(None))
    cnt = int(d_c.download(np.uint32, 2)[0])
    scanned = d_h.download(bt.HIT_DTYPE, cnt)
    assert cnt == len(hits)
    _run(cap, scanned, kw, engine, "as scanned")
    for b in (d_w, d_h, d_c):
        b.free()


def test_host_wrapper_equals_chain_and_oracle(engine):
    cap, kw = sv.capture_multi()
    hits = cap.hits()
    want, want_cand = sv.expected(engine, cap, hits, **kw)
    recs, cand = bt.survey(cap.words(), cap.search_bits, n_streams=cap.n_streams, pitch_words=cap.pitch_words, channels=cap.channels,
                           clkn0=kw["clkn0"], clk_phase=kw["clk_phase"], candidates=True, n_words=cap.n_words)
    # the wrapper's list is the ordered scan's: (stream, offset) order, as cap.hits() -- settled_hit indexes the same list
    sv.assert_records_equal(recs, cand, want, want_cand, "survey()")
    # scan -> survey chained on one stream, the count left on the device
    import torch
    lib = bt.lib()
    words = torch.from_numpy(cap.words().view(np.int64)).cuda()
    capn = 4096
    d_hits = torch.zeros(2 * capn, dtype=torch.int64, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    ob = lib.btbbx_scan_ordered_scratch_bytes(cap.search_bits, cap.n_streams, bt.LAP_ANY, capn)
    sb = lib.btbbx_survey_scratch_bytes(capn)
    d_order = torch.zeros(ob // 8 + 2, dtype=torch.int64, device="cuda")
    d_scr = torch.zeros(sb // 8 + 2, dtype=torch.int64, device="cuda")
    d_recs = torch.zeros(capn * 8, dtype=torch.int64, device="cuda")
    d_cand = torch.zeros(capn * 64, dtype=torch.int16, device="cuda")
    q = torch.cuda.Stream()
    torch.cuda.synchronize()
    entry = sv.entry_state(kw["clkn0"])
    table = np.ascontiguousarray(cap.channels, dtype=np.uint8)
    bt.check(lib.btbbx_scan_ordered_device(words.data_ptr(), cap.n_words, cap.pitch_words, cap.n_streams, cap.search_bits, bt.LAP_ANY, 2,
                                           d_hits.data_ptr(), capn, d_cnt.data_ptr(), d_order.data_ptr(), ob, q.cuda_stream))
    bt.check(lib.btbbx_survey_hits_device(words.data_ptr(), cap.n_words, cap.pitch_words, cap.n_streams, d_hits.data_ptr(),
                                          d_cnt.data_ptr(), capn, bt._ptr(table), bt._ptr(entry), cap.clk_div, kw["clk_phase"],
                                          bt.MAX_SYMBOLS, d_recs.data_ptr(), capn, d_cnt.data_ptr() + 4, d_cand.data_ptr(),
                                          d_scr.data_ptr(), sb, q.cuda_stream))
    q.synchronize()
    n_hits, n_recs = (int(x) for x in d_cnt.cpu().numpy()[:2])
    assert n_hits == len(hits) and n_recs == len(want)
    chain = d_recs.cpu().numpy().view(bt.SURVEY_DTYPE)[:n_recs]
    chain_cand = d_cand.cpu().numpy().reshape(-1, 64)[:n_recs]
    sv.assert_records_equal(chain, chain_cand, recs, cand, "chain == wrapper")


def test_caps(engine):
    cap, kw = sv.capture_multi()
    hits = cap.hits()
    perm = np.random.default_rng(6).permutation(len(hits))
    some = hits[perm]
    _run(cap, some, kw, engine, "cap below the list", count=len(some), cap=len(some) // 2)           # the first cap of the list
    _run(cap, some, kw, engine, "count below cap", count=len(some) // 3)
    n, recs, cand, want, _ = _run(cap, some, kw, engine, "rec_cap below the piconets", rec_cap=7)
    assert n == len(want) > 7 and len(recs) == 7 and recs["lap"].tolist() == sorted(want["lap"].tolist())[:7]
    n, recs, cand, want, _ = _run(cap, some, kw, engine, "rec_cap 1", rec_cap=1)
    assert len(recs) == 1
    _run(cap, some, kw, engine, "cap 1", count=len(some), cap=1)
    n, recs, cand = bt.run_survey_hits(cap.words(), some, sv.entry_state(0), channels=cap.channels, count=0, n_words=cap.n_words)
    assert n == 0 and len(recs) == 0
    n, recs, cand, want, _ = _run(cap, some, kw, engine, "no candidates wanted", candidates=False)
    assert cand is None
    n, recs, cand = bt.run_survey_hits(cap.words(), some, sv.entry_state(0), channels=cap.channels, cap=0, n_words=cap.n_words)
    assert n == 0 and len(recs) == 0                                       # cap 0: nothing launched but the count's reset
    n, recs, cand = bt.run_survey_hits(cap.words(), some, sv.entry_state(kw["clkn0"]), channels=cap.channels, clk_phase=kw["clk_phase"],
                                       rec_cap=0, n_words=cap.n_words)
    assert n == len(want) and len(recs) == 0                               # rec_cap 0: piconets counted, none stored


def _device_ms(cap, hits, kw, repeats=5):
    """median time of btbbx_survey_hits_device alone (HIP events, everything resident)"""
    import torch
    lib = bt.lib()
    words = torch.from_numpy(cap.words().view(np.int64)).cuda()
    d_hits = torch.from_numpy(np.ascontiguousarray(hits).view(np.int64)).cuda()
    n = len(hits)
    sb = lib.btbbx_survey_scratch_bytes(n)
    scr = torch.empty(sb // 8 + 2, dtype=torch.int64, device="cuda")
    recs = torch.empty(n * 8, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    entry = sv.entry_state(kw["clkn0"])
    q = torch.cuda.current_stream().cuda_stream
    out = []
    for k in range(repeats + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        bt.check(lib.btbbx_survey_hits_device(words.data_ptr(), cap.n_words, cap.pitch_words, cap.n_streams, d_hits.data_ptr(), None, n,
                                              None, bt._ptr(entry), cap.clk_div, 0, kw.get("max_length", bt.MAX_SYMBOLS), recs.data_ptr(),
                                              n, cnt.data_ptr(), None, scr.data_ptr(), sb, q))
        b.record()
        b.synchronize()
        if k >= 2:
            out.append(a.elapsed_time(b))
    return float(np.median(out))


def test_walk_that_never_settles(engine):
    """2^17 header-bearing packets of one LAP that never settle: the pattern memory fills and resets 130 times.  The time of
    the device call is printed, and what a further walked packet costs, whatever it is."""
    n_same = 1 << 17
    cap, kw = sv.capture_oops(seed=14, n_same=n_same)
    hits = cap.hits()
    assert (hits["lap"] == 0x3A71C5).sum() == n_same
    n, recs, cand = bt.run_survey_hits(cap.words(), hits, sv.entry_state(kw["clkn0"]), clk_div=cap.clk_div, max_length=kw["max_length"])
    r = recs[recs["lap"] == 0x3A71C5][0]
    # the device call alone, HIP events: this list, and the same list cut to its first 2^13 packets.  Sort, gather and trials
    # are parallel over the list; what grows with the list beyond them is the one wave's walk.
    ms_all = _device_ms(cap, hits, kw)
    ms_few = _device_ms(cap, hits[:1 << 13], kw)
    per_packet_ns = 1e6 * (ms_all - ms_few) / (n_same - (1 << 13))
    print("\nnever-settling walk: %d packets, %d resets: device call %.3f ms (2^13 packets: %.3f ms) -> %.0f ns per further walked packet;"
          " a memory latency per packet would be 500-2000 ns, the wave keeps 16 trial rows in flight"
          % (r["n_walked"], r["n_resets"], ms_all, ms_few, per_packet_ns))
    # the reference on the first 2100 packets gives the period: 1000 counted, one reset, again
    few = hits[hits["lap"] == 0x3A71C5][:2100]
    want, want_cand = sv.expected(engine, cap, few, kw["clkn0"], 0, kw["max_length"])
    assert want[0]["n_resets"] == 2 and want[0]["packets_observed"] == 2100 - 2002
    assert r["settled_by"] == 0 and r["n_walked"] == n_same and r["n_resets"] == n_same // 1001
    assert r["packets_observed"] == n_same - 1001 * (n_same // 1001) and r["total_packets_observed"] == n_same - n_same // 1001
    assert (cand[recs["lap"] == 0x3A71C5][0] == want_cand[0]).all()


class _Line:
    """a stream held as packed words, unpacked where it is read"""

    def __init__(self, words):
        self.words = words

    def __len__(self):
        return 64 * len(self.words)

    def __getitem__(self, sl):
        lo, hi = sl.start, min(sl.stop, len(self))
        return synth.unpack_bits(self.words[lo // 64:-(-hi // 64)])[lo - 64 * (lo // 64):][:hi - lo]


def test_one_piconet_owning_a_million_hits_among_singletons(engine):
    """The config-3 shape, built on the device: stream 0 carries ONE LAP every 512 symbols (2^20 hits), stream 1 a random LAP
    every 8192 symbols (2^16 singletons).  The first symbols of stream 0 are replaced by real packets of the big piconet, so its
    walk opens, goes on and settles on a CRC before the million header-less access codes behind them only mark their channel."""
    import torch
    lib = bt.lib()
    big, uap, off6, clkn0 = 0x5A7C31, 0xB3, 17, 1000
    n_words = 1 << 23
    words = torch.empty(2 * n_words, dtype=torch.int64, device="cuda")
    bt.check(lib.btbbx_synth_device(words.data_ptr(), 0, n_words, 7, 512, big, 3, None))
    bt.check(lib.btbbx_synth_device(words.data_ptr() + 8 * n_words, 0, n_words, 8, 8192, -1, 3, None))
    head = sv.Capture(31, 1, 64 * 256)
    for slot, ptype in ((0, synth.TYPE_POLL), (3, synth.TYPE_NULL), (4, synth.TYPE_POLL), (9, synth.TYPE_DM1), (12, synth.TYPE_POLL)):
        head.put(0, slot, sv._pkt(big, uap, (clkn0 + slot + off6) & 63, ptype, head.rng))
    words[:256] = torch.from_numpy(head.words()[0].view(np.int64)).cuda()
    search_bits = n_words * 64 - 63
    cap = (1 << 20) + (1 << 16) + (1 << 16)
    d_hits = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    ob = lib.btbbx_scan_ordered_scratch_bytes(search_bits, 2, bt.LAP_ANY, cap)
    sb = lib.btbbx_survey_scratch_bytes(cap)
    order = torch.empty(ob // 8 + 2, dtype=torch.int64, device="cuda")
    scratch = torch.empty(sb // 8 + 2, dtype=torch.int64, device="cuda")
    d_recs = torch.zeros(cap * 8, dtype=torch.int64, device="cuda")
    d_cand = torch.zeros(cap * 64, dtype=torch.int16, device="cuda")
    entry = sv.entry_state(clkn0)
    q = torch.cuda.current_stream().cuda_stream
    bt.check(lib.btbbx_scan_ordered_device(words.data_ptr(), n_words, n_words, 2, search_bits, bt.LAP_ANY, 2, d_hits.data_ptr(), cap,
                                           cnt.data_ptr(), order.data_ptr(), ob, q))
    bt.check(lib.btbbx_survey_hits_device(words.data_ptr(), n_words, n_words, 2, d_hits.data_ptr(), cnt.data_ptr(), cap, None,
                                          bt._ptr(entry), 625, 0, bt.MAX_SYMBOLS, d_recs.data_ptr(), cap, cnt.data_ptr() + 4,
                                          d_cand.data_ptr(), scratch.data_ptr(), sb, q))
    torch.cuda.synchronize()
    n_hits, n_pn = (int(x) for x in cnt.cpu().numpy()[:2])
    assert (1 << 20) + (1 << 16) - 64 <= n_hits <= cap
    hits = d_hits.cpu().numpy().view(bt.HIT_DTYPE)[:n_hits]
    recs = d_recs.cpu().numpy().view(bt.SURVEY_DTYPE)[:n_pn]
    cand = d_cand.cpu().numpy().reshape(-1, 64)[:n_pn]
    # properties over all records
    assert int(recs["n_packets"].sum()) == n_hits
    assert (np.diff(recs["lap"].astype(np.int64)) > 0).all()
    assert n_pn == len(np.unique(hits["lap"]))
    bits = np.unpackbits(recs["afh_map"], axis=1).sum(axis=1)
    assert (recs["used_channels"] == bits).all() and (bits >= 1).all() and (bits <= 2).all()
    one = recs[recs["lap"] == big][0]
    # (the 256 replaced words held 32 of the generator's 2^20 access codes; five packets took their place)
    assert (1 << 20) - 32 <= one["n_packets"] <= (1 << 20) + 5 and one["settled_by"] == 2 and one["uap"] == uap and one["clk_offset"] == off6
    # the survey loop over the oracle: the big piconet and a sample of the others
    host = words.cpu().numpy().view(np.uint64).reshape(2, n_words)

    class Both:
        sym, channels, clk_div = [_Line(host[0]), _Line(host[1])], None, 625
    rng = np.random.default_rng(9)
    sample = set(int(x) for x in rng.choice(recs["lap"], 300, replace=False)) | {big}
    want, want_cand = sv.expected(engine, Both, hits, clkn0, only_laps=sample)
    keep = np.isin(recs["lap"], sorted(sample))
    sv.assert_records_equal(recs[keep], cand[keep], want, want_cand, "sample of the million-hit capture")


_CHILD = r"""
import sys, json, ctypes as C
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tests")
import libbtbb_amd as bt, _survey as sv
lib = bt.lib()
lib.btbb_init(2)
cap, kw = sv.capture_single()
hits = cap.hits()
lib.btbb_init_survey()
out = []
sys.stdout.flush()
for k in np.lexsort((hits["stream"], hits["offset"])):
    h = hits[k]
    sym = sv.packet_symbols(cap, h)
    buf = np.ascontiguousarray(np.concatenate([sym, np.zeros(64, np.uint8)]))
    pkt = C.c_void_p(None)
    at = lib.btbb_find_ac(bt._ptr(buf), 1, bt.LAP_ANY, 2, C.byref(pkt))
    assert at == 0, at
    clkn = (kw["clkn0"] + int(h["offset"]) // cap.clk_div) & 0x7FFFFFFF
    lib.btbb_packet_set_data(pkt, bt._ptr(sym), len(sym), int(h["stream"]), clkn << 1)
    lib.btbb_process_packet(pkt, None)
    lib.btbb_packet_unref(pkt)
while True:
    pn = lib.btbb_next_survey_result()
    if not pn:
        break
    amap = bytes((C.c_uint8 * 10).from_address(lib.btbb_piconet_get_afh_map(pn)))
    out.append(dict(lap=lib.btbb_piconet_get_lap(pn), uap=lib.btbb_piconet_get_uap(pn), clk_offset=lib.btbb_piconet_get_clk_offset(pn) & 0xff,
                    flags=int(lib.btbbx_piconet_state(pn, 5)), packets_observed=int(lib.btbbx_piconet_state(pn, 2)),
                    total=int(lib.btbbx_piconet_state(pn, 3)), first_pkt_time=int(lib.btbbx_piconet_state(pn, 4)),
                    used=int(lib.btbbx_piconet_state(pn, 6)), afh=list(amap)))
sys.stderr.write("SURVEY_JSON " + json.dumps(out) + "\n")
"""


def test_batch_survey_equals_drop_in_survey_mode():
    """the product's own btbb_init_survey / btbb_process_packet / btbb_next_survey_result, one packet per call, in a child
    process (its survey mode has no off switch)"""
    bt.init(2)
    cap, kw = sv.capture_single()
    recs = bt.survey(cap.words(), cap.search_bits, clkn0=kw["clkn0"])
    child = subprocess.run([sys.executable, "-c", _CHILD % dict(root=ROOT)], capture_output=True, text=True, timeout=600)
    assert child.returncode == 0, child.stderr[-2000:]
    line = [ln for ln in child.stderr.splitlines() if ln.startswith("SURVEY_JSON ")][-1]
    got = {d["lap"]: d for d in json.loads(line[len("SURVEY_JSON "):])}
    assert sorted(got) == recs["lap"].tolist() and len(recs) > 30
    for r in recs:
        d = got[int(r["lap"])]
        assert (d["uap"], d["clk_offset"], d["flags"], d["packets_observed"], d["total"], d["first_pkt_time"], d["used"], d["afh"]) == \
            (r["uap"], r["clk_offset"], r["flags"], r["packets_observed"], r["total_packets_observed"], r["first_pkt_time"],
             r["used_channels"], r["afh_map"].tolist()), hex(int(r["lap"]))


def test_two_host_threads(engine):
    caps = [sv.capture_single(), sv.capture_multi()]
    wants = [sv.expected(engine, c, c.hits(), **kw) for c, kw in caps]
    results, errors = [None, None], []

    def work(i):
        try:
            c, kw = caps[i]
            for _ in range(4):
                results[i] = bt.survey(c.words(), c.search_bits, n_streams=c.n_streams, pitch_words=c.pitch_words, channels=c.channels,
                                       clkn0=kw["clkn0"], clk_phase=kw["clk_phase"], candidates=True, n_words=c.n_words)
        except Exception as e:                                          # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        sv.assert_records_equal(results[i][0], results[i][1], wants[i][0], wants[i][1], "thread %d" % i)
