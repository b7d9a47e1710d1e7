"""Times of the FOLLOWING stage on cuda:0: btbbx_follow_hits_device behind survey -> job builder -> batch reversal, on the
2301-piconet crowd of tests/_crowd.py (its placement list) and on the 79-channel hopping capture of tests/_acquire.py (three
piconets; hits from btbbx_scan_ordered_device).  One JSON line per capture:
  follow_ms    HIP events around btbbx_follow_hits_device (the chain done before, nothing read back)
  decoder_ms   ... around btbbx_decode_hits_counted_device over the d_in the follow left: the decoder's share of follow_ms
  own_ms       follow_ms - decoder_ms of the same round: the follow's three launches
  plain_ms     ... around btbbx_decode_hits_piconet_phase_device over the same list: the same decoder without per-piconet
               state (every hit with the entry state and the receiver's clock) -- the yardstick
  host_ms      host clock around the composition the follow replaces, after the same chain: download records, job records and
               results, build btbbx_pkt_in per hit in numpy, upload, btbbx_decode_hits_counted_device, synchronise (no hop
               check, no summaries: a lower bound of the host path)
Events: 3 warm-ups of every call, then --launches rounds; a round times --inner calls of each of the three device paths one
after the other (alternating, so that a drift of the machine hits all three), per-call times as [median, min, max] over the
rounds.  host_ms: median, min, max of 5.  The tool asserts that the host composition builds the same d_in and gets the same
d_out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def host_pkt_in(bt, hits, recs, job_rec, results, clkn0, clk_div, clk_phase):
    """btbbx_pkt_in of every hit as include/btbbx.h states the stages, in numpy"""
    pin = np.zeros(len(hits), dtype=bt.PKTIN_DTYPE)
    c = ((clkn0 + (hits["offset"] + np.uint64(clk_phase)) // np.uint64(clk_div)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    pos = np.minimum(np.searchsorted(recs["lap"], hits["lap"]), len(recs) - 1)
    known = recs["lap"][pos] == hits["lap"]
    stage = (recs["settled_by"] != 0).astype(np.uint8)
    cand0 = np.zeros(len(recs), dtype=np.uint32)
    ok = (results["status"] == 0) & (results["count"] == 1)
    stage[job_rec[ok]] = 2
    cand0[job_rec[ok]] = results["cand0"][ok]
    st = np.where(known, stage[pos], 0)
    pin["flags"] = 1 | np.where(st >= 1, (1 << 2) | (1 << 4), 0) | np.where(st == 2, 1 << 5, 0)
    pin["uap"] = np.where(st >= 1, recs["uap"][pos], 0)
    pin["clkn"] = np.where(st == 2, (cand0[pos] + c - recs["first_pkt_time"][pos]) & np.uint32((1 << 27) - 1),
                           np.where(st == 1, (recs["clk_offset"][pos] + c) & 63, c))
    return pin


def measure(name, words_np, n_words, channels, clkn0, clk_div, hits_np, args):
    import torch
    import bench
    import libbtbb_amd as bt
    lib = bt.lib()
    n_streams, pitch = words_np.shape
    words = torch.from_numpy(np.ascontiguousarray(words_np).view(np.int64)).cuda()
    q = torch.cuda.current_stream().cuda_stream
    search_bits = n_words * 64 - 63
    table = None if channels is None else np.ascontiguousarray(channels, dtype=np.uint8)
    tp = None if table is None else bt._ptr(table)
    cnt = torch.zeros(8, dtype=torch.int32, device="cuda")       # hits, piconets, jobs, observations
    if hits_np is None:
        cap = 1 << 16
        d_hits = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
        ob = lib.btbbx_scan_ordered_scratch_bytes(search_bits, n_streams, bt.LAP_ANY, cap)
        order = torch.empty(ob // 8 + 2, dtype=torch.int64, device="cuda")
        bt.check(lib.btbbx_scan_ordered_device(words.data_ptr(), n_words, pitch, n_streams, search_bits, bt.LAP_ANY, 2, d_hits.data_ptr(), cap,
                                               cnt.data_ptr(), order.data_ptr(), ob, q))
        torch.cuda.synchronize()
        n_hits = int(cnt[0])
        assert 0 < n_hits <= cap
        cap = n_hits
    else:
        n_hits = cap = len(hits_np)
        d_hits = torch.from_numpy(np.frombuffer(np.ascontiguousarray(hits_np).tobytes(), dtype=np.int64).copy()).cuda()
        cnt[0] = n_hits
    sb = lib.btbbx_survey_scratch_bytes(cap)
    scratch = torch.empty(sb // 8 + 2, dtype=torch.int64, device="cuda")
    d_recs = torch.zeros(cap * 8, dtype=torch.int64, device="cuda")
    d_jobs = torch.zeros(cap * 13, dtype=torch.int64, device="cuda")
    d_jrec = torch.zeros(cap, dtype=torch.int32, device="cuda")
    d_off = torch.zeros(cap, dtype=torch.int32, device="cuda")
    d_ch = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    entry = np.zeros(1, dtype=bt.PKTIN_DTYPE)
    entry["clkn"], entry["flags"] = clkn0, 1
    ep = bt._ptr(entry)
    bt.check(lib.btbbx_survey_hits_device(words.data_ptr(), n_words, pitch, n_streams, d_hits.data_ptr(), cnt.data_ptr(), cap, tp, ep, clk_div, 0,
                                          bt.MAX_SYMBOLS, d_recs.data_ptr(), cap, cnt.data_ptr() + 4, None, scratch.data_ptr(), sb, q))
    bt.check(lib.btbbx_survey_clock_jobs_device(d_recs.data_ptr(), cnt.data_ptr() + 4, cap, scratch.data_ptr(), sb, cap, tp, n_streams, 0, 1024,
                                                d_jobs.data_ptr(), cap, cnt.data_ptr() + 8, d_jrec.data_ptr(), d_off.data_ptr(),
                                                d_ch.data_ptr(), None, cap, cnt.data_ptr() + 12, q))
    torch.cuda.synchronize()
    n_recs, n_jobs, n_obs = (int(x) for x in cnt.cpu().numpy()[1:4])
    rev_cap = max(n_jobs, 1)
    bs = lib.btbbx_hop_reversal_batch_scratch_bytes(rev_cap, 0)
    bscr = torch.empty(bs // 8 + 2, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(rev_cap * 6, dtype=torch.int32, device="cuda")
    bt.check(lib.btbbx_hop_reversal_batch_device(d_jobs.data_ptr(), cnt.data_ptr() + 8, rev_cap, d_off.data_ptr(), d_ch.data_ptr(), cap,
                                                 d_res.data_ptr(), None, 0, bscr.data_ptr(), bs, q))
    out_words = bt.PKTOUT_DTYPE.itemsize // 8
    d_in = torch.zeros(cap * 2, dtype=torch.int64, device="cuda")
    d_fol = torch.zeros(cap * 2, dtype=torch.int64, device="cuda")
    d_out = torch.zeros(cap * out_words, dtype=torch.int64, device="cuda")
    d_out2 = torch.zeros(cap * out_words, dtype=torch.int64, device="cuda")
    d_out4 = torch.zeros(cap * out_words, dtype=torch.int64, device="cuda")
    d_sums = torch.zeros(cap * 4, dtype=torch.int64, device="cuda")

    def follow():
        bt.check(lib.btbbx_follow_hits_device(words.data_ptr(), n_words, pitch, n_streams, d_hits.data_ptr(), cnt.data_ptr(), cap, d_recs.data_ptr(),
                                              cnt.data_ptr() + 4, cap, d_jobs.data_ptr(), d_jrec.data_ptr(), d_res.data_ptr(), cnt.data_ptr() + 8,
                                              rev_cap, tp, ep, clk_div, 0, bt.MAX_SYMBOLS, d_in.data_ptr(), d_fol.data_ptr(), d_out.data_ptr(),
                                              None, d_sums.data_ptr(), q))

    def decoder(in_ptr=None, out=None):
        bt.check(lib.btbbx_decode_hits_counted_device(words.data_ptr(), n_words, pitch, d_hits.data_ptr(), in_ptr or d_in.data_ptr(),
                                                      cnt.data_ptr(), cap, bt.MAX_SYMBOLS, (d_out2 if out is None else out).data_ptr(), None, q))

    def plain():
        bt.check(lib.btbbx_decode_hits_piconet_phase_device(words.data_ptr(), n_words, pitch, d_hits.data_ptr(), cnt.data_ptr(), cap, ep, clk_div,
                                                            0, bt.MAX_SYMBOLS, d_out4.data_ptr(), None, q))
    paths = (follow, decoder, plain)
    for fn in paths:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in paths]
    for _ in range(args.launches):
        for k, fn in enumerate(paths):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.inner):
                fn()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / args.inner)
    stat = lambda v: [round(float(x), 4) for x in (np.median(v), min(v), max(v))]
    own = [f - d for f, d in zip(times[0], times[1])]
    d_out.zero_()                                                 # (the decoders take a record's content for the packet's earlier state)
    follow()
    torch.cuda.synchronize()
    want_in = d_in.cpu().numpy().view(bt.PKTIN_DTYPE)[:n_hits].copy()
    want_out = d_out.cpu().numpy().tobytes()[:n_hits * bt.PKTOUT_DTYPE.itemsize]
    sums = d_sums.cpu().numpy().view(bt.FOLLOW_SUM_DTYPE)[:n_recs]
    fol = d_fol.cpu().numpy().view(bt.FOLLOW_PKT_DTYPE)[:n_hits]
    d_out3 = torch.zeros(cap * out_words, dtype=torch.int64, device="cuda")

    def host():
        h_recs = d_recs[:n_recs * 8].cpu().numpy().view(bt.SURVEY_DTYPE)
        h_hits = d_hits[:n_hits * 2].cpu().numpy().view(bt.HIT_DTYPE)
        h_jrec = d_jrec[:n_jobs].cpu().numpy().view(np.uint32)
        h_res = d_res[:n_jobs * 6].cpu().numpy().view(bt.CLOCK_RESULT_DTYPE)
        pin = host_pkt_in(bt, h_hits, h_recs, h_jrec, h_res, clkn0, clk_div, 0)
        u_in = torch.from_numpy(np.frombuffer(pin.tobytes(), dtype=np.int64).copy()).cuda()
        d_out3.zero_()
        decoder(u_in.data_ptr(), d_out3)
        torch.cuda.synchronize()
        return pin
    assert host().tobytes() == want_in.tobytes(), "the host composition builds another d_in"
    assert d_out3.cpu().numpy().tobytes()[:len(want_out)] == want_out, "the host composition decodes differently"
    out = []
    for _ in range(5):
        t0 = time.perf_counter()
        host()
        out.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(capture=name, hits=n_hits, records=n_recs, jobs=n_jobs, stage_hits=np.bincount(fol["stage"], minlength=3).tolist(),
                          on_hop=int(sums["n_on_hop"].sum()), off_hop=int(sums["n_off_hop"].sum()), headers=int(sums["n_header"].sum()),
                          follow_ms=stat(times[0]), decoder_ms=stat(times[1]), own_ms=stat(own), plain_ms=stat(times[2]),
                          host_ms=[round(float(x), 3) for x in (np.median(out), min(out), max(out))], launches=args.launches,
                          inner=args.inner, device=torch.cuda.get_device_name(0), csrc_sha16=bench.csrc_fingerprint())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--only", choices=("crowd", "hopping"), default=None)
    args = ap.parse_args()
    import torch
    import libbtbb_amd as bt
    assert torch.cuda.is_available(), "the measurement needs the GPU"
    torch.cuda.set_device(0)
    bt.init(2)
    if args.only != "hopping":
        import _crowd
        c = _crowd.crowd()
        measure("crowd", c.cap.words(), c.cap.n_words, c.cap.channels, c.kw["clkn0"], c.cap.clk_div, c.hits, args)
    if args.only != "crowd":
        import _acquire as aq
        planted = aq.three_piconets()
        cap, kw = aq.hopping_capture(43, planted, lambda p, clocks: bt.hop_channels(bt.hop_cfg(p.lap, p.uap, p.afh_map), clocks), clkn0=0x0ABCDEF1)
        measure("hopping", cap.words(), cap.n_words, cap.channels, kw["clkn0"], cap.clk_div, None, args)


if __name__ == "__main__":
    main()
