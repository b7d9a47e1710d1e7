"""Times of the clock acquisition chain on cuda:0: survey -> job builder -> batch reversal, against the host composition.

A 79-channel capture (channel = stream) of --slots slots with --piconets planted piconets, --packets packets each on the
channel the library's own hop selection gives for the master's clock; hits from btbbx_scan_ordered_device.  One JSON line:
  builder_ms   HIP events around btbbx_survey_clock_jobs_device alone (survey done before), 3 warm-ups, --launches launches:
               [median, min, max]
  chain_ms     HIP events around btbbx_survey_hits_device + builder + btbbx_hop_reversal_batch_device, nothing read back
  survey_ms    ... around btbbx_survey_hits_device alone, for scale
  host_ms      host clock around the composition the builder replaces, after the same survey: download records and hits,
               build the jobs in numpy (bt.clock_jobs), upload, btbbx_hop_reversal_batch_device, synchronise.  WHICH packets
               a job takes is handed to it for nothing (the builder's obs_hits): a real caller would also recompute
               header_present for every packet of a settled LAP, so this is a lower bound of the host path.
  unique       jobs that ended with count == 1 at the planted clock
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--piconets", type=int, default=300)
    ap.add_argument("--packets", type=int, default=30)
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=20)
    args = ap.parse_args()
    import torch
    import bench
    import libbtbb_amd as bt
    from libbtbb_amd import synth
    lib = bt.lib()
    torch.cuda.set_device(0)
    bt.init(2)
    rng = np.random.default_rng(17)
    n_sym = -(-(args.slots * 625 + 700) // 64) * 64
    sym = rng.integers(0, 2, (79, n_sym), dtype=np.uint8)
    used, truth, clkn0 = set(), {}, 0x0ABCDEF1
    types = (synth.TYPE_POLL, synth.TYPE_DM1, synth.TYPE_DH1, synth.TYPE_FHS)
    for _ in range(args.piconets):
        lap, uap, c0 = int(rng.integers(1, 1 << 24)), int(rng.integers(1, 256)), int(rng.integers(0, 1 << 27))
        chans = bt.hop_channels(bt.hop_cfg(lap, uap), ((c0 + np.arange(args.slots)) & ((1 << 27) - 1)).astype(np.uint32))
        free = [k for k in range(args.slots) if (int(chans[k]), k) not in used]
        slots = sorted(int(k) for k in rng.choice(free, size=args.packets, replace=False))
        for i, k in enumerate(slots):
            t = types[(i + (i >> 2)) % 4]
            body = rng.integers(0, 256, 9, dtype=np.uint8).tobytes() if t in (synth.TYPE_DM1, synth.TYPE_DH1) else b""
            s = synth.build_packet(lap, uap=uap, clk6=(c0 + k) & 63, ptype=t, lt_addr=1, body=body,
                                   fhs_bits=synth.fhs_payload(lap, uap, 1, 0, rng))
            sym[int(chans[k]), k * 625:k * 625 + len(s)] = s
            used.add((int(chans[k]), k))
        truth[lap] = (c0, slots)
    n_words = n_sym // 64
    words = torch.from_numpy(np.stack([synth.pack_bits(sym[s]) for s in range(79)]).view(np.int64)).cuda()
    search_bits = n_sym - 63
    cap = args.piconets * args.packets * 2 + 4096
    q = torch.cuda.current_stream().cuda_stream
    d_hits = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(8, dtype=torch.int32, device="cuda")       # hits, piconets, jobs, observations
    ob = lib.btbbx_scan_ordered_scratch_bytes(search_bits, 79, bt.LAP_ANY, cap)
    sb = lib.btbbx_survey_scratch_bytes(cap)
    order = torch.empty(ob // 8 + 2, dtype=torch.int64, device="cuda")
    scratch = torch.empty(sb // 8 + 2, dtype=torch.int64, device="cuda")
    d_recs = torch.zeros(cap * 8, dtype=torch.int64, device="cuda")
    job_cap = cap
    d_jobs = torch.zeros(job_cap * 13, dtype=torch.int64, device="cuda")
    d_jrec = torch.zeros(job_cap, dtype=torch.int32, device="cuda")
    d_off = torch.zeros(cap, dtype=torch.int32, device="cuda")
    d_ch = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    d_oh = torch.zeros(cap, dtype=torch.int32, device="cuda")
    entry = np.zeros(1, dtype=bt.PKTIN_DTYPE)
    entry["clkn"], entry["flags"] = clkn0, 1
    bt.check(lib.btbbx_scan_ordered_device(words.data_ptr(), n_words, n_words, 79, search_bits, bt.LAP_ANY, 2, d_hits.data_ptr(), cap,
                                           cnt.data_ptr(), order.data_ptr(), ob, q))
    torch.cuda.synchronize()
    n_hits = int(cnt[0])
    assert n_hits <= cap

    def survey():
        bt.check(lib.btbbx_survey_hits_device(words.data_ptr(), n_words, n_words, 79, d_hits.data_ptr(), cnt.data_ptr(), cap, None,
                                              bt._ptr(entry), 625, 0, bt.MAX_SYMBOLS, d_recs.data_ptr(), cap, cnt.data_ptr() + 4, None,
                                              scratch.data_ptr(), sb, q))

    def builder():
        bt.check(lib.btbbx_survey_clock_jobs_device(d_recs.data_ptr(), cnt.data_ptr() + 4, cap, scratch.data_ptr(), sb, cap, None, 79, 0, 1024,
                                                    d_jobs.data_ptr(), job_cap, cnt.data_ptr() + 8, d_jrec.data_ptr(), d_off.data_ptr(),
                                                    d_ch.data_ptr(), d_oh.data_ptr(), cap, cnt.data_ptr() + 12, q))
    survey()
    builder()
    torch.cuda.synchronize()
    n_recs, n_jobs, n_obs = (int(x) for x in cnt.cpu().numpy()[1:4])
    rev_cap = max(n_jobs, 1)                                      # (a caller sizes this from what it expects; here: exact)
    bs = lib.btbbx_hop_reversal_batch_scratch_bytes(rev_cap, 0)
    bscr = torch.empty(bs // 8 + 2, dtype=torch.int64, device="cuda")
    d_res = torch.zeros(rev_cap * 6, dtype=torch.int32, device="cuda")

    def reversal(jobs_ptr, off_ptr, ch_ptr):
        bt.check(lib.btbbx_hop_reversal_batch_device(jobs_ptr, cnt.data_ptr() + 8, rev_cap, off_ptr, ch_ptr, cap, d_res.data_ptr(), None, 0,
                                                     bscr.data_ptr(), bs, q))

    def chain():
        survey()
        builder()
        reversal(d_jobs.data_ptr(), d_off.data_ptr(), d_ch.data_ptr())

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.launches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return [round(float(x), 4) for x in (np.median(out), min(out), max(out))]
    survey_ms, builder_ms, chain_ms = timed(survey), timed(builder), timed(chain)
    res = d_res.cpu().numpy().view(bt.CLOCK_RESULT_DTYPE)[:n_jobs]
    recs = d_recs.cpu().numpy().view(bt.SURVEY_DTYPE)[:n_recs]
    jrec = d_jrec.cpu().numpy().view(np.uint32)[:n_jobs]
    unique = 0
    for j in range(n_jobs):
        r = recs[jrec[j]]
        if int(r["lap"]) in truth:
            c0 = truth[int(r["lap"])][0]
            k = (int(r["first_pkt_time"]) - clkn0) & 0xFFFFFFFF
            unique += int(res["count"][j] == 1 and res["cand0"][j] == (c0 + k) % (1 << 27))
    # the host composition
    dev_jobs = d_jobs.cpu().numpy().view(bt.CLOCK_JOB_DTYPE)[:n_jobs]
    picked = d_oh.cpu().numpy().view(np.uint32)[:n_obs]
    runs = [picked[int(j["obs_first"]):int(j["obs_first"]) + int(j["n_obs"])] for j in dev_jobs]

    def host():
        h_recs = d_recs[:n_recs * 8].cpu().numpy().view(bt.SURVEY_DTYPE)
        h_hits = d_hits[:n_hits * 2].cpu().numpy().view(bt.HIT_DTYPE)
        settled = np.nonzero(h_recs["settled_by"])[0]
        cfgs, clk6, obs = [], [], []
        for g, run in zip(settled, runs):
            r = h_recs[g]
            clk = (clkn0 + h_hits["offset"][run] // 625).astype(np.uint32)
            obs.append(((clk - r["first_pkt_time"]).view(np.int32), h_hits["stream"][run].astype(np.uint8)))
            cfgs.append(bt.hop_cfg(int(r["lap"]), int(r["uap"])))
            clk6.append((int(r["clk_offset"]) + int(r["first_pkt_time"])) & 63)
        jobs, offsets, channels = bt.clock_jobs(cfgs, clk6, obs)
        pad = lambda a, n: np.frombuffer(np.ascontiguousarray(a).tobytes() + bytes(n), dtype=np.uint8).copy()
        u_jobs, u_off = torch.from_numpy(pad(jobs, 16)).cuda(), torch.from_numpy(pad(offsets, 4 * cap - offsets.nbytes + 16)).cuda()
        u_ch = torch.from_numpy(pad(channels, cap - channels.nbytes + 16)).cuda()
        reversal(u_jobs.data_ptr(), u_off.data_ptr(), u_ch.data_ptr())
        torch.cuda.synchronize()
        return jobs
    assert host().tobytes() == dev_jobs.tobytes()
    assert d_res.cpu().numpy().view(bt.CLOCK_RESULT_DTYPE)[:n_jobs].tobytes() == res.tobytes()
    out = []
    for _ in range(5):
        t0 = time.perf_counter()
        host()
        out.append((time.perf_counter() - t0) * 1e3)
    host_ms = [round(float(x), 3) for x in (np.median(out), min(out), max(out))]
    print(json.dumps(dict(piconets=args.piconets, packets=args.packets, slots=args.slots, hits=n_hits, records=n_recs, jobs=n_jobs,
                          observations=n_obs, unique=unique, survey_ms=survey_ms, builder_ms=builder_ms, chain_ms=chain_ms, host_ms=host_ms,
                          launches=args.launches, device=torch.cuda.get_device_name(0), csrc_sha16=bench.csrc_fingerprint())))


if __name__ == "__main__":
    main()
