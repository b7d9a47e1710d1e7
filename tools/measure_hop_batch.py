"""Times of the batch CLK1-27 reversal (btbbx_hop_reversal_batch_device) on cuda:0, against the single-piconet path.

--jobs piconets (basic hopping, or an AFH map of --used channels), --obs observed hops each, drawn from the library's own hop
selection (btbbx_hop_channels_device) at random clocks.  One JSON line:
  batch_ms          HIP events around one btbbx_hop_reversal_batch_device call over all jobs, 3 warm-ups, --launches launches:
                    [median, min, max]; with --cand-cap > 0 the candidate pass is part of it
  loop_ms           the same piconets through btbbx_hop_reversal_open + _winnow + _close, one after the other, host clock around
                    the whole loop (every call of it ends in a stream synchronise), one warm-up loop, --loops loops:
                    [median, min, max]
  unique            jobs that ended with count == 1 and the clock the observations were drawn from
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
    ap.add_argument("--jobs", type=int, default=1024)
    ap.add_argument("--obs", type=int, default=30)
    ap.add_argument("--used", type=int, default=0, help="AFH map with this many channels (0: basic hopping)")
    ap.add_argument("--cand-cap", type=int, default=0)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--loops", type=int, default=3)
    args = ap.parse_args()
    import torch
    import bench
    import libbtbb_amd as bt
    lib = bt.lib()
    torch.cuda.set_device(0)
    bt.init(2)
    rng = np.random.default_rng(11)
    cfgs, c0s, obs = [], [], []
    for _ in range(args.jobs):
        amap = None
        if args.used:
            amap = np.zeros(10, np.uint8)
            for c in rng.choice(79, size=args.used, replace=False):
                amap[c // 8] |= 1 << (c % 8)
        cfg = bt.hop_cfg(int(rng.integers(0, 1 << 24)), int(rng.integers(0, 256)), amap)
        c0 = int(rng.integers(0, (1 << 27) - 400 * args.obs))
        off = np.concatenate([[0], np.cumsum(rng.integers(1, 400, args.obs - 1))]).astype(np.int32)
        cfgs.append(cfg)
        c0s.append(c0)
        obs.append((off, bt.hop_channels(cfg, (c0 + off).astype(np.uint32))))
    jobs, offsets, channels = bt.clock_jobs(cfgs, [c & 63 for c in c0s], obs)

    def dev(a):
        return torch.from_numpy(np.frombuffer(np.ascontiguousarray(a).tobytes() + bytes(16), dtype=np.uint8).copy()).cuda()
    d_jobs, d_off, d_ch = dev(jobs), dev(offsets), dev(channels)
    d_res = torch.zeros(args.jobs * 6, dtype=torch.int32, device="cuda")
    d_cand = torch.zeros(max(args.jobs * args.cand_cap, 4), dtype=torch.int32, device="cuda")
    sb = lib.btbbx_hop_reversal_batch_scratch_bytes(args.jobs, args.cand_cap)
    scratch = torch.empty(sb // 8 + 2, dtype=torch.int64, device="cuda")
    q = torch.cuda.current_stream().cuda_stream

    def batch():
        bt.check(lib.btbbx_hop_reversal_batch_device(d_jobs.data_ptr(), None, args.jobs, d_off.data_ptr(), d_ch.data_ptr(), len(offsets),
                                                     d_res.data_ptr(), d_cand.data_ptr() if args.cand_cap else None, args.cand_cap,
                                                     scratch.data_ptr(), sb, q), "btbbx_hop_reversal_batch_device")

    for _ in range(3):
        batch()
    torch.cuda.synchronize()
    out = []
    for _ in range(args.launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        batch()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    batch_ms = [round(float(x), 4) for x in (np.median(out), min(out), max(out))]
    res = d_res.cpu().numpy().view(bt.CLOCK_RESULT_DTYPE)

    def loop():
        got = []
        for cfg, c0, (off, ch) in zip(cfgs, c0s, obs):
            rev = bt.HopReversal(cfg, c0 & 63, int(ch[0]))
            got.append(rev.winnow(off, ch))
            rev.close()
        return got
    single = loop()
    out = []
    for _ in range(args.loops):
        t0 = time.perf_counter()
        loop()
        out.append((time.perf_counter() - t0) * 1e3)
    loop_ms = [round(float(x), 3) for x in (np.median(out), min(out), max(out))]
    assert [(int(r["stop"]), int(r["count"]), int(r["cand0"])) for r in res] == [tuple(s) for s in single]
    unique = int(sum(int(r["count"]) == 1 and int(r["cand0"]) == c for r, c in zip(res, c0s)))
    print(json.dumps(dict(jobs=args.jobs, obs=args.obs, used=args.used or 79, cand_cap=args.cand_cap, batch_ms=batch_ms, loop_ms=loop_ms,
                          launches=args.launches, loops=args.loops, unique=unique, scratch_mib=round(sb / 2**20, 2),
                          csrc_sha16=bench.csrc_fingerprint())))


if __name__ == "__main__":
    main()
