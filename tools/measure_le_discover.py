#!/usr/bin/env python3
"""LE connection discovery measurement, on the capture of tools/measure_le.py (4 GiB, 40 streams, built on the GPU from a seed:
iid noise, advertising packets on channels 37 / 38 / 39 and one connection's packets on the data channels, one planted packet per
4096 bits).  HIP events, 3 warm-ups and 20 launches per figure.  Prints one JSON line:

* yardstick_ms: btbbx_le_scan_device at limit 0 with the connection's AA (known beforehand), re-measured in this run
* scan_ms[max_len] / candidates[max_len]: btbbx_le_discover_scan_device for max_len 0, 27 and 255, with the candidates it counts
* group_ms / connections: btbbx_le_discover_group_device over the candidate list of max_len 27 (min_count 2)
* found / planted_packets / channels: whether the planted connection came out with its AA and CRCInit, with how many packets and
  on how many data channels (the capture's packets have random header octets: 3 in 32 are plausible data PDUs)
* csrc_sha16: the source fingerprint of bench.py
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import libbtbb_amd as bt  # noqa: E402
from measure_le import CONN_AA, build_capture, mhz_of, time_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--streams", type=int, default=40)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import bench
    torch.cuda.set_device(0)
    bt.init(2)
    lib = bt.lib()
    n_streams = args.streams
    n_words = int(args.gib * (1 << 30) / 8 / n_streams) // 512 * 512
    conn_crc = int(np.random.default_rng(args.seed).integers(0, 1 << 24))
    words = build_capture(args.seed, n_streams, n_words, conn_crc)
    phys = torch.tensor([mhz_of(s) for s in range(n_streams)], dtype=torch.int16, device="cuda")
    search_bits = n_words * 64 - 39
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")

    # the yardstick: the known-AA scan at limit 0
    hit_cap = n_words * n_streams // 64 * 2 + (1 << 16)
    hits = torch.zeros(2 * hit_cap, dtype=torch.int64, device="cuda")

    def known():
        cnt.zero_()
        bt.check(lib.btbbx_le_scan_device(words.data_ptr(), n_words, n_words, n_streams, search_bits, CONN_AA, 0, hits.data_ptr(), hit_cap,
                                          cnt.data_ptr(), None), "btbbx_le_scan_device")

    yardstick_ms = round(time_ms(known, args.warmup, args.steps), 4)
    yardstick_hits = int(cnt[0].item())
    del hits

    def discover(max_len, cands, cap):
        cnt.zero_()
        bt.check(lib.btbbx_le_discover_scan_device(words.data_ptr(), n_words, n_words, n_streams, search_bits, phys.data_ptr(), max_len,
                                                   cands.data_ptr() if cands is not None else None, cap, cnt.data_ptr(), None),
                 "btbbx_le_discover_scan_device")

    scan_ms, counts = {}, {}
    cands = None
    for max_len in (0, 255, 27):                                     # (27 last: its list goes to the grouping)
        discover(max_len, None, 0)                                   # a counting launch sizes the buffer
        torch.cuda.synchronize()
        counts[max_len] = int(cnt[0].item()) & 0xFFFFFFFF
        cap = counts[max_len] + 1024
        del cands
        cands = torch.zeros(3 * cap, dtype=torch.int64, device="cuda")
        scan_ms[max_len] = round(time_ms(lambda: discover(max_len, cands, cap), args.warmup, args.steps), 4)
    scratch_bytes = lib.btbbx_le_discover_scratch_bytes(cap)
    scratch = torch.zeros(scratch_bytes // 8 + 2, dtype=torch.int64, device="cuda")
    conn_cap = 1 << 16
    conns = torch.zeros(4 * conn_cap, dtype=torch.int64, device="cuda")
    listed = cands.clone()                                           # (grouping sorts in place: every launch starts from the scan's order)

    def group():
        cands.copy_(listed)
        bt.check(lib.btbbx_le_discover_group_device(cands.data_ptr(), cnt.data_ptr(), cap, 2, conns.data_ptr(), conn_cap, cnt.data_ptr() + 4,
                                                    scratch.data_ptr(), scratch_bytes, None), "btbbx_le_discover_group_device")

    both_ms = time_ms(group, args.warmup, args.steps)
    copy_ms = time_ms(lambda: cands.copy_(listed), args.warmup, args.steps)
    n_conns = int(cnt[1].item())
    recs = conns.cpu().numpy().view(bt.LE_CONN_DTYPE)[:min(n_conns, conn_cap)]
    mine = recs[(recs["access_address"] == CONN_AA) & (recs["crc_init"] == conn_crc)]
    found = bool(len(mine) == 1)
    line = dict(metric="le_discover", gib=round(n_words * 8 * n_streams / (1 << 30), 3), streams=n_streams, seed=args.seed,
                yardstick_ms=yardstick_ms, yardstick_hits=yardstick_hits, scan_ms=scan_ms, candidates=counts,
                group_ms=round(both_ms - copy_ms, 4), connections=n_conns, found=found,
                planted_packets=int(mine[0]["n_packets"]) if len(mine) else 0,
                channels=bin(int(mine[0]["channel_mask"])).count("1") if len(mine) else 0, device=torch.cuda.get_device_name(0),
                csrc_sha16=bench.csrc_fingerprint())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
