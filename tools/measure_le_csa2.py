#!/usr/bin/env python3
"""LE channel selection #2 measurement: btbbx_le_csa2_device behind btbbx_le_track_device on the workload of
tools/measure_le_track.py -- two grouped candidate lists of about one million candidates (two packets per connection event, every
data channel used, anchors jittered by +-20 bits), hopping by algorithm #1 -- and on a third list that hops by algorithm #2:

* many: 2 000 connections of 250 events (#1)
* one:  a single connection of 500 000 events (#1) -- 64 work items, each with 977 tiles of events
* csa2: 2 000 connections of 250 events (#2), random access addresses and first counters

HIP events, 3 warm-ups and 20 launches per figure.  Prints one JSON line:

* csa2_ms[list]: btbbx_le_csa2_device (BTBBX_LE_CSA2_REMAP) on what the tracking left
* track_ms[list]: btbbx_le_track_device over the same list, measured in this run: the yardstick (the stage has no predecessor)
* evaluated / unique / preferred[list]: connections with these flags; on the csa2 list `recovered` counts those that came out
  PREFERRED with the planted counter and every event on the prediction
* launches: kernel launches of one call; csrc_sha16: the source fingerprint of bench.py

The split over the kernels comes from a separate run under the profiler, which slows the host:
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/measure_le_csa2.py --profile-run 5 --only many`
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

import _le_csa2 as lc  # noqa: E402
import libbtbb_amd as bt  # noqa: E402
from measure_le import time_ms  # noqa: E402
from measure_le_track import DATA_MHZ, UNIT, build_list  # noqa: E402


def build_csa2_list(n_conns, n_events, seed):
    """build_list's layout with the channels of algorithm #2: (cands, conns, planted first counters)."""
    rng = np.random.default_rng(seed)
    cands, conns, _ = build_list(n_conns, n_events, seed)
    per = 2 * n_events
    planted = rng.integers(0, 1 << 16, n_conns)
    n = np.arange(n_events, dtype=np.int64)
    for g in range(n_conns):
        aa = 0x10000000 + 7919 * g
        part = cands[g * per:(g + 1) * per]
        at = np.sort(part["offset"].astype(np.int64))[0::2]              # the anchors, in event order
        ch = lc.expected_table(aa, lc.FULL_MAP, lc.REMAP)[(int(planted[g]) + n) & 0xFFFF].astype(np.int64)
        off = np.stack([at, at + 80 + 150], 1).reshape(-1)
        stream = np.repeat(ch, 2)
        order = np.lexsort((off, stream))
        part["offset"], part["stream"] = off[order], stream[order]
        conns[g]["channel_mask"] = int(np.bitwise_or.reduce(1 << np.unique(ch)))
    return cands, conns, planted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conns", type=int, default=2000)
    ap.add_argument("--events", type=int, default=250)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("many", "one", "csa2"), default=None)
    ap.add_argument("--profile-run", type=int, default=0, help="no timing: this many calls of both stages per list, for the profiler")
    args = ap.parse_args()
    import bench
    torch.cuda.set_device(0)
    bt.init(2)
    lib = bt.lib()
    phys = torch.tensor(DATA_MHZ, dtype=torch.int16, device="cuda")
    track_ms, csa2_ms, sizes, counts, recovered = {}, {}, {}, {}, {}
    conn_cap = args.conns
    for name, n_conns, n_events in (("many", args.conns, args.events), ("one", 1, args.conns * args.events), ("csa2", args.conns, args.events)):
        if args.only and name != args.only:
            continue
        if name == "csa2":
            cands, conns, planted = build_csa2_list(n_conns, n_events, args.seed)
        else:
            cands, conns, planted = build_list(n_conns, n_events, args.seed)
        n = len(cands)
        sizes[name] = n
        d_cands = torch.from_numpy(cands.view(np.int64)).cuda()
        d_conns = torch.zeros(4 * conn_cap, dtype=torch.int64, device="cuda")
        d_conns[:4 * n_conns] = torch.from_numpy(conns.view(np.int64)).cuda()
        cnt = torch.tensor([n, n_conns, 0, 0], dtype=torch.int32, device="cuda")
        d_tracks = torch.zeros(6 * conn_cap, dtype=torch.int64, device="cuda")
        d_pkts = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
        d_sel = torch.zeros(3 * conn_cap, dtype=torch.int64, device="cuda")
        d_sel_pkts = torch.zeros(n, dtype=torch.int64, device="cuda")
        tscratch_bytes, scratch_bytes = lib.btbbx_le_track_scratch_bytes(n, conn_cap), lib.btbbx_le_csa2_scratch_bytes(n, conn_cap)
        tscratch = torch.zeros(tscratch_bytes // 8 + 2, dtype=torch.int64, device="cuda")
        scratch = torch.zeros(scratch_bytes // 8 + 2, dtype=torch.int64, device="cuda")

        def track():
            bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), cnt.data_ptr(), n, d_conns.data_ptr(), cnt.data_ptr() + 4, conn_cap,
                                               phys.data_ptr(), 37, UNIT, 200, 50, bt.LE_TRACK_REMAP, d_tracks.data_ptr(), d_pkts.data_ptr(),
                                               tscratch.data_ptr(), tscratch_bytes, None), "btbbx_le_track_device")

        def select():
            bt.check(lib.btbbx_le_csa2_device(d_cands.data_ptr(), cnt.data_ptr(), n, d_conns.data_ptr(), cnt.data_ptr() + 4, conn_cap,
                                              d_tracks.data_ptr(), d_pkts.data_ptr(), bt.LE_CSA2_REMAP, d_sel.data_ptr(), d_sel_pkts.data_ptr(),
                                              scratch.data_ptr(), scratch_bytes, None), "btbbx_le_csa2_device")

        if args.profile_run:
            for _ in range(args.profile_run):
                track()
                select()
            torch.cuda.synchronize()
            continue
        track_ms[name] = round(time_ms(track, args.warmup, args.steps), 4)
        csa2_ms[name] = round(time_ms(select, args.warmup, args.steps), 4)
        s = d_sel.cpu().numpy().view(bt.LE_CSA2_DTYPE)[:n_conns]
        counts[name] = dict(evaluated=int((s["flags"] & 1 != 0).sum()), unique=int((s["flags"] & 2 != 0).sum()),
                            preferred=int((s["flags"] & 4 != 0).sum()))
        if name == "csa2":
            recovered[name] = int(((s["flags"] == 7) & (s["counter0"] == planted) & (s["n_on"] == n_events) & (s["n_off"] == 0)).sum())
        del d_cands, d_pkts, d_sel_pkts, scratch, tscratch
    if args.profile_run:
        return
    line = dict(metric="le_csa2", candidates=sizes, conn_cap=conn_cap, csa2_ms=csa2_ms, track_ms=track_ms,
                csa2_over_track={k: round(csa2_ms[k] / track_ms[k], 2) for k in csa2_ms}, flags=counts, recovered=recovered, launches=5,
                steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0), csrc_sha16=bench.csrc_fingerprint())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
