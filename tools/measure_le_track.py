#!/usr/bin/env python3
"""LE connection tracking measurement: btbbx_le_track_device over two grouped candidate lists built on the host with numpy, both of
about one million candidates (two packets per connection event, every data channel used, anchors jittered by +-20 bits):

* many: 2 000 connections of 250 events
* one:  a single connection of 500 000 events -- the shape the kernels' grids must keep from becoming one workgroup's serial job

HIP events, 3 warm-ups and 20 launches per figure.  Prints one JSON line:

* track_ms[list]: btbbx_le_track_device (BTBBX_LE_TRACK_REMAP, unit 1250, ifs 200, jitter 50)
* yardstick_ms[list]: btbbx_le_discover_group_device over the same candidates, re-measured in this run (less the copy that puts
  the list back in front of every launch)
* recovered[list]: connections that came out with their planted interval, increment and first unmapped channel, HOPPING set and
  no event off the hop
* launches: kernel launches of one tracking call at this conn_cap
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
from measure_le import time_ms  # noqa: E402

DATA_MHZ = [m for m in range(2404, 2480, 2) if m != 2426]
UNIT = 1250


def build_list(n_conns, n_events, seed):
    """(cands in grouped order with conn = the connection index, conns, planted (interval, increment, first unmapped channel))."""
    rng = np.random.default_rng(seed)
    per = 2 * n_events
    cands = np.zeros(n_conns * per, bt.LE_CAND_DTYPE)
    conns = np.zeros(n_conns, bt.LE_CONN_DTYPE)
    planted = np.zeros((n_conns, 3), np.int64)
    n = np.arange(n_events, dtype=np.int64)
    for g in range(n_conns):
        iv, h, u0 = int(rng.integers(6, 40)), int(rng.integers(5, 17)), int(rng.integers(0, 37))
        ch = (u0 + h * n) % 37                                           # every channel used: the unmapped channel is the channel
        at = 4000 + 131 * g + n * iv * UNIT + rng.integers(-20, 21, n_events)
        off = np.stack([at, at + 80 + 150], 1).reshape(-1)
        stream = np.repeat(ch, 2)
        order = np.lexsort((off, stream))                                # the grouping's order within a connection: (stream, offset)
        part = cands[g * per:(g + 1) * per]
        part["offset"], part["stream"] = off[order], stream[order]
        part["access_address"], part["crc_init"] = 0x10000000 + 7919 * g, (104729 * g + 1) & 0xFFFFFF
        part["header0"], part["length"], part["conn"] = 1, 0, g
        conns[g] = (0x10000000 + 7919 * g, (104729 * g + 1) & 0xFFFFFF, per, per, int(np.bitwise_or.reduce(1 << np.unique(ch))), g * per)
        planted[g] = (iv, h, u0)
    return cands, conns, planted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conns", type=int, default=2000)
    ap.add_argument("--events", type=int, default=250)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import bench
    torch.cuda.set_device(0)
    bt.init(2)
    lib = bt.lib()
    phys = torch.tensor(DATA_MHZ, dtype=torch.int16, device="cuda")
    track_ms, yard_ms, recovered, sizes = {}, {}, {}, {}
    conn_cap = args.conns
    for name, n_conns, n_events in (("many", args.conns, args.events), ("one", 1, args.conns * args.events)):
        cands, conns, planted = build_list(n_conns, n_events, args.seed)
        n = len(cands)
        sizes[name] = n
        d_cands = torch.from_numpy(cands.view(np.int64)).cuda()
        d_conns = torch.zeros(4 * conn_cap, dtype=torch.int64, device="cuda")
        d_conns[:4 * n_conns] = torch.from_numpy(conns.view(np.int64)).cuda()
        cnt = torch.tensor([n, n_conns, 0, 0], dtype=torch.int32, device="cuda")
        d_tracks = torch.zeros(6 * conn_cap, dtype=torch.int64, device="cuda")
        d_pkts = torch.zeros(2 * n, dtype=torch.int64, device="cuda")
        scratch_bytes = lib.btbbx_le_track_scratch_bytes(n, conn_cap)
        scratch = torch.zeros(scratch_bytes // 8 + 2, dtype=torch.int64, device="cuda")

        def track():
            bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), cnt.data_ptr(), n, d_conns.data_ptr(), cnt.data_ptr() + 4, conn_cap,
                                               phys.data_ptr(), 37, UNIT, 200, 50, bt.LE_TRACK_REMAP, d_tracks.data_ptr(), d_pkts.data_ptr(),
                                               scratch.data_ptr(), scratch_bytes, None), "btbbx_le_track_device")

        track_ms[name] = round(time_ms(track, args.warmup, args.steps), 4)
        t = d_tracks.cpu().numpy().view(bt.LE_TRACK_DTYPE)[:n_conns]
        good = ((t["interval"] == planted[:, 0]) & (t["hop_increment"] == planted[:, 1]) & (t["first_unmapped"] == planted[:, 2]) &
                (t["flags"] == 3) & (t["n_off_hop"] == 0) & (t["n_events"] == n_events))
        recovered[name] = int(good.sum())
        # the yardstick: the discovery's grouping of the same candidates, as the scan would leave them (conn = the channel index)
        listed = cands.copy()
        listed["conn"] = listed["stream"]
        d_listed = torch.from_numpy(listed.view(np.int64)).cuda()
        d_work = d_listed.clone()
        gscratch_bytes = lib.btbbx_le_discover_scratch_bytes(n)
        gscratch = torch.zeros(gscratch_bytes // 8 + 2, dtype=torch.int64, device="cuda")
        gcnt = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device="cuda")

        def group():
            d_work.copy_(d_listed)
            bt.check(lib.btbbx_le_discover_group_device(d_work.data_ptr(), gcnt.data_ptr(), n, 2, d_conns.data_ptr(), conn_cap,
                                                        gcnt.data_ptr() + 4, gscratch.data_ptr(), gscratch_bytes, None),
                     "btbbx_le_discover_group_device")

        both = time_ms(group, args.warmup, args.steps)
        yard_ms[name] = round(both - time_ms(lambda: d_work.copy_(d_listed), args.warmup, args.steps), 4)
        assert int(gcnt[1].item()) == n_conns
        del d_cands, d_pkts, scratch, d_listed, d_work, gscratch
    conn_passes = 1
    while conn_passes < 4 and conn_cap >> (8 * conn_passes):
        conn_passes += 1
    line = dict(metric="le_track", candidates=sizes, connections=dict(many=args.conns, one=1), conn_cap=conn_cap, track_ms=track_ms,
                yardstick_ms=yard_ms, recovered=recovered, one_over_many=round(track_ms["one"] / track_ms["many"], 3),
                launches=13 + 3 * (8 + conn_passes), steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0),
                csrc_sha16=bench.csrc_fingerprint())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
