#!/usr/bin/env python3
"""LE data extraction measurement: btbbx_le_data_device beside btbbx_le_track_device over the same list in the same run,
alternating, and its gather beside a device-to-device copy of the same number of octets.  The list is the other LE tools' -- 2 000
connections of 250 events, two packets per connection event, anchors jittered by +-20 bits, algorithm #1 over the full map -- here
with data PDUs of mixed lengths: the central sends messages of three fragments (27, 27 and one of 5, 27, 100 or 251 octets), the
peripheral a one-fragment message of 1 to 27 octets in every second event and an empty PDU otherwise; every packet is new.  The
streams hold random bits: the stage reads whatever payload stands there.

The gather cannot be launched alone through the public entries, so its time is a difference: the stage with room for every octet
less the stage with byte_cap 0, which stores no message and leaves the gather's lanes nothing to move (it still starts and reads each
slot's state).  HIP events, 3 warm-ups and 20 launches per figure, two rounds.  Prints one JSON line:

* data_ms, data_nobytes_ms, track_ms, copy_ms: both rounds' figures; gather_ms: the difference of the means; data_over_track and
  gather_over_copy: the ratios of the means
* messages, octets, candidates; complete: messages whose length the L2CAP header (random here) happens to match
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
from measure_le_track import DATA_MHZ, UNIT  # noqa: E402

N_WORDS = 195000
LAST = (5, 27, 100, 251)


def build(n_conns, n_events, seed):
    rng = np.random.default_rng(seed)
    per = 2 * n_events
    cands = np.zeros(n_conns * per, bt.LE_CAND_DTYPE)
    conns = np.zeros(n_conns, bt.LE_CONN_DTYPE)
    words = rng.integers(0, 1 << 63, (37, N_WORDS), dtype=np.uint64)
    c = np.arange(n_events, dtype=np.int64)
    octets = 0
    for g in range(n_conns):
        h = int(rng.integers(5, 17))
        aa, ci = 0x10000000 + 7919 * g, (104729 * g + 1) & 0xFFFFFF
        ch = (h * ((c + 1) % 37)) % 37
        at = 3000 + 131 * g + c * 6 * UNIT + rng.integers(-20, 21, n_events)
        third = c % 3
        len_c = np.where(third < 2, 27, np.asarray(LAST)[rng.integers(0, 4, n_events)])
        llid_c = np.where(third == 0, 2, 1)
        len_p = np.where(c % 2 == 0, rng.integers(1, 28, n_events), 0)
        llid_p = np.where(c % 2 == 0, 2, 1)
        sn = c & 1                                                           # one packet per role and event, every one new
        off = np.stack([at, at + 80 + 8 * len_c + 150], 1).reshape(-1)
        stream = np.repeat(ch, 2)
        h0 = np.stack([llid_c | sn << 3, llid_p | sn << 3], 1).reshape(-1)
        ln = np.stack([len_c, len_p], 1).reshape(-1)
        octets += int(ln.sum())
        order = np.lexsort((off, stream))
        part = cands[g * per:(g + 1) * per]
        part["offset"], part["stream"], part["header0"], part["length"] = off[order], stream[order], h0[order], ln[order]
        part["access_address"], part["crc_init"], part["conn"] = aa, ci, g
        conns[g] = (aa, ci, per, int((ln == 0).sum()), int(np.bitwise_or.reduce(1 << np.unique(ch))), g * per)
    return cands, conns, words, octets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conns", type=int, default=2000)
    ap.add_argument("--events", type=int, default=250)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="for a counter run: the tracking once, the stage `steps` times with room for every octet")
    args = ap.parse_args()
    import bench
    torch.cuda.set_device(0)
    bt.init(2)
    lib = bt.lib()
    phys = torch.tensor(DATA_MHZ, dtype=torch.int16, device="cuda")
    cands, conns, words, octets = build(args.conns, args.events, args.seed)
    n, k = len(cands), len(conns)
    d_cands, d_words = torch.from_numpy(cands.view(np.int64)).cuda(), torch.from_numpy(words.view(np.int64)).cuda()
    d_conns = torch.from_numpy(conns.view(np.int64)).cuda()
    cnt = torch.tensor([n, k, 0, 0, 0, 0], dtype=torch.int32, device="cuda")
    d_tracks, d_pkts = torch.zeros(6 * k, dtype=torch.int64, device="cuda"), torch.zeros(2 * n, dtype=torch.int64, device="cuda")
    d_data, d_dpkts = torch.zeros(6 * k, dtype=torch.int64, device="cuda"), torch.zeros(3 * n, dtype=torch.int32, device="cuda")
    d_msgs = torch.zeros(4 * n, dtype=torch.int64, device="cuda")
    d_bytes, d_copy = torch.zeros(octets + 64, dtype=torch.uint8, device="cuda"), torch.zeros(octets + 64, dtype=torch.uint8, device="cuda")
    tscratch_bytes, dscratch_bytes = lib.btbbx_le_track_scratch_bytes(n, k), lib.btbbx_le_data_scratch_bytes(n, k)
    tscratch = torch.zeros(tscratch_bytes // 8 + 2, dtype=torch.int64, device="cuda")
    dscratch = torch.zeros(dscratch_bytes // 8 + 2, dtype=torch.int64, device="cuda")
    p = cnt.data_ptr()

    def track():
        bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), p, n, d_conns.data_ptr(), p + 4, k, phys.data_ptr(), 37, UNIT, 200, 50,
                                           bt.LE_TRACK_REMAP, d_tracks.data_ptr(), d_pkts.data_ptr(), tscratch.data_ptr(), tscratch_bytes, None),
                 "btbbx_le_track_device")

    def data(byte_cap):
        bt.check(lib.btbbx_le_data_device(d_words.data_ptr(), N_WORDS, N_WORDS, 37, phys.data_ptr(), d_cands.data_ptr(), p, n, d_conns.data_ptr(),
                                          p + 4, k, d_tracks.data_ptr(), d_pkts.data_ptr(), d_data.data_ptr(), d_dpkts.data_ptr(),
                                          d_msgs.data_ptr(), n, p + 8, d_bytes.data_ptr(), byte_cap, p + 16, dscratch.data_ptr(), dscratch_bytes,
                                          None), "btbbx_le_data_device")

    def copy():
        d_copy[:octets].copy_(d_bytes[:octets])

    track()
    data(octets)
    torch.cuda.synchronize()
    counts = cnt.cpu().numpy()
    n_msgs, n_bytes = int(counts[2:3].view(np.uint32)[0]), int(counts[4:6].view(np.uint64)[0])
    rec = d_data.cpu().numpy().view(bt.LE_DATA_DTYPE)
    assert n_bytes == octets and int(rec["n_unknown"].sum()) == 0 and int(rec["n_retransmit"].sum()) == 0, (n_bytes, octets)
    if args.once:
        for _ in range(args.steps):
            data(octets)
        torch.cuda.synchronize()
        print(json.dumps(dict(metric="le_data_once", octets=n_bytes, messages=n_msgs, launches_of_the_stage=args.steps + 1)))
        return
    data_ms, nobytes_ms, track_ms, copy_ms = [], [], [], []
    for _ in range(2):
        data_ms.append(round(time_ms(lambda: data(octets), args.warmup, args.steps), 4))
        nobytes_ms.append(round(time_ms(lambda: data(0), args.warmup, args.steps), 4))
        track_ms.append(round(time_ms(track, args.warmup, args.steps), 4))
        copy_ms.append(round(time_ms(copy, args.warmup, args.steps), 4))
    gather = (sum(data_ms) - sum(nobytes_ms)) / 2
    line = dict(metric="le_data", candidates=n, connections=k, messages=n_msgs, octets=n_bytes, complete=int(rec["n_complete"].sum()),
                data_ms=data_ms, data_nobytes_ms=nobytes_ms, track_ms=track_ms, copy_ms=copy_ms, gather_ms=round(gather, 4),
                data_over_track=round(sum(data_ms) / sum(track_ms), 2), gather_over_copy=round(gather / (sum(copy_ms) / 2), 2), launches=18,
                steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0), csrc_sha16=bench.csrc_fingerprint())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
