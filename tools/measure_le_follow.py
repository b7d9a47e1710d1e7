#!/usr/bin/env python3
"""LE following measurement: btbbx_le_seed_device and btbbx_le_epoch_device behind btbbx_le_track_device, on two grouped
candidate lists of about one million candidates in the layout of tools/measure_le_track.py (two packets per connection event,
anchors jittered by +-20 bits), every connection seeded by a CONNECT_IND record and hopping by algorithm #1 through four channel
map updates, each announced ten events ahead by an LL_CHANNEL_MAP_IND whose payload stands, whitened, in the streams:

* many: 2 000 connections of 250 events, updates in force from events 50, 100, 150 and 200
* one:  a single connection of 500 000 events, updates in force from events 200, 400, 600 and 800

HIP events, 3 warm-ups and 20 launches per figure.  Prints one JSON line:

* seed_ms / follow_ms[list]: the two stages on what the tracking left
* track_ms[list]: btbbx_le_track_device over the same list, measured in this run: the yardstick
* followed[list]: connections that came out SEEDED with four map updates and every event on the prediction (two update PDUs of
  different connections can fall on the same stream bits of the many list; such a connection is not among them)
* track_off_hop[list]: events the tracking alone leaves off its hop
* launches: kernel launches of one follow call; csrc_sha16: the source fingerprint of bench.py
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

import _le  # noqa: E402
import _le_follow as lf  # noqa: E402
import libbtbb_amd as bt  # noqa: E402
from measure_le import time_ms  # noqa: E402
from measure_le_track import DATA_MHZ, UNIT  # noqa: E402

N_WORDS = 195000                                       # 12.5 Mbit per stream: 250 events of interval 39 and the request in front


def remap1(unmapped, chmap):
    """Algorithm #1's mapping of an array of unmapped channels through one map."""
    used = np.array([c for c in range(37) if (chmap >> c) & 1], np.int64)
    in_map = ((chmap >> unmapped) & 1).astype(bool)
    return np.where(in_map, unmapped, used[unmapped % len(used)])


def build(n_conns, n_events, instants, seed, max_interval=39):
    """(cands, conns, adv records, words): the grouped list, one CONNECT_IND record per connection, the streams with the update
    PDUs' payloads."""
    rng = np.random.default_rng(seed)
    per = 2 * n_events
    cands = np.zeros(n_conns * per, bt.LE_CAND_DTYPE)
    conns = np.zeros(n_conns, bt.LE_CONN_DTYPE)
    words = rng.integers(0, 1 << 63, (37, N_WORDS), dtype=np.uint64)
    white = [_le.bits_value(_le.whitening_bits(ch, 80)[16:]) for ch in range(37)]
    adv = []
    c = np.arange(n_events, dtype=np.int64)
    for g in range(n_conns):
        iv, h = min(int(rng.integers(6, 40)), max_interval), int(rng.integers(5, 17))
        aa, ci = 0x10000000 + 7919 * g, (104729 * g + 1) & 0xFFFFFF
        req = 600 + 131 * g
        t0 = req + 352 + 2 * UNIT
        first = int(rng.integers(10, 38))
        maps = [(0, (1 << 37) - 1)] + [(i, lf.lt.random_map(rng, first + 3 * u) | 3) for u, i in enumerate(instants)]
        adv.append(lf.adv_record(req, 0, lf.connect_ind(aa, ci, maps[0][1], h, iv)))
        unmapped = (h * ((c + 1) % 37)) % 37
        ch = np.zeros(n_events, np.int64)
        for k, (i, m) in enumerate(maps):
            end = maps[k + 1][0] if k + 1 < len(maps) else n_events
            ch[i:end] = remap1(unmapped[i:end], m)
        at = t0 + 100 + c * iv * UNIT + rng.integers(-20, 21, n_events)
        length = np.zeros(n_events, np.int64)
        for i, m in maps[1:]:                                            # the LL_CHANNEL_MAP_IND, ten events ahead of its instant
            e = i - 10
            length[e] = 8
            payload = int.from_bytes(lf.map_ind(m, i)[1], "little") ^ white[ch[e]]
            bit = int(at[e]) + 56
            if bit + 64 <= 64 * N_WORDS:
                w, sh = bit >> 6, bit & 63
                lo = (int(words[ch[e], w]) & ~(((1 << 64) - 1) << sh & ((1 << 64) - 1))) | ((payload << sh) & ((1 << 64) - 1))
                words[ch[e], w] = lo
                if sh:
                    hi = (int(words[ch[e], w + 1]) & ~((1 << sh) - 1)) | (payload >> (64 - sh))
                    words[ch[e], w + 1] = hi
        off = np.stack([at, at + 80 + 8 * length + 150], 1).reshape(-1)
        stream = np.repeat(ch, 2)
        h0 = np.stack([np.where(length > 0, 3, 1), np.ones(n_events, np.int64)], 1).reshape(-1)
        ln = np.stack([length, np.zeros(n_events, np.int64)], 1).reshape(-1)
        order = np.lexsort((off, stream))                                # the grouping's order within a connection: (stream, offset)
        part = cands[g * per:(g + 1) * per]
        part["offset"], part["stream"], part["header0"], part["length"] = off[order], stream[order], h0[order], ln[order]
        part["access_address"], part["crc_init"], part["conn"] = aa, ci, g
        conns[g] = (aa, ci, per, int((ln == 0).sum()), int(np.bitwise_or.reduce(1 << np.unique(ch))), g * per)
    return cands, conns, lf.adv_array(adv, bt.LE_PKT_DTYPE), words


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conns", type=int, default=2000)
    ap.add_argument("--events", type=int, default=250)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=("many", "one"), default=None)
    args = ap.parse_args()
    import bench
    torch.cuda.set_device(0)
    bt.init(2)
    lib = bt.lib()
    phys = torch.tensor(DATA_MHZ, dtype=torch.int16, device="cuda")
    track_ms, seed_ms, follow_ms, sizes, followed, off_hop = {}, {}, {}, {}, {}, {}
    conn_cap = args.conns
    passes = 6 + sum(1 for k in range(4) if k == 0 or conn_cap >> (8 * k))
    for name, n_conns, n_events, instants in (("many", args.conns, args.events, (50, 100, 150, 200)),
                                              ("one", 1, args.conns * args.events, (200, 400, 600, 800))):
        if args.only and name != args.only:
            continue
        cands, conns, adv, words = build(n_conns, n_events, instants, args.seed, 39 if n_conns > 1 else 12)   # (the PDUs inside the streams)
        n = len(cands)
        sizes[name] = n
        d_cands, d_words, d_adv = torch.from_numpy(cands.view(np.int64)).cuda(), torch.from_numpy(words.view(np.int64)).cuda(), \
            torch.from_numpy(adv.view(np.int64)).cuda()
        d_conns = torch.zeros(4 * conn_cap, dtype=torch.int64, device="cuda")
        d_conns[:4 * n_conns] = torch.from_numpy(conns.view(np.int64)).cuda()
        cnt = torch.tensor([n, n_conns, len(adv), 0], dtype=torch.int32, device="cuda")
        d_tracks, d_pkts = torch.zeros(6 * conn_cap, dtype=torch.int64, device="cuda"), torch.zeros(2 * n, dtype=torch.int64, device="cuda")
        d_seeds, d_follows = torch.zeros(7 * conn_cap, dtype=torch.int64, device="cuda"), torch.zeros(6 * conn_cap, dtype=torch.int64, device="cuda")
        d_fpkts = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
        tscratch_bytes, scratch_bytes = lib.btbbx_le_track_scratch_bytes(n, conn_cap), lib.btbbx_le_epoch_scratch_bytes(n, conn_cap)
        tscratch = torch.zeros(tscratch_bytes // 8 + 2, dtype=torch.int64, device="cuda")
        scratch = torch.zeros(scratch_bytes // 8 + 2, dtype=torch.int64, device="cuda")
        p = cnt.data_ptr()

        def track():
            bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), p, n, d_conns.data_ptr(), p + 4, conn_cap, phys.data_ptr(), 37, UNIT, 200,
                                               50, bt.LE_TRACK_REMAP, d_tracks.data_ptr(), d_pkts.data_ptr(), tscratch.data_ptr(),
                                               tscratch_bytes, None), "btbbx_le_track_device")

        def seed():
            bt.check(lib.btbbx_le_seed_device(d_adv.data_ptr(), p + 8, len(adv), d_conns.data_ptr(), p + 4, conn_cap, d_tracks.data_ptr(), UNIT,
                                              d_seeds.data_ptr(), None), "btbbx_le_seed_device")

        def follow():
            bt.check(lib.btbbx_le_epoch_device(d_words.data_ptr(), N_WORDS, N_WORDS, 37, phys.data_ptr(), d_cands.data_ptr(), p, n,
                                                d_conns.data_ptr(), p + 4, conn_cap, d_tracks.data_ptr(), d_pkts.data_ptr(), d_seeds.data_ptr(),
                                                UNIT, 50, d_follows.data_ptr(), d_fpkts.data_ptr(), scratch.data_ptr(), scratch_bytes, None),
                     "btbbx_le_epoch_device")

        track_ms[name] = round(time_ms(track, args.warmup, args.steps), 4)
        seed_ms[name] = round(time_ms(seed, args.warmup, args.steps), 4)
        follow_ms[name] = round(time_ms(follow, args.warmup, args.steps), 4)
        f = d_follows.cpu().numpy().view(bt.LE_FOLLOW_DTYPE)[:n_conns]
        t = d_tracks.cpu().numpy().view(bt.LE_TRACK_DTYPE)[:n_conns]
        followed[name] = int(((f["flags"] == 3) & (f["n_map_updates"] == 4) & (f["n_on"] == n_events) & (f["n_off"] == 0)).sum())
        off_hop[name] = int(t["n_off_hop"].sum())
        del d_cands, d_pkts, d_fpkts, d_words, scratch, tscratch
    line = dict(metric="le_follow", candidates=sizes, conn_cap=conn_cap, seed_ms=seed_ms, follow_ms=follow_ms, track_ms=track_ms,
                follow_over_track={k: round((seed_ms[k] + follow_ms[k]) / track_ms[k], 2) for k in follow_ms}, followed=followed,
                track_off_hop=off_hop, launches=15 + 3 * passes, steps=args.steps, warmup=args.warmup,
                device=torch.cuda.get_device_name(0), csrc_sha16=bench.csrc_fingerprint())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
