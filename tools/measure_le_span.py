#!/usr/bin/env python3
"""LE span following measurement: btbbx_le_span_device at max_updates 0, 2 and 4 beside btbbx_le_epoch_device and
btbbx_le_track_device over the same lists in the same run, alternating.  The lists are those of tools/measure_le_follow.py (two
packets per connection event, anchors jittered by +-20 bits, every connection seeded, algorithm #1 through four channel map updates
announced ten events ahead) with two connection parameter updates on top, 6 -> 8 -> 6 units, each announced ten events ahead by an
LL_CONNECTION_UPDATE_IND whose payload stands, whitened, in the streams; the anchors are walked forward through the transmit windows:

* many: 2 000 connections of 250 events, parameter updates at events 80 and 170, map updates at 50, 100, 150 and 200
* one:  a single connection of 500 000 events, parameter updates at events 300 and 700, map updates at 200, 400, 600 and 800

HIP events, 3 warm-ups and 20 launches per figure, two rounds.  Prints one JSON line:

* span_ms[list][max_updates], epoch_ms[list], track_ms[list]: both rounds' figures; span_over_epoch: the means' ratio
* launches[max_updates]; followed[list][max_updates]: connections that came out with three spans, four map updates and every event
  on the prediction; clean[list]: connections none of whose six update PDUs shares stream bits with another connection's (all
  connections have the same intervals here, so neighbours' PDUs meet when their events fall on one channel), and
  followed_clean[list][max_updates]: the followed ones among them; epoch_beyond[list]: the events btbbx_le_epoch_device leaves
  BEYOND on the same list
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
import _le_span as ls  # noqa: E402
import libbtbb_amd as bt  # noqa: E402
from measure_le import time_ms  # noqa: E402
from measure_le_follow import remap1  # noqa: E402
from measure_le_track import DATA_MHZ, UNIT  # noqa: E402

N_WORDS = 195000
UPDATES = (0, 2, 4)


def put(words, row, bit, value, nbits):
    """value's nbits low bits at bit offset `bit` of one stream."""
    if bit + nbits > 64 * words.shape[1]:
        return
    while nbits:
        w, sh = bit >> 6, bit & 63
        take = min(64 - sh, nbits)
        mask = ((1 << take) - 1) << sh
        words[row, w] = (int(words[row, w]) & ~mask & ((1 << 64) - 1)) | ((value & ((1 << take) - 1)) << sh)
        value >>= take
        bit += take
        nbits -= take


def build(n_conns, n_events, map_instants, param_instants, seed, intervals=(8, 6)):
    """intervals: what the two parameter updates change the 6 units to."""
    rng = np.random.default_rng(seed)
    per = 2 * n_events
    cands = np.zeros(n_conns * per, bt.LE_CAND_DTYPE)
    conns = np.zeros(n_conns, bt.LE_CONN_DTYPE)
    words = rng.integers(0, 1 << 63, (37, N_WORDS), dtype=np.uint64)
    white = [_le.bits_value(_le.whitening_bits(ch, 16 + 96)[16:]) for ch in range(37)]
    adv, written = [], [[] for _ in range(37)]                            # per channel: (first bit, last bit + 1, connection) of the PDUs
    c = np.arange(n_events, dtype=np.int64)
    for g in range(n_conns):
        h = int(rng.integers(5, 17))
        aa, ci = 0x10000000 + 7919 * g, (104729 * g + 1) & 0xFFFFFF
        req = 600 + 131 * g
        t0 = req + 352 + 2 * UNIT
        first = int(rng.integers(10, 38))
        maps = [(0, (1 << 37) - 1)] + [(i, lf.lt.random_map(rng, first + 3 * u) | 3) for u, i in enumerate(map_instants)]
        adv.append(lf.adv_record(req, 0, lf.connect_ind(aa, ci, maps[0][1], h, 6)))
        unmapped = (h * ((c + 1) % 37)) % 37
        ch = np.zeros(n_events, np.int64)
        for k, (i, m) in enumerate(maps):
            end = maps[k + 1][0] if k + 1 < len(maps) else n_events
            ch[i:end] = remap1(unmapped[i:end], m)
        # the forward walk: 6 units, then 8 from the first instant, 6 from the second; each new window WinOffset units + pos behind
        gap = np.full(n_events, 6 * UNIT, np.int64)
        gap[0] = 0
        ups = [(param_instants[0], intervals[0], int(rng.integers(0, 4)), 1), (param_instants[1], intervals[1], int(rng.integers(0, 4)), 2)]
        iv = 6
        for i, new, wo, ws in ups:
            gap[i] = iv * UNIT + wo * UNIT + int(rng.integers(0, ws * UNIT - 200))
            gap[i + 1:] = new * UNIT
            iv = new
        at = t0 + 100 + np.cumsum(gap) + rng.integers(-20, 21, n_events)
        length = np.zeros(n_events, np.int64)
        pdus = [(i - 10, lf.map_ind(m, i)[1]) for i, m in maps[1:]] + [(i - 10, ls.param_ind(i, new, wo, ws)[1]) for i, new, wo, ws in ups]
        for e, payload in pdus:
            length[e] = len(payload)
            nbits = 8 * len(payload)
            put(words, ch[e], int(at[e]) + 56, int.from_bytes(payload, "little") ^ (white[ch[e]] & ((1 << nbits) - 1)), nbits)
            written[ch[e]].append((int(at[e]) + 56, int(at[e]) + 56 + nbits, g))
        off = np.stack([at, at + 80 + 8 * length + 150], 1).reshape(-1)
        stream = np.repeat(ch, 2)
        h0 = np.stack([np.where(length > 0, 3, 1), np.ones(n_events, np.int64)], 1).reshape(-1)
        ln = np.stack([length, np.zeros(n_events, np.int64)], 1).reshape(-1)
        order = np.lexsort((off, stream))
        part = cands[g * per:(g + 1) * per]
        part["offset"], part["stream"], part["header0"], part["length"] = off[order], stream[order], h0[order], ln[order]
        part["access_address"], part["crc_init"], part["conn"] = aa, ci, g
        conns[g] = (aa, ci, per, int((ln == 0).sum()), int(np.bitwise_or.reduce(1 << np.unique(ch))), g * per)
    clean = np.ones(n_conns, bool)
    for spans in written:
        spans.sort()
        for (a0, a1, ga), (b0, b1, gb) in zip(spans, spans[1:]):
            if b0 < a1 and ga != gb:
                clean[ga] = clean[gb] = False
    return cands, conns, lf.adv_array(adv, bt.LE_PKT_DTYPE), words, clean


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
    conn_cap = args.conns
    passes = 6 + sum(1 for k in range(4) if k == 0 or conn_cap >> (8 * k))
    out = dict(span_ms={}, epoch_ms={}, track_ms={}, span_over_epoch={}, followed={}, clean={}, followed_clean={}, epoch_beyond={}, candidates={})
    for name, n_conns, n_events, map_instants, param_instants in (("many", args.conns, args.events, (50, 100, 150, 200), (80, 170)),
                                                                  ("one", 1, args.conns * args.events, (200, 400, 600, 800), (300, 700))):
        if args.only and name != args.only:
            continue
        cands, conns, adv, words, clean = build(n_conns, n_events, map_instants, param_instants, args.seed)
        n = len(cands)
        out["candidates"][name] = n
        d_cands, d_words, d_adv = torch.from_numpy(cands.view(np.int64)).cuda(), torch.from_numpy(words.view(np.int64)).cuda(), \
            torch.from_numpy(adv.view(np.int64)).cuda()
        d_conns = torch.zeros(4 * conn_cap, dtype=torch.int64, device="cuda")
        d_conns[:4 * n_conns] = torch.from_numpy(conns.view(np.int64)).cuda()
        cnt = torch.tensor([n, n_conns, len(adv), 0], dtype=torch.int32, device="cuda")
        d_tracks, d_pkts = torch.zeros(6 * conn_cap, dtype=torch.int64, device="cuda"), torch.zeros(2 * n, dtype=torch.int64, device="cuda")
        d_seeds, d_follows = torch.zeros(7 * conn_cap, dtype=torch.int64, device="cuda"), torch.zeros(6 * conn_cap, dtype=torch.int64, device="cuda")
        d_fpkts = torch.zeros(3 * n, dtype=torch.int32, device="cuda")
        d_spans, d_spkts = torch.zeros(7 * conn_cap, dtype=torch.int64, device="cuda"), torch.zeros(2 * n, dtype=torch.int64, device="cuda")
        d_recs = torch.zeros(5 * conn_cap * 5, dtype=torch.int64, device="cuda")
        tscratch_bytes, escratch_bytes = lib.btbbx_le_track_scratch_bytes(n, conn_cap), lib.btbbx_le_epoch_scratch_bytes(n, conn_cap)
        sscratch_bytes = lib.btbbx_le_span_scratch_bytes(n, conn_cap, max(UPDATES))
        tscratch = torch.zeros(tscratch_bytes // 8 + 2, dtype=torch.int64, device="cuda")
        escratch = torch.zeros(escratch_bytes // 8 + 2, dtype=torch.int64, device="cuda")
        sscratch = torch.zeros(sscratch_bytes // 8 + 2, dtype=torch.int64, device="cuda")
        p = cnt.data_ptr()
        front = (d_words.data_ptr(), N_WORDS, N_WORDS, 37, phys.data_ptr(), d_cands.data_ptr(), p, n, d_conns.data_ptr(), p + 4, conn_cap,
                 d_tracks.data_ptr(), d_pkts.data_ptr(), d_seeds.data_ptr(), UNIT, 50)

        def track():
            bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), p, n, d_conns.data_ptr(), p + 4, conn_cap, phys.data_ptr(), 37, UNIT, 200,
                                               50, bt.LE_TRACK_REMAP, d_tracks.data_ptr(), d_pkts.data_ptr(), tscratch.data_ptr(),
                                               tscratch_bytes, None), "btbbx_le_track_device")

        def epoch():
            bt.check(lib.btbbx_le_epoch_device(*front, d_follows.data_ptr(), d_fpkts.data_ptr(), escratch.data_ptr(), escratch_bytes, None),
                     "btbbx_le_epoch_device")

        def span(ups):
            bt.check(lib.btbbx_le_span_device(*front, ups, d_spans.data_ptr(), d_spkts.data_ptr(), d_recs.data_ptr(), sscratch.data_ptr(),
                                              sscratch_bytes, None), "btbbx_le_span_device")

        track()
        bt.check(lib.btbbx_le_seed_device(d_adv.data_ptr(), p + 8, len(adv), d_conns.data_ptr(), p + 4, conn_cap, d_tracks.data_ptr(), UNIT,
                                          d_seeds.data_ptr(), None), "btbbx_le_seed_device")
        span_ms, epoch_ms, track_ms, followed, followed_clean = {u: [] for u in UPDATES}, [], [], {}, {}
        for _ in range(2):
            epoch_ms.append(round(time_ms(epoch, args.warmup, args.steps), 4))
            for u in UPDATES:
                span_ms[u].append(round(time_ms(lambda u=u: span(u), args.warmup, args.steps), 4))
            track_ms.append(round(time_ms(track, args.warmup, args.steps), 4))
        for u in UPDATES:
            span(u)
            torch.cuda.synchronize()
            s = d_spans.cpu().numpy().view(bt.LE_SPAN_DTYPE)[:n_conns]
            ok = (s["n_spans"] == 3) & (s["n_map_updates"] == 4) & (s["n_on"] == n_events) & (s["n_off"] == 0)
            followed[u], followed_clean[u] = int(ok.sum()), int((ok & clean).sum())
        epoch()
        torch.cuda.synchronize()
        f = d_follows.cpu().numpy().view(bt.LE_FOLLOW_DTYPE)[:n_conns]
        out["epoch_beyond"][name] = int(f["n_beyond"].sum())
        out["span_ms"][name], out["epoch_ms"][name], out["track_ms"][name], out["followed"][name] = span_ms, epoch_ms, track_ms, followed
        out["clean"][name], out["followed_clean"][name] = int(clean.sum()), followed_clean
        out["span_over_epoch"][name] = {u: round(sum(span_ms[u]) / sum(epoch_ms), 2) for u in UPDATES}
        del d_cands, d_pkts, d_fpkts, d_spkts, d_words, escratch, sscratch, tscratch
    line = dict(metric="le_span", conn_cap=conn_cap, launches={u: 13 + 6 * (u + 1) + 3 * passes for u in UPDATES}, epoch_launches=15 + 3 * passes,
                steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0), csrc_sha16=bench.csrc_fingerprint(), **out)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
