#!/usr/bin/env python3
"""Keyed LE span following measurement: btbbx_le_keyed_span_device beside btbbx_le_span_device over the same lists in the same run,
in alternating pairs, max_updates 2, and the decryption stage that feeds it.  The world is that of tools/measure_le_span.py's "many"
list (2 000 connections of 250 events, four channel map updates and two connection parameter updates each, every PDU announced ten
events ahead), but with the parameter updates going 6 -> 12 -> 6 units where that tool's go 6 -> 8 -> 6: the tracking fits one
interval to a connection, 6 and 8 units share none of 6 units or more, and a connection the tracking cannot time gets no roles from
the data stage and nothing VERIFIED from the decryption stage.  Every connection encrypts: the central's LL_ENC_REQ and the peripheral's LL_ENC_RSP stand in event 2 (g % 4) of
connection g, the peripheral's LL_START_ENC_REQ in the event behind it (the shift keeps neighbours' procedure PDUs off each other:
connections start 131 bits apart, an LL_ENC_REQ is 184 bits long), and all six update PDUs go out under AES-CCM with the connection's
own session key -- from key g % 16 of a table of 16 -- and their true packet counters.  Every packet carries its event's parity as SN,
so none is a retransmission.  data_pkts, crypt and crypt_pkts are what btbbx_le_data_device and btbbx_le_crypt_device (window 8,
nothing stored) leave on these lists, fed to the keyed stage as they are; where a neighbour's PDU overwrote one of a connection's
procedure PDUs the stage finds no key and the connection stays unread, which the counts below show.

HIP events, 3 warm-ups and 20 launches per figure, `pairs` alternating pairs.  Prints one JSON line:

* keyed_ms, span_ms: the pairs' figures on the encrypted world; keyed_over_span: the means' ratio
* clear_keyed_ms, clear_span_ms, clear_keyed_over_span: the same pairs with every crypt_pkts state CLEAR -- no member is READABLE
  and the outputs are the unkeyed stage's --, and spread: the largest relative deviation of a figure from its series' mean
* crypt_ms, data_ms: the decryption stage and the data stage on this world, in the same pairs; keyed_conns, verified, failed: what
  the decryption stage found (of 6 encrypted PDUs per connection)
* followed_keyed / followed_span: connections that came out with three spans, four map updates and every event on the prediction;
  clean: connections none of whose update PDUs shares stream bits with another connection's
* lost_events: events the unkeyed stage leaves off the hop or BEYOND and the keyed stage predicts (n_off + n_beyond, summed)
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
import _le_crypt as cm  # noqa: E402
import libbtbb_amd as bt  # noqa: E402
import measure_le_span as ms  # noqa: E402
from measure_le import time_ms  # noqa: E402
from measure_le_track import DATA_MHZ, UNIT  # noqa: E402

MAX_UPDATES = 2


def get(words, row, bit, nbits):
    v, at = 0, 0
    while at < nbits:
        w, sh = (bit + at) >> 6, (bit + at) & 63
        take = min(64 - sh, nbits - at)
        v |= ((int(words[row, w]) >> sh) & ((1 << take) - 1)) << at
        at += take
    return v


N_KEYS, WINDOW = 16, 8
INTERVALS = (12, 6)                                              # 6 -> 12 -> 6 units


def encrypt(cands, conns, words, rng):
    """ms.build's lists with every connection encrypting: the procedure's three PDUs, the update PDUs as ciphertext | MIC, four octets
    longer, every peripheral's packet moved behind its central's new end, SN = the event's parity.  -> the key table."""
    white = [_le.bits_value(_le.whitening_bits(ch, 16 + 256)[16:]) for ch in range(37)]
    keys = [cm.ltk(700 + j) for j in range(N_KEYS)]

    def write(i, payload):
        row, bit = int(cands[i]["stream"]), int(cands[i]["offset"]) + 56
        ms.put(words, row, bit, int.from_bytes(payload, "little") ^ (white[row] & ((1 << 8 * len(payload)) - 1)), 8 * len(payload))
        cands[i]["header0"], cands[i]["length"] = (int(cands[i]["header0"]) & ~3) | 3, len(payload)

    for g, conn in enumerate(conns):
        first, per = int(conn["first"]), int(conn["n_packets"])
        part = cands[first:first + per]
        order = first + np.argsort(part["offset"], kind="stable")          # 2e: the central's packet of event e, 2e + 1: the peripheral's
        cands["header0"][order] |= ((np.arange(per) >> 1) & 1).astype(cands["header0"].dtype) << 3
        skdm, skds, ivm, ivs = (bytes(rng.integers(0, 256, count, dtype=np.uint8).tolist()) for count in (8, 8, 4, 4))
        sk, iv = cm.session_key(keys[g % N_KEYS], skdm, skds), ivm + ivs
        e0 = 2 * (g % 4)
        grown = {}                                                          # event -> octets its central's PDU grew by
        write(int(order[2 * e0]), bytes([3]) + bytes(10) + skdm + ivm)      # LL_ENC_REQ
        grown[e0] = 23
        counter = 0
        for e in range(e0 + 2, per // 2):
            i = int(order[2 * e])
            length = int(cands[i]["length"])
            if length not in (8, 12):
                continue
            row, bit = int(cands[i]["stream"]), int(cands[i]["offset"]) + 56
            plain = (get(words, row, bit, 8 * length) ^ (white[row] & ((1 << 8 * length) - 1))).to_bytes(length, "little")
            write(i, cm.ccm_encrypt(sk, iv, counter, 1, int(cands[i]["header0"]), plain))
            grown[e] = 4
            counter += 1
        for e, octets in grown.items():
            cands["offset"][order[2 * e + 1]] += 8 * octets
        write(int(order[2 * e0 + 1]), bytes([4]) + skds + ivs)              # LL_ENC_RSP
        write(int(order[2 * e0 + 3]), bytes([5]))                           # LL_START_ENC_REQ
        assert (np.diff(cands["offset"][order].astype(np.int64)) > 0).all()
        part[:] = part[np.lexsort((part["offset"], part["stream"]))]
        conn["n_empty"] = int((part["length"] == 0).sum())
    return keys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conns", type=int, default=2000)
    ap.add_argument("--events", type=int, default=250)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=4)
    args = ap.parse_args()
    import bench
    torch.cuda.set_device(0)
    bt.init(2)
    lib = bt.lib()
    phys = torch.tensor(DATA_MHZ, dtype=torch.int16, device="cuda")
    k = args.conns
    cands, conns, adv, words, clean = ms.build(k, args.events, (50, 100, 150, 200), (80, 170), args.seed, INTERVALS)
    keys = encrypt(cands, conns, words, np.random.default_rng(args.seed + 1))
    n = len(cands)
    up = lambda a: torch.from_numpy(np.frombuffer(a.tobytes() + bytes((-a.nbytes) % 8), np.int64).copy()).cuda()   # noqa: E731
    zeros = lambda count, dtype=torch.int64: torch.zeros(count, dtype=dtype, device="cuda")                        # noqa: E731
    d_cands, d_words, d_adv, d_conns = up(cands), up(words), up(adv), up(conns)
    d_keys = torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).copy()).cuda()
    cnt = torch.tensor([n, k, len(adv), 0] + [0] * 12, dtype=torch.int32, device="cuda")
    d_tracks, d_pkts, d_seeds = zeros(6 * k), zeros(2 * n), zeros(7 * k)
    d_data, d_dpkts, d_crypt, d_cpkts, d_ppkts = zeros(6 * k), zeros(3 * n, torch.int32), zeros(7 * k), zeros(2 * n), zeros(3 * n, torch.int32)
    d_msgs, d_bytes = zeros(4 * 64), zeros(64, torch.uint8)
    outs = {name: (zeros(7 * k), zeros(2 * n), zeros(5 * k * (MAX_UPDATES + 1))) for name in ("keyed", "span")}
    tbytes, sbytes = lib.btbbx_le_track_scratch_bytes(n, k), lib.btbbx_le_span_scratch_bytes(n, k, MAX_UPDATES)
    kbytes = lib.btbbx_le_keyed_span_scratch_bytes(n, k, MAX_UPDATES)
    dbytes, cbytes = lib.btbbx_le_data_scratch_bytes(n, k), lib.btbbx_le_crypt_scratch_bytes(n, k, N_KEYS)
    tscratch, sscratch, kscratch, dscratch, cscratch = (zeros(b // 8 + 2) for b in (tbytes, sbytes, kbytes, dbytes, cbytes))
    p = cnt.data_ptr()
    front = (d_words.data_ptr(), ms.N_WORDS, ms.N_WORDS, 37, phys.data_ptr(), d_cands.data_ptr(), p, n, d_conns.data_ptr(), p + 4, k,
             d_tracks.data_ptr(), d_pkts.data_ptr(), d_seeds.data_ptr())
    bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), p, n, d_conns.data_ptr(), p + 4, k, phys.data_ptr(), 37, UNIT, 200, 50,
                                       bt.LE_TRACK_REMAP, d_tracks.data_ptr(), d_pkts.data_ptr(), tscratch.data_ptr(), tbytes, None),
             "btbbx_le_track_device")
    bt.check(lib.btbbx_le_seed_device(d_adv.data_ptr(), p + 8, len(adv), d_conns.data_ptr(), p + 4, k, d_tracks.data_ptr(), UNIT,
                                      d_seeds.data_ptr(), None), "btbbx_le_seed_device")

    def data():                                                 # (no message and no octet is kept: caps 0)
        bt.check(lib.btbbx_le_data_device(*front[:13], d_data.data_ptr(), d_dpkts.data_ptr(), d_msgs.data_ptr(), 0, p + 16, d_bytes.data_ptr(), 0,
                                          p + 24, dscratch.data_ptr(), dbytes, None), "btbbx_le_data_device")

    def crypt():
        bt.check(lib.btbbx_le_crypt_device(*front[:13], d_dpkts.data_ptr(), d_keys.data_ptr(), N_KEYS, WINDOW, d_crypt.data_ptr(), d_cpkts.data_ptr(),
                                           d_ppkts.data_ptr(), d_msgs.data_ptr(), 0, p + 32, d_bytes.data_ptr(), 0, p + 40, cscratch.data_ptr(),
                                           cbytes, None), "btbbx_le_crypt_device")

    data()
    crypt()
    torch.cuda.synchronize()
    rec = d_crypt.cpu().numpy().view(bt.LE_CRYPT_DTYPE)[:k]
    found = dict(keyed_conns=int((rec["flags"] & bt.LE_CRYPT_KEYED != 0).sum()), verified=int(rec["n_verified"].sum()),
                 failed=int(rec["n_failed"].sum()), skipped=int(rec["n_skipped"].sum()))
    clear = d_cpkts.cpu().numpy().view(bt.LE_CRYPT_PKT_DTYPE).copy()
    clear["state"][clear["state"] != 0xFF] = cm.CLEAR
    d_clear = up(clear)

    def span():
        o = outs["span"]
        bt.check(lib.btbbx_le_span_device(*front, UNIT, 50, MAX_UPDATES, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), sscratch.data_ptr(),
                                          sbytes, None), "btbbx_le_span_device")

    def keyed(states):
        o = outs["keyed"]
        bt.check(lib.btbbx_le_keyed_span_device(*front, d_dpkts.data_ptr(), d_crypt.data_ptr(), states.data_ptr(), UNIT, 50, MAX_UPDATES,
                                                o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), kscratch.data_ptr(), kbytes, None),
                 "btbbx_le_keyed_span_device")

    series = dict(keyed_ms=[], span_ms=[], clear_keyed_ms=[], clear_span_ms=[], crypt_ms=[], data_ms=[])
    for _ in range(args.pairs):
        series["keyed_ms"].append(round(time_ms(lambda: keyed(d_cpkts), args.warmup, args.steps), 4))
        series["span_ms"].append(round(time_ms(span, args.warmup, args.steps), 4))
        series["clear_keyed_ms"].append(round(time_ms(lambda: keyed(d_clear), args.warmup, args.steps), 4))
        series["clear_span_ms"].append(round(time_ms(span, args.warmup, args.steps), 4))
        series["crypt_ms"].append(round(time_ms(crypt, args.warmup, args.steps), 4))
        series["data_ms"].append(round(time_ms(data, args.warmup, args.steps), 4))
    mean = {name: sum(v) / len(v) for name, v in series.items()}
    spread = max(abs(x - mean[name]) / mean[name] for name, v in series.items() for x in v)
    keyed(d_clear)
    span()
    torch.cuda.synchronize()
    same = all(a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() for a, b in zip(outs["keyed"], outs["span"]))
    keyed(d_cpkts)
    torch.cuda.synchronize()
    got = {name: o[0].cpu().numpy().view(bt.LE_SPAN_DTYPE)[:k] for name, o in outs.items()}
    ok = {name: (s["n_spans"] == 3) & (s["n_map_updates"] == 4) & (s["n_on"] == args.events) & (s["n_off"] == 0) for name, s in got.items()}
    lost = {name: int(s["n_off"].sum()) + int(s["n_beyond"].sum()) for name, s in got.items()}
    passes = 6 + sum(1 for b in range(4) if b == 0 or k >> (8 * b))
    launches = 13 + 6 * (MAX_UPDATES + 1) + 3 * passes
    line = dict(metric="le_keyed", conns=k, candidates=n, max_updates=MAX_UPDATES, launches=dict(span=launches, keyed=launches),
                keyed_over_span=round(mean["keyed_ms"] / mean["span_ms"], 3), clear_keyed_over_span=round(mean["clear_keyed_ms"] / mean["clear_span_ms"], 3),
                spread=round(spread, 3), clear_outputs_equal=same, decrypted=int((got["keyed"]["flags"] & bt.LE_FOLLOW_DECRYPTED != 0).sum()),
                followed_keyed=int(ok["keyed"].sum()), followed_keyed_clean=int((ok["keyed"] & clean).sum()), followed_span=int(ok["span"].sum()),
                clean=int(clean.sum()), keys=N_KEYS, window=WINDOW, **found, lost_events=lost["span"] - lost["keyed"], off_or_beyond=lost, steps=args.steps, warmup=args.warmup,
                pairs=args.pairs, device=torch.cuda.get_device_name(0), csrc_sha16=bench.csrc_fingerprint(), **series)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
