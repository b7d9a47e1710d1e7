#!/usr/bin/env python3
"""LE Coded PHY measurement (include/btbbx.h, LE Coded PHY scan).  Prints one JSON line:

* coded_scan_ms[limit]: btbbx_le_coded_scan_device at max_errors 0, 16 and 63 on tools/measure_le.py's capture (4 GiB, 40 streams)
  with coded advertising packets planted in its three advertising streams; le_scan_ms: the 1M advertising-AA scan at limit 2 on the
  same buffer, timed alternating with the coded scan in the same process; ratio, stream Tbit/s and the fraction of the 8 TB/s HBM
  roofline (algorithmic bytes: the stream once + 16 B per hit)
* decode_ms_per_2p20[S][L]: btbbx_le_coded_decode_hits_device per 2^20 hits (measured on --hits hits and scaled) of clean packets
  with S = 8 / 2 and L = 37 / 255, the hits cycling over 64 planted packets at 64 bit phases; le_decode_ms_per_2p20: the 1M decoder
  on as many 1M hits (L = 37)
* csrc_sha16: the source fingerprint of bench.py

HIP events; every figure is the median of --reps repetitions of --steps launches after --warmup launches, with the fastest and the
slowest repetition beside it."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

import libbtbb_amd as bt  # noqa: E402
import _le  # noqa: E402
import _le_coded as lc  # noqa: E402
import measure_le  # noqa: E402

HBM_BPS = 8e12


def timed(fn, warmup, steps, reps):
    """[median, min, max] ms per launch over `reps` repetitions"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / steps)
    return [round(statistics.median(out), 4), round(min(out), 4), round(max(out), 4)]


def plant_coded(words, n_words, rng, every_words=4096):
    """One coded advertising packet (S alternating, L < 38, clean) per `every_words` words of streams 0..2, at word 100 + a bit phase
    of each span (the 1M packets of measure_le.build_capture lie in words 2..9 of every 64: the coded ones overwrite a few)."""
    planted = 0
    for s in range(3):
        chan = _le.channel_index(measure_le.mhz_of(s)) & 0x3F
        lib = []
        for k in range(8):
            sym = lc.coded_symbols(_le.ADV_AA, chan, lc.pdu_of(rng, int(rng.integers(0, 38))), _le.ADV_CRC_INIT, (2, 8)[k & 1])
            line = np.zeros(64 * 52, np.uint8)
            phase = int(rng.integers(0, 64))
            line[phase:phase + len(sym)] = sym
            msk = np.zeros(64 * 52, np.uint8)
            msk[phase:phase + len(sym)] = 1
            lib.append((np.packbits(line, bitorder="little").view(np.int64), np.packbits(msk, bitorder="little").view(np.int64)))
        spans = n_words // every_words
        w = words[s, :spans * every_words].view(spans, every_words)
        for k, (pk, mk) in enumerate(lib):
            pk_t, mk_t = torch.from_numpy(pk.copy()).cuda(), torch.from_numpy(mk.copy()).cuda()
            w[k::8, 100:152] = (w[k::8, 100:152] & ~mk_t) | pk_t
        planted += spans
    return planted


def decode_bench(lib, args, s, length, coded=True):
    """n hits cycling over 64 packets at 64 bit phases in one stream -> ms per 2^20 hits [median, min, max], crc_ok count"""
    rng = np.random.default_rng(args.seed + s + length)
    sym_len = (376 + s * (8 * (length + 5) + 3)) if coded else 40 + 8 * (length + 5)
    slot = (sym_len + 64 + 63) // 64 * 64
    line = rng.integers(0, 2, 64 * slot, dtype=np.uint8)
    offs = []
    for k in range(64):
        pdu = lc.pdu_of(rng, length)
        sym = lc.coded_symbols(_le.ADV_AA, 37, pdu, _le.ADV_CRC_INIT, s) if coded else _le.tx_bits(_le.ADV_AA, 37, pdu, _le.ADV_CRC_INIT)
        line[k * slot + k:k * slot + k + len(sym)] = sym
        offs.append(k * slot + k)
    words = torch.from_numpy(_le.pack(line).view(np.int64).copy()).cuda()
    n = args.hits
    hits = np.zeros(n, bt.HIT_DTYPE)
    hits["offset"] = np.array(offs, np.uint64)[np.arange(n) % 64]
    hits["lap"] = _le.ADV_AA
    d_hits = torch.from_numpy(np.frombuffer(hits.tobytes(), np.int64).copy()).cuda()
    d_cnt = torch.tensor([n, 0, 0, 0], dtype=torch.int32, device="cuda")
    phys = torch.tensor([2402], dtype=torch.int16, device="cuda")
    out = torch.empty(n * 13 + 1, dtype=torch.int64, device="cuda")
    info = torch.empty(n * 2 + 1, dtype=torch.int64, device="cuda")
    nw = len(line) // 64
    if coded:
        def fn():
            bt.check(lib.btbbx_le_coded_decode_hits_device(words.data_ptr(), nw, nw, d_hits.data_ptr(), d_cnt.data_ptr(), n, phys.data_ptr(),
                                                           _le.ADV_CRC_INIT, out.data_ptr(), info.data_ptr(), None, 0, None))
    else:
        def fn():
            bt.check(lib.btbbx_le_decode_hits_device(words.data_ptr(), nw, nw, d_hits.data_ptr(), d_cnt.data_ptr(), n, phys.data_ptr(),
                                                     _le.ADV_CRC_INIT, out.data_ptr(), None))
    ms = timed(fn, args.warmup, args.steps, args.reps)
    ok = int(out[:n * 13].cpu().numpy().view(bt.LE_PKT_DTYPE)["crc_ok"].sum())
    assert ok == n, (s, length, ok)
    return [round(x * (1 << 20) / n, 3) for x in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--streams", type=int, default=40)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hits", type=int, default=1 << 18)
    args = ap.parse_args()
    import bench
    torch.cuda.set_device(0)
    bt.init(2)
    lib = bt.lib()
    n_streams = args.streams
    n_words = int(args.gib * (1 << 30) / 8 / n_streams) // 4096 * 4096
    rng = np.random.default_rng(args.seed)
    words = measure_le.build_capture(args.seed, n_streams, n_words, int(rng.integers(0, 1 << 24)))
    planted = plant_coded(words, n_words, rng)
    cap = n_words * n_streams // 64 * 2 + (1 << 16)
    hits = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")

    def coded(limit):
        cnt.zero_()
        bt.check(lib.btbbx_le_coded_scan_device(words.data_ptr(), n_words, n_words, n_streams, n_words * 64 - 335, _le.ADV_AA, limit,
                                                hits.data_ptr(), cap, cnt.data_ptr(), None), "btbbx_le_coded_scan_device")

    def one_m():
        cnt.zero_()
        bt.check(lib.btbbx_le_scan_device(words.data_ptr(), n_words, n_words, n_streams, n_words * 64 - 39, _le.ADV_AA, 2, hits.data_ptr(), cap,
                                          cnt.data_ptr(), None), "btbbx_le_scan_device")

    coded_ms, coded_hits, le_ms = {}, {}, []
    for limit in (0, 16, 63):                           # alternating: coded, 1M, coded, 1M, ...
        coded_ms[limit] = timed(lambda: coded(limit), args.warmup, args.steps, args.reps)
        coded_hits[limit] = int(cnt[0].item())
        assert coded_hits[limit] == planted, (limit, coded_hits[limit], planted)
        le_ms.append(timed(one_m, args.warmup, args.steps, args.reps))
    le_hits = int(cnt[0].item())
    le_med = statistics.median(x[0] for x in le_ms)
    stream_bytes = n_words * 8 * n_streams
    decode = {s: {L: decode_bench(lib, args, s, L) for L in (37, 255)} for s in (8, 2)}
    line = dict(metric="le_coded", gib=round(stream_bytes / (1 << 30), 3), streams=n_streams, seed=args.seed, planted=planted,
                coded_scan_ms=coded_ms, coded_hits=coded_hits, le_scan_ms=le_ms, le_hits=le_hits,
                ratio_to_1m={k: round(v[0] / le_med, 2) for k, v in coded_ms.items()},
                tbit_s={k: round(n_words * 64 * n_streams / (v[0] * 1e-3) / 1e12, 3) for k, v in coded_ms.items()},
                hbm_fraction={k: round((stream_bytes + 16 * coded_hits[k]) / (v[0] * 1e-3) / HBM_BPS, 4) for k, v in coded_ms.items()},
                decode_hits=args.hits, decode_ms_per_2p20=decode, le_decode_ms_per_2p20=decode_bench(lib, args, 0, 37, coded=False),
                csrc_sha16=bench.csrc_fingerprint())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
