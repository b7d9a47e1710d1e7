#!/usr/bin/env python3
"""Bluetooth LE scan measurement: a 4 GiB capture of 40 streams built on the GPU from a seed -- iid noise, advertising packets
on channels 37 / 38 / 39 and one connection's packets on the data channels, one planted packet per 4096 bits -- scanned with
btbbx_le_scan_device and decoded with btbbx_le_decode_hits_device.  Prints one JSON line:

* scan_ms[aa][limit]: ms per launch (HIP events, after warm-up) for the advertising AA (its filter bits folded into the
  adders) and the connection AA (run-time XORs), limits 0..4
* tbit_s / hbm_fraction at limit 2: stream bits per second, and algorithmic bytes (stream bytes + 16 B per hit) per second
  over the 8 TB/s HBM roofline
* decode_ms_per_2p20: btbbx_le_decode_hits_device time per 2^20 hits (the connection AA's hit list at limit 2)
* csrc_sha16: the source fingerprint of bench.py

Kernel times from the profiler come from a separate `rocprofv3 --kernel-trace --stats -- python tools/measure_le.py` run.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import libbtbb_amd as bt  # noqa: E402
import _le  # noqa: E402

CONN_AA = 0x50654C3B
HBM_BPS = 8e12


def mhz_of(s):
    data = [m for m in range(2404, 2480, 2) if m != 2426]
    return ([2402, 2426, 2480] + data)[s % 40]


def build_capture(seed, n_streams, n_words, conn_crc, lib_n=16):
    """Noise, then one packet per 64-word slot at word 2 + a bit phase, from a per-stream library of lib_n packets."""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    words = torch.randint(-2 ** 31, 2 ** 31 - 1, (n_streams, 2 * n_words), dtype=torch.int32, device="cuda", generator=g)
    words = words.view(torch.int64)
    rng = np.random.default_rng(seed)
    slots = n_words // 64
    for s in range(n_streams):
        adv = s < 3
        aa, crc_init = (_le.ADV_AA, _le.ADV_CRC_INIT) if adv else (CONN_AA, conn_crc)
        chan = _le.channel_index(mhz_of(s)) & 0x3F
        pk = np.zeros((lib_n, 8), np.uint64)
        mk = np.zeros((lib_n, 8), np.uint64)
        for k in range(lib_n):
            pdu = _le.make_pdu(int(rng.integers(0, 256)), rng.integers(0, 256, int(rng.integers(0, 28)), dtype=np.uint8).tobytes())
            b = _le.tx_bits(aa, chan, pdu, crc_init)
            phase = int(rng.integers(0, 64))
            sym = np.zeros(512, np.uint8)
            msk = np.zeros(512, np.uint8)
            sym[phase:phase + len(b)] = b
            msk[phase:phase + len(b)] = 1
            pk[k] = np.packbits(sym, bitorder="little").view(np.uint64)
            mk[k] = np.packbits(msk, bitorder="little").view(np.uint64)
        sel = torch.arange(slots, device="cuda") % lib_n
        pk_t = torch.from_numpy(pk.view(np.int64)).cuda()[sel]
        mk_t = torch.from_numpy(mk.view(np.int64)).cuda()[sel]
        w = words[s, :slots * 64].view(slots, 64)
        w[:, 2:10] = (w[:, 2:10] & ~mk_t) | pk_t
        del pk_t, mk_t
    return words


def time_ms(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


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
    cap = n_words * n_streams // 64 * 2 + (1 << 16)
    hits = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")

    def scan(aa, limit):
        cnt.zero_()
        bt.check(lib.btbbx_le_scan_device(words.data_ptr(), n_words, n_words, n_streams, search_bits, aa, limit, hits.data_ptr(), cap,
                                          cnt.data_ptr(), None), "btbbx_le_scan_device")

    scan_ms, counts = {}, {}
    for name, aa in (("adv", _le.ADV_AA), ("conn", CONN_AA)):
        scan_ms[name], counts[name] = {}, {}
        for limit in range(5):
            scan_ms[name][limit] = round(time_ms(lambda: scan(aa, limit), args.warmup, args.steps), 4)
            counts[name][limit] = int(cnt[0].item())
    # decode: the connection AA's hits at limit 2
    scan(CONN_AA, 2)
    torch.cuda.synchronize()
    n = min(int(cnt[0].item()), cap)
    out = torch.empty(n * 104 // 8 + 1, dtype=torch.int64, device="cuda")
    dec_ms = time_ms(lambda: bt.check(lib.btbbx_le_decode_hits_device(words.data_ptr(), n_words, n_words, hits.data_ptr(), cnt.data_ptr(), n,
                                                                      phys.data_ptr(), conn_crc, out.data_ptr(), None)), args.warmup, args.steps)
    recs = out[:n * 104 // 8].cpu().numpy().view(bt.LE_PKT_DTYPE)
    crc_ok = int(recs["crc_ok"].sum())
    stream_bytes = n_words * 8 * n_streams
    ms2 = scan_ms["conn"][2]
    line = dict(metric="le_scan", gib=round(stream_bytes / (1 << 30), 3), streams=n_streams, seed=args.seed, scan_ms=scan_ms, hits=counts,
                tbit_s=round(n_words * 64 * n_streams / (ms2 * 1e-3) / 1e12, 3),
                hbm_fraction=round((stream_bytes + 16 * counts["conn"][2]) / (ms2 * 1e-3) / HBM_BPS, 4),
                tbit_s_adv=round(n_words * 64 * n_streams / (scan_ms["adv"][2] * 1e-3) / 1e12, 3),
                hbm_fraction_adv=round((stream_bytes + 16 * counts["adv"][2]) / (scan_ms["adv"][2] * 1e-3) / HBM_BPS, 4),
                decode_ms_per_2p20=round(dec_ms * (1 << 20) / max(n, 1), 4), decode_hits=n, decode_crc_ok=crc_ok,
                csrc_sha16=bench.csrc_fingerprint())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
