#!/usr/bin/env python3
"""Promiscuous LE Coded connection discovery measurement (include/btbbx.h btbbx_le_cfind_*).  Prints one JSON line:

* cfind_ms[limit]: btbbx_le_cfind_scan_device (both kernels) at max_errors 0, 16 and 63 on tools/measure_le.py's capture (4 GiB, 40
  streams) with the packets of one coded connection planted on its 37 data streams; coded_scan_ms[limit]: the yardstick,
  btbbx_le_coded_scan_device told that connection's access address at the same limit, timed alternating with it in the same
  process; ratio = cfind / coded; candidates, pre-records and the yardstick's hits of every limit
* decode_ms_per_2p18[S, L]: the entry on a stream of back-to-back clean packets (64 different ones, repeated) at max_errors 0, where
  nearly every pre-record is a packet; scan_share_ms is an ESTIMATE, not a measurement: the capture's limit-0 time per word (which
  holds some decoder work) times this stream's words.  The two kernels are not timed apart
* group_ms: btbbx_le_discover_group_device on that run's candidate list
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
import _le_discover as ld  # noqa: E402
import measure_le  # noqa: E402
from measure_le_coded import timed  # noqa: E402


def plant_connection(words, n_words, n_streams, aa, crc_init, rng, every_words=4096):
    """One coded data packet of the connection (S alternating, L < 28, clean) per `every_words` words of every data stream, at word
    100 + a bit phase of each span."""
    planted = 0
    for s in range(3, n_streams):
        chan = _le.channel_index(measure_le.mhz_of(s)) & 0x3F
        lib = []
        for k in range(8):
            pdu = _le.make_pdu((1, 2, 3)[k % 3], rng.integers(0, 256, int(rng.integers(0, 28)), dtype=np.uint8).tobytes())
            sym = lc.coded_symbols(aa, chan, pdu, crc_init, (2, 8)[k & 1])
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


def dense_bench(lib, args, s, length, aa, crc_init):
    """--pre packets back to back in one data-channel stream -> (entry ms, grouping ms, pre-records, candidates)"""
    rng = np.random.default_rng(args.seed + s + length)
    mhz = 2440
    chan = _le.channel_index(mhz)
    block = np.concatenate([lc.coded_symbols(aa, chan, _le.make_pdu(1 + k % 3, rng.integers(0, 256, length, dtype=np.uint8).tobytes()), crc_init, s)
                            for k in range(64)])
    assert len(block) % 64 == 0
    reps = args.pre // 64
    words = torch.from_numpy(_le.pack(block).view(np.int64).copy()).cuda().repeat(reps)
    words = torch.cat([words, torch.zeros(8, dtype=torch.int64, device="cuda")])
    n_words = words.numel()
    cap = args.pre * 2
    phys = torch.tensor([mhz], dtype=torch.int16, device="cuda")
    cands = torch.empty(cap * 3, dtype=torch.int64, device="cuda")
    pre = torch.empty(cap * 2, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    conns = torch.empty(cap * 4, dtype=torch.int64, device="cuda")
    scratch = torch.empty(lib.btbbx_le_discover_scratch_bytes(cap), dtype=torch.uint8, device="cuda")

    def scan():
        cnt.zero_()
        bt.check(lib.btbbx_le_cfind_scan_device(words.data_ptr(), n_words, n_words, 1, n_words * 64 - 335, phys.data_ptr(), 255, 0, cands.data_ptr(),
                                                None, cap, cnt.data_ptr(), cnt.data_ptr() + 4, pre.data_ptr(), 16 * cap, None),
                 "btbbx_le_cfind_scan_device")

    ms = timed(scan, args.warmup, args.steps, args.reps)
    n_cands, n_pre = int(cnt[0].item()), int(cnt[1].item())
    assert n_cands >= args.pre - 64 and n_pre <= cap, (n_cands, n_pre)
    keep = cands.clone()

    def group():
        cands.copy_(keep)
        bt.check(lib.btbbx_le_discover_group_device(cands.data_ptr(), cnt.data_ptr(), cap, 2, conns.data_ptr(), cap, cnt.data_ptr() + 8,
                                                    scratch.data_ptr(), scratch.numel(), None), "btbbx_le_discover_group_device")

    def copy_only():
        cands.copy_(keep)

    g_ms, c_ms = timed(group, args.warmup, args.steps, args.reps), timed(copy_only, args.warmup, args.steps, args.reps)
    assert int(cnt[2].item()) >= 1
    return dict(ms=ms, group_ms=[round(a - c_ms[0], 4) for a in g_ms], pre_records=n_pre, candidates=n_cands, words=n_words)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--streams", type=int, default=40)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pre", type=int, default=1 << 18)
    ap.add_argument("--pre-cap", type=int, default=48 << 20)
    args = ap.parse_args()
    import bench
    torch.cuda.set_device(0)
    bt.init(2)
    lib = bt.lib()
    n_streams = args.streams
    n_words = int(args.gib * (1 << 30) / 8 / n_streams) // 4096 * 4096
    rng = np.random.default_rng(args.seed)
    words = measure_le.build_capture(args.seed, n_streams, n_words, int(rng.integers(0, 1 << 24)))
    aa, crc_init = ld.good_aa(rng), int(rng.integers(0, 1 << 24))
    planted = plant_connection(words, n_words, n_streams, aa, crc_init, rng)
    phys = torch.tensor([measure_le.mhz_of(s) for s in range(n_streams)], dtype=torch.int16, device="cuda")
    cap = n_words * n_streams // 64 * 2 + (1 << 16)
    hits = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")       # the yardstick's hits
    # (every S = 8 packet leaves some 500 pre-records at max_errors 63: the offsets inside its block 2 that lie on a mapped group)
    pre = torch.zeros(2 * args.pre_cap, dtype=torch.int64, device="cuda")
    cands = torch.zeros(3 * (1 << 20), dtype=torch.int64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    search_bits = n_words * 64 - 335

    def cfind(limit):
        cnt.zero_()
        bt.check(lib.btbbx_le_cfind_scan_device(words.data_ptr(), n_words, n_words, n_streams, search_bits, phys.data_ptr(), 27, limit,
                                                cands.data_ptr(), None, 1 << 20, cnt.data_ptr(), cnt.data_ptr() + 4, pre.data_ptr(), 16 * args.pre_cap, None),
                 "btbbx_le_cfind_scan_device")

    def coded(limit):
        cnt.zero_()
        bt.check(lib.btbbx_le_coded_scan_device(words.data_ptr(), n_words, n_words, n_streams, search_bits, aa, limit, hits.data_ptr(), cap,
                                                cnt.data_ptr(), None), "btbbx_le_coded_scan_device")

    cfind_ms, coded_ms, counts = {}, {}, {}
    for limit in (0, 16, 63):                           # alternating: this stage, the yardstick, this stage, ...
        cfind_ms[limit] = timed(lambda: cfind(limit), args.warmup, args.steps, args.reps)
        n_cands, n_pre = int(cnt[0].item()), int(cnt[1].item())
        coded_ms[limit] = timed(lambda: coded(limit), args.warmup, args.steps, args.reps)
        counts[limit] = dict(candidates=n_cands, pre_records=n_pre, coded_hits=int(cnt[0].item()))
        assert n_pre <= args.pre_cap and n_cands >= planted and counts[limit]["coded_hits"] == planted, (limit, counts[limit], planted)
    stream_bytes = n_words * 8 * n_streams
    del words, hits, pre
    dense = {"S%d_L%d" % (s, length): dense_bench(lib, args, s, length, aa, crc_init) for s, length in ((2, 0), (8, 27))}
    for v in dense.values():                            # the scan's share of a dense run, by the capture's time per word at limit 0
        v["scan_share_ms"] = round(cfind_ms[0][0] * v["words"] / (n_words * n_streams), 4)
    line = dict(metric="le_cfind", gib=round(stream_bytes / (1 << 30), 3), streams=n_streams, seed=args.seed, planted=planted,
                cfind_ms=cfind_ms, coded_scan_ms=coded_ms, counts=counts,
                ratio_to_coded_scan={k: round(v[0] / coded_ms[k][0], 3) for k, v in cfind_ms.items()},
                tbit_s={k: round(n_words * 64 * n_streams / (v[0] * 1e-3) / 1e12, 3) for k, v in cfind_ms.items()},
                dense=dense, csrc_sha16=bench.csrc_fingerprint())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
