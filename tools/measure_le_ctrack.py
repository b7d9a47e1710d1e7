#!/usr/bin/env python3
"""LE Coded connection tracking measurement (include/btbbx.h btbbx_le_ctrack_*).  Prints one JSON line:

* symbols_ms[S, n]: btbbx_le_ctrack_symbols_device on the candidates of n = 2^18 and 2^20 clean empty packets back to back, S = 8 and
  S = 2; cfind_ms beside it: btbbx_le_cfind_scan_device (BOTH its kernels: the entry does not run its decoder apart) on the same
  packets at max_errors 0, alternating in the same process.  The decoder decodes block 1 and much more: an upper yardstick
* track_ms / ctrack_ms: btbbx_le_track_device and btbbx_le_ctrack_device with 1M durations on one list of --conns connections of
  --events events, alternating, each timed twice: the two runs of the parent's tracking give the spread the stand-in is held against
* chain: on tools/measure_le_cfind.py's capture (4 GiB, 40 streams, one coded connection planted) the device part of the coded
  discovery -- scan at max_errors 16 and grouping -- and behind it durations, tracking and channel selection #2
* csrc_sha16: the source fingerprint of bench.py

HIP events; every figure is the median of --reps repetitions of --steps launches after --warmup launches, with the fastest and the
slowest repetition beside it."""
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
import _le  # noqa: E402
import _le_coded as lc  # noqa: E402
import _le_discover as ld  # noqa: E402
import measure_le  # noqa: E402
from measure_le_cfind import plant_connection  # noqa: E402
from measure_le_coded import timed  # noqa: E402


def symbols_bench(lib, args, s, n, aa, crc_init):
    """n empty packets back to back in one data-channel stream: the discovery's candidates of them, then the durations of that list"""
    mhz = 2440
    block = np.concatenate([lc.coded_symbols(aa, _le.channel_index(mhz), _le.make_pdu(1, b""), crc_init, s) for _ in range(64)])
    assert len(block) % 64 == 0 and len(block) == 64 * (376 + s * 43)
    words = torch.from_numpy(_le.pack(block).view(np.int64).copy()).cuda().repeat(n // 64)
    words = torch.cat([words, torch.zeros(8, dtype=torch.int64, device="cuda")])
    n_words = words.numel()
    cap = n * 2
    phys = torch.tensor([mhz], dtype=torch.int16, device="cuda")
    cands = torch.empty(cap * 3, dtype=torch.int64, device="cuda")
    pre = torch.empty(cap * 2, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    out = torch.zeros(cap, dtype=torch.int32, device="cuda")

    def scan():
        cnt.zero_()
        bt.check(lib.btbbx_le_cfind_scan_device(words.data_ptr(), n_words, n_words, 1, n_words * 64 - 335, phys.data_ptr(), 255, 0, cands.data_ptr(),
                                                None, cap, cnt.data_ptr(), cnt.data_ptr() + 4, pre.data_ptr(), 16 * cap, None),
                 "btbbx_le_cfind_scan_device")

    def symbols():
        bt.check(lib.btbbx_le_ctrack_symbols_device(words.data_ptr(), n_words, n_words, 1, cands.data_ptr(), cnt.data_ptr(), cap, out.data_ptr(), None),
                 "btbbx_le_ctrack_symbols_device")

    scan_ms = timed(scan, args.warmup, args.steps, args.reps)
    n_cands = int(cnt[0].item())
    sym_ms = timed(symbols, args.warmup, args.steps, args.reps)
    scan_ms2 = timed(scan, args.warmup, args.steps, args.reps)
    sym_ms2 = timed(symbols, args.warmup, args.steps, args.reps)
    assert n_cands >= n - 64 and int((out[:n_cands] == 376 + s * 43).sum().item()) >= n - 64, n_cands
    return dict(candidates=n_cands, symbols_ms=[sym_ms, sym_ms2], cfind_ms=[scan_ms, scan_ms2])


def track_bench(lib, args):
    """--conns connections of --events events of one packet, hopping over all data channels, as the grouping would leave them"""
    k, e = args.conns, args.events
    g = np.repeat(np.arange(k, dtype=np.int64), e)
    ev = np.tile(np.arange(e, dtype=np.int64), k)
    interval = 6 + g % 30
    arr = np.zeros(k * e, bt.LE_CAND_DTYPE)
    arr["offset"] = 4000 + 97 * g + ev * interval * 1250
    arr["access_address"] = 0x20000000 + 0x1000 * g
    arr["crc_init"] = (7 * g + 1) & 0xFFFFFF
    ch = ((3 * g) % 37 + (5 + g % 12) * ev) % 37
    arr["stream"] = ch
    arr["header0"] = 1
    arr["length"] = ev % 4
    arr["conn"] = g
    order = np.lexsort((arr["offset"], arr["stream"], g))                   # the grouping's order: connection, stream, offset
    arr = arr[order]
    conns = np.zeros(k, bt.LE_CONN_DTYPE)
    conns["access_address"], conns["crc_init"], conns["n_packets"], conns["first"] = 0x20000000 + 0x1000 * np.arange(k), (7 * np.arange(k) + 1) & 0xFFFFFF, e, e * np.arange(k)
    mhz = np.array([m for m in range(2404, 2480, 2) if m != 2426], np.uint16)
    n = len(arr)
    dev = lambda a: torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).cuda()      # noqa: E731
    d_cands, d_conns, d_phys = dev(arr), dev(conns), dev(mhz)
    d_sym = dev((80 + 8 * arr["length"].astype(np.uint32)).astype(np.uint32))
    d_cnt = torch.tensor([n, k], dtype=torch.int32, device="cuda")
    scratch = lib.btbbx_le_track_scratch_bytes(n, k)
    d_scr = torch.empty(scratch, dtype=torch.uint8, device="cuda")
    outs = [(torch.zeros(48 * k, dtype=torch.uint8, device="cuda"), torch.zeros(16 * n, dtype=torch.uint8, device="cuda")) for _ in range(2)]
    head = (d_cands.data_ptr(), d_cnt.data_ptr(), n, d_conns.data_ptr(), d_cnt.data_ptr() + 4, k, d_phys.data_ptr(), 37)

    def track():
        bt.check(lib.btbbx_le_track_device(*head, 1250, 200, 50, 1, outs[0][0].data_ptr(), outs[0][1].data_ptr(), d_scr.data_ptr(), scratch, None),
                 "btbbx_le_track_device")

    def ctrack():
        bt.check(lib.btbbx_le_ctrack_device(*head, d_sym.data_ptr(), 1250, 200, 50, 1, outs[1][0].data_ptr(), outs[1][1].data_ptr(), d_scr.data_ptr(),
                                            scratch, None), "btbbx_le_ctrack_device")

    ms = dict(track=[], ctrack=[])
    for _ in range(2):                                  # alternating: the parent's tracking, the stand-in, the parent's, the stand-in
        ms["track"].append(timed(track, args.warmup, args.steps, args.reps))
        ms["ctrack"].append(timed(ctrack, args.warmup, args.steps, args.reps))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    timed_conns = int((outs[0][0].cpu().numpy().view(bt.LE_TRACK_DTYPE)["flags"] & 1).sum())
    spread = abs(ms["track"][0][0] - ms["track"][1][0]) / min(ms["track"][0][0], ms["track"][1][0])
    return dict(candidates=n, connections=k, timed=timed_conns, track_ms=ms["track"], ctrack_ms=ms["ctrack"],
                ratio=round(min(x[0] for x in ms["ctrack"]) / min(x[0] for x in ms["track"]), 4), parent_spread=round(spread, 4))


def chain_bench(lib, args):
    n_streams = args.streams
    n_words = int(args.gib * (1 << 30) / 8 / n_streams) // 4096 * 4096
    rng = np.random.default_rng(args.seed)
    words = measure_le.build_capture(args.seed, n_streams, n_words, int(rng.integers(0, 1 << 24)))
    aa, crc_init = ld.good_aa(rng), int(rng.integers(0, 1 << 24))
    planted = plant_connection(words, n_words, n_streams, aa, crc_init, rng)
    phys = torch.tensor([measure_le.mhz_of(s) for s in range(n_streams)], dtype=torch.int16, device="cuda")
    cap, conn_cap, pre_cap = 1 << 20, 1 << 12, args.pre_cap
    pre = torch.zeros(2 * pre_cap, dtype=torch.int64, device="cuda")
    cands = torch.zeros(3 * cap, dtype=torch.int64, device="cuda")
    conns = torch.zeros(4 * cap, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    sym = torch.zeros(cap, dtype=torch.int32, device="cuda")
    tracks, pkts = torch.zeros(6 * conn_cap, dtype=torch.int64, device="cuda"), torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
    sel, sel_pkts = torch.zeros(4 * conn_cap, dtype=torch.int64, device="cuda"), torch.zeros(cap, dtype=torch.int64, device="cuda")
    g_scr = torch.empty(lib.btbbx_le_discover_scratch_bytes(cap), dtype=torch.uint8, device="cuda")
    t_scr = torch.empty(lib.btbbx_le_track_scratch_bytes(cap, conn_cap), dtype=torch.uint8, device="cuda")
    c_scr = torch.empty(lib.btbbx_le_csa2_scratch_bytes(cap, conn_cap), dtype=torch.uint8, device="cuda")
    search_bits = n_words * 64 - 335

    def discover():
        cnt.zero_()
        bt.check(lib.btbbx_le_cfind_scan_device(words.data_ptr(), n_words, n_words, n_streams, search_bits, phys.data_ptr(), 27, 16, cands.data_ptr(),
                                                None, cap, cnt.data_ptr(), cnt.data_ptr() + 4, pre.data_ptr(), 16 * pre_cap, None), "btbbx_le_cfind_scan_device")
        bt.check(lib.btbbx_le_discover_group_device(cands.data_ptr(), cnt.data_ptr(), cap, 2, conns.data_ptr(), conn_cap, cnt.data_ptr() + 8,
                                                    g_scr.data_ptr(), g_scr.numel(), None), "btbbx_le_discover_group_device")

    def chain():
        discover()
        bt.check(lib.btbbx_le_ctrack_symbols_device(words.data_ptr(), n_words, n_words, n_streams, cands.data_ptr(), cnt.data_ptr(), cap, sym.data_ptr(),
                                                    None), "btbbx_le_ctrack_symbols_device")
        bt.check(lib.btbbx_le_ctrack_device(cands.data_ptr(), cnt.data_ptr(), cap, conns.data_ptr(), cnt.data_ptr() + 8, conn_cap, phys.data_ptr(),
                                            n_streams, sym.data_ptr(), 1250, 200, 50, 1, tracks.data_ptr(), pkts.data_ptr(), t_scr.data_ptr(),
                                            t_scr.numel(), None), "btbbx_le_ctrack_device")
        bt.check(lib.btbbx_le_csa2_device(cands.data_ptr(), cnt.data_ptr(), cap, conns.data_ptr(), cnt.data_ptr() + 8, conn_cap, tracks.data_ptr(),
                                          pkts.data_ptr(), 1, sel.data_ptr(), sel_pkts.data_ptr(), c_scr.data_ptr(), c_scr.numel(), None),
                 "btbbx_le_csa2_device")

    d_ms = timed(discover, args.warmup, args.steps, args.reps)
    c_ms = timed(chain, args.warmup, args.steps, args.reps)
    d_ms2 = timed(discover, args.warmup, args.steps, args.reps)
    c_ms2 = timed(chain, args.warmup, args.steps, args.reps)
    counts = cnt.cpu().numpy().tolist()
    assert counts[0] >= planted and counts[1] <= pre_cap and counts[0] <= cap and 1 <= counts[2] <= conn_cap, (counts, planted)
    return dict(gib=round(n_words * 8 * n_streams / (1 << 30), 3), streams=n_streams, planted=planted, candidates=counts[0], connections=counts[2],
                discover_ms=[d_ms, d_ms2], chain_ms=[c_ms, c_ms2], ratio=round(min(c_ms[0], c_ms2[0]) / min(d_ms[0], d_ms2[0]), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--streams", type=int, default=40)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--conns", type=int, default=2000)
    ap.add_argument("--events", type=int, default=250)
    ap.add_argument("--pre-cap", type=int, default=8 << 20)
    ap.add_argument("--skip-chain", action="store_true")
    args = ap.parse_args()
    import bench
    torch.cuda.set_device(0)
    bt.init(2)
    lib = bt.lib()
    rng = np.random.default_rng(args.seed)
    aa, crc_init = ld.good_aa(rng), int(rng.integers(0, 1 << 24))
    symbols = {"S%d_2p%d" % (s, p): symbols_bench(lib, args, s, 1 << p, aa, crc_init) for s in (8, 2) for p in (18, 20)}
    track = track_bench(lib, args)
    line = dict(metric="le_ctrack", seed=args.seed, symbols=symbols, track=track, csrc_sha16=bench.csrc_fingerprint())
    if not args.skip_chain:
        line["chain"] = chain_bench(lib, args)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
