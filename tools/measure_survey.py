"""Times of the piconet survey (btbbx_survey_hits_device) on cuda:0.

Shapes (both built in HBM by btbbx_synth_device, two streams of --words words each):
  config3     stream 0 carries one LAP every 512 symbols (one piconet owning 2^20 hits at the default size), stream 1 a random LAP
              every 8192 symbols (2^16 singletons)
  singletons  the headline's shape: a random LAP every 4096 symbols on both streams (--words 268435456 = 4 GiB in all)
The generator's packets are a sync word followed by noise: almost none carries a header, so the walk has next to nothing to
visit; what a walked packet costs is timed by tests/test_gpu_survey.py's never-settling capture.

Modes, one JSON line each:
  (default)          HIP events, 3 warm-ups and --launches launches: survey_ms and chain_ms (ordered scan + survey) as
                     [median, min, max], hits, piconets, csrc_sha16
  --profile-run N    one scan, then N survey calls and nothing else: the program to put behind
                     `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/measure_survey.py --profile-run N`
  --kernel-stats CSV --profile-run N
                     no GPU: reads that run's *kernel_stats.csv and prints the survey stage split in ms per call --
                     sort / group table + channel map (one kernel does both) / gather + trials + header flags / walk list / walk
  --baselines        the two other routes, per packet, on 10^4 packets each of (a) this shape's first hits and (b) a piconet of
                     header-bearing packets that never settles (tests/_survey.py capture_oops): the compiled reference's loop
                     (oracle/_ref, one thread, only the library calls are timed) and the drop-in survey mode through
                     libbtbb_amd.so (btbb_find_ac + btbb_packet_set_data + btbb_process_packet per packet)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=("config3", "singletons"), default="config3")
    ap.add_argument("--words", type=int, default=1 << 23, help="words per stream (2^23 = 2^29 symbols)")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--profile-run", type=int, default=0)
    ap.add_argument("--kernel-stats")
    ap.add_argument("--baselines", action="store_true")
    args = ap.parse_args()
    if args.kernel_stats:
        return stage_split(args.kernel_stats, args.profile_run)
    import torch
    import bench
    import libbtbb_amd as bt
    lib = bt.lib()
    torch.cuda.set_device(0)
    bt.init(2)
    n_words, n_streams = args.words, 2
    words = torch.empty(n_streams * n_words, dtype=torch.int64, device="cuda")
    fixed = 0x5A7C31 if args.shape == "config3" else -1
    strides = (512, 8192) if fixed >= 0 else (4096, 4096)
    bt.check(lib.btbbx_synth_device(words.data_ptr(), 0, n_words, 7, strides[0], fixed, 3, None))
    bt.check(lib.btbbx_synth_device(words.data_ptr() + 8 * n_words, 0, n_words, 8, strides[1], -1, 3, None))
    search_bits = n_words * 64 - 63
    cap = int(n_words * 64 / strides[0] + n_words * 64 / strides[1]) + 65536
    hits = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    ob = lib.btbbx_scan_ordered_scratch_bytes(search_bits, n_streams, bt.LAP_ANY, cap)
    sb = lib.btbbx_survey_scratch_bytes(cap)
    order = torch.empty(ob // 8 + 2, dtype=torch.int64, device="cuda")
    scratch = torch.empty(sb // 8 + 2, dtype=torch.int64, device="cuda")
    recs = torch.empty(cap * 8, dtype=torch.int64, device="cuda")
    entry = np.zeros(1, bt.PKTIN_DTYPE)
    entry["flags"] = 1
    q = torch.cuda.current_stream().cuda_stream

    def scan():
        bt.check(lib.btbbx_scan_ordered_device(words.data_ptr(), n_words, n_words, n_streams, search_bits, bt.LAP_ANY, 2, hits.data_ptr(), cap,
                                               cnt.data_ptr(), order.data_ptr(), ob, q))

    def survey():
        bt.check(lib.btbbx_survey_hits_device(words.data_ptr(), n_words, n_words, n_streams, hits.data_ptr(), cnt.data_ptr(), cap, None,
                                              bt._ptr(entry), 625, 0, bt.MAX_SYMBOLS, recs.data_ptr(), cap, cnt.data_ptr() + 4, None,
                                              scratch.data_ptr(), sb, q))

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.launches):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return [round(float(x), 4) for x in (np.median(out), min(out), max(out))]

    scan()
    torch.cuda.synchronize()
    if args.profile_run:
        for _ in range(args.profile_run):
            survey()
        torch.cuda.synchronize()
        return
    if args.baselines:
        n_hits = int(cnt.cpu().numpy()[0])
        first = hits.cpu().numpy().view(bt.HIT_DTYPE)[:n_hits]
        first = first[(first["stream"] == 0) & (first["offset"] < (1 << 24))][:10000]
        line = np.ascontiguousarray(words[:(1 << 18) + 64].cpu().numpy().view(np.uint64))
        return baselines(args.shape, first, synth_line=line)
    survey_ms = timed(survey)
    chain_ms = timed(lambda: (scan(), survey()))
    n_hits, n_pn = (int(x) for x in cnt.cpu().numpy()[:2])
    r = recs.cpu().numpy().view(bt.SURVEY_DTYPE)[:n_pn]
    assert int(r["n_packets"].sum()) == n_hits and (np.diff(r["lap"].astype(np.int64)) > 0).all()
    print(json.dumps(dict(shape=args.shape, words_per_stream=n_words, hits=n_hits, piconets=n_pn, largest=int(r["n_packets"].max()),
                          walked=int(r["n_walked"].sum()), survey_ms=survey_ms, chain_ms=chain_ms, launches=args.launches,
                          scratch_mib=round(sb / 2**20, 1), csrc_sha16=bench.csrc_fingerprint())))


STAGES = (("sort", ("survey_key", "survey_hist", "survey_rows", "survey_scatter")),
          ("group_table_and_channel_map", ("survey_mark", "survey_tiles", "survey_group")),
          ("gather_trials_header_flags", ("gather_kernel", "trials_", "header_flags")),
          ("walk_list", ("survey_wmark", "survey_wtiles", "survey_wlist")),
          ("walk", ("survey_walk",)))


def stage_split(path, calls):
    import csv
    assert calls > 0, "--profile-run N: the number of survey calls the profiled run made"
    ms = {name: 0.0 for name, _ in STAGES}
    kernels = {}
    for r in csv.DictReader(open(path)):
        for name, pats in STAGES:
            if any(p in r["Name"] for p in pats):
                ms[name] += float(r["TotalDurationNs"]) / 1e6 / calls
                kernels[r["Name"].split("(")[0]] = round(float(r["TotalDurationNs"]) / 1e6 / calls, 4)
    print(json.dumps(dict(ms_per_survey_call={k: round(v, 4) for k, v in ms.items()}, sum_ms=round(sum(ms.values()), 4),
                          kernels_ms=kernels, calls=calls)))


def baselines(shape, first_hits, synth_line):
    import ctypes as C
    import time
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _survey as sv
    import libbtbb_amd as bt
    from libbtbb_amd import synth
    oops, kw = sv.capture_oops(n_same=10000)
    oops_hits = oops.hits()[:10000]
    sets = {shape + "_first_hits": [(h, np.ascontiguousarray(synth.unpack_bits(synth_line[int(h["offset"]) // 64:int(h["offset"]) // 64 + 51])
                                                                [int(h["offset"]) % 64:][:bt.MAX_SYMBOLS])) for h in first_hits],
            "never_settling": [(h, sv.packet_symbols(oops, h, kw["max_length"])) for h in oops_hits]}
    out = {}
    ref = sv.ReferenceEngine()
    with sv._Stdout():
        for name, pkts in sets.items():
            pns, spent = {}, 0
            for h, sym in pkts:
                lap = int(h["lap"])
                pn = pns.get(lap) or pns.setdefault(lap, ref.piconet(lap))
                p = ref.packet(lap, int(h["ac_errors"]), sym, 0, int(h["offset"]) // 625)
                t0 = time.perf_counter_ns()
                ref.channel_seen(pn, 0)
                if ref.header_present(p) and not ref.flag(pn, sv.UAP_VALID):
                    ref.uap_from_header(p, pn)
                spent += time.perf_counter_ns() - t0
                ref.free_packet(p)
            out["reference_us_per_packet_" + name] = round(spent / 1e3 / max(len(pkts), 1), 3)
        lib = bt.lib()
        lib.btbb_init_survey()
        for name, pkts in sets.items():
            spent = 0
            for h, sym in pkts:
                buf = np.ascontiguousarray(np.concatenate([sym, np.zeros(64, np.uint8)]))
                pkt = C.c_void_p(None)
                t0 = time.perf_counter_ns()
                at = lib.btbb_find_ac(bt._ptr(buf), 1, bt.LAP_ANY, 2, C.byref(pkt))
                if at == 0:
                    lib.btbb_packet_set_data(pkt, bt._ptr(sym), len(sym), 0, (int(h["offset"]) // 625) << 1)
                    lib.btbb_process_packet(pkt, None)
                spent += time.perf_counter_ns() - t0
                if pkt:
                    lib.btbb_packet_unref(pkt)
            out["drop_in_us_per_packet_" + name] = round(spent / 1e3 / max(len(pkts), 1), 3)
    out["packets"] = {k: len(v) for k, v in sets.items()}
    import bench
    out["csrc_sha16"] = bench.csrc_fingerprint()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
