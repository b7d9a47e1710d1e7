#!/usr/bin/env python3
"""LE address resolution measurement: btbbx_le_resolve_device over 2^20 distinct resolvable private addresses against tables of 1, 64
and 4096 identity resolving keys, and over 2^12 addresses against 4096.  Every record is an ADV_IND with a random RPA of no key, so
every (address, key) pair is one trial of one AES block and none ends early; sixteen more addresses are made under the table's last
key, and the run asserts that they come out on a key that matches them.  The figure is the WHOLE stage (the slot keys, seven radix
passes, ranks, tallies, schedules, trials, records: 32 launches) in HIP events, and the AES blocks per second that follow from it.
The yardstick is the pairing stage's search on tools/measure_le_pair.py's workload, timed in the same process.  Prints one JSON line:

* resolve: per (addresses, keys) the distinct addresses the device counted, the median of `reps` repetitions of `steps` launches each
  in milliseconds, the fastest and the slowest repetition, trials and AES blocks per second (one block per trial) at the median
* pair: tools/measure_le_pair.py's figures for `pair_conns` connections
"""
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

import _le_resolve as rm  # noqa: E402
import libbtbb_amd as bt  # noqa: E402
import measure_le_pair as mp  # noqa: E402
from measure_le import time_ms  # noqa: E402

PLANTED = 16


def records(n_addr, last_key, seed):
    """n_addr ADV_IND records on channel 37 with distinct random RPAs, the last PLANTED of them under last_key."""
    rng = np.random.default_rng(seed)
    a = np.zeros(n_addr, bt.LE_PKT_DTYPE)
    a["offset"] = rng.permutation(n_addr).astype(np.uint64) * 400
    a["crc_ok"], a["channel_idx"], a["length"], a["adv_tx_add"], a["pdu_bytes"] = 1, 37, 6, 1, 8
    body = rng.integers(0, 256, (n_addr, 6), dtype=np.uint8)
    body[:, 5] = (body[:, 5] & 0x3F) | 0x40
    body[:, :4] = np.arange(n_addr, dtype=np.uint32).view(np.uint8).reshape(-1, 4)    # distinct: a[0..3] count up
    planted = [rm.rpa(last_key, 100 + j) for j in range(PLANTED)]
    for j, addr in enumerate(planted):
        body[n_addr - PLANTED + j] = np.frombuffer(addr, np.uint8)
    a["bytes"][:, 4], a["bytes"][:, 5] = 0x40, 6
    a["bytes"][:, 6:12] = body
    return a, planted


def resolve_case(n_addr, n_keys, warmup, steps, reps):
    lib = bt.lib()
    keys = [rm.octets(300000 + j, 16) for j in range(n_keys)]
    adv, planted = records(n_addr, keys[-1], n_addr + n_keys)
    dev = lambda x: torch.from_numpy(np.frombuffer(np.ascontiguousarray(x).tobytes() + bytes(8), np.uint8).copy()).cuda()   # noqa: E731
    d_adv, d_given = dev(adv), dev(np.frombuffer(b"".join(keys), np.uint8))
    cnt = torch.tensor([n_addr, 0, 0, 0], dtype=torch.int32, device="cuda")
    d_slots = torch.zeros(2 * n_addr, dtype=torch.int32, device="cuda")
    d_addrs = torch.zeros(n_addr * bt.LE_ADDR_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_irks = torch.zeros(n_keys * bt.LE_IRK_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    size = lib.btbbx_le_resolve_scratch_bytes(n_addr, 0, n_keys)
    scratch = torch.zeros(size // 8 + 2, dtype=torch.int64, device="cuda")
    p = cnt.data_ptr()

    def run():
        bt.check(lib.btbbx_le_resolve_device(d_adv.data_ptr(), p, n_addr, None, 0, None, None, None, 0, None, 0, d_given.data_ptr(), n_keys,
                                             d_slots.data_ptr(), d_addrs.data_ptr(), n_addr, p + 4, d_irks.data_ptr(), n_keys, p + 8, None,
                                             scratch.data_ptr(), size, None), "btbbx_le_resolve_device")

    run()
    torch.cuda.synchronize()
    n_found, n_irks = int(cnt.cpu()[1]), int(cnt.cpu()[2])
    rec = d_addrs.cpu().numpy().view(bt.LE_ADDR_DTYPE)[:n_found]
    assert n_irks == n_keys and (rec["kind"] == bt.LE_ADDR_RESOLVABLE).all() and int(rec["n_slots"].sum()) == n_addr
    as_int = (rec["addr"].astype(np.uint64) << (8 * np.arange(6, dtype=np.uint64))).sum(axis=1)
    for addr in planted:                                    # on the last key, or on a smaller slot that matches by accident
        at = np.flatnonzero(as_int == int.from_bytes(addr, "little"))
        assert len(at) == 1, addr
        irk = int(rec["irk"][at[0]])
        assert irk <= n_keys - 1 and rm.matches(keys[irk], addr), (addr, irk)
    table = d_irks.cpu().numpy().view(bt.LE_IRK_DTYPE)
    assert int(table["n_addrs"].sum()) == int((rec["irk"] != bt.LE_NO_IRK).sum()) >= PLANTED
    ms = sorted(time_ms(run, warmup if r == 0 else 0, steps) for r in range(reps))
    mid = statistics.median(ms)
    trials = n_found * n_keys
    return dict(addresses=n_addr, keys=n_keys, distinct=n_found, resolved=int(table["n_addrs"].sum()), ms=round(mid, 4), ms_min=round(ms[0], 4),
                ms_max=round(ms[-1], 4), trials_per_s=round(trials / (mid * 1e-3)), aes_blocks_per_s=round(trials / (mid * 1e-3)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=str, nargs="+", default=["1048576x1", "1048576x64", "1048576x4096", "4096x4096"], help="addresses x keys")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--pair-conns", type=int, default=16, help="connections of the pairing search's workload; 0 leaves it out")
    args = ap.parse_args()
    import bench
    torch.cuda.set_device(0)
    bt.init(2)
    cases = [tuple(int(v) for v in c.split("x")) for c in args.cases]
    line = dict(metric="le_resolve", resolve=[resolve_case(n, k, args.warmup, args.steps, args.reps) for n, k in cases], launches=32)
    if args.pair_conns:
        line["pair"] = mp.pair_case(args.pair_conns, args.warmup, args.steps)
    line.update(steps=args.steps, warmup=args.warmup, reps=args.reps, device=torch.cuda.get_device_name(0), csrc_sha16=bench.csrc_fingerprint())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
