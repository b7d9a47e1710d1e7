#!/usr/bin/env python3
"""LE legacy pairing key recovery measurement: btbbx_le_pair_device for 1, 16 and 256 ARMED connections at tk_limit 1 000 000.
Every connection carries one whole exchange (tests/_le_pair.py's exchange) whose passkey is 999999, so no trial is skipped and
every one of the million values is tried per connection; both checks exist, the second runs only after the first held, so a trial is
one key schedule and two AES blocks.  The run asserts that every connection comes out CRACKED at 999999 with its STK in the table.
For scale, btbbx_le_crypt_device over tools/measure_le_crypt.py's default workload is timed in the same run.  HIP events, 3
warm-ups and 20 launches per figure.  Prints one JSON line:

* pair: per number of connections the stage's milliseconds, trials per second, AES blocks per second (two per trial) and key
  schedules per second (one per trial), counted separately
* crypt_ms, crypt_aes_blocks_per_s: the decryption stage, as tools/measure_le_crypt.py counts its blocks
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

import _le_data as dm  # noqa: E402
import _le_pair as pm  # noqa: E402
import libbtbb_amd as bt  # noqa: E402
import measure_le_crypt as mc  # noqa: E402
from measure_le import time_ms  # noqa: E402
from measure_le_track import DATA_MHZ, UNIT  # noqa: E402

TK, TK_LIMIT, KEY_CAP = 999999, 1000000, 64


def pair_case(n_conns, warmup, steps):
    lib = bt.lib()
    plant = pm.Plant()
    seeds = [pm.seed_of(g) for g in range(n_conns)]
    for g in range(n_conns):
        plant.all(g, pm.exchange(TK, seeds[g], n=g)[0])
    a = np.zeros(n_conns, bt.LE_SEED_DTYPE)
    for g, s in enumerate(seeds):
        a[g]["init_a"], a[g]["adv_a"] = np.frombuffer(s.init_a, np.uint8), np.frombuffer(s.adv_a, np.uint8)
        a[g]["tx_add"], a[g]["rx_add"], a[g]["flags"] = s.tx_add, s.rx_add, s.flags
    dev = lambda x: torch.from_numpy(np.frombuffer(np.ascontiguousarray(x).tobytes() + bytes(8), np.uint8).copy()).cuda()   # noqa: E731
    d_seeds, d_msgs, d_bytes = dev(a), dev(dm.msg_array(plant.msgs, bt.LE_MSG_DTYPE)), dev(np.frombuffer(bytes(plant.payload), np.uint8))
    cnt = torch.tensor([n_conns, len(plant.msgs), 0, 0], dtype=torch.int32, device="cuda")
    d_pairs = torch.zeros(n_conns * bt.LE_PAIR_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_keys = torch.zeros(16 * KEY_CAP, dtype=torch.uint8, device="cuda")
    size = lib.btbbx_le_pair_scratch_bytes(n_conns)
    scratch = torch.zeros(size // 8 + 2, dtype=torch.int64, device="cuda")
    p = cnt.data_ptr()

    def run():
        bt.check(lib.btbbx_le_pair_device(p, n_conns, d_seeds.data_ptr(), d_msgs.data_ptr(), p + 4, len(plant.msgs), d_bytes.data_ptr(),
                                          len(plant.payload), TK_LIMIT, d_pairs.data_ptr(), d_keys.data_ptr(), KEY_CAP, p + 8, scratch.data_ptr(),
                                          size, None), "btbbx_le_pair_device")

    run()
    torch.cuda.synchronize()
    rec = d_pairs.cpu().numpy().view(bt.LE_PAIR_DTYPE)
    assert (rec["tk"] == TK).all() and (rec["flags"] == 0xFF).all() and int(cnt.cpu()[2]) == n_conns, rec[:4]
    want = [pm.s1(TK, *pm.exchange(TK, seeds[g], n=g)[1:]) for g in range(min(n_conns, KEY_CAP))]
    assert d_keys.cpu().numpy()[:16 * len(want)].tobytes() == b"".join(want)
    ms = time_ms(run, warmup, steps)
    trials = n_conns * TK_LIMIT
    return dict(connections=n_conns, ms=round(ms, 4), trials_per_s=round(trials / (ms * 1e-3)), aes_blocks_per_s=round(2 * trials / (ms * 1e-3)),
                key_schedules_per_s=round(trials / (ms * 1e-3)))


def crypt_scale(warmup, steps):
    """btbbx_le_crypt_device over tools/measure_le_crypt.py's default workload, set up as that tool sets it up."""
    lib = bt.lib()
    dev = torch.device("cuda")
    phys = torch.tensor(DATA_MHZ, dtype=torch.int16, device=dev)
    cands, conns, d_words, n_words, keys, stats = mc.build(2000, 250, 2024, dev)
    n, k = len(cands), len(conns)
    d_cands, d_conns = torch.from_numpy(cands.view(np.int64)).cuda(), torch.from_numpy(conns.view(np.int64)).cuda()
    d_keys = torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).copy()).cuda()
    cnt = torch.tensor([n, k, 0, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)
    zeros = lambda count, dtype=torch.int64: torch.zeros(count, dtype=dtype, device=dev)      # noqa: E731
    d_tracks, d_pkts, d_data, d_dpkts, d_msgs = zeros(6 * k), zeros(2 * n), zeros(6 * k), zeros(3 * n, torch.int32), zeros(4 * n)
    d_crypt, d_cpkts, d_ppkts, d_cmsgs = zeros(7 * k), zeros(2 * n), zeros(3 * n, torch.int32), zeros(4 * n)
    room = stats["octets"] + 4 * stats["encrypted"] + 64
    d_bytes, d_plain = zeros(room, torch.uint8), zeros(room, torch.uint8)
    sizes = (lib.btbbx_le_track_scratch_bytes(n, k), lib.btbbx_le_data_scratch_bytes(n, k), lib.btbbx_le_crypt_scratch_bytes(n, k, mc.N_KEYS))
    tscratch, dscratch, cscratch = (zeros(b // 8 + 2) for b in sizes)
    p = cnt.data_ptr()
    bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), p, n, d_conns.data_ptr(), p + 4, k, phys.data_ptr(), 37, UNIT, 200, 50,
                                       bt.LE_TRACK_REMAP, d_tracks.data_ptr(), d_pkts.data_ptr(), tscratch.data_ptr(), sizes[0], None), "track")
    bt.check(lib.btbbx_le_data_device(d_words.data_ptr(), n_words, n_words, 37, phys.data_ptr(), d_cands.data_ptr(), p, n, d_conns.data_ptr(),
                                      p + 4, k, d_tracks.data_ptr(), d_pkts.data_ptr(), d_data.data_ptr(), d_dpkts.data_ptr(), d_msgs.data_ptr(),
                                      n, p + 8, d_bytes.data_ptr(), room, p + 16, dscratch.data_ptr(), sizes[1], None), "data")

    def crypt():
        bt.check(lib.btbbx_le_crypt_device(d_words.data_ptr(), n_words, n_words, 37, phys.data_ptr(), d_cands.data_ptr(), p, n, d_conns.data_ptr(),
                                           p + 4, k, d_tracks.data_ptr(), d_pkts.data_ptr(), d_dpkts.data_ptr(), d_keys.data_ptr(), mc.N_KEYS,
                                           mc.WINDOW, d_crypt.data_ptr(), d_cpkts.data_ptr(), d_ppkts.data_ptr(), d_cmsgs.data_ptr(), n, p + 24,
                                           d_plain.data_ptr(), room, p + 32, cscratch.data_ptr(), sizes[2], None), "btbbx_le_crypt_device")

    crypt()
    torch.cuda.synchronize()
    rec = d_crypt.cpu().numpy().view(bt.LE_CRYPT_DTYPE)
    assert int(rec["n_verified"].sum()) == stats["encrypted"] and int(rec["n_failed"].sum()) == 0
    per_trial = stats["ccm_blocks"] / stats["encrypted"]
    aes_blocks = int(k * mc.N_KEYS + 4 * k * (1 + (mc.N_KEYS - 1) * mc.WINDOW) * per_trial + stats["ccm_blocks"] + stats["encrypted"] +
                     (stats["ccm_blocks"] - 3 * stats["encrypted"]) // 2)
    ms = time_ms(crypt, warmup, steps)
    return round(ms, 4), round(aes_blocks / (ms * 1e-3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conns", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-crypt", action="store_true", help="leave out the decryption stage's figure")
    args = ap.parse_args()
    import bench
    torch.cuda.set_device(0)
    bt.init(2)
    line = dict(metric="le_pair", tk_limit=TK_LIMIT, tk=TK, pair=[pair_case(n, args.warmup, args.steps) for n in args.conns], launches=12)
    if not args.no_crypt:
        line["crypt_ms"], line["crypt_aes_blocks_per_s"] = crypt_scale(args.warmup, args.steps)
    line.update(steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(0), csrc_sha16=bench.csrc_fingerprint())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
