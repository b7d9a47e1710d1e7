#!/usr/bin/env python3
"""LE decryption measurement: btbbx_le_crypt_device beside btbbx_le_data_device over the same list in the same run, and its plaintext
write beside a device-to-device copy of the same number of octets.  The workload is that of tools/measure_le_data.py -- 2 000
connections of 250 events, two packets per connection event, the central's messages of three fragments (27, 27 and one of 5, 27, 100
or 251 octets), the peripheral's one-fragment message of 1 to 27 octets in every second event -- but every connection runs
LL_ENC_REQ / LL_ENC_RSP in its first event and LL_START_ENC_REQ in its second, and every non-empty PDU behind that is encrypted under
the connection's session key with its true counter and a valid MIC.  Decryption reads what stands in the streams, so the packets
are laid out without overlap: one hop increment for all, 37 first channels, two time slots per event and 28 spans of time one
behind the other.  The key table holds 16 keys, connection g uses key g % 16, window is 8.

The ciphertext is made on the device with torch (a table-driven AES over all packets at once; plumbing, not the product) and
checked by the product: every encrypted PDU must come out VERIFIED at skew 0.  The plaintext write cannot be launched alone through
the public entries, so its time is a difference, as tools/measure_le_data.py does for the gather: the stage with room for every
octet less the stage with byte_cap 0.  HIP events, 3 warm-ups and 20 launches per figure, two rounds.  Prints one JSON line:

* crypt_ms, crypt_nobytes_ms, data_ms, copy_ms: both rounds' figures; plain_ms: the difference of the means; crypt_over_data and
  plain_over_copy: the ratios of the means
* aes_blocks: the AES blocks the rules ask of one run (session keys, probes under 16 keys -- a wrong key costs `window` trials per
  probe --, one trial per encrypted PDU, one block per VERIFIED PDU for its first octets, the keystream of every stored fragment);
  aes_blocks_per_s = aes_blocks / crypt_ms
* --once: for a kernel trace: the chain once, the stage `steps` times
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
from measure_le import time_ms  # noqa: E402
from measure_le_track import DATA_MHZ, UNIT  # noqa: E402

LAST = (5, 27, 100, 251)
HOP, N_KEYS, WINDOW = 7, 16, 8
PER_SPAN = 74                                                   # connections that share a span of time: 37 first channels x 2 slots


class Aes:
    """AES-128 over n blocks at once, each under the schedule of its connection: (n, 16) int64 tensors of octets."""

    def __init__(self, schedules, dev):
        self.sbox = torch.tensor(cm.SBOX, dtype=torch.int64, device=dev)
        self.mul2 = torch.tensor(cm._MUL2, dtype=torch.int64, device=dev)
        self.shift = torch.tensor([4 * ((c + r) % 4) + r for c in range(4) for r in range(4)], dtype=torch.int64, device=dev)
        self.rk = torch.tensor(schedules, dtype=torch.int64, device=dev)                       # (connections, 11, 16)

    def __call__(self, conn, x):
        s = x ^ self.rk[conn, 0]
        for r in range(1, 11):
            s = self.sbox[s][:, self.shift]
            if r < 10:
                a = s.view(-1, 4, 4)
                m2 = self.mul2[a]
                m3 = m2 ^ a
                s = torch.stack([m2[..., 0] ^ m3[..., 1] ^ a[..., 2] ^ a[..., 3], a[..., 0] ^ m2[..., 1] ^ m3[..., 2] ^ a[..., 3],
                                 a[..., 0] ^ a[..., 1] ^ m2[..., 2] ^ m3[..., 3], m3[..., 0] ^ a[..., 1] ^ a[..., 2] ^ m2[..., 3]], -1).reshape(-1, 16)
            s = s ^ self.rk[conn, r]
        return s


def ccm(aes, conn, iv, counter, direction, h0, plain, m):
    """Rule 5 over n packets at once: plain (n, 256) octets of which m count -> (n, 256) ciphertext with the MIC behind it."""
    dev, n = plain.device, len(m)
    nonce = torch.cat([(counter[:, None] >> (8 * torch.arange(4, device=dev))) & 0xFF, (direction << 7)[:, None], iv[conn]], 1)
    block = lambda flags, last: torch.cat([torch.full((n, 1), flags, dtype=torch.int64, device=dev), nonce, (last >> 8)[:, None],     # noqa: E731
                                           (last & 0xFF)[:, None]], 1)
    x = aes(conn, block(0x49, m))
    b1 = torch.zeros((n, 16), dtype=torch.int64, device=dev)
    b1[:, 1], b1[:, 2] = 1, h0 & 0xE3
    x = aes(conn, x ^ b1)
    out = torch.zeros((n, 260), dtype=torch.int64, device=dev)
    at = torch.arange(16, device=dev)
    blocks = 0
    for b in range(16):
        sel = torch.nonzero(m > 16 * b).reshape(-1)
        if not len(sel):
            break
        p = plain[sel, 16 * b:16 * b + 16] * ((16 * b + at)[None, :] < m[sel, None])
        x[sel] = aes(conn[sel], x[sel] ^ p)
        out[sel, 16 * b:16 * b + 16] = p ^ aes(conn[sel], block(0x01, torch.full_like(m, b + 1))[sel])
        blocks += 2 * len(sel)
    mic = (x ^ aes(conn, block(0x01, torch.zeros_like(m))))[:, :4]
    out.scatter_(1, m[:, None] + torch.arange(4, device=dev), mic)
    return out[:, :256], blocks + 3 * n


def build(n_conns, n_events, seed, dev):
    """-> cands, conns, words (37, n_words) on the device, keys, the octets of all plaintext messages, what the stage must find."""
    rng = np.random.default_rng(seed)
    per = 2 * n_events
    spans = (n_conns + PER_SPAN - 1) // PER_SPAN
    n_bits = spans * (n_events + 1) * 6 * UNIT + 8192
    n_words = (n_bits + 63) // 64
    cands = np.zeros(n_conns * per, bt.LE_CAND_DTYPE)
    conns = np.zeros(n_conns, bt.LE_CONN_DTYPE)
    keys = [cm.ltk(500 + k) for k in range(N_KEYS)]
    c = np.arange(n_events, dtype=np.int64)
    plain_len = np.zeros((n_conns, per), np.int64)                # per packet in (event, role) order; 0: not encrypted
    payload = torch.zeros((n_conns * per, 256), dtype=torch.int64, device=dev)
    schedules, ivs = [], []
    for g in range(n_conns):
        aa, ci = 0x10000000 + 7919 * g, (104729 * g + 1) & 0xFFFFFF
        ch = (g % 37 + HOP * c) % 37
        at = 3000 + (g // PER_SPAN) * (n_events + 1) * 6 * UNIT + ((g // 37) % 2) * 3 * UNIT + c * 6 * UNIT + rng.integers(-20, 21, n_events)
        third = c % 3
        len_c = np.where(third < 2, 27, np.asarray(LAST)[rng.integers(0, 4, n_events)])
        llid_c = np.where(third == 0, 2, 1)
        len_p = np.where(c % 2 == 0, rng.integers(1, 28, n_events), 0)
        llid_p = np.where(c % 2 == 0, 2, 1)
        plain = np.stack([len_c, len_p], 1)
        plain[:2] = 0
        plain_len[g] = plain.reshape(-1)
        air_c, air_p = np.where(plain[:, 0] > 0, plain[:, 0] + 4, 0), np.where(plain[:, 1] > 0, plain[:, 1] + 4, 0)
        air_c[0], air_p[0], llid_c[0], llid_p[0] = 23, 13, 3, 3   # LL_ENC_REQ, LL_ENC_RSP
        air_c[1], air_p[1], llid_c[1], llid_p[1] = 0, 1, 1, 3     # an empty PDU, LL_START_ENC_REQ
        sn = c & 1                                                   # one packet per role and event, every one new
        off = np.stack([at, at + 80 + 8 * air_c + 150], 1).reshape(-1)
        stream = np.repeat(ch, 2)
        h0 = np.stack([llid_c | sn << 3, llid_p | sn << 3], 1).reshape(-1)
        ln = np.stack([air_c, air_p], 1).reshape(-1)
        assert off[-1] + 80 + 8 * 35 < n_bits and (np.diff(at) > 80 + 8 * 255 + 150 + 80 + 8 * 31 + 40).all()
        skdm, skds, ivm, ivs_ = (bytes(rng.integers(0, 256, k, dtype=np.uint8).tolist()) for k in (8, 8, 4, 4))
        schedules.append(cm._schedule(cm.session_key(keys[g % N_KEYS], skdm, skds)))
        ivs.append(list(ivm + ivs_))
        first = torch.tensor([list(bytes([3]) + bytes(10) + skdm + ivm) + [0] * 233, list(bytes([4]) + skds + ivs_) + [0] * 243,
                              [0] * 256, [5] + [0] * 255], dtype=torch.int64, device=dev)
        payload[g * per:g * per + 4] = first
        part = cands[g * per:(g + 1) * per]                       # in (event, role) order; the list itself is sorted below
        part["offset"], part["stream"], part["header0"], part["length"] = off, stream, h0, ln
        part["access_address"], part["crc_init"], part["conn"] = aa, ci, g
        conns[g] = (aa, ci, per, int((ln == 0).sum()), int(np.bitwise_or.reduce(1 << np.unique(ch))), g * per)
    # every encrypted PDU at once: its counter is its number among its role's encrypted PDUs
    m_all = torch.from_numpy(plain_len.reshape(-1)).to(dev)
    enc = torch.nonzero(m_all > 0).reshape(-1)
    role = enc % 2
    conn = enc // per
    ordinal = torch.from_numpy(np.concatenate([(np.cumsum(plain_len[g].reshape(-1, 2) > 0, 0) - 1).reshape(-1) for g in range(n_conns)])).to(dev)[enc]
    aes = Aes(schedules, dev)
    plain = torch.randint(0, 256, (len(enc), 256), dtype=torch.int64, device=dev)
    h0 = torch.from_numpy(cands["header0"].astype(np.int64)).to(dev)[enc]
    cipher, blocks = ccm(aes, conn, torch.tensor(ivs, dtype=torch.int64, device=dev), ordinal, 1 - role, h0, plain, m_all[enc])
    payload[enc] = cipher
    # into the streams: the payload's bits behind 56 bits of preamble, address and header, whitened from the sequence's 17th bit on
    white = torch.from_numpy(np.stack([_le._whitening_2080(s)[16:16 + 2048] for s in range(37)]).astype(np.int64)).to(dev)
    bits = torch.randint(0, 2, (37 * n_words * 64,), dtype=torch.uint8, device=dev)
    offset = torch.from_numpy(cands["offset"].astype(np.int64)).to(dev)
    stream = torch.from_numpy(cands["stream"].astype(np.int64)).to(dev)
    length = torch.from_numpy(cands["length"].astype(np.int64)).to(dev)
    j = torch.arange(2048, device=dev)
    for lo in range(0, len(cands), 1 << 15):
        hi = min(lo + (1 << 15), len(cands))
        v = ((payload[lo:hi, :, None] >> torch.arange(8, device=dev)) & 1).reshape(hi - lo, 2048) ^ white[stream[lo:hi]]
        keep = j[None, :] < 8 * length[lo:hi, None]
        where = (stream[lo:hi, None] * (64 * n_words) + offset[lo:hi, None] + 56 + j[None, :])[keep]
        bits[where] = v[keep].to(torch.uint8)
    words = torch.empty((37, n_words), dtype=torch.int64, device=dev)
    weights = torch.ones(64, dtype=torch.int64, device=dev) << torch.arange(64, device=dev)
    for s in range(37):
        words[s] = (bits[s * 64 * n_words:(s + 1) * 64 * n_words].view(n_words, 64).to(torch.int64) * weights).sum(1)
    stats = dict(encrypted=len(enc), ccm_blocks=blocks, octets=int(m_all.sum()))
    for g in range(n_conns):                                      # the list as the grouping leaves it: by (stream, offset) per connection
        part = cands[g * per:(g + 1) * per]
        part[:] = part[np.lexsort((part["offset"], part["stream"]))]
    return cands, conns, words, n_words, keys, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conns", type=int, default=2000)
    ap.add_argument("--events", type=int, default=250)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--once", action="store_true", help="for a kernel trace: tracking and data stage once, the stage `steps` times")
    args = ap.parse_args()
    import bench
    torch.cuda.set_device(0)
    bt.init(2)
    lib = bt.lib()
    dev = torch.device("cuda")
    phys = torch.tensor(DATA_MHZ, dtype=torch.int16, device=dev)
    cands, conns, d_words, n_words, keys, stats = build(args.conns, args.events, args.seed, dev)
    n, k, octets = len(cands), len(conns), stats["octets"]
    d_cands, d_conns = torch.from_numpy(cands.view(np.int64)).cuda(), torch.from_numpy(conns.view(np.int64)).cuda()
    d_keys = torch.from_numpy(np.frombuffer(b"".join(keys), np.uint8).copy()).cuda()
    cnt = torch.tensor([n, k, 0, 0, 0, 0, 0, 0, 0, 0], dtype=torch.int32, device=dev)
    zeros = lambda count, dtype=torch.int64: torch.zeros(count, dtype=dtype, device=dev)      # noqa: E731
    d_tracks, d_pkts, d_data, d_dpkts, d_msgs = zeros(6 * k), zeros(2 * n), zeros(6 * k), zeros(3 * n, torch.int32), zeros(4 * n)
    d_crypt, d_cpkts, d_ppkts, d_cmsgs = zeros(7 * k), zeros(2 * n), zeros(3 * n, torch.int32), zeros(4 * n)
    room = octets + 4 * stats["encrypted"] + 64
    d_bytes, d_plain, d_copy = zeros(room, torch.uint8), zeros(room, torch.uint8), zeros(room, torch.uint8)
    sizes = (lib.btbbx_le_track_scratch_bytes(n, k), lib.btbbx_le_data_scratch_bytes(n, k), lib.btbbx_le_crypt_scratch_bytes(n, k, N_KEYS))
    tscratch, dscratch, cscratch = (zeros(b // 8 + 2) for b in sizes)
    p = cnt.data_ptr()

    def track():
        bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), p, n, d_conns.data_ptr(), p + 4, k, phys.data_ptr(), 37, UNIT, 200, 50,
                                           bt.LE_TRACK_REMAP, d_tracks.data_ptr(), d_pkts.data_ptr(), tscratch.data_ptr(), sizes[0], None),
                 "btbbx_le_track_device")

    def data():
        bt.check(lib.btbbx_le_data_device(d_words.data_ptr(), n_words, n_words, 37, phys.data_ptr(), d_cands.data_ptr(), p, n, d_conns.data_ptr(),
                                          p + 4, k, d_tracks.data_ptr(), d_pkts.data_ptr(), d_data.data_ptr(), d_dpkts.data_ptr(),
                                          d_msgs.data_ptr(), n, p + 8, d_bytes.data_ptr(), room, p + 16, dscratch.data_ptr(), sizes[1], None),
                 "btbbx_le_data_device")

    def crypt(byte_cap):
        bt.check(lib.btbbx_le_crypt_device(d_words.data_ptr(), n_words, n_words, 37, phys.data_ptr(), d_cands.data_ptr(), p, n, d_conns.data_ptr(),
                                           p + 4, k, d_tracks.data_ptr(), d_pkts.data_ptr(), d_dpkts.data_ptr(), d_keys.data_ptr(), N_KEYS, WINDOW,
                                           d_crypt.data_ptr(), d_cpkts.data_ptr(), d_ppkts.data_ptr(), d_cmsgs.data_ptr(), n, p + 24,
                                           d_plain.data_ptr(), byte_cap, p + 32, cscratch.data_ptr(), sizes[2], None), "btbbx_le_crypt_device")

    def copy():
        d_copy[:octets].copy_(d_plain[:octets])

    track()
    data()
    crypt(room)
    torch.cuda.synchronize()
    counts = cnt.cpu().numpy()
    n_msgs, n_bytes = int(counts[6:7].view(np.uint32)[0]), int(counts[8:10].view(np.uint64)[0])
    rec = d_crypt.cpu().numpy().view(bt.LE_CRYPT_DTYPE)
    found = dict(keyed=int((rec["flags"] & bt.LE_CRYPT_KEYED != 0).sum()), verified=int(rec["n_verified"].sum()), failed=int(rec["n_failed"].sum()),
                 skipped=int(rec["n_skipped"].sum()), max_skew=int(rec["max_skew"].max()), octets=n_bytes)
    assert (found["keyed"], found["verified"], found["failed"], found["max_skew"]) == (k, stats["encrypted"], 0, 0), (found, stats)
    assert 0.98 * octets < n_bytes <= octets, (found, stats)    # (the central's continuation in front of its first START is an ORPHAN)
    octets = n_bytes
    assert (rec["key"] == np.arange(k) % N_KEYS).all()
    if args.once:
        for _ in range(args.steps):
            crypt(room)
        torch.cuda.synchronize()
        print(json.dumps(dict(metric="le_crypt_once", octets=n_bytes, messages=n_msgs, launches_of_the_stage=args.steps + 1)))
        return
    # what the rules ask: a block per (connection, key); four probes under the right key once and under each wrong
    # key `window` times; a trial per encrypted PDU; a block per VERIFIED PDU; the keystream of every stored fragment
    per_trial = stats["ccm_blocks"] / stats["encrypted"]
    aes_blocks = int(k * N_KEYS + 4 * k * (1 + (N_KEYS - 1) * WINDOW) * per_trial + stats["ccm_blocks"] + stats["encrypted"] +
                     (stats["ccm_blocks"] - 3 * stats["encrypted"]) // 2)
    crypt_ms, nobytes_ms, data_ms, copy_ms = [], [], [], []
    for _ in range(2):
        crypt_ms.append(round(time_ms(lambda: crypt(room), args.warmup, args.steps), 4))
        nobytes_ms.append(round(time_ms(lambda: crypt(0), args.warmup, args.steps), 4))
        data_ms.append(round(time_ms(data, args.warmup, args.steps), 4))
        copy_ms.append(round(time_ms(copy, args.warmup, args.steps), 4))
    plain = (sum(crypt_ms) - sum(nobytes_ms)) / 2
    line = dict(metric="le_crypt", candidates=n, connections=k, keys=N_KEYS, window=WINDOW, encrypted=stats["encrypted"], messages=n_msgs,
                octets=n_bytes, crypt_ms=crypt_ms, crypt_nobytes_ms=nobytes_ms, data_ms=data_ms, copy_ms=copy_ms, plain_ms=round(plain, 4),
                crypt_over_data=round(sum(crypt_ms) / sum(data_ms), 2), plain_over_copy=round(plain / (sum(copy_ms) / 2), 2),
                aes_blocks=aes_blocks, aes_blocks_per_s=round(aes_blocks / (sum(crypt_ms) / 2 * 1e-3)), launches=24, steps=args.steps,
                warmup=args.warmup, device=torch.cuda.get_device_name(0), csrc_sha16=bench.csrc_fingerprint())
    print(json.dumps(line))


if __name__ == "__main__":
    main()
