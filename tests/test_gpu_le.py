"""Bluetooth LE scan on the GPU (btbbx_le_*) against the test-side model (tests/_le.py) and, for the lell fields, the
compiled reference's lell_allocate_and_decode (oracle/_ref/libbtbb_ref.so, when present).  All captures are generated
from seeds."""
import functools
import time

import numpy as np
import pytest

import _le
import _libs
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu

ADV_MHZ = _le.ADV_MHZ
CONN_AA = 0x50654C3B


@pytest.fixture(scope="module", autouse=True)
def _init():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    bt.init(2)


_mhz_of, _pack, _compare = _le.mhz_of, _le.pack, _le.compare        # (shared with tests/test_gpu_le_lattice.py)


@functools.lru_cache(maxsize=None)
def _wh(chan, n):
    return _le.whitening_bits(chan, n)


def _packet_bits(rng, mhz, adv, length=None, errors=0, corrupt=False, crc_init=_le.ADV_CRC_INIT):
    aa = _le.ADV_AA if adv else CONN_AA
    if length is None:
        length = int(rng.integers(0, 40)) if rng.random() < 0.9 else int(rng.integers(40, 256 if not adv else 256))
    h0 = int(rng.integers(0, 256))
    pdu = _le.make_pdu(h0, rng.integers(0, 256, length, dtype=np.uint8).tobytes())
    bits = _le.tx_bits(aa, _le.channel_index(int(mhz)) & 0x3F, pdu, crc_init).copy()
    if errors:
        bits[rng.choice(40, errors, replace=False)] ^= 1
    if corrupt:
        bits[40 + int(rng.integers(0, 8 * len(pdu) + 24))] ^= 1
    return bits


def _model(words2d, n_words, search_bits, phys, aa, crc_init, max_errors, cache):
    out = []
    for s in range(words2d.shape[0]):
        mkey = ("match", s, aa, search_bits)
        if mkey not in cache:          # (the matches within four errors, filtered per limit below)
            cache[mkey] = _le.match_all(words2d[s], n_words, search_bits, aa, 4)
        off, err, _ = cache[mkey]
        for o, e in zip(off, err):
            if e > max_errors:
                continue
            key = (s, int(o), aa, crc_init)
            if key not in cache:
                cache[key] = _le.decode(words2d[s], n_words, s, int(o), int(e), int(phys[s]), crc_init)
            out.append(cache[key])
    return out


@pytest.fixture(scope="module")
def capture40():
    """40 streams of 2^22 bits: advertising packets on 37 / 38 / 39, one connection's packets on the data channels."""
    rng = np.random.default_rng(_libs.seed(700))
    n_streams, n_bits = 40, 1 << 22
    phys = _mhz_of(n_streams)
    conn_crc = int(rng.integers(0, 1 << 24))
    sym = rng.integers(0, 2, (n_streams, n_bits), dtype=np.uint8)
    for s in range(n_streams):
        adv = s < 3
        crc_init = _le.ADV_CRC_INIT if adv else conn_crc
        pos = 1000
        k = 0
        while pos < n_bits - 30000:
            length = 251 if k % 11 == 5 else None
            b = _packet_bits(rng, phys[s], adv, length=length, errors=k % 6, corrupt=(k % 7 == 3), crc_init=crc_init)
            if adv and k < 16:      # every advertising PDU type
                hdr = _le.octet_bits(bytes([k | (int(rng.integers(0, 4)) << 6), 0]))[:4]
                b = b.copy()
                b[40:44] = hdr ^ _wh(_le.channel_index(int(phys[s])) & 0x3F, 4)
                # (the header changed after the CRC was formed: the CRC fails, the type is still read)
            sym[s, pos:pos + len(b)] = b
            gap = int(rng.integers(10, 39)) if k % 13 == 7 else int(rng.integers(2000, 60000))
            pos += len(b) + gap     # (k % 13 == 7: the next packet starts fewer than 40 bits after this one's end)
            k += 1
        b = _packet_bits(rng, phys[s], adv, length=200, crc_init=crc_init)   # runs off the stream's end
        sym[s, n_bits - 400:] = b[:400]
    words = np.stack([_pack(sym[s]) for s in range(n_streams)])
    return dict(words=words, n_words=n_bits // 64, phys=phys, conn_crc=conn_crc, search_bits=n_bits - 39)


@pytest.mark.parametrize("max_errors", [0, 1, 2, 3, 4])
def test_le_parity_40_streams(capture40, max_errors):
    c = capture40
    ref = _libs.ref()
    cache = c.setdefault("cache", {})
    for aa, crc_init in ((_le.ADV_AA, _le.ADV_CRC_INIT), (CONN_AA, c["conn_crc"])):
        got = bt.le_scan(c["words"], c["search_bits"], c["phys"], aa=aa, crc_init=crc_init, max_errors=max_errors, n_streams=40)
        want = _model(c["words"], c["n_words"], c["search_bits"], c["phys"], aa, crc_init, max_errors, cache)
        _compare(got, want, c["phys"], ref)
        assert len(got) > 50
        if max_errors >= 2:
            assert got["crc_ok"].sum() > 50 and got["truncated"].sum() >= 1
            assert (got["crc_ok"] == 0).sum() > 10


def test_le_device_chain_matches_host_wrapper(capture40):
    import torch
    c = capture40
    lib = bt.lib()
    want = bt.le_scan(c["words"], c["search_bits"], c["phys"], crc_init=_le.ADV_CRC_INIT, max_errors=3, n_streams=40)
    n_words = c["n_words"]
    d_words = torch.from_numpy(c["words"].view(np.int64)).cuda()
    d_phys = torch.from_numpy(c["phys"].astype(np.int16)).cuda()
    cap = 1 << 16
    d_hits = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    scratch_bytes = lib.btbbx_order_hits_scratch_bytes(cap)
    d_scr = torch.zeros((scratch_bytes + 15) // 8 + 2, dtype=torch.int64, device="cuda")
    d_out = torch.zeros(cap * 104 // 8, dtype=torch.int64, device="cuda")
    bt.check(lib.btbbx_le_scan_device(d_words.data_ptr(), n_words, n_words, 40, c["search_bits"], _le.ADV_AA, 3, d_hits.data_ptr(),
                                      cap, d_cnt.data_ptr(), None))
    bt.check(lib.btbbx_order_hits_device(d_hits.data_ptr(), d_cnt.data_ptr(), cap, d_scr.data_ptr(), scratch_bytes, None))
    bt.check(lib.btbbx_le_decode_hits_device(d_words.data_ptr(), n_words, n_words, d_hits.data_ptr(), d_cnt.data_ptr(), cap,
                                             d_phys.data_ptr(), _le.ADV_CRC_INIT, d_out.data_ptr(), None))
    torch.cuda.synchronize()
    n = int(d_cnt[0].item())
    got = d_out.cpu().numpy().view(bt.LE_PKT_DTYPE)[:n]
    assert n == len(want) > 0
    assert got.tobytes() == want.tobytes()


def test_le_overflow(capture40):
    import torch
    c = capture40
    lib = bt.lib()
    full = bt.le_scan(c["words"], c["search_bits"], c["phys"], max_errors=4, n_streams=40)
    n = len(full)
    for cap in (1, 7, n // 3):
        part = bt.le_scan(c["words"], c["search_bits"], c["phys"], max_errors=4, n_streams=40, cap=cap, truncate=True)
        assert len(part) == cap and part.tobytes() == full[:cap].tobytes()
    d_words = torch.from_numpy(c["words"].view(np.int64)).cuda()
    d_hits = torch.zeros(2 * 16, dtype=torch.int64, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    bt.check(lib.btbbx_le_scan_device(d_words.data_ptr(), c["n_words"], c["n_words"], 40, c["search_bits"], _le.ADV_AA, 4,
                                      d_hits.data_ptr(), 16, d_cnt.data_ptr(), None))
    torch.cuda.synchronize()
    assert int(d_cnt[0].item()) == n


@pytest.mark.parametrize("n_streams", [1, 80])
def test_le_seams(n_streams):
    rng = np.random.default_rng(_libs.seed(710 + n_streams))
    n_words, pitch = 3 * 512 + 77, 3 * 512 + 77 + 13
    n_bits = n_words * 64
    search_bits = n_bits - 39 - 5
    phys = _mhz_of(n_streams)
    words = np.zeros((n_streams, pitch), np.uint64)
    conn_crc = 0x3A9C41
    for s in range(n_streams):
        adv = int(phys[s]) in ADV_MHZ
        sym = rng.integers(0, 2, n_bits, dtype=np.uint8)
        # offsets: every residue mod 64 (one per residue, 1600 bits apart), then the lane / wave / tile seams
        spots = [64 * 25 * r + r for r in range(0, 48)]
        spots += [b + d for b in (128 * 7, 8192, 8192 * 3, 32768, 65536) for d in (-40, -39, -20, -1, 0) if b + d >= 0]
        spots += [search_bits - 1]
        spots = sorted(set(p for p in spots if p < search_bits))
        last = -10**9
        for p in spots:
            if p < last:
                continue
            b = _packet_bits(rng, phys[s], adv, length=int(rng.integers(0, 12)), crc_init=_le.ADV_CRC_INIT if adv else conn_crc)
            sym[p:p + len(b)] = b[:n_bits - p]
            last = p + len(b)
        words[s, :n_words] = _pack(sym)
        words[s, n_words:] = rng.integers(0, 1 << 63, pitch - n_words, dtype=np.uint64)   # behind the stream: never read
    total = 0
    for aa, crc_init in ((_le.ADV_AA, _le.ADV_CRC_INIT), (CONN_AA, conn_crc)):
        got = bt.le_scan(words, search_bits, phys, aa=aa, crc_init=crc_init, max_errors=2, n_streams=n_streams, pitch_words=pitch,
                         n_words=n_words)
        want = _model(words, n_words, search_bits, phys, aa, crc_init, 2, {})
        _compare(got, want, phys)
        total += int(got["crc_ok"].sum())
    assert total >= (10 if n_streams == 1 else 100)       # (one stream: an advertising channel, the connection AA finds nothing)


def test_le_adversarial_alternating_stream():
    """Alternating bits (the preamble matches at every offset) with advertising AAs back to back."""
    rng = np.random.default_rng(_libs.seed(720))
    n_bits = 1 << 20
    sym = (np.arange(n_bits) & 1).astype(np.uint8)
    aa_bits = _le.octet_bits(_le.ADV_AA.to_bytes(4, "little"))
    pos = 5000
    while pos < n_bits - 40000:
        reps = int(rng.integers(1, 200))
        run = np.tile(aa_bits, reps)
        sym[pos:pos + len(run)] = run
        pos += len(run) + int(rng.integers(100, 5000))
    words = _pack(sym)[None, :]
    t0 = time.time()
    got = bt.le_scan(words, n_bits - 39, [2402], max_errors=4, n_streams=1, cap=1 << 21)
    took = time.time() - t0
    want = _model(words, n_bits // 64, n_bits - 39, [2402], _le.ADV_AA, _le.ADV_CRC_INIT, 4, {})
    _compare(got, want, [2402])
    assert took < 30, took


def test_le_one_gib_capture():
    rng = np.random.default_rng(_libs.seed(730))
    n_words = 1 << 27                       # 1 GiB
    slot_words = 1024                       # one packet per 65536 bits
    words = rng.integers(0, 1 << 63, n_words, dtype=np.uint64) ^ (rng.integers(0, 2, n_words, dtype=np.uint64) << np.uint64(63))
    w2 = words.reshape(-1, slot_words)
    n_slots = w2.shape[0]
    lib_n = 32
    entries = []
    for k in range(lib_n):                  # 32 distinct packets at distinct bit phases
        phase = int(rng.integers(0, 64))
        b = _packet_bits(rng, 2426, True, length=int(rng.integers(0, 60)))
        sym = np.zeros(64 * 64, np.uint8)
        msk = np.zeros(64 * 64, np.uint8)
        sym[phase:phase + len(b)] = b
        msk[phase:phase + len(b)] = 1
        entries.append((phase, _pack(sym), _pack(msk)))
    which = np.arange(n_slots) % lib_n
    planted = []
    for k, (phase, pw, pm) in enumerate(entries):
        rows = np.nonzero(which == k)[0]
        seg = w2[rows, 100:164]
        w2[rows, 100:164] = (seg & ~pm) | pw
        planted.append(rows.astype(np.uint64) * np.uint64(slot_words * 64) + np.uint64(100 * 64 + phase))
    planted = np.sort(np.concatenate(planted))
    search_bits = n_words * 64 - 39
    got = bt.le_scan(words, search_bits, [2426], max_errors=2, cap=1 << 19)
    offs = got["offset"]
    idx = np.searchsorted(offs, planted)
    assert (idx < len(offs)).all() and (offs[idx] == planted).all()
    assert got["crc_ok"][idx].all()
    for first in (0, n_words * 64 // 2 + 12345, search_bits - (1 << 20)):
        fw = first // 64
        sl = words[fw:fw + (1 << 20) // 64 + 2]
        lo = first - 64 * fw
        off, _, _ = _le.match_all(sl, len(sl), lo + (1 << 20), _le.ADV_AA, 2)
        want = int((off >= lo).sum())
        have = int(((offs >= first) & (offs < first + (1 << 20))).sum())
        assert have == want
