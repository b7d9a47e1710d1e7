"""The LE connection discovery (libbtbb_amd/csrc/le_discover.h) on the GPU: le_disc_scan_kernel on the lattice of
tests/_le_discover.py -- every bit phase, the seams of lane, wave and tile, the stream's end, search_bits, and the branch points
of the six rules of a candidate --, the grouping chain on hand-built candidate lists, and the whole chain on a capture of three
hopping connections.  Every expectation is the model's (tests/_le_discover.py); every found CRCInit is also handed to
btbbx_le_decode_hits_device, which must report a good CRC.  Output buffers start as 0xA5, so a byte a kernel leaves unwritten,
or writes where it should not, shows."""
import numpy as np
import pytest

import _le
import _le_discover as ld
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu

CAND, CONN = bt.LE_CAND_DTYPE, bt.LE_CONN_DTYPE


@pytest.fixture(scope="module", autouse=True)
def _init():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    bt.init(2)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    pad = (-a.nbytes) % 8
    raw = np.frombuffer(a.tobytes() + bytes(pad), np.int64).copy() if a.nbytes else np.zeros(1, np.int64)
    return torch.from_numpy(raw).cuda()


def _filled(nbytes):
    import torch
    return torch.full(((nbytes + 7) // 8 * 8 + 8,), 0xA5, dtype=torch.uint8, device="cuda")


def _scan_launch(cap, max_len, cand_cap, d_words, d_phys, d_cands, d_cnt):
    bt.check(bt.lib().btbbx_le_discover_scan_device(d_words.data_ptr(), cap.n_words, cap.pitch_words, len(cap.mhz), cap.search_bits,
                                                    d_phys.data_ptr(), max_len, d_cands.data_ptr(), cand_cap, d_cnt.data_ptr(), None),
             "btbbx_le_discover_scan_device")


def _scan_device(cap, max_len, cand_cap, alloc):
    """One scan launch -> (the counter, all `alloc` records of a buffer that was 0xA5)."""
    import torch
    d_words, d_phys = _dev(cap.words.reshape(-1)), _dev(cap.mhz.astype(np.uint16))
    d_cands = _filled(alloc * CAND.itemsize)
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    _scan_launch(cap, max_len, cand_cap, d_words, d_phys, d_cands, d_cnt)
    torch.cuda.synchronize()
    return int(d_cnt[0].item()) & 0xFFFFFFFF, d_cands.cpu().numpy()[:alloc * CAND.itemsize].view(CAND)


def _decode_crc_ok(cap, cands):
    """btbbx_le_decode_hits_device over the candidates, one launch per CRCInit -> crc_ok of each."""
    import torch
    lib = bt.lib()
    d_words, d_phys = _dev(cap.words.reshape(-1)), _dev(cap.mhz.astype(np.uint16))
    ok = {}
    by_init = {}
    for c in cands:
        by_init.setdefault(c.crc_init, []).append(c)
    for init, members in by_init.items():
        hits = np.zeros(len(members), bt.HIT_DTYPE)
        for i, c in enumerate(members):
            hits[i] = (c.offset, c.access_address, 0, 0, c.stream)
        d_hits = _dev(hits)
        d_cnt = torch.from_numpy(np.array([len(members), 0], np.int32)).cuda()
        d_out = torch.zeros(len(members) * bt.LE_PKT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        bt.check(lib.btbbx_le_decode_hits_device(d_words.data_ptr(), cap.n_words, cap.pitch_words, d_hits.data_ptr(), d_cnt.data_ptr(),
                                                 len(members), d_phys.data_ptr(), init, d_out.data_ptr(), None))
        torch.cuda.synchronize()
        out = d_out.cpu().numpy().view(bt.LE_PKT_DTYPE)
        for c, o in zip(members, out):
            assert int(o["pdu_bytes"]) == 2 + c.length and int(o["access_address"]) == c.access_address, (c, o)
            ok[c] = int(o["crc_ok"])
    return ok


@pytest.mark.parametrize("max_len", [0, 27, 255])
@pytest.mark.parametrize("tight", [False, True])
def test_scan_on_the_lattice(max_len, tight):
    cap = ld.scan_lattice(max_len, tight)
    want = ld.lattice_model(max_len, tight)
    alloc = len(want) + 64
    count, recs = _scan_device(cap, max_len, alloc, alloc + 1)
    got = ld.cand_tuples(recs[:min(count, alloc)])
    print("max_len %d, tight %d: %d candidates, %d of them planted, model %d" % (
        max_len, tight, count, sum(ld.plant_expected(cap, p) for p in cap.planted), len(want)))
    assert count == len(want) and len(set(got)) == len(got)
    assert set(got) == set(want), (sorted(set(got) - set(want))[:3], sorted(set(want) - set(got))[:3])
    assert recs[count:].tobytes() == b"\xa5" * (CAND.itemsize * (alloc + 1 - count))
    found = {(c.stream, c.offset) for c in got}
    for p in cap.planted:
        assert ((p.stream, p.offset) in found) == ld.plant_expected(cap, p), p
    crc_ok = _decode_crc_ok(cap, got)
    assert all(crc_ok[c] == 1 for c in got), [c for c in got if crc_ok[c] != 1][:3]


def test_scan_overflow_counts_every_candidate():
    cap = ld.scan_lattice(27, False)
    want = set(ld.lattice_model(27, False))
    for cand_cap in (0, 1, 63, 64, 65, len(want) - 1):
        count, recs = _scan_device(cap, 27, cand_cap, cand_cap + 2)
        assert count == len(want), cand_cap
        got = ld.cand_tuples(recs[:cand_cap])
        assert len(set(got)) == cand_cap and set(got) <= want, cand_cap
        assert recs[cand_cap:].tobytes() == b"\xa5" * (2 * CAND.itemsize), cand_cap


# ---- the grouping chain on hand-built lists ---------------------------------------------------------------------------
def _group_device(cands, min_count, conn_cap=None, count=None, cand_cap=None):
    """btbbx_le_discover_group_device over a candidate list -> (the connection counter, conns buffer, cands buffer), the two
    buffers whole, one record longer than their caps, and 0xA5 where nothing was written."""
    import torch
    lib = bt.lib()
    arr = ld.cand_array(cands, CAND)
    n = len(arr)
    count = n if count is None else count
    cand_cap = n if cand_cap is None else cand_cap
    conn_cap = n + 1 if conn_cap is None else conn_cap
    d_cands = _filled((max(cand_cap, n) + 1) * CAND.itemsize)
    if n:
        d_cands[:arr.nbytes] = torch.from_numpy(np.frombuffer(arr.tobytes(), np.uint8).copy()).cuda()
    d_conns = _filled((conn_cap + 1) * CONN.itemsize)
    d_cnt = torch.from_numpy(np.array([count, 0xA5A5A5A5 - (1 << 32), 0, 0], np.int64).astype(np.int32)).cuda()
    scratch = lib.btbbx_le_discover_scratch_bytes(cand_cap)
    d_scr = torch.zeros(scratch // 8 + 2, dtype=torch.int64, device="cuda")
    bt.check(lib.btbbx_le_discover_group_device(d_cands.data_ptr(), d_cnt.data_ptr(), cand_cap, min_count, d_conns.data_ptr(), conn_cap,
                                                d_cnt.data_ptr() + 4, d_scr.data_ptr(), scratch, None), "btbbx_le_discover_group_device")
    torch.cuda.synchronize()
    return (int(d_cnt[1].item()) & 0xFFFFFFFF, d_conns.cpu().numpy()[:(conn_cap + 1) * CONN.itemsize].view(CONN),
            d_cands.cpu().numpy()[:(max(cand_cap, n) + 1) * CAND.itemsize].view(CAND))


def _check_group(cands, min_count, conn_cap=None, count=None, cand_cap=None):
    n = len(cands)
    work = min(n if count is None else count, n if cand_cap is None else cand_cap)
    want_conns, want_cands = ld.group(list(cands[:work]), min_count)
    n_conns, conns, out = _group_device(cands, min_count, conn_cap, count, cand_cap)
    assert n_conns == len(want_conns), (n_conns, len(want_conns))
    kept = len(want_conns) if conn_cap is None else min(conn_cap, len(want_conns))
    assert conns[:kept].tobytes() == ld.conn_array(want_conns[:kept], CONN).tobytes()
    assert conns[kept:].tobytes() == b"\xa5" * (CONN.itemsize * (len(conns) - kept))
    assert out[:work].tobytes() == ld.cand_array(want_cands, CAND).tobytes()
    assert out[work:n].tobytes() == ld.cand_array(cands[work:], CAND).tobytes()              # (beyond the count: as it was)
    assert out[n:].tobytes() == b"\xa5" * (CAND.itemsize * (len(out) - n))
    return want_conns


def _hand_list(min_count):
    """Groups at min_count - 1 and min_count; keys that differ in one bit of every radix digit; one AA under two CRCInits and one
    CRCInit under two AAs; ties in (key, stream) with descending input offsets; streams and offsets in every digit of the first sort."""
    rng = np.random.default_rng(5)
    c = ld.Cand
    out = []
    base_aa, base_ci = 0x52A3C6D1, 0x3B5A17

    def members(aa, ci, n):
        for k in range(n):
            s = (0, 1, 256, 65535, 7)[k % 5]
            o = (5, 1 << 33, (1 << 40) - 1, 300, 1 << 17)[(k + aa) % 5] + k
            out.append(c(o, aa, ci, s, 1 + (k & 1), (0, 3, 0, 27)[k & 3], (k * 5 + aa) % 37))

    members(base_aa, base_ci, min_count)
    for d in range(3):
        members(base_aa, base_ci ^ (1 << (8 * d)), min_count if d != 1 else max(min_count - 1, 0))
    for d in range(4):
        members(base_aa ^ (1 << (8 * d)), base_ci, min_count + (d & 1))
    members(base_aa ^ (1 << 31), base_ci, min_count)
    members(base_aa ^ (1 << 31), base_ci ^ 0x800000, min_count - 1)
    members(0x00000001, 0x000000, min_count)
    members(0xFFFFFFFE, 0xFFFFFF, min_count)
    # ties in (key, stream): one stream, offsets descending in the list
    for k in range(2 * min_count + 1):
        out.append(c(90000 - 13 * k, 0x6B7D9A35, 0x010203, 9, 1, k & 1, 20))
    order = rng.permutation(len(out) - (2 * min_count + 1))
    return [out[i] for i in order] + out[len(order):]


@pytest.mark.parametrize("min_count", [1, 2, 3])
def test_group_on_hand_built_lists(min_count):
    lst = _hand_list(min_count)
    conns = _check_group(lst, min_count)
    assert len(conns) >= 9
    _check_group(lst, min_count, conn_cap=3)
    _check_group(lst, min_count, conn_cap=0)
    _check_group(lst, min_count, count=len(lst) + 1000)                  # a counter beyond the cap: the cap's worth is worked on
    _check_group(lst, min_count, count=len(lst) - 5)
    _check_group(lst, min_count, cand_cap=len(lst) - 7)


def test_group_of_nothing_and_of_one():
    c = ld.Cand(77, 0x52A3C6D1, 0x3B5A17, 4, 1, 0, 11)
    assert _check_group([c], 1) == [ld.Conn(0x52A3C6D1, 0x3B5A17, 1, 1, 1 << 11, 0)]
    assert _check_group([c], 2) == []
    assert _check_group([c], 1, count=0) == []
    assert _check_group([], 1) == []                                   # cand_cap 0: the counter is cleared, nothing else is touched


def test_group_beyond_one_sort_block():
    """20 000 candidates: one group of 5 000 over many streams and channels and 15 000 singletons -- five sort blocks, ten flag
    tiles, and with min_count 1 more connections than one tile of groups."""
    rng = np.random.default_rng(6)
    big = [ld.Cand(int(o), 0x8E5A3C71, 0x5EED01, int(s), 1, int(n), int(ch)) for o, s, n, ch in
           zip(rng.permutation(1 << 20)[:5000], rng.integers(0, 40, 5000), rng.integers(0, 2, 5000) * 9, rng.integers(0, 37, 5000))]
    keys = rng.permutation(1 << 22)[:15000]
    rest = [ld.Cand(int(rng.integers(0, 1 << 30)), 0x10000000 + int(k) * 600, int(k) * 3 & 0xFFFFFF, int(k) % 40, 2, 5, int(k) % 37) for k in keys]
    lst = big + rest
    lst = [lst[i] for i in rng.permutation(len(lst))]
    conns = _check_group(lst, 2)
    assert len(conns) == 1 and conns[0].n_packets == 5000
    assert len(_check_group(lst, 1)) == 15001
    _check_group(lst, 1, conn_cap=4000)


# ---- the chain ----------------------------------------------------------------------------------------------------------
def test_chain_finds_the_planted_connections():
    import torch
    lib = bt.lib()
    cap, planted_conns = ld.chain_capture()
    model = ld.capture_candidates(cap, 27)
    want_conns, want_cands = ld.group(model, 2)
    # from Python, through the host wrapper
    conns, cands = bt.le_discover(cap.words, cap.search_bits, cap.mhz, max_len=27, min_count=2, n_streams=len(cap.mhz),
                                  pitch_words=cap.pitch_words, n_words=cap.n_words)
    assert conns.tobytes() == ld.conn_array(want_conns, CONN).tobytes()
    assert cands.tobytes() == ld.cand_array(want_cands, CAND).tobytes()
    # the device chain, nothing read back between the stages
    cand_cap, conn_cap = len(model) + 100, 64
    d_words, d_phys = _dev(cap.words.reshape(-1)), _dev(cap.mhz.astype(np.uint16))
    d_cands, d_conns = _filled(cand_cap * CAND.itemsize), _filled(conn_cap * CONN.itemsize)
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    scratch = lib.btbbx_le_discover_scratch_bytes(cand_cap)
    d_scr = torch.zeros(scratch // 8 + 2, dtype=torch.int64, device="cuda")
    _scan_launch(cap, 27, cand_cap, d_words, d_phys, d_cands, d_cnt)
    bt.check(lib.btbbx_le_discover_group_device(d_cands.data_ptr(), d_cnt.data_ptr(), cand_cap, 2, d_conns.data_ptr(), conn_cap,
                                                d_cnt.data_ptr() + 4, d_scr.data_ptr(), scratch, None))
    torch.cuda.synchronize()
    n_cands, n_conns = int(d_cnt[0].item()), int(d_cnt[1].item())
    assert n_cands == len(model) and n_conns == len(want_conns)
    assert d_conns.cpu().numpy()[:n_conns * CONN.itemsize].tobytes() == conns.tobytes()
    assert d_cands.cpu().numpy()[:n_cands * CAND.itemsize].tobytes() == cands.tobytes()
    # every planted connection with its packets and channels
    by_key = {(int(k["access_address"]), int(k["crc_init"])): k for k in conns}
    for i, (aa, ci) in enumerate(planted_conns):
        mine = [p for p in cap.planted if p.note == "connection %d" % i]
        k = by_key.pop((aa, ci))
        mask = 0
        for p in mine:
            mask |= 1 << _le.channel_index(int(cap.mhz[p.stream]))
        assert int(k["n_packets"]) == len(mine) and int(k["channel_mask"]) == mask and int(k["n_empty"]) == sum(p.length == 0 for p in mine), (i, k)
        first = int(k["first"])
        assert {(int(c["stream"]), int(c["offset"])) for c in cands[first:first + len(mine)]} == {(p.stream, p.offset) for p in mine}
        assert (cands["conn"][first:first + len(mine)] == list(conns["access_address"]).index(aa)).all()
    assert bin(int(conns[list(conns["access_address"]).index(planted_conns[0][0])]["channel_mask"])).count("1") == 12
    # a group that was not planted is an alias: identical packets of one connection on one channel, seen at one common shift
    spans = {}
    for p in cap.planted:
        spans.setdefault(p.stream, []).append(p)
    for key, k in by_key.items():
        shifts = set()
        for c in cands[int(k["first"]):int(k["first"]) + int(k["n_packets"])]:
            near = [p for p in spans.get(int(c["stream"]), []) if p.offset - 8 <= int(c["offset"]) < p.offset + 80 + 8 * p.length]
            assert len(near) == 1, (key, c)
            shifts.add((int(c["offset"]) - near[0].offset, near[0].aa, near[0].length, near[0].header0))
        assert len(shifts) == 1 and list(shifts)[0][0] != 0, (key, shifts)
    print("chain: %d candidates, %d connections, %d of them aliases" % (n_cands, n_conns, len(by_key)))
