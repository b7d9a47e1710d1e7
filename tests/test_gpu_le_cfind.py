"""The kernels of the promiscuous LE Coded connection discovery (libbtbb_amd/csrc/le_cfind.h) against the model
(tests/_le_cfind.py): the candidate set, every byte of the candidate and info records, and both counts.  Output buffers start as
0xA5 and are longer than their caps, so a byte a kernel leaves unwritten, or writes where it should not, shows.  The captures are
_le_cfind.lattice() in both pitch forms -- six streams of 1029 words, four on data channels -- and chain_capture();
tests/test_le_cfind_model.py shows what they hold and that they tell every wrong variant from the model."""
import numpy as np
import pytest

import _le_discover as d
import _le_cfind as f
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu

CAND, INFO, CONN, HIT, PKT = (bt.LE_CAND_DTYPE.itemsize, bt.LE_CODED_CAND_INFO_DTYPE.itemsize, bt.LE_CONN_DTYPE.itemsize, bt.HIT_DTYPE.itemsize,
                              bt.LE_PKT_DTYPE.itemsize)


@pytest.fixture(scope="module", autouse=True)
def _init():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    bt.init(2)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def _device_scan(cap, max_len, max_errors, cand_cap, pre_cap, alloc=None, with_info=True):
    """One call -> (candidate count, pre-record count, candidate buffer, info buffer, pre-record buffer); the buffers were 0xA5 and
    are `alloc` records long."""
    import torch
    alloc = max(cand_cap, pre_cap) + 3 if alloc is None else alloc
    assert alloc >= max(cand_cap, pre_cap)
    d_words, d_phys = _dev(cap.words), _dev(cap.mhz)
    d_cands = torch.full((alloc * CAND,), 0xA5, dtype=torch.uint8, device="cuda")
    d_info = torch.full((alloc * INFO,), 0xA5, dtype=torch.uint8, device="cuda")
    d_pre = torch.full((alloc * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(8, dtype=torch.int32, device="cuda")
    d_cnt[4] = 77                                           # (the pre-record counter is cleared by the call)
    bt.check(bt.lib().btbbx_le_cfind_scan_device(d_words.data_ptr(), cap.n_words, cap.pitch_words, len(cap.mhz), cap.search_bits, d_phys.data_ptr(),
                                                 max_len, max_errors, d_cands.data_ptr(), d_info.data_ptr() if with_info else None, cand_cap,
                                                 d_cnt.data_ptr(), d_cnt.data_ptr() + 16, d_pre.data_ptr(), 16 * pre_cap, None),
             "btbbx_le_cfind_scan_device")
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy()
    assert not cnt[[1, 2, 3, 5, 6, 7]].any()
    return (int(cnt[0]), int(cnt[4]), d_cands.cpu().numpy().view(bt.LE_CAND_DTYPE), d_info.cpu().numpy().view(bt.LE_CODED_CAND_INFO_DTYPE),
            d_pre.cpu().numpy().view(np.uint32).reshape(-1, 4))


def _records(model):
    """[(Cand, Info)] -> the two record arrays"""
    cands = d.cand_array([x for x, _ in model], bt.LE_CAND_DTYPE)
    info = np.zeros(len(model), bt.LE_CODED_CAND_INFO_DTYPE)
    for i, (_, x) in enumerate(model):
        info[i] = (x.symbols, x.metric2, x.metric1, x.errors, x.ci, x.s, (0, 0, 0))
    return cands, info


def _pre_model(cap, max_errors):
    return sorted((o, s, b) for s in range(len(cap.mhz)) for o, b in f.pre_records(cap.model(s), cap.search_bits, max_errors))


@pytest.mark.parametrize("tight", [False, True])
@pytest.mark.parametrize("max_errors", f.LIMITS)
@pytest.mark.parametrize("max_len", f.MAX_LENS)
def test_scan_equals_the_model(tight, max_errors, max_len):
    cap = f.lattice(tight)
    model = list(f.lattice_model(tight, max_len, max_errors))
    want_c, want_i = _records(model)
    pre = _pre_model(cap, max_errors)
    assert len(model) >= (30 if max_len == 0 else 50) and len(pre) >= len(model)
    count, pre_count, cands, info, pre_recs = _device_scan(cap, max_len, max_errors, len(model) + 2, len(pre) + 2)
    print("candidates %d (model %d), pre-records %d (model %d)" % (count, len(model), pre_count, len(pre)))
    assert (count, pre_count) == (len(model), len(pre))
    got = sorted(cands[i].tobytes() + info[i].tobytes() for i in range(count))
    assert got == sorted(want_c[i].tobytes() + want_i[i].tobytes() for i in range(count))
    assert cands[count:].tobytes() == b"\xa5" * CAND * (len(cands) - count) and info[count:].tobytes() == b"\xa5" * INFO * (len(info) - count)
    got_pre = sorted((int(r[0]) | int(r[1]) << 32, int(r[2]), int(r[3])) for r in pre_recs[:pre_count])
    assert got_pre == pre and pre_recs[pre_count:].tobytes() == b"\xa5" * 16 * (len(pre_recs) - pre_count)


def test_caps_below_the_counts_and_no_info():
    cap = f.lattice(False)
    model = list(f.lattice_model(False, 255, 16))
    want_c, want_i = _records(model)
    full = {want_c[i].tobytes(): want_i[i].tobytes() for i in range(len(model))}
    n_pre = len(_pre_model(cap, 16))
    # cand_cap below the count: the count is the whole number, cand_cap distinct true records are written and nothing behind them
    k = len(model) // 2
    count, pre_count, cands, info, _ = _device_scan(cap, 255, 16, k, n_pre, alloc=n_pre + 5)
    assert (count, pre_count) == (len(model), n_pre)
    got = [cands[i].tobytes() for i in range(k)]
    assert len(set(got)) == k and all(full.get(c) == info[i].tobytes() for i, c in enumerate(got))
    assert cands[k:].tobytes() == b"\xa5" * CAND * (len(cands) - k) and info[k:].tobytes() == b"\xa5" * INFO * (len(info) - k)
    # pre_cap below its count: the count says so, and what was decoded of the pre-records kept is true
    k = n_pre // 3
    count, pre_count, cands, info, pre_recs = _device_scan(cap, 255, 16, len(model), k, alloc=max(len(model), k) + 5)
    assert pre_count == n_pre and 0 < count <= len(model)
    got = [cands[i].tobytes() for i in range(count)]
    assert len(set(got)) == count and all(full.get(c) == info[i].tobytes() for i, c in enumerate(got))
    assert cands[count:].tobytes() == b"\xa5" * CAND * (len(cands) - count) and pre_recs[k:].tobytes() == b"\xa5" * 16 * (len(pre_recs) - k)
    # no info records asked for
    count, _, cands, info, _ = _device_scan(cap, 255, 16, len(model) + 1, n_pre, with_info=False)
    assert count == len(model) and sorted(cands[i].tobytes() for i in range(count)) == sorted(full)
    assert info.tobytes() == b"\xa5" * INFO * len(info)
    # cand_cap 0 with no candidate buffer and no info buffer: the counts alone
    import torch
    d_words, d_phys = _dev(cap.words), _dev(cap.mhz)
    d_pre = torch.zeros(16 * n_pre, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    bt.check(bt.lib().btbbx_le_cfind_scan_device(d_words.data_ptr(), cap.n_words, cap.pitch_words, len(cap.mhz), cap.search_bits, d_phys.data_ptr(),
                                                 255, 16, None, None, 0, d_cnt.data_ptr(), d_cnt.data_ptr() + 4, d_pre.data_ptr(), 16 * n_pre, None),
             "btbbx_le_cfind_scan_device")
    torch.cuda.synchronize()
    assert d_cnt.cpu().numpy().tolist() == [len(model), n_pre, 0, 0]


@pytest.mark.parametrize("tight,max_len,max_errors", [(False, 255, 16), (True, 255, 63), (False, 27, 1)])
def test_candidates_against_the_coded_scan_and_decoder(tight, max_len, max_errors):
    """For EVERY candidate, btbbx_le_coded_scan_device told its AA' at the same limit finds its offset with the same count, and
    btbbx_le_coded_decode_hits_device under its crc_init reports crc_ok and the same header.  One scan per distinct AA', one decode
    per distinct (AA', crc_init) over all of its candidates."""
    import torch
    cap = f.lattice(tight)
    model = list(f.lattice_model(tight, max_len, max_errors))
    lib = bt.lib()
    d_words, d_phys = _dev(cap.words), _dev(cap.mhz)
    by_aa = {}
    for cand, info in model:
        by_aa.setdefault(cand.access_address, []).append((cand, info))
    hit_cap, checked = 4096, 0
    for aa, members in by_aa.items():
        d_hits = torch.zeros(hit_cap * HIT, dtype=torch.uint8, device="cuda")
        d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
        bt.check(lib.btbbx_le_coded_scan_device(d_words.data_ptr(), cap.n_words, cap.pitch_words, len(cap.mhz), cap.search_bits, aa, max_errors,
                                                d_hits.data_ptr(), hit_cap, d_cnt.data_ptr(), None))
        torch.cuda.synchronize()
        n = int(d_cnt[0].item())
        assert n <= hit_cap, (aa, n)
        hits = d_hits.cpu().numpy().view(bt.HIT_DTYPE)[:n]
        found = {(int(h["stream"]), int(h["offset"])): h for h in hits}
        assert len(found) == n
        by_init = {}
        for cand, info in members:
            h = found.get((cand.stream, cand.offset))
            assert h is not None and int(h["ac_errors"]) == info.errors and int(h["lap"]) == aa, cand
            by_init.setdefault(cand.crc_init, []).append((cand, info, h))
        for init, group in by_init.items():
            k = len(group)
            hit = np.zeros(k + 1, bt.HIT_DTYPE)
            for i, (_, _, h) in enumerate(group):
                hit[i] = h
            d_hit = _dev(hit)
            d_out = torch.zeros(k * PKT, dtype=torch.uint8, device="cuda")
            d_inf = torch.zeros(k * 16, dtype=torch.uint8, device="cuda")
            d_k = torch.full((1,), k, dtype=torch.int32, device="cuda")
            bt.check(lib.btbbx_le_coded_decode_hits_device(d_words.data_ptr(), cap.n_words, cap.pitch_words, d_hit.data_ptr(), d_k.data_ptr(), k,
                                                           d_phys.data_ptr(), init, d_out.data_ptr(), d_inf.data_ptr(), None, 0, None))
            torch.cuda.synchronize()
            pkts, infs = d_out.cpu().numpy().view(bt.LE_PKT_DTYPE), d_inf.cpu().numpy().view(bt.LE_CODED_INFO_DTYPE)
            for (cand, info, _), pkt, inf in zip(group, pkts, infs):
                assert int(pkt["crc_ok"]) == 1 and int(pkt["access_address"]) == aa and int(pkt["pdu_bytes"]) == 2 + cand.length, cand
                assert (int(pkt["bytes"][4]), int(inf["symbols"]), int(inf["header_moved"]), int(inf["s"])) == (cand.header0, info.symbols, 0, info.s), cand
                checked += 1
    assert checked == len(model) and checked >= 50


def test_host_wrapper_repeats_the_scan_when_its_first_guess_is_short():
    """le_coded_discover on the lattice at max_errors 63: the S = 8 packets leave more pre-records than the wrapper's first guess
    has room for, so its first pass drops some and a second pass with room follows; the result is the model's, grouped."""
    cap = f.lattice(False)
    first_guess = cap.search_bits // 4096 * len(cap.mhz) + 4096
    assert len(_pre_model(cap, 63)) > first_guess > len(f.lattice_model(False, 255, 63))
    conns, cands = d.group([x for x, _ in f.lattice_model(False, 255, 63)], 1)
    want_conns, want_cands = d.conn_array(conns, bt.LE_CONN_DTYPE), d.cand_array(cands, bt.LE_CAND_DTYPE)
    got_conns, got_cands = bt.le_coded_discover(cap.words, cap.search_bits, cap.mhz, max_len=255, max_errors=63, min_count=1,
                                                n_streams=len(cap.mhz), pitch_words=cap.pitch_words, n_words=cap.n_words)
    assert got_cands.tobytes() == want_cands.tobytes() and got_conns.tobytes() == want_conns.tobytes()


def test_chain_device_resident_and_through_python():
    """Three coded connections over twelve streams: scan, then the unchanged grouping, byte for byte against the model's candidates
    grouped by tests/_le_discover.py."""
    import torch
    cap, sent = f.chain_capture()
    model = cap.candidates(27, 16)
    conns, cands = d.group([x for x, _ in model], 3)
    want_conns, want_cands = d.conn_array(conns, bt.LE_CONN_DTYPE), d.cand_array(cands, bt.LE_CAND_DTYPE)
    planted = {}
    for p in cap.planted:
        planted.setdefault((p.aa, p.crc_init), []).append(p)
    assert len(conns) >= 3
    for aa, init in sent:
        rec = next(x for x in conns if (x.access_address, x.crc_init) == (aa, init))
        mask = 0
        for p in planted[(aa, init)]:
            mask |= 1 << f._le.channel_index(int(cap.mhz[p.stream]))
        assert rec.n_packets == len(planted[(aa, init)]) and rec.channel_mask == mask
    lib = bt.lib()
    k = len(model)
    alloc = k + 4
    d_words, d_phys = _dev(cap.words), _dev(cap.mhz)
    d_cands = torch.full((alloc * CAND,), 0xA5, dtype=torch.uint8, device="cuda")
    d_conns = torch.full((alloc * CONN,), 0xA5, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(8, dtype=torch.int32, device="cuda")
    pre_cap = 4096
    d_pre = torch.zeros(16 * pre_cap, dtype=torch.uint8, device="cuda")
    scratch = torch.zeros(lib.btbbx_le_discover_scratch_bytes(alloc), dtype=torch.uint8, device="cuda")
    bt.check(lib.btbbx_le_cfind_scan_device(d_words.data_ptr(), cap.n_words, cap.pitch_words, len(cap.mhz), cap.search_bits, d_phys.data_ptr(), 27, 16,
                                            d_cands.data_ptr(), None, alloc, d_cnt.data_ptr(), d_cnt.data_ptr() + 4, d_pre.data_ptr(), 16 * pre_cap, None))
    bt.check(lib.btbbx_le_discover_group_device(d_cands.data_ptr(), d_cnt.data_ptr(), alloc, 3, d_conns.data_ptr(), alloc, d_cnt.data_ptr() + 8,
                                                scratch.data_ptr(), scratch.numel(), None))
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy()
    assert (int(cnt[0]), int(cnt[2])) == (k, len(conns)) and int(cnt[1]) <= pre_cap
    assert d_cands.cpu().numpy().view(bt.LE_CAND_DTYPE)[:k].tobytes() == want_cands.tobytes()
    assert d_conns.cpu().numpy().view(bt.LE_CONN_DTYPE)[:len(conns)].tobytes() == want_conns.tobytes()
    assert d_cands.cpu().numpy()[k * CAND:].tobytes() == b"\xa5" * CAND * (alloc - k)
    # through Python, both pitch forms of the host entry's copy (the capture's pitch is above n_words)
    got_conns, got_cands = bt.le_coded_discover(cap.words, cap.search_bits, cap.mhz, max_len=27, max_errors=16, min_count=3, n_streams=len(cap.mhz),
                                                pitch_words=cap.pitch_words, n_words=cap.n_words)
    assert got_conns.tobytes() == want_conns.tobytes() and got_cands.tobytes() == want_cands.tobytes()
    got_conns, got_cands = bt.le_coded_discover(cap.words, cap.search_bits, cap.mhz, max_len=27, max_errors=16, min_count=3, n_streams=len(cap.mhz),
                                                pitch_words=cap.pitch_words, n_words=cap.n_words, conn_cap=2, cand_cap=5, truncate=True)
    assert got_conns.tobytes() == want_conns[:2].tobytes() and got_cands.tobytes() == want_cands[:5].tobytes()
    with pytest.raises(bt.BtbbError):
        bt.le_coded_discover(cap.words, cap.search_bits, cap.mhz, max_len=27, max_errors=16, min_count=3, n_streams=len(cap.mhz),
                             pitch_words=cap.pitch_words, n_words=cap.n_words, cand_cap=5)
