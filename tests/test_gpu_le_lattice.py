"""The LE kernels (libbtbb_amd/csrc/le.hip) on the lattice of tests/_le_lattice.py: btbbx_le_decode_hits_device over a
hand-built hit list -- every length, bit phase, stream end, MHz value and the access addresses at the branch points of the
offense rules --, and the generic scan kernel le_scan_kernel<-1, L> over access addresses of both preamble values and
eight top octets.  Every expectation is the model's (tests/_le.py); where the compiled reference is present
(oracle/_ref/libbtbb_ref.so) its lell_allocate_and_decode is asked about every record as well.  Output buffers start as
0xA5, so a byte the kernel leaves unwritten, or writes where it should not, shows."""
import numpy as np
import pytest

import _le
import _le_lattice as ll
import _libs
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu

CRC_INITS = (0x555555, 0x000000, 0xFFFFFF, 0x7B31C9, 0xAB123456)        # (the last one: bits above 24, which the entry masks)
REC = bt.LE_PKT_DTYPE.itemsize


@pytest.fixture(scope="module", autouse=True)
def _init():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    bt.init(2)


def _device_decode(lat, crc_init, count=None, cap=None, alloc=None):
    """One btbbx_le_decode_hits_device launch over the lattice's hit list -> all `alloc` records of a buffer that was 0xA5."""
    import torch
    lib = bt.lib()
    n = len(lat.hits)
    count = n if count is None else count
    cap = n if cap is None else cap
    alloc = max(cap, count) + 1 if alloc is None else alloc
    assert alloc >= min(cap, count)
    d_words = torch.from_numpy(lat.words.reshape(-1).view(np.int64).copy()).cuda()
    d_hits = torch.from_numpy(np.frombuffer(lat.hits.tobytes(), np.int64).copy()).cuda()
    d_phys = torch.from_numpy(lat.mhz.astype(np.int16)).cuda()
    d_cnt = torch.from_numpy(np.array([count, 0, 0, 0], np.uint32).view(np.int32)).cuda()
    d_out = torch.full((alloc * REC,), 0xA5, dtype=torch.uint8, device="cuda")
    bt.check(lib.btbbx_le_decode_hits_device(d_words.data_ptr(), lat.n_words, lat.pitch_words, d_hits.data_ptr(), d_cnt.data_ptr(),
                                             cap, d_phys.data_ptr(), crc_init, d_out.data_ptr(), None))
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(bt.LE_PKT_DTYPE)


def _check_records(lat, got, want, ref=None):
    """Every byte of every record against the model's; the tags' promise about crc_ok; the lell fields against the reference."""
    want_arr = ll.records_array(want)
    bad = [i for i in range(len(want)) if got[i].tobytes() != want_arr[i].tobytes()]
    assert not bad, (len(bad), [(i, lat.tags[i], lat.hits[i], _le.record_dict(got[i]), want[i]) for i in bad[:3]])
    for t, g in zip(lat.tags, got):
        if t.flip is None and (t.dist or 0) <= 0:
            assert g["crc_ok"] == 1 and g["truncated"] == 0, t
        else:
            assert g["crc_ok"] == 0 and g["truncated"] == int(t.flip is None), t
    checked = 0
    if ref is not None:
        for h, g in zip(lat.hits, got):
            rf = _le.ref_lell_fields(ref, bytes(g["bytes"]), int(lat.mhz[int(h["stream"])]))
            assert {k: int(g[k]) for k in rf} == rf, h
            checked += 1
    return checked


@pytest.mark.parametrize("tight", [False, True])
def test_decoder_on_the_lattice(tight):
    """The whole lattice at CRCInit 0x555555, a thinned copy of it at each further value; both pitch variants."""
    ref = _libs.ref()
    checked = 0
    for k, crc_init in enumerate(CRC_INITS):
        lat = ll.decode_lattice(tight=tight, crc_init=crc_init, full=k == 0)
        want = ll.expected(tight=tight, crc_init=crc_init, full=k == 0)
        n = len(lat.hits)
        got = _device_decode(lat, crc_init)
        assert got[n:].tobytes() == b"\xa5" * REC
        checked += _check_records(lat, got[:n], want, ref)
        assert int(got["crc_ok"][:n].sum()) > n // 2
    print("records checked against the compiled reference: %d" % checked)


def test_decoder_count_forms():
    import torch
    lat, want = ll.decode_lattice(crc_init=CRC_INITS[3], full=False), ll.expected(crc_init=CRC_INITS[3], full=False)
    want_arr = ll.records_array(want)
    n = len(lat.hits)
    # *d_count < cap: what lies at and behind the count stays as it was
    for count in (0, 1, 255, 256, 257, n - 1):
        got = _device_decode(lat, CRC_INITS[3], count=count, cap=n, alloc=n + 2)
        assert got[:count].tobytes() == want_arr[:count].tobytes(), count
        assert got[count:].tobytes() == b"\xa5" * (REC * (n + 2 - count)), count
    # *d_count > cap: exactly cap records
    for cap in (1, 255, 256, 257, n - 1):
        got = _device_decode(lat, CRC_INITS[3], count=n, cap=cap, alloc=cap + 1)
        assert got[:cap].tobytes() == want_arr[:cap].tobytes(), cap
        assert got[cap:].tobytes() == b"\xa5" * REC, cap
    got = _device_decode(lat, CRC_INITS[3], count=0xFFFFFFFF, cap=300, alloc=301)
    assert got[:300].tobytes() == want_arr[:300].tobytes() and got[300:].tobytes() == b"\xa5" * REC
    # cap == 0 takes no pointers
    assert bt.lib().btbbx_le_decode_hits_device(None, lat.n_words, lat.pitch_words, None, None, 0, None, CRC_INITS[3], None, None) == 0
    torch.cuda.synchronize()


def _scan(case, max_errors, only=None):
    crc_init = ll.scan_crc_init(case.aa)
    if only is not None:
        return bt.le_scan(case.words[only], case.search_bits, [int(case.mhz[only])], aa=case.aa, crc_init=crc_init,
                          max_errors=max_errors, n_streams=1)
    return bt.le_scan(case.words, case.search_bits, case.mhz, aa=case.aa, crc_init=crc_init, max_errors=max_errors,
                      n_streams=len(case.words))


@pytest.mark.parametrize("max_errors", [0, 1, 2, 3, 4])
def test_generic_scan_kernel_on_every_access_address(max_errors):
    ref = _libs.ref()
    for case in ll.scan_lattice():
        cache = _model_cache(case.aa)
        got = _scan(case, max_errors)
        want = ll.scan_model(case, max_errors, cache)
        _le.compare(got, want, case.mhz, ref if max_errors == 4 else None)
        found = {(int(g["stream"]), int(g["offset"])): int(g["aa_errors"]) for g in got}
        index = {(int(g["stream"]), int(g["offset"])): i for i, g in enumerate(got)}
        for p in case.planted:
            if p.errors <= max_errors and p.offset < case.search_bits:
                assert found.get((p.stream, p.offset)) == p.errors, (hex(case.aa), p)
            else:
                assert (p.stream, p.offset) not in found, (hex(case.aa), p)
        assert sum(p.errors == max_errors for p in case.planted) >= 6 and sum(p.errors == max_errors + 1 for p in case.planted) >= 6
        # a true advertising packet lies at its real distance from a neighbour of the advertising AA: the preamble counts,
        # so ADV_AA ^ 1 (the other preamble) is nine bits away and must never report one
        dist = int((_le.pattern_bits(case.aa) != _le.pattern_bits(_le.ADV_AA)).sum())
        for s, o in case.adv_packets:
            assert dist in (1, 9)
            if dist <= max_errors:
                assert found.get((s, o)) == dist, (hex(case.aa), s, o)
                g = got[index[(s, o)]]
                assert int(g["access_address"]) == _le.ADV_AA and int(g["pdu_bytes"]) == 8
            else:
                assert (s, o) not in found
    assert sum(len(c.adv_packets) for c in ll.scan_lattice()) >= 24


_caches = {}


def _model_cache(aa):
    return _caches.setdefault(aa, {})


@pytest.mark.parametrize("max_errors", [0, 4])
def test_dense_streams_through_the_generic_kernel(max_errors):
    """The pattern back to back: a hit every 40 bits, more per wave and tile than the hit ring holds; complete and in order."""
    n_cases = 0
    for case in ll.scan_lattice():
        if case.dense_stream is None:
            continue
        got = _scan(case, max_errors, only=case.dense_stream)
        want = ll.scan_model(case, max_errors, _model_cache(case.aa), only=case.dense_stream)
        assert len(got) == len(want) >= case.search_bits // 40
        assert (np.diff(got["offset"].astype(np.int64)) > 0).all()
        _le.compare(got, want, [int(case.mhz[case.dense_stream])])
        n_cases += 1
    assert n_cases == ll.DENSE_AAS


def test_device_chain_with_pitch_equal_to_n_words():
    """Scan, order and decode on the device over three streams that lie back to back (pitch_words == n_words), for an even
    access address (preamble 0xaa): byte-identical to bt.le_scan."""
    import torch
    lib = bt.lib()
    case = [c for c in ll.scan_lattice() if c.dense_stream is not None and not c.aa & 1][0]
    crc_init = ll.scan_crc_init(case.aa)
    want = _scan(case, 3)
    n_words, n_streams = case.n_words, len(case.words)
    assert n_streams == 3 and case.words.shape == (3, n_words)
    d_words = torch.from_numpy(case.words.reshape(-1).view(np.int64).copy()).cuda()
    d_phys = torch.from_numpy(case.mhz.astype(np.int16)).cuda()
    cap = 1 << 13
    assert len(want) < cap
    d_hits = torch.zeros(2 * cap, dtype=torch.int64, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    scratch_bytes = lib.btbbx_order_hits_scratch_bytes(cap)
    d_scr = torch.zeros((scratch_bytes + 15) // 8 + 2, dtype=torch.int64, device="cuda")
    d_out = torch.full(((cap + 1) * REC,), 0xA5, dtype=torch.uint8, device="cuda")
    bt.check(lib.btbbx_le_scan_device(d_words.data_ptr(), n_words, n_words, n_streams, case.search_bits, case.aa, 3,
                                      d_hits.data_ptr(), cap, d_cnt.data_ptr(), None))
    bt.check(lib.btbbx_order_hits_device(d_hits.data_ptr(), d_cnt.data_ptr(), cap, d_scr.data_ptr(), scratch_bytes, None))
    bt.check(lib.btbbx_le_decode_hits_device(d_words.data_ptr(), n_words, n_words, d_hits.data_ptr(), d_cnt.data_ptr(), cap,
                                             d_phys.data_ptr(), crc_init, d_out.data_ptr(), None))
    torch.cuda.synchronize()
    n = int(d_cnt[0].item())
    out = d_out.cpu().numpy().view(bt.LE_PKT_DTYPE)
    assert n == len(want) > 1000
    assert out[:n].tobytes() == want.tobytes()
    assert out[n:].tobytes() == b"\xa5" * (REC * (cap + 1 - n))
    assert set(want["stream"].tolist()) == {0, 1, 2}
