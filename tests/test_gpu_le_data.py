"""LE data extraction (libbtbb_amd/csrc/le_data.h) on the GPU: btbbx_le_data_device over the planted world and the hand-made lists of
tests/_le_data.py, held against the model, every byte of its four outputs and both counts; the host wrapper and the Python entry on
the planted capture against discovery, tracking and data models composed.  Output buffers start as 0xA5 and are longer than their
caps, so a byte a kernel leaves unwritten, or writes where it should not, shows; the two counts start as 0xA5 too, since the stage
writes them and does not add to them."""
import numpy as np
import pytest

import _le_data as dm
import _le_discover as ld
import _le_track as lt
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu

CAND, CONN, TRACK, PKT = bt.LE_CAND_DTYPE, bt.LE_CONN_DTYPE, bt.LE_TRACK_DTYPE, bt.LE_TRACK_PKT_DTYPE
DATA, DPKT, MSG = bt.LE_DATA_DTYPE, bt.LE_DATA_PKT_DTYPE, bt.LE_MSG_DTYPE
E_ARG = -3
BIG = (1 << 20, 1 << 30)


@pytest.fixture(scope="module", autouse=True)
def _init():
    import torch                                            # (a torch that does not import fails these tests, it does not skip them)
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
    return torch.full(((nbytes + 15) // 16 * 16 + 16,), 0xA5, dtype=torch.uint8, device="cuda")


def _records(buf, n, dtype):
    return buf.cpu().numpy()[:n * dtype.itemsize].view(dtype)


def _device(b, msg_cap, byte_cap, cand_cap=None, conn_cap=None, count=None, conn_count=None, d_words=None, pitch=None, n_streams=None):
    """btbbx_le_data_device over b's records -> (data, dpkts, msgs, bytes, n_msgs, n_bytes), the buffers whole: one record (64 octets)
    longer than their caps."""
    import torch
    lib = bt.lib()
    n, k = len(b.cands), len(b.conns)
    count, cand_cap = n if count is None else count, n if cand_cap is None else cand_cap
    conn_count, conn_cap = k if conn_count is None else conn_count, k if conn_cap is None else conn_cap
    words = np.asarray(b.words)
    d_cands, d_conns, d_pkts = _dev(ld.cand_array(b.cands, CAND)), _dev(ld.conn_array(b.conns, CONN)), _dev(lt.pkt_array(b.pkts, PKT))
    d_phys, d_tracks = _dev(np.asarray(dm.MHZ, np.uint16)), _filled(max(k, 1) * TRACK.itemsize)
    if d_words is None:
        d_words, pitch, n_streams = _dev(words.reshape(-1)), words.shape[1], words.shape[0]
    d_data, d_dpkts = _filled((conn_cap + 1) * DATA.itemsize), _filled((cand_cap + 1) * DPKT.itemsize)
    d_msgs, d_bytes, d_counts = _filled((msg_cap + 1) * MSG.itemsize), _filled(byte_cap + 64), _filled(16)
    d_cnt = torch.from_numpy(np.array([count, conn_count], np.int64).astype(np.uint32).view(np.int32)).cuda()
    scratch = lib.btbbx_le_data_scratch_bytes(cand_cap, conn_cap)
    d_scr = _filled(scratch)
    p = d_cnt.data_ptr()
    bt.check(lib.btbbx_le_data_device(d_words.data_ptr(), b.n_words, pitch, n_streams, d_phys.data_ptr(), d_cands.data_ptr(), p, cand_cap,
                                      d_conns.data_ptr(), p + 4, conn_cap, d_tracks.data_ptr(), d_pkts.data_ptr(), d_data.data_ptr(),
                                      d_dpkts.data_ptr(), d_msgs.data_ptr() if msg_cap else None, msg_cap, d_counts.data_ptr() + 8,
                                      d_bytes.data_ptr() if byte_cap else None, byte_cap, d_counts.data_ptr(), d_scr.data_ptr(), scratch,
                                      None), "btbbx_le_data_device")
    torch.cuda.synchronize()
    assert set(d_scr.cpu().numpy()[scratch:].tolist()) == {0xA5}                # nothing behind the scratch
    counts = d_counts.cpu().numpy()
    assert counts[12:].tobytes() == b"\xa5" * (len(counts) - 12)
    return (_records(d_data, conn_cap + 1, DATA), _records(d_dpkts, cand_cap + 1, DPKT), _records(d_msgs, msg_cap + 1, MSG),
            d_bytes.cpu().numpy()[:byte_cap + 64], int(counts[8:12].view(np.uint32)[0]), int(counts[:8].view(np.uint64)[0]))


def _same(got, want, kept, what):
    if got[:kept].tobytes() != want.tobytes():
        bad = [g for g in range(kept) if got[g].tobytes() != want[g].tobytes()]
        raise AssertionError("%s %d: %s, model %s (%d of %d differ)" % (what, bad[0], got[bad[0]], want[bad[0]], len(bad), kept))
    assert got[kept:].tobytes() == b"\xa5" * (got.dtype.itemsize * (len(got) - kept)), what


_WHOLE, _CUT = {}, {}


def _cut(b, work, kept):
    """b as the stage sees it through caps and counts that cut the list: the tracking's records are those of the cut list (ranks and
    events number the members that are left without gaps, as the stage's input promises)."""
    key = (id(b), work, kept)
    if key not in _CUT:
        pkts = lt.track(b.cands[:work], kept, dm.MHZ, dm.N_STREAMS, dm.UNIT, dm.IFS, dm.JITTER, lt.REMAP)[1]
        _CUT[key] = b._replace(pkts=pkts + [None] * (len(b.cands) - work))
    return _CUT[key]


def _model(b, work, kept, rows, msg_cap, byte_cap):
    """The model on the first `work` candidates and `kept` connections (what the device sees through caps and counts), computed once
    without caps: caps at or above the totals change nothing."""
    key = (id(b), work, kept)
    if key not in _WHOLE:
        _WHOLE[key] = dm.data(b.conns[:kept], b.cands[:work], b.pkts[:work], b.words if rows is None else rows, b.n_words, *BIG)
    whole = _WHOLE[key]
    if msg_cap >= whole.n_msgs and byte_cap >= whole.n_bytes:
        return whole
    return dm.data(b.conns[:kept], b.cands[:work], b.pkts[:work], b.words if rows is None else rows, b.n_words, msg_cap, byte_cap)


def _check(b, msg_cap=BIG[0], byte_cap=BIG[1], want=None, rows=None, **kw):
    """The device against the model; buffers as large as the caps ask for, but no larger than the totals need."""
    n, k = len(b.cands), len(b.conns)
    get = lambda name, default: default if kw.get(name) is None else kw[name]          # noqa: E731
    work, kept = min(get("count", n), get("cand_cap", n)), min(get("conn_count", k), get("conn_cap", k))
    if (work, kept) != (n, k):
        b = _cut(b, work, kept)
    if want is None:
        want = _model(b, work, kept, rows, msg_cap, byte_cap)
    room_m, room_b = min(msg_cap, want.n_msgs + 3), min(byte_cap, want.n_bytes + 11)
    data, dpkts, msgs, octets, n_msgs, n_bytes = _device(b, room_m, room_b, **kw)
    assert (n_msgs, n_bytes) == (want.n_msgs, want.n_bytes)
    if kw.get("conn_cap") == 0 or kw.get("cand_cap") == 0:
        work = kept = 0
    _same(data, dm.data_array(want.data[:kept], DATA), kept, "connection")
    _same(dpkts, dm.dpkt_array(want.dpkts[:work], DPKT), work, "candidate")
    _same(msgs, dm.msg_array(want.msgs, MSG), len(want.msgs), "message")
    stored = len(want.payload)
    if octets[:stored].tobytes() != want.payload:
        bad = [j for j in range(stored) if octets[j] != want.payload[j]]
        raise AssertionError("octet %d: %#x, model %#x (%d of %d differ)" % (bad[0], octets[bad[0]], want.payload[bad[0]], len(bad), stored))
    assert octets[stored:].tobytes() == b"\xa5" * (len(octets) - stored)              # nothing behind the stored prefix
    return want


def test_the_planted_world():
    b = dm.planted_world()
    want = _check(b, want=dm.planted_model())
    assert dm.check_planted(b, want) == 116
    print("planted world: %d connections, %d candidates, %d messages, %d octets" % (len(b.conns), len(b.cands), want.n_msgs, want.n_bytes))


def test_the_alignment_lattice():
    b = dm.align_list()
    want = _check(b)
    assert {m.byte_offset % 8 for m in want.msgs} == set(range(8)) and want.n_bytes > 14000


@pytest.mark.parametrize("which", ["long", "crowd", "both"])
def test_seams(which):
    b = dm.seam_list(which)
    n, k = len(b.cands), len(b.conns)
    assert which != "both" or (n % 64 and n % 256 and k % 64 and k % 256)
    want = _check(b)
    if which != "crowd":                                    # the patterns lie across the kernels' seams: wave, workgroup, tile
        seen = dm.check_seams(b, want)
        assert seen[64] >= 44 and seen[256] >= 11 and seen[2048] == 1, seen


def test_caps():
    b = dm.align_list()
    whole = dm.built_model(b)
    n_msgs, n_bytes = whole.n_msgs, whole.n_bytes
    mid = whole.msgs[n_msgs // 2]
    for msg_cap, byte_cap in ((0, 0), (0, 1 << 30), (1 << 20, 0), (n_msgs - 1, 1 << 30), (n_msgs, n_bytes), (n_msgs + 5, n_bytes + 9),
                              (1 << 20, n_bytes - 1), (1 << 20, mid.byte_offset + mid.bytes - 1), (1 << 20, mid.byte_offset + mid.bytes),
                              (n_msgs // 3, mid.byte_offset + 1), (1, 1 << 30)):
        want = _check(b, msg_cap, byte_cap)
        stored = [bool(m.flags & dm.STORED) for m in want.msgs]
        assert stored == sorted(stored, reverse=True) and (want.n_msgs, want.n_bytes) == (n_msgs, n_bytes)


def test_counts_and_caps_of_the_input():
    b = dm.planted_world()
    n, k = len(b.cands), len(b.conns)
    inside = b.conns[k // 2].first + 3                                     # a count that cuts a connection
    for kw in (dict(conn_cap=k - 1), dict(conn_cap=1), dict(conn_cap=k + 300), dict(conn_count=k - 2), dict(conn_count=k + 1000),
               dict(count=inside), dict(count=n + 1000), dict(cand_cap=n - 9), dict(cand_cap=inside + 2), dict(count=0), dict(conn_count=0),
               dict(conn_cap=0), dict(cand_cap=0)):
        _check(b, **kw)


def test_pitch_beyond_2_to_32_bits():
    """Two streams, pitch_words = 2^26 + 1: stream 1 begins beyond 2^32 bits; only the words under the packets are written."""
    import torch
    n_words, pitch = 64, (1 << 26) + 1
    members = [dm.H(e, e, 2 | (e & 1) << 3, 5 + 2 * e, 400 * e + e, 1 - (e & 1)) for e in range(9)]
    b = dm.hand_built([members], n_words, n_streams=2)
    d_words = torch.empty(pitch + n_words, dtype=torch.int64, device="cuda")
    d_words[:n_words] = torch.from_numpy(b.words[0].view(np.int64).copy()).cuda()
    d_words[pitch:pitch + n_words] = torch.from_numpy(b.words[1].view(np.int64).copy()).cuda()
    want = _check(b, d_words=d_words, pitch=pitch, n_streams=2)
    assert want.n_msgs == 9 and 64 * pitch > 1 << 32


def test_bad_arguments_are_refused_before_any_launch():
    import torch
    lib = bt.lib()
    buf = _filled(1 << 17)
    p = buf.data_ptr()
    scratch = lib.btbbx_le_data_scratch_bytes(8, 4)
    assert scratch <= (1 << 17) - 32768

    def run(words=p, phys=p + 512, cands=p + 1024, cnt=p + 2048, conns=p + 3072, ccnt=p + 2052, tracks=p + 4096, pkts=p + 6144,
            data=p + 8192, dpkts=p + 10240, msgs=p + 12288, msg_cap=4, mcnt=p + 2056, octets=p + 14336, byte_cap=64, bcnt=p + 2064,
            scr=p + 32768, scr_bytes=scratch, n_words=8, pitch=8, n_streams=2):
        return lib.btbbx_le_data_device(words, n_words, pitch, n_streams, phys, cands, cnt, 8, conns, ccnt, 4, tracks, pkts, data, dpkts, msgs,
                                        msg_cap, mcnt, octets, byte_cap, bcnt, scr, scr_bytes, None)

    for kw in (dict(words=None), dict(phys=None), dict(cands=None), dict(cnt=None), dict(conns=None), dict(ccnt=None), dict(tracks=None),
               dict(pkts=None), dict(data=None), dict(dpkts=None), dict(msgs=None), dict(mcnt=None), dict(octets=None), dict(bcnt=None),
               dict(scr=None), dict(words=p + 4), dict(phys=p + 513), dict(cands=p + 1028), dict(conns=p + 3076), dict(tracks=p + 4100),
               dict(pkts=p + 6148), dict(data=p + 8196), dict(dpkts=p + 10242), dict(msgs=p + 12292), dict(octets=p + 14340),
               dict(scr=p + 32776), dict(cnt=p + 2050), dict(ccnt=p + 2054), dict(mcnt=p + 2058), dict(bcnt=p + 2068),
               dict(scr_bytes=scratch - 1), dict(n_words=0), dict(n_words=(1 << 42) + 1, pitch=1 << 43), dict(pitch=7), dict(n_streams=0)):
        assert run(**kw) == E_ARG, kw
        assert b"btbbx_le_data_device" in lib.btbbx_last_error()
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == b"\xa5" * len(buf)
    # null buffers with a cap of 0 are fine; counts of 0xa5a5a5a5: the caps' worth of 0xa5 records is read, no candidate is a member
    assert run(msgs=None, msg_cap=0, octets=None, byte_cap=0) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert got[8192:8192 + 4 * 48].tobytes() == bytes(4 * 48) and got[10240:10240 + 96].tobytes() == b"\xff" * 96
    assert got[2056:2060].tobytes() == bytes(4) and got[2064:2072].tobytes() == bytes(8)
    assert got[12288:32768].tobytes() == b"\xa5" * (32768 - 12288) and got[:2056].tobytes() == b"\xa5" * 2056
    assert got[32768 + scratch:].tobytes() == b"\xa5" * (len(got) - 32768 - scratch)


@pytest.fixture(scope="module")
def chain():
    """The planted world as a capture, and discovery, tracking and data models composed on it."""
    b = dm.planted_world()
    cap = ld.Capture(b.words, b.n_words, b.n_words, 64 * b.n_words - 39, dm.MHZ, (), 27)
    conns, cands = ld.group(ld.capture_candidates(cap, 27), 2)
    tracks, pkts = lt.track(cands, len(conns), dm.MHZ, dm.N_STREAMS, dm.UNIT, dm.IFS, dm.JITTER, lt.REMAP)
    return cap, conns, cands, tracks, pkts


def test_the_host_wrapper_on_the_planted_capture(chain):
    cap, conns, cands, tracks, pkts = chain
    lib = bt.lib()
    planted = {(p.aa, p.crc_init) for p in dm.planted_world().planted}
    assert planted <= {(c.access_address, c.crc_init) for c in conns}
    for msg_cap, byte_cap in ((1 << 12, 1 << 16), (40, 1 << 16), (1 << 12, 500), (0, 0)):
        want = dm.data(conns, cands, pkts, cap.words, cap.n_words, msg_cap, byte_cap)
        k, n = len(conns) + 1, len(cands) + 1
        o_conns, o_cands, o_tracks, o_pkts = np.zeros(k, CONN), np.zeros(n, CAND), np.zeros(k, TRACK), np.zeros(n, PKT)
        o_data, o_dpkts = np.full(k * DATA.itemsize, 0xA5, np.uint8).view(DATA), np.full(n * DPKT.itemsize, 0xA5, np.uint8).view(DPKT)
        o_msgs, o_bytes = np.full((msg_cap + 1) * MSG.itemsize, 0xA5, np.uint8).view(MSG), np.full(byte_cap + 8, 0xA5, np.uint8)
        counts = np.zeros(3, np.uint64)
        words = np.ascontiguousarray(cap.words).reshape(-1)
        phys = np.ascontiguousarray(cap.mhz, dtype=np.uint16)
        got = lib.btbbx_le_data_host(bt._ptr(words), cap.n_words, cap.pitch_words, len(cap.mhz), cap.search_bits, bt._ptr(phys), 27, 2,
                                     bt._ptr(o_conns), k, bt._ptr(o_cands), n, counts.ctypes.data, dm.UNIT, dm.IFS, dm.JITTER, lt.REMAP,
                                     bt._ptr(o_tracks), bt._ptr(o_pkts), bt._ptr(o_data), bt._ptr(o_dpkts),
                                     bt._ptr(o_msgs) if msg_cap else None, msg_cap, counts.ctypes.data + 8,
                                     bt._ptr(o_bytes) if byte_cap else None, byte_cap, counts.ctypes.data + 16)
        assert got == len(conns) and counts.tolist() == [len(cands), want.n_msgs, want.n_bytes]
        assert o_conns[:k - 1].tobytes() == ld.conn_array(conns, CONN).tobytes() and o_cands[:n - 1].tobytes() == ld.cand_array(cands, CAND).tobytes()
        assert o_tracks[:k - 1].tobytes() == lt.track_array(tracks, TRACK).tobytes() and o_pkts[:n - 1].tobytes() == lt.pkt_array(pkts, PKT).tobytes()
        _same(o_data, dm.data_array(want.data, DATA), k - 1, "connection")
        _same(o_dpkts, dm.dpkt_array(want.dpkts, DPKT), n - 1, "candidate")
        _same(o_msgs, dm.msg_array(want.msgs, MSG), len(want.msgs), "message")
        assert o_bytes[:len(want.payload)].tobytes() == want.payload and set(o_bytes[len(want.payload):].tolist()) == {0xA5}


def test_le_data_from_python_on_the_planted_capture(chain):
    cap, conns, cands, tracks, pkts = chain
    want = dm.data(conns, cands, pkts, cap.words, cap.n_words, *BIG)
    kw = dict(max_len=27, min_count=2, n_streams=len(cap.mhz), pitch_words=cap.pitch_words, n_words=cap.n_words, unit_bits=dm.UNIT,
              ifs_bits=dm.IFS, jitter_bits=dm.JITTER)
    g_conns, g_cands, g_tracks, g_pkts, data, dpkts, msgs, payload = bt.le_data(cap.words, cap.search_bits, cap.mhz, **kw)
    assert g_conns.tobytes() == ld.conn_array(conns, CONN).tobytes() and g_cands.tobytes() == ld.cand_array(cands, CAND).tobytes()
    assert g_pkts.tobytes() == lt.pkt_array(pkts, PKT).tobytes() and g_tracks.tobytes() == lt.track_array(tracks, TRACK).tobytes()
    assert data.tobytes() == dm.data_array(want.data, DATA).tobytes() and dpkts.tobytes() == dm.dpkt_array(want.dpkts, DPKT).tobytes()
    assert msgs.tobytes() == dm.msg_array(want.msgs, MSG).tobytes() and payload.tobytes() == want.payload
    # the planted messages come out of the capture, octet for octet (the llid-0 packet is no candidate of the scan: nothing hangs on it)
    by = {(int(c["access_address"]), int(c["crc_init"])): g for g, c in enumerate(g_conns)}
    for p in dm.planted_world().planted:
        mine = msgs[msgs["conn"] == by[(p.aa, p.crc_init)]]
        assert [(int(m["role"]), payload[int(m["byte_offset"]):int(m["byte_offset"]) + int(m["bytes"])].tobytes()) for m in mine] == p.messages
    with pytest.raises(bt.BtbbError):
        bt.le_data(cap.words, cap.search_bits, cap.mhz, msg_cap=5, **kw)
    cut = bt.le_data(cap.words, cap.search_bits, cap.mhz, msg_cap=5, byte_cap=60, truncate=True, **kw)
    assert len(cut[6]) == 5 and cut[7].tobytes() == want.payload[:len(cut[7])] and 0 < len(cut[7]) <= 60
