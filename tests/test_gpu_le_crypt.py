"""LE decryption (libbtbb_amd/csrc/le_crypt.h) on the GPU: btbbx_le_crypt_device over the planted world and the hand-made lists of
tests/_le_crypt.py, held against the model, every byte of its five outputs and both counts; the host wrapper and the Python entry on
the planted capture against discovery, tracking, data and decryption models composed.  Output buffers start as 0xA5 and are longer
than their caps, so a byte a kernel leaves unwritten, or writes where it should not, shows.  The data stage's records the device
entry reads are the data MODEL's, so a fault of the data stage does not pass through here."""
import numpy as np
import pytest

import _le_crypt as cm
import _le_data as dm
import _le_discover as ld
import _le_track as lt
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu

CAND, CONN, TRACK, PKT = bt.LE_CAND_DTYPE, bt.LE_CONN_DTYPE, bt.LE_TRACK_DTYPE, bt.LE_TRACK_PKT_DTYPE
DATA, DPKT, MSG, CRYPT, CPKT = bt.LE_DATA_DTYPE, bt.LE_DATA_PKT_DTYPE, bt.LE_MSG_DTYPE, bt.LE_CRYPT_DTYPE, bt.LE_CRYPT_PKT_DTYPE
E_ARG = -3
P, E = cm.P, cm.E


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


def _keys(keys):
    return np.frombuffer(b"".join(keys), np.uint8)


def _device(b, dpkts, keys, window, msg_cap, byte_cap):
    """btbbx_le_crypt_device over b's records and the data stage's dpkts -> (crypt, cpkts, ppkts, msgs, bytes, n_msgs, n_bytes), the
    buffers whole: one record (64 octets) longer than their caps."""
    import torch
    lib = bt.lib()
    n, k = len(b.cands), len(b.conns)
    words = np.asarray(b.words)
    d_cands, d_conns, d_pkts = _dev(ld.cand_array(b.cands, CAND)), _dev(ld.conn_array(b.conns, CONN)), _dev(lt.pkt_array(b.pkts, PKT))
    d_phys, d_tracks, d_in, d_keys = _dev(np.asarray(dm.MHZ, np.uint16)), _filled(max(k, 1) * TRACK.itemsize), _dev(dpkts), _dev(_keys(keys))
    d_words = _dev(words.reshape(-1))
    d_crypt, d_cpkts, d_ppkts = _filled((k + 1) * CRYPT.itemsize), _filled((n + 1) * CPKT.itemsize), _filled((n + 1) * DPKT.itemsize)
    d_msgs, d_bytes, d_counts = _filled((msg_cap + 1) * MSG.itemsize), _filled(byte_cap + 64), _filled(16)
    d_cnt = torch.from_numpy(np.array([n, k], np.uint32).view(np.int32)).cuda()
    scratch = lib.btbbx_le_crypt_scratch_bytes(n, k, len(keys))
    d_scr = _filled(scratch)
    p = d_cnt.data_ptr()
    bt.check(lib.btbbx_le_crypt_device(d_words.data_ptr(), b.n_words, words.shape[1], words.shape[0], d_phys.data_ptr(), d_cands.data_ptr(), p, n,
                                       d_conns.data_ptr(), p + 4, k, d_tracks.data_ptr(), d_pkts.data_ptr(), d_in.data_ptr(), d_keys.data_ptr(),
                                       len(keys), window, d_crypt.data_ptr(), d_cpkts.data_ptr(), d_ppkts.data_ptr(),
                                       d_msgs.data_ptr() if msg_cap else None, msg_cap, d_counts.data_ptr() + 8,
                                       d_bytes.data_ptr() if byte_cap else None, byte_cap, d_counts.data_ptr(), d_scr.data_ptr(), scratch,
                                       None), "btbbx_le_crypt_device")
    torch.cuda.synchronize()
    assert set(d_scr.cpu().numpy()[scratch:].tolist()) == {0xA5}                # nothing behind the scratch
    counts = d_counts.cpu().numpy()
    assert counts[12:].tobytes() == b"\xa5" * (len(counts) - 12)
    return (_records(d_crypt, k + 1, CRYPT), _records(d_cpkts, n + 1, CPKT), _records(d_ppkts, n + 1, DPKT), _records(d_msgs, msg_cap + 1, MSG),
            d_bytes.cpu().numpy()[:byte_cap + 64], int(counts[8:12].view(np.uint32)[0]), int(counts[:8].view(np.uint64)[0]))


def _same(got, want, kept, what):
    if got[:kept].tobytes() != want.tobytes():
        bad = [g for g in range(kept) if got[g].tobytes() != want[g].tobytes()]
        raise AssertionError("%s %d: %s, model %s (%d of %d differ)" % (what, bad[0], got[bad[0]], want[bad[0]], len(bad), kept))
    assert got[kept:].tobytes() == b"\xa5" * (got.dtype.itemsize * (len(got) - kept)), what


def _against(got, want, n, k):
    crypt, cpkts, ppkts, msgs, octets, n_msgs, n_bytes = got
    assert (n_msgs, n_bytes) == (want.n_msgs, want.n_bytes)
    _same(crypt, cm.crypt_array(want.crypt, CRYPT), k, "connection")
    _same(cpkts, cm.cpkt_array(want.cpkts, CPKT), n, "candidate")
    _same(ppkts, dm.dpkt_array(want.ppkts, DPKT), n, "plain candidate")
    _same(msgs, dm.msg_array(want.msgs, MSG), len(want.msgs), "message")
    stored = len(want.payload)
    if octets[:stored].tobytes() != want.payload:
        bad = [j for j in range(stored) if octets[j] != want.payload[j]]
        raise AssertionError("octet %d: %#x, model %#x (%d of %d differ)" % (bad[0], octets[bad[0]], want.payload[bad[0]], len(bad), stored))
    assert octets[stored:].tobytes() == b"\xa5" * (len(octets) - stored)              # nothing behind the stored prefix


def _check(b, keys, window=4, msg_cap=1 << 20, byte_cap=1 << 30, data=None):
    """The device against the model; buffers as large as the caps ask for, but no larger than the totals need."""
    data = dm.built_model(b) if data is None else data
    want = cm.crypt(b.conns, b.cands, b.pkts, data.dpkts, b.words, b.n_words, keys, window, msg_cap, byte_cap)
    got = _device(b, dm.dpkt_array(data.dpkts, DPKT), keys, window, min(msg_cap, want.n_msgs + 3), min(byte_cap, want.n_bytes + 11))
    _against(got, want, len(b.cands), len(b.conns))
    return want


def _octets(seed, n):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tolist())


def _states(b, want, g=0):
    """(role, state, skew) of connection g's members behind its START, in time order."""
    mine = sorted((i for i, c in enumerate(b.cands) if c.channel == g and b.pkts[i] is not None), key=lambda i: b.pkts[i].rank)
    start = want.crypt[g].start
    behind = mine[mine.index(start) + 1:] if start != cm.NONE else []
    return [(want.ppkts[i].role, want.cpkts[i].state, want.cpkts[i].skew) for i in behind]


# ---- the planted world ---------------------------------------------------------------------------------------------------------------
def test_the_planted_world():
    b = cm.planted_world()
    want = _check(b, list(cm.WORLD_KEYS), window=8)
    names = ("crypt: encrypts", "crypt: never encrypts", "crypt: a lost packet")
    assert cm.check_planted(b, want, names) == 19
    assert sorted(r.key for r in want.crypt if r.flags & cm.F_ARMED) == [1, 2, 0xFF]


def test_without_an_armed_connection_the_outputs_are_the_data_stages():
    """Rule 8's identity, against btbbx_le_data_device itself on the data stage's planted world."""
    import torch
    from test_gpu_le_data import _device as data_device
    b = dm.planted_world()
    for msg_cap, byte_cap in ((1 << 12, 1 << 16), (40, 1 << 16), (1 << 12, 500)):
        data, dpkts, msgs, octets, n_msgs, n_bytes = data_device(b, msg_cap, byte_cap)
        got = _device(b, dpkts[:len(b.cands)], list(cm.WORLD_KEYS), 8, msg_cap, byte_cap)
        torch.cuda.synchronize()
        assert (got[5], got[6]) == (n_msgs, n_bytes) and n_msgs > 100
        assert got[3].tobytes() == msgs.tobytes() and got[4].tobytes() == octets.tobytes() and got[2].tobytes() == dpkts.tobytes()
        assert not got[0][:-1]["flags"].any() and set(got[1][:-1]["state"].tolist()) <= {cm.CLEAR, 0xFF}


def _identity_world(name):
    """-> (world, msg_cap, byte_cap); caps None: room for every message and octet, as many as the data stage counts."""
    import _le_data_lattice as dl
    if name == "product":
        return dl.product_list(), None, None
    b = dl.sequence_world()
    assert len(b.cands) > 2048 and len(b.cands) % 2048 and len(b.conns) % 256
    if name == "sequence":
        return b, None, None
    from test_le_data_lattice_model import sequence_caps
    return (b,) + sequence_caps(dl.sequence_model())


@pytest.mark.parametrize("name", ["sequence", "sequence_under_caps", "product"])
def test_without_an_armed_connection_across_waves_and_tiles(name):
    """Rule 8's identity where the messages cross waves, workgroups and a tile of 2048 slots (the sequence worlds of
    tests/_le_data_lattice.py, with room for everything and under caps that cut the stored prefix short) and over every source residue,
    destination residue and length of a fragment (the product list): no CONTROL member of these worlds has the length of a procedure
    PDU, so no connection is ARMED (tests/test_le_crypt_model.py holds that on the model) and every output is the data stage's."""
    from test_gpu_le_data import _device as data_device
    b, msg_cap, byte_cap = _identity_world(name)
    if msg_cap is None:
        totals = data_device(b, 0, 0)
        msg_cap, byte_cap = totals[4] + 3, totals[5] + 11
    data, dpkts, msgs, octets, n_msgs, n_bytes = data_device(b, msg_cap, byte_cap)
    stored = int((msgs[:min(n_msgs, msg_cap)]["flags"] & dm.STORED != 0).sum())
    assert n_msgs > 2048 and (0 < stored < msg_cap < n_msgs if name == "sequence_under_caps" else stored == n_msgs)
    got = _device(b, dpkts[:len(b.cands)], list(cm.WORLD_KEYS), 8, msg_cap, byte_cap)
    assert (got[5], got[6]) == (n_msgs, n_bytes)
    assert got[3].tobytes() == msgs.tobytes() and got[4].tobytes() == octets.tobytes() and got[2].tobytes() == dpkts.tobytes()
    assert not got[0][:-1]["flags"].any() and set(got[1][:-1]["state"].tolist()) <= {cm.CLEAR, 0xFF}


# ---- the lattice where the kernel can go wrong ----------------------------------------------------------------------------------------
LENGTHS = (1, 15, 16, 17, 31, 32, 33, 247, 251)
MODS = (0, 1, 31, 63)


@pytest.fixture(scope="module")
def lattice():
    """Two connections under different keys on two streams: every plaintext length of LENGTHS at every packet offset of MODS mod 64
    in both roles; at the end of stream 0 a packet whose MIC lies across the stream's end, at the end of stream 1 one whose MIC lies
    wholly beyond it."""
    n_words = 1500
    h = cm.Hand(n_words, n_streams=2, seed=8)
    a, c = h.link(cm.ltk(0), stream=0), h.link(cm.ltk(1), stream=1)
    for k in (a, c):
        k.event([P(2, dm.l2cap(4, b"in the clear")), E])
        k.start()
    for n, m in enumerate(LENGTHS):
        for j, mod in enumerate(MODS):
            k = (a, c)[(n + j) & 1]
            k.event([P(2 if j & 1 else 1, _octets(100 + 4 * n + j, m)), P(2, _octets(200 + 4 * n + j, m))], mod=mod)
    end = 64 * n_words
    a.event([P(2, _octets(300, 20))], at=end - 56 - 8 * 22)                      # two octets of the MIC inside
    c.event([P(2, _octets(301, 20))], at=end - 56 - 8 * 20)                      # the MIC begins at the end
    for k in (a, c):                                                             # (counters go on behind the one that fails)
        k.event([P(2, _octets(302, 9)), P(2, _octets(303, 9))])
    assert max(h.free) < end - 56 - 8 * 22
    return h.built(), a, c


def test_the_block_and_alignment_lattice(lattice):
    b, a, c = lattice
    assert {m.offset % 64 for m in a.members + c.members if m.length >= 5} >= set(MODS)
    want = _check(b, [cm.ltk(1), cm.ltk(2), cm.ltk(0)], window=4)
    assert [r.key for r in want.crypt] == [2, 0] and [(r.n_failed, r.max_skew) for r in want.crypt] == [(1, 0), (1, 0)]
    assert want.crypt[0].n_verified + want.crypt[1].n_verified == 2 * len(LENGTHS) * len(MODS) + 4
    failed = [i for i, p in enumerate(want.cpkts) if p is not None and p.state == cm.FAILED]
    assert sorted(b.cands[i].offset + 56 + 8 * b.cands[i].length - 64 * b.n_words for i in failed) == [16, 32]   # bits of the MIC beyond the end
    plain = sorted(p for role, counter, p in a.plain + c.plain)
    seen = [want.payload[m.byte_offset:m.byte_offset + m.bytes] for m in want.msgs]
    assert all(any(p in s for s in seen) for p in plain if len(p) not in (20,))


# ---- skew ---------------------------------------------------------------------------------------------------------------------------
def _skew_link(h, removed):
    k = h.link(cm.ltk(0))
    k.start()
    k.event([P(3, b"\x06"), P(3, b"\x06")])
    k.event([P(2, _octets(1, 9)), P(2, _octets(2, 9))])
    for n in range(removed):
        k.event([E, P(2, _octets(20 + n, 6)), P(2, _octets(10 + n, 7), lost=True)])
    k.event([P(2, _octets(3, 12)), P(2, _octets(4, 12))])
    k.event([P(1, _octets(5, 30)), P(1, _octets(6, 30))])
    return k


def test_skew():
    window = 4
    h = cm.Hand(400, n_streams=1)
    for removed in (1, window - 1, window):
        _skew_link(h, removed)
    k = h.link(cm.ltk(0))                                   # a retransmission in each role and a tail event behind START
    k.start()
    k.event([P(2, _octets(30, 9)), P(2, _octets(31, 9))])
    k.event([P(0, retx=True), P(0, retx=True)])
    k.event([P(2, _octets(32, 9)), P(2, _octets(33, 9))], tail=True, clear=True)
    k.event([P(2, _octets(34, 9)), P(2, _octets(35, 9))])
    b = h.built()
    want = _check(b, [cm.ltk(0)], window=window)
    for g, removed in enumerate((1, window - 1, window)):
        st = _states(b, want, g)
        central, peripheral = ([s for s in st if s[0] == role and s[1] != cm.CLEAR] for role in (dm.CENTRAL, dm.PERIPHERAL))
        assert all(s[1:] == (cm.VERIFIED, 0) for s in peripheral) and len(peripheral) == 4 + removed     # the other role's counters stay
        tail = (cm.VERIFIED, removed) if removed < window else (cm.FAILED, 0xFF)
        assert [s[1:] for s in central] == [(cm.VERIFIED, 0)] * 2 + [tail] * 2, (removed, central)
        assert want.crypt[g].max_skew == (removed if removed < window else 0)
    st = _states(b, want, 3)
    assert [s[1] for s in st] == [cm.VERIFIED] * 2 + [cm.SKIPPED] * 4 + [cm.VERIFIED] * 2 and all(s[2] == 0 for s in st)
    assert [s[0] for s in st][4:6] == [dm.ROLE_UNKNOWN] * 2 and want.crypt[3].n_skipped == 4 and want.crypt[3].n_encrypted == 4


# ---- keys ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def two_keys():
    h = cm.Hand(200, n_streams=1, seed=4)
    for n in (0, 1):
        k = h.link(cm.ltk(n))
        k.start()
        k.event([P(3, b"\x06"), P(3, b"\x06")])
        k.event([P(2, dm.l2cap(4, _octets(40 + n, 20))), P(2, dm.l2cap(6, _octets(50 + n, 3)))])
        k.event([P(1, _octets(60 + n, 3)), E])
    b = h.built()
    return b, dm.built_model(b)


@pytest.mark.parametrize("table,keys", [
    ("first", [cm.ltk(0), cm.ltk(1), cm.ltk(5)]),
    ("last of 64", [cm.ltk(100 + n) for n in range(62)] + [cm.ltk(1), cm.ltk(0)]),
    ("absent", [cm.ltk(5), cm.ltk(6)]),
    ("twice", [cm.ltk(5), cm.ltk(1), cm.ltk(0), cm.ltk(1), cm.ltk(0)]),
    ("one key", [cm.ltk(1)])])
def test_key_tables(two_keys, table, keys):
    b, data = two_keys
    want = _check(b, keys, window=2, data=data)
    expect = {"first": [0, 1], "last of 64": [63, 62], "absent": [0xFF, 0xFF], "twice": [2, 1], "one key": [0xFF, 0]}[table]
    assert [r.key for r in want.crypt] == expect
    for r in want.crypt:
        assert r.flags == 15 + (16 if r.key != 0xFF else 0) and (r.n_verified, r.n_failed) == ((5, 0) if r.key != 0xFF else (0, 5))
    if table == "absent":                                   # rule 8: no encrypted member is a fragment; nothing else carried octets
        assert want.n_msgs == 0 and want.n_bytes == 0


# ---- the procedure --------------------------------------------------------------------------------------------------------------------
def test_malformed_procedures():
    h = cm.Hand(400, n_streams=1, seed=6)
    start5 = P(3, b"\x05")

    def traffic(k):                                         # what an encrypting pair would send behind the procedure
        k.on = True
        k.event([P(3, b"\x06"), P(3, b"\x06")])
        k.event([P(2, dm.l2cap(4, _octets(70, 11))), P(2, dm.l2cap(4, _octets(71, 5)))])

    def link(*events):
        k = h.link(cm.ltk(0))
        for e in events:
            k.event(e(k))
        traffic(k)
        return k

    cut = lambda p, n: p._replace(payload=p.payload[:n] if n < len(p.payload) else p.payload + bytes(n - len(p.payload)))   # noqa: E731
    link(lambda k: [E, k.rsp()], lambda k: [k.req(), E], lambda k: [E, start5])                          # 0: RSP before REQ
    link(lambda k: [k.req(), start5], lambda k: [E, k.rsp()])                                             # 1: START before RSP
    link(lambda k: [E, k.req()], lambda k: [E, k.rsp()], lambda k: [E, start5])                           # 2: REQ from the peripheral
    link(lambda k: [k.req(), k.rsp()], lambda k: [P(3, bytes([3]) + _octets(72, 22)), E], lambda k: [E, start5])   # 3: a second REQ
    for n in (22, 24):                                                                                      # 4, 5: L of the REQ
        link(lambda k: [cut(k.req(), n), k.rsp()], lambda k: [E, start5])
    for n in (12, 14):                                                                                      # 6, 7: L of the RSP
        link(lambda k: [k.req(), cut(k.rsp(), n)], lambda k: [E, start5])
    link(lambda k: [k.req(), k.rsp()], lambda k: [start5, E])                                             # 8: opcode 5 from the central
    link(lambda k: [k.req(), k.rsp()], lambda k: [E, P(3, b"\x05\x00")])                                  # 9: START of two octets
    b = h.built()
    want = _check(b, [cm.ltk(0)], window=2)
    assert [r.flags for r in want.crypt] == [1, 3, 0, 31, 0, 0, 1, 1, 3, 3]
    assert want.crypt[3].n_verified == 4 and [r.n_encrypted for r in want.crypt if r.flags != 31] == [0] * 9


# ---- caps and guards --------------------------------------------------------------------------------------------------------------------
def test_caps(two_keys):
    b, data = two_keys
    keys = [cm.ltk(0), cm.ltk(1)]
    whole = cm.crypt(b.conns, b.cands, b.pkts, data.dpkts, b.words, b.n_words, keys, 2, 1 << 20, 1 << 30)
    n_msgs, n_bytes = whole.n_msgs, whole.n_bytes
    assert n_msgs == 4 and n_bytes == 2 * (24 + 7 + 3)
    mid = whole.msgs[1]
    for msg_cap, byte_cap in ((0, 0), (0, 1 << 30), (1 << 20, 0), (n_msgs - 1, 1 << 30), (n_msgs, n_bytes), (1 << 20, n_bytes - 1),
                              (1 << 20, mid.byte_offset + mid.bytes - 1), (1 << 20, mid.byte_offset + mid.bytes), (1, 1 << 30)):
        want = _check(b, keys, window=2, msg_cap=msg_cap, byte_cap=byte_cap, data=data)
        assert (want.n_msgs, want.n_bytes) == (n_msgs, n_bytes)


def test_bad_arguments_are_refused_before_any_launch():
    import torch
    lib = bt.lib()
    buf = _filled(1 << 18)
    p = buf.data_ptr()
    scratch = lib.btbbx_le_crypt_scratch_bytes(8, 4, 2)
    assert scratch <= (1 << 18) - 65536

    def run(words=p, phys=p + 512, cands=p + 1024, cnt=p + 2048, conns=p + 3072, ccnt=p + 2052, tracks=p + 4096, pkts=p + 6144,
            in_dpkts=p + 8192, keys=p + 9216, n_keys=2, window=4, crypt=p + 10240, cpkts=p + 12288, ppkts=p + 14336, msgs=p + 16384, msg_cap=4,
            mcnt=p + 2056, octets=p + 18432, byte_cap=64, bcnt=p + 2064, scr=p + 65536, scr_bytes=scratch, n_words=8, pitch=8, n_streams=2):
        return lib.btbbx_le_crypt_device(words, n_words, pitch, n_streams, phys, cands, cnt, 8, conns, ccnt, 4, tracks, pkts, in_dpkts, keys,
                                         n_keys, window, crypt, cpkts, ppkts, msgs, msg_cap, mcnt, octets, byte_cap, bcnt, scr, scr_bytes, None)

    for kw in (dict(words=None), dict(phys=None), dict(cands=None), dict(cnt=None), dict(conns=None), dict(ccnt=None), dict(tracks=None),
               dict(pkts=None), dict(in_dpkts=None), dict(keys=None), dict(crypt=None), dict(cpkts=None), dict(ppkts=None), dict(msgs=None),
               dict(mcnt=None), dict(octets=None), dict(bcnt=None), dict(scr=None), dict(n_keys=0), dict(n_keys=65), dict(window=0),
               dict(window=33), dict(words=p + 4), dict(phys=p + 513), dict(cands=p + 1028), dict(conns=p + 3076), dict(tracks=p + 4100),
               dict(pkts=p + 6148), dict(in_dpkts=p + 8194), dict(crypt=p + 10244), dict(cpkts=p + 12296), dict(ppkts=p + 14338),
               dict(msgs=p + 16388), dict(octets=p + 18436), dict(scr=p + 65544), dict(cnt=p + 2050), dict(ccnt=p + 2054), dict(mcnt=p + 2058),
               dict(bcnt=p + 2068), dict(scr_bytes=scratch - 1), dict(n_words=0), dict(n_words=(1 << 42) + 1, pitch=1 << 43), dict(pitch=7),
               dict(n_streams=0)):
        assert run(**kw) == E_ARG, kw
        assert b"btbbx_le_crypt_device" in lib.btbbx_last_error()
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == b"\xa5" * len(buf)
    # null buffers with a cap of 0 are fine; counts of 0xa5a5a5a5: the caps' worth of 0xa5 records is read, no candidate is a member
    assert run(msgs=None, msg_cap=0, octets=None, byte_cap=0) == 0
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    assert got[10240:10240 + 4 * 56].tobytes() == bytes(4 * 56) and got[12288:12288 + 128].tobytes() == b"\xff" * 128
    assert got[14336:14336 + 96].tobytes() == b"\xff" * 96 and got[2056:2060].tobytes() == bytes(4) and got[2064:2072].tobytes() == bytes(8)
    assert got[16384:65536].tobytes() == b"\xa5" * (65536 - 16384) and got[:2056].tobytes() == b"\xa5" * 2056
    assert got[65536 + scratch:].tobytes() == b"\xa5" * (len(got) - 65536 - scratch)


# ---- the host wrapper and the Python entry --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain():
    """The planted world as a capture, and discovery (max_len 31), tracking, data and decryption models composed on it."""
    b = cm.planted_world()
    cap = ld.Capture(b.words, b.n_words, b.n_words, 64 * b.n_words - 39, dm.MHZ, (), 31)
    conns, cands = ld.group(ld.capture_candidates(cap, 31), 2)
    tracks, pkts = lt.track(cands, len(conns), dm.MHZ, dm.N_STREAMS, dm.UNIT, dm.IFS, dm.JITTER, lt.REMAP)
    data = dm.data(conns, cands, pkts, cap.words, cap.n_words, 1 << 20, 1 << 30)
    return cap, conns, cands, tracks, pkts, data


def test_the_host_wrapper_on_the_planted_capture(chain):
    cap, conns, cands, tracks, pkts, data = chain
    lib = bt.lib()
    keys = list(cm.WORLD_KEYS)
    planted = {(p.aa, p.crc_init) for p in cm.planted_world().planted}
    assert planted <= {(c.access_address, c.crc_init) for c in conns}
    words, phys, kbytes = np.ascontiguousarray(cap.words).reshape(-1), np.ascontiguousarray(cap.mhz, dtype=np.uint16), _keys(keys)
    for msg_cap, byte_cap in ((1 << 12, 1 << 16), (12, 1 << 16), (1 << 12, 200), (0, 0)):
        want = cm.crypt(conns, cands, pkts, data.dpkts, cap.words, cap.n_words, keys, 8, msg_cap, byte_cap)
        k, n = len(conns) + 1, len(cands) + 1
        o_conns, o_cands, o_tracks, o_pkts = np.zeros(k, CONN), np.zeros(n, CAND), np.zeros(k, TRACK), np.zeros(n, PKT)
        fill = lambda count, dtype: np.full(count * dtype.itemsize, 0xA5, np.uint8).view(dtype)          # noqa: E731
        o_data, o_dpkts, o_crypt, o_cpkts, o_ppkts = fill(k, DATA), fill(n, DPKT), fill(k, CRYPT), fill(n, CPKT), fill(n, DPKT)
        o_msgs, o_bytes = fill(msg_cap + 1, MSG), np.full(byte_cap + 8, 0xA5, np.uint8)
        counts = np.zeros(3, np.uint64)
        got = lib.btbbx_le_crypt_host(bt._ptr(words), cap.n_words, cap.pitch_words, len(cap.mhz), cap.search_bits, bt._ptr(phys), 31, 2,
                                      bt._ptr(o_conns), k, bt._ptr(o_cands), n, counts.ctypes.data, dm.UNIT, dm.IFS, dm.JITTER, lt.REMAP,
                                      bt._ptr(o_tracks), bt._ptr(o_pkts), bt._ptr(o_data), bt._ptr(o_dpkts), bt._ptr(kbytes), len(keys), 8,
                                      bt._ptr(o_crypt), bt._ptr(o_cpkts), bt._ptr(o_ppkts), bt._ptr(o_msgs) if msg_cap else None, msg_cap,
                                      counts.ctypes.data + 8, bt._ptr(o_bytes) if byte_cap else None, byte_cap, counts.ctypes.data + 16)
        assert got == len(conns), lib.btbbx_last_error()
        assert counts.tolist() == [len(cands), want.n_msgs, want.n_bytes]
        assert o_conns[:k - 1].tobytes() == ld.conn_array(conns, CONN).tobytes() and o_cands[:n - 1].tobytes() == ld.cand_array(cands, CAND).tobytes()
        assert o_tracks[:k - 1].tobytes() == lt.track_array(tracks, TRACK).tobytes() and o_pkts[:n - 1].tobytes() == lt.pkt_array(pkts, PKT).tobytes()
        _same(o_data, dm.data_array(data.data, DATA), k - 1, "data record")
        _same(o_dpkts, dm.dpkt_array(data.dpkts, DPKT), n - 1, "data candidate")
        _same(o_crypt, cm.crypt_array(want.crypt, CRYPT), k - 1, "connection")
        _same(o_cpkts, cm.cpkt_array(want.cpkts, CPKT), n - 1, "candidate")
        _same(o_ppkts, dm.dpkt_array(want.ppkts, DPKT), n - 1, "plain candidate")
        _same(o_msgs, dm.msg_array(want.msgs, MSG), len(want.msgs), "message")
        assert o_bytes[:len(want.payload)].tobytes() == want.payload and set(o_bytes[len(want.payload):].tolist()) == {0xA5}
    # the wrapper's own conditions
    def host(keys=bt._ptr(kbytes), n_keys=5, window=8, crypt=bt._ptr(o_crypt), max_len=31):
        return lib.btbbx_le_crypt_host(bt._ptr(words), cap.n_words, cap.pitch_words, len(cap.mhz), cap.search_bits, bt._ptr(phys), max_len, 2,
                                       bt._ptr(o_conns), k, bt._ptr(o_cands), n, None, dm.UNIT, dm.IFS, dm.JITTER, lt.REMAP, bt._ptr(o_tracks),
                                       bt._ptr(o_pkts), bt._ptr(o_data), bt._ptr(o_dpkts), keys, n_keys, window, crypt, bt._ptr(o_cpkts),
                                       bt._ptr(o_ppkts), None, 0, None, None, 0, None)
    for kw in (dict(keys=None), dict(n_keys=0), dict(n_keys=65), dict(window=0), dict(window=33), dict(crypt=None), dict(max_len=256)):
        assert host(**kw) == E_ARG, kw
        assert b"btbbx_le_crypt_host" in lib.btbbx_last_error()


def test_le_decrypt_from_python_on_the_planted_capture(chain):
    cap, conns, cands, tracks, pkts, data = chain
    keys = list(cm.WORLD_KEYS)
    want = cm.crypt(conns, cands, pkts, data.dpkts, cap.words, cap.n_words, keys, 8, 1 << 20, 1 << 30)
    kw = dict(max_len=31, min_count=2, n_streams=len(cap.mhz), pitch_words=cap.pitch_words, n_words=cap.n_words, unit_bits=dm.UNIT,
              ifs_bits=dm.IFS, jitter_bits=dm.JITTER)
    out = bt.le_decrypt(cap.words, cap.search_bits, cap.mhz, keys, **kw)
    g_conns, g_cands, g_tracks, g_pkts, g_data, g_dpkts, msgs, payload, crypt, cpkts, ppkts = out
    assert g_conns.tobytes() == ld.conn_array(conns, CONN).tobytes() and g_cands.tobytes() == ld.cand_array(cands, CAND).tobytes()
    assert g_data.tobytes() == dm.data_array(data.data, DATA).tobytes() and g_dpkts.tobytes() == dm.dpkt_array(data.dpkts, DPKT).tobytes()
    assert crypt.tobytes() == cm.crypt_array(want.crypt, CRYPT).tobytes() and cpkts.tobytes() == cm.cpkt_array(want.cpkts, CPKT).tobytes()
    assert ppkts.tobytes() == dm.dpkt_array(want.ppkts, DPKT).tobytes()
    assert msgs.tobytes() == dm.msg_array(want.msgs, MSG).tobytes() and payload.tobytes() == want.payload
    # the planted plaintext comes out of the capture, octet for octet
    by = {(int(c["access_address"]), int(c["crc_init"])): g for g, c in enumerate(g_conns)}
    for p in cm.planted_world().planted:
        if p.name != "crypt: a key that is not in the table":
            mine = msgs[msgs["conn"] == by[(p.aa, p.crc_init)]]
            assert [(int(m["role"]), payload[int(m["byte_offset"]):int(m["byte_offset"]) + int(m["bytes"])].tobytes()) for m in mine] == p.messages
    with pytest.raises(bt.BtbbError):
        bt.le_decrypt(cap.words, cap.search_bits, cap.mhz, keys, msg_cap=5, **kw)
    # the same key as an array, a window of one: the connection with two lost packets keeps its key (the probes lie before them)
    one = bt.le_decrypt(cap.words, cap.search_bits, cap.mhz, np.frombuffer(b"".join(keys), np.uint8).reshape(-1, 16), window=1, **kw)
    assert one[8]["key"].tolist() == crypt["key"].tolist() and one[8]["n_failed"].sum() > crypt["n_failed"].sum()
