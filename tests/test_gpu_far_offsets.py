"""Every stream-taking entry beyond bit 2^32 and byte 2^32: the far capture of tests/_far.py -- two streams of a little more
than 2^29 words, zero except for copies of a short capture near the start, across word 2^26 and across word 2^29 -- built once
in HBM.  The expectation is always the model's result on the short references (the oracle port, the plain-Python LE models)
moved by each copy's base; the same entry on the short reference must give the untranslated list as well.  Integer logic
throughout: everything is compared for equality, every count included; output buffers start as 0xA5 and are checked behind their
counts (the records of a d_out that a call decodes start as zeros: the decoders take them for the packet's earlier state)."""
import collections
import ctypes as C

import numpy as np
import pytest

import _far
import _acquire as aq
import _follow as fw
import _hop
import _le
import _le_discover as ld
import _libs
import _order_model as om
import _survey as sv
import _trial_lattice as tl
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu
LAPS = (bt.LAP_ANY,) + _far.KNOWN_LAPS
CAND, CONN = bt.LE_CAND_DTYPE, bt.LE_CONN_DTYPE
Cap = collections.namedtuple("Cap", "t ptr n_words pitch bits far")


@pytest.fixture(scope="module", autouse=True)
def ready():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    bt.lib().btbbx_shutdown()
    bt.init(2)
    orc = _libs.oracle()
    orc.orc_reset_syndrome_map()
    orc.orc_init(2)
    yield
    bt.lib().btbbx_shutdown()


@pytest.fixture(scope="module")
def cap():
    """The far capture: about 8 GiB of zeros allocated on the device, the copies of S written by slice assignment."""
    import torch
    f = _far.far()
    t = torch.zeros(2 * f.pitch_words, dtype=torch.int64, device="cuda")
    for c in f.copies:
        at = c.stream * f.pitch_words + c.base
        t[at:at + len(f.words[c.stream])] = _dev(f.words[c.stream])[:len(f.words[c.stream])]
    torch.cuda.synchronize()
    yield Cap(t, t.data_ptr(), f.n_words, f.pitch_words, 64 * f.n_words - 63, f)
    del t
    torch.cuda.empty_cache()


_FAULT = []


@pytest.fixture(autouse=True)
def nothing_is_launched_after_a_gpu_fault():
    """a HIP error is sticky: once a test has met one, the others fail here instead of launching more work on that device"""
    import torch
    assert not _FAULT, _FAULT
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        _FAULT.append(str(e))
        raise


def _dev(a):
    """a host array in HBM, as int64 words (padded by at least eight bytes)"""
    import torch
    a = np.ascontiguousarray(a)
    raw = a.tobytes()
    raw += bytes((-len(raw)) % 8 + 8)
    return torch.from_numpy(np.frombuffer(raw, np.int64).copy()).cuda()


def _filled(nbytes, value=0xA5):
    import torch
    return torch.full(((nbytes + 7) // 8 * 8 + 8,), value, dtype=torch.uint8, device="cuda")


def _host(t, dtype, n):
    return t.cpu().numpy()[:n * np.dtype(dtype).itemsize].view(dtype)


def _sync():
    import torch
    torch.cuda.synchronize()


def _tuples(recs):
    return [(int(h["stream"]), int(h["offset"]), int(h["lap"]), int(h["ac_errors"])) for h in recs]


def _same(got, want, ctx):
    if got != want:
        g, w = set(got), set(want)
        raise AssertionError((ctx, len(got), len(want), "missing", sorted(w - g)[:6], "extra", sorted(g - w)[:6],
                              "first difference", next((i, a, b) for i, (a, b) in enumerate(zip(got + [None], want + [None])) if a != b)))


# ---- scans -------------------------------------------------------------------------------------------------------------
def _scan(ptr, n_words, pitch, n_streams, bits, lap, max_err, room, mode, fmt=None):
    """One scan launch -> (count, records up to the count as tuples, the rest of the buffer untouched?, slot header or None).
    mode: "plain", "slots" (the ordered call with the segment-slot scratch) or "general" (with the general-ordering scratch)."""
    import torch
    lib = bt.lib()
    hit_cap = room + 64
    d_h = _filled(hit_cap * 16)
    header = None
    if mode == "plain":
        d_c = torch.zeros(4, dtype=torch.int32, device="cuda")
        if fmt is None:
            bt.check(lib.btbbx_scan_device(ptr, n_words, pitch, n_streams, bits, lap, max_err, d_h.data_ptr(), hit_cap, d_c.data_ptr(), None), "scan")
        else:
            bt.check(lib.btbbx_scan_device_fmt(ptr, n_words, pitch, n_streams, bits, lap, max_err, fmt, d_h.data_ptr(), hit_cap, d_c.data_ptr(), None), "scan_fmt")
    else:
        front = lib.btbbx_order_hits_scratch_bytes(hit_cap)
        sb = lib.btbbx_scan_ordered_scratch_bytes(bits, n_streams, lap, hit_cap) if mode == "slots" else front
        assert (sb > front) == (mode == "slots")
        d_s = torch.empty(sb // 8 + 2, dtype=torch.int64, device="cuda")
        d_c = torch.full((4,), 12345, dtype=torch.int32, device="cuda")          # stale: the call zeroes it itself
        if fmt is None:
            bt.check(lib.btbbx_scan_ordered_device(ptr, n_words, pitch, n_streams, bits, lap, max_err, d_h.data_ptr(), hit_cap, d_c.data_ptr(),
                                                   d_s.data_ptr(), sb, None), "scan_ordered")
        else:
            bt.check(lib.btbbx_scan_ordered_device_fmt(ptr, n_words, pitch, n_streams, bits, lap, max_err, fmt, d_h.data_ptr(), hit_cap,
                                                       d_c.data_ptr(), d_s.data_ptr(), sb, None), "scan_ordered_fmt")
        _sync()
        if mode == "slots":
            at = om.slot_header_offset(front) // 8
            header = om.slot_header(d_s[at:at + 2].cpu().numpy().view(np.uint32))
        del d_s
    _sync()
    cnt = int(d_c[0].item()) & 0xFFFFFFFF
    recs = _host(d_h, bt.HIT_DTYPE, hit_cap)
    k = min(cnt, hit_cap)
    assert (recs["reserved"][:k] == 0).all()
    return cnt, _tuples(recs[:k]), recs[k:].tobytes() == b"\xa5" * (16 * (hit_cap - k)), header


def _far_want(lap, max_err=2):
    return _far.union(lambda s, ends: _far.find_all(s, ends, lap, max_err))


def _check_scan(cap, lap, mode, fmt=None, max_err=2):
    want = _far_want(lap, max_err)
    cnt, got, clean, header = _scan(cap.ptr, cap.n_words, cap.pitch, 2, cap.bits, lap, max_err, len(want), mode, fmt)
    ctx = (hex(lap), mode, fmt, max_err)
    assert cnt == len(want), (ctx, cnt, len(want))
    _same(got if mode != "plain" else sorted(got), want, ctx)
    assert clean, ctx                                     # nothing behind the count, in the ordered calls too
    if header is not None:
        assert header.irregular == 0, (ctx, header)
    return len(want)


_REV = np.array([int("{:08b}".format(b)[::-1], 2) for b in range(256)], np.uint8)      # a byte's bits turned round


def _check_short(lap, mode, max_err=2, fmt=None):
    """the same entry on the short references: the untranslated list (fmt: the reference turned MSB-first on the host)"""
    for s in (0, 1):
        for ends in (False, True):
            w = _far.ref_words(s, ends)
            want = [(0,) + h for h in _far.find_all(s, ends, lap, max_err)]
            d_w = _dev(w if fmt is None else _REV[w.view(np.uint8)].view(np.uint64))
            cnt, got, clean, _ = _scan(d_w.data_ptr(), len(w), len(w), 1, 64 * len(w) - 63, lap, max_err, len(want), mode, fmt)
            assert cnt == len(want) and clean, (hex(lap), mode, fmt, s, ends, cnt, len(want))
            _same(got if mode != "plain" else sorted(got), want, (hex(lap), mode, fmt, s, ends))


def _short_cap(s, ends):
    """the short reference (s, ends) in HBM, as a capture of one stream"""
    w = _far.ref_words(s, ends)
    t = _dev(w)
    return Cap(t, t.data_ptr(), len(w), len(w), 64 * len(w) - 63, None)


def _short_sets(rows):
    """[((stream, ends), indices into rows)]: the rows that each short reference models"""
    return [((s, ends), [i for i, r in enumerate(rows) if (r.stream, r.ends) == (s, ends)]) for s in (0, 1) for ends in (False, True)]


@pytest.mark.parametrize("mode", ["plain", "slots", "general"])
@pytest.mark.parametrize("lap", LAPS)
def test_scan(cap, lap, mode):
    """btbbx_scan_device and btbbx_scan_ordered_device (segment slots + compaction; the general ordering) over both streams with the
    full search_bits: the sorted / the ordered list equals the oracle port's on the short references, moved; the slots'
    irregular flag stays clear."""
    n = _check_scan(cap, lap, mode)
    assert n > (200 if lap == bt.LAP_ANY else 40)
    _check_short(lap, mode)


@pytest.mark.parametrize("lap", LAPS)
def test_scan_with_search_bits_inside_the_last_copy(cap, lap):
    """search_bits ends right behind a hit of the copy across byte 2^32, with more hits in the words behind it: the ragged tile's
    validity mask is formed from search_bits - first_off at offsets beyond 2^35.  The hit at search_bits - 1 is reported, the one
    behind it is not."""
    everything = _far_want(lap)
    above = [w for w in everything if w[0] == 1 and w[1] >= 1 << 35]
    pivot = [a for a, b in zip(above, above[1:]) if b[1] - a[1] <= 128 and (a[1] + 1) % 32][-1]      # the next hit lies within two words
    bits = pivot[1] + 1
    want = [w for w in everything if w[1] < bits]
    assert pivot in want and any(w[0] == 1 and bits <= w[1] < bits + 128 for w in everything) and bits % 32
    for mode in ("plain", "slots"):
        cnt, got, clean, header = _scan(cap.ptr, cap.n_words, cap.pitch, 2, bits, lap, 2, len(want), mode)
        assert cnt == len(want), (hex(lap), mode, cnt, len(want))
        _same(got if mode != "plain" else sorted(got), want, (hex(lap), mode, bits))
        assert header is None or header.irregular == 0


def test_msb_first_scans_and_the_turn_round_kernel(cap):
    """btbbx_msb_to_lsb_device over the whole far capture (2^30 words) turns it into the MSB-first capture of the same symbols
    (byte-wise bit reversal, its own inverse: test_far_model.py); the MSB-first scans then give the same lists; turned back the
    capture is what it was; and the MSB-first scans of the short references give the untranslated lists."""
    import torch
    lib, f = bt.lib(), cap.far
    rev = _REV
    sample = np.unique(np.concatenate([np.arange(0, 4096), np.random.default_rng(5).integers(0, 2 * cap.pitch, 4096),
                                       (1 << 26) + np.arange(-2048, 2048) - 4000, 2 * cap.pitch - 1 - np.arange(4096)]))
    d_sample = torch.from_numpy(sample).cuda()

    def look(turned):
        for c in f.copies:
            at = c.stream * cap.pitch + c.base
            got = cap.t[at - 64:at + len(f.words[c.stream]) + (0 if c.ends else 64)].cpu().numpy().view(np.uint8)
            want = (f.R_end if c.ends else f.R_in)[c.stream].view(np.uint8)
            assert np.array_equal(got, rev[want] if turned else want), (c.name, turned)
        inside = np.zeros(len(sample), bool)
        for c in f.copies:
            at = c.stream * cap.pitch + c.base
            inside |= (sample >= at) & (sample < at + len(f.words[c.stream]))
        assert (cap.t[d_sample].cpu().numpy()[~inside] == 0).all() and (~inside).sum() > 5000, turned

    bt.check(lib.btbbx_msb_to_lsb_device(cap.ptr, 2 * cap.pitch, None), "msb_to_lsb")
    _sync()
    try:
        look(True)
        for lap in LAPS:
            _check_scan(cap, lap, "plain", fmt=2)
            _check_scan(cap, lap, "slots", fmt=2)
    finally:
        bt.check(lib.btbbx_msb_to_lsb_device(cap.ptr, 2 * cap.pitch, None), "msb_to_lsb")
        _sync()
    look(False)
    for lap in LAPS:                                       # the same two entries on the short references, turned round on the host
        _check_short(lap, "plain", fmt=2)
        _check_short(lap, "slots", fmt=2)


@pytest.mark.parametrize("n_init", [3, 5])
def test_scan_with_larger_tables(cap, n_init):
    """btbb_init(3): the two-level form of scan_slide_kernel; btbb_init(5): scan_lap_any_kernel.  LAP_ANY at max_ac_errors = the
    table's; the oracle port with the same tables on the short references."""
    lib, orc = bt.lib(), _libs.oracle()
    try:
        lib.btbbx_shutdown()
        orc.orc_reset_syndrome_map()
        assert lib.btbb_init(n_init) == 0 and orc.orc_init(n_init) == 0
        assert lib.btbbx_table_errors() == n_init
        n = _check_scan(cap, bt.LAP_ANY, "plain", max_err=n_init)
        assert n > len(_far_want(bt.LAP_ANY, 2))
        _check_short(bt.LAP_ANY, "plain", max_err=n_init)
    finally:
        lib.btbbx_shutdown()
        orc.orc_reset_syndrome_map()
        bt.init(2)
        orc.orc_init(2)


# ---- cut and decode ----------------------------------------------------------------------------------------------------
Row = collections.namedtuple("Row", "stream offset ref_offset ends index")


def _rows():
    """the translated hit list of (b), in (stream, offset) order"""
    rows = [Row(s, 64 * c.base + o, 64 * _far.PAD + o, c.ends, i) for s in (0, 1) for c in _far.copies_of(s) for o, i in _far.br_hits(s)]
    # ... and cuts in the near copy where the low 32 bits of total_bits - offset pass max_length: a captured length formed in 32 bits
    # would be 0, 1, 122, 3124 there (whatever S holds at these places is cut out and decoded)
    f = _far.far()
    a = f.copies[0]
    low = (64 * f.n_words) % (1 << 32)
    for r in (0, 1, 122, 1000, 3124, 3125, 3126):
        o = low - r - 64 * a.base
        assert a.stream == 0 and 0 <= o < len(f.S[0]) - 4096 and 64 * f.n_words - (low - r) >= 1 << 32
        rows.append(Row(0, low - r, 64 * _far.PAD + o, False, _far.br_hits(0)[0][1]))
    return sorted(rows)


def _hit_array(rows, far=True):
    hits = np.zeros(len(rows), bt.HIT_DTYPE)
    hits["stream"] = [r.stream if far else 0 for r in rows]
    hits["offset"] = [r.offset if far else r.ref_offset for r in rows]
    hits["lap"] = [0x111111 + r.index for r in rows]
    return hits


def _entries(rows, lat):
    idx = np.array([r.index for r in rows])
    pin = lat.pin[idx].copy()
    pin["clkn"] = lat.clk6[idx].astype(np.uint32) | (((idx * 2654435761) >> 8) & 0xFFFFF).astype(np.uint32) << 6
    pin["uap"] = lat.uap[idx]
    pin["flags"] |= tl.F_UAP_VALID | tl.F_CLK6_VALID
    pin["length"] = 0xA5A5A5A5                             # ignored by the entries that cut for themselves
    return pin


def _slices(rows, max_length=bt.MAX_SYMBOLS):
    return [_far.br_slice(r.stream, r.ends, r.ref_offset, max_length) for r in rows]


def _fields_equal(got, want, rows, lat, ctx):
    for f in bt.PKTOUT_DTYPE.names:
        bad = np.nonzero((got[f] != want[f]).reshape(len(got), -1).any(axis=1))[0]
        assert not len(bad), (ctx, f, len(bad), [(int(r), rows[r], lat.tags[rows[r].index]) for r in bad[:5]])


@pytest.fixture(scope="module")
def cut():
    """rows, hits, entries, the plain slices of the short references and the oracle port's decode of them -- computed once"""
    lat = tl.lattice()
    rows = _rows()
    pin = _entries(rows, lat)
    syms = _slices(rows)
    want = tl.oracle_decode(_libs.oracle(), syms, pin)
    assert (want["payload_rv"] == 10).sum() >= 20 and sum(len(s) < bt.MAX_SYMBOLS for s in syms) >= 4
    assert sum(r.offset >= 1 << 32 for r in rows) >= 80 and sum(r.offset >= 1 << 35 for r in rows) >= 30
    return collections.namedtuple("Cut", "lat rows hits pin syms want")(lat, rows, _hit_array(rows), pin, syms, want)


def test_gather_packets(cap, cut):
    """btbbx_gather_packets_device: packets and lengths are plain slices of the short references, on the far capture and on the
    short references themselves"""
    def gather(c, hits, max_length):
        n = len(hits)
        d_h, d_pk, d_len = _dev(hits), _filled((n + 1) * 400), _filled((n + 1) * 4)
        bt.check(bt.lib().btbbx_gather_packets_device(c.ptr, c.n_words, c.pitch, d_h.data_ptr(), n, max_length, d_pk.data_ptr(),
                                                      d_len.data_ptr(), None), "gather")
        _sync()
        got_len, got = _host(d_len, np.uint32, n + 1), _host(d_pk, np.uint64, (n + 1) * 50).reshape(n + 1, 50)
        assert got_len[n] == 0xA5A5A5A5 and (got[n] == 0xA5A5A5A5A5A5A5A5).all()
        return got[:n], got_len[:n]

    for max_length in (bt.MAX_SYMBOLS, 1000):
        words, lengths = bt.packets_to_words(_slices(cut.rows, max_length))
        got, got_len = gather(cap, cut.hits, max_length)
        assert np.array_equal(got_len, lengths), (max_length, np.nonzero(got_len != lengths)[0][:5])
        bad = np.nonzero((got != words).any(axis=1))[0]
        assert not len(bad), (max_length, [(cut.rows[i], np.nonzero(got[i] != words[i])[0][:4]) for i in bad[:4]])
        for key, sel in _short_sets(cut.rows):             # the short references: the same rows at their untranslated offsets
            got, got_len = gather(_short_cap(*key), _hit_array([cut.rows[i] for i in sel], far=False), max_length)
            assert np.array_equal(got_len, lengths[sel]) and np.array_equal(got, words[sel]), (max_length, key)
    assert (lengths == 1000).sum() > 100


def _decode_hits_far(cap, hits, pin, counted=None, room=0):
    import torch
    lib = bt.lib()
    n = len(hits)
    d_h = _dev(np.concatenate([hits, np.zeros(room, bt.HIT_DTYPE)]))
    d_in = _dev(np.concatenate([pin, np.zeros(room, bt.PKTIN_DTYPE)]))
    # d_out is the one table these entries want zeroed on entry: the decoders take what a record holds for the packet's earlier
    # state and leave alone what they do not assign (as a fresh packet of the oracle starts from zeros; tests/test_gpu_follow.py
    # does the same).  So the n records the call decodes start as zeros and everything behind them as 0xA5.
    d_out = _filled((n + room + 1) * bt.PKTOUT_DTYPE.itemsize)
    d_out[:n * bt.PKTOUT_DTYPE.itemsize] = 0
    d_len = _filled((n + room + 1) * 4)
    if counted is None:
        bt.check(lib.btbbx_decode_hits_device(cap.ptr, cap.n_words, cap.pitch, d_h.data_ptr(), d_in.data_ptr(), n, bt.MAX_SYMBOLS,
                                              d_out.data_ptr(), d_len.data_ptr(), None), "decode_hits")
    else:
        d_c = _dev(np.array([counted, 0], np.uint32))
        bt.check(lib.btbbx_decode_hits_counted_device(cap.ptr, cap.n_words, cap.pitch, d_h.data_ptr(), d_in.data_ptr(), d_c.data_ptr(), n + room,
                                                      bt.MAX_SYMBOLS, d_out.data_ptr(), d_len.data_ptr(), None), "decode_hits_counted")
    _sync()
    return _host(d_out, bt.PKTOUT_DTYPE, n + room + 1), _host(d_len, np.uint32, n + room + 1)


def test_decode_hits(cap, cut):
    """btbbx_decode_hits_device against the oracle port's decode of the slices, every field; against gather + btbbx_decode_device
    byte for byte; the same list on the short references; btbbx_decode_hits_counted_device with the count in HBM."""
    import torch
    lib, n = bt.lib(), len(cut.rows)
    want_len = np.array([len(s) for s in cut.syms], np.uint32)
    out, lens = _decode_hits_far(cap, cut.hits, cut.pin)
    assert np.array_equal(lens[:n], want_len) and lens[n] == 0xA5A5A5A5
    _fields_equal(out[:n], cut.want, cut.rows, cut.lat, "far")
    assert out[n:].tobytes() == b"\xa5" * bt.PKTOUT_DTYPE.itemsize
    # gather + decode
    d_h, d_pk, d_len = _dev(cut.hits), _filled(n * 400), _filled(n * 4)
    bt.check(lib.btbbx_gather_packets_device(cap.ptr, cap.n_words, cap.pitch, d_h.data_ptr(), n, bt.MAX_SYMBOLS, d_pk.data_ptr(), d_len.data_ptr(), None))
    _sync()
    pin = cut.pin.copy()
    pin["length"] = _host(d_len, np.uint32, n)
    d_in = _dev(pin)
    d_out = torch.zeros(n * bt.PKTOUT_DTYPE.itemsize + 8, dtype=torch.uint8, device="cuda")
    bt.check(lib.btbbx_decode_device(d_pk.data_ptr(), d_in.data_ptr(), n, d_out.data_ptr(), None), "decode")
    _sync()
    two_step = _host(d_out, bt.PKTOUT_DTYPE, n)
    bad = [i for i in range(n) if two_step[i].tobytes() != out[i].tobytes()]
    assert not bad, (len(bad), [cut.rows[i] for i in bad[:5]])
    # the short references
    for s in (0, 1):
        for ends in (False, True):
            sel = [i for i, r in enumerate(cut.rows) if (r.stream, r.ends) == (s, ends)]
            short, short_len = bt.run_decode_hits(_far.ref_words(s, ends)[None, :], _hit_array([cut.rows[i] for i in sel], far=False), cut.pin[sel])
            assert np.array_equal(short_len, want_len[sel]) and short.tobytes() == out[sel].tobytes(), (s, ends)
    # counted: eight records of room behind the list, which stay as they were
    out_c, len_c = _decode_hits_far(cap, cut.hits, cut.pin, counted=n, room=8)
    assert out_c[:n].tobytes() == out[:n].tobytes() and np.array_equal(len_c[:n], want_len)
    assert out_c[n:].tobytes() == b"\xa5" * (9 * bt.PKTOUT_DTYPE.itemsize) and (len_c[n:] == 0xA5A5A5A5).all()
    for key, sel in _short_sets(cut.rows):                 # ... and on the short references
        k = len(sel)
        out_s, len_s = _decode_hits_far(_short_cap(*key), _hit_array([cut.rows[i] for i in sel], far=False), cut.pin[sel], counted=k, room=8)
        assert out_s[:k].tobytes() == out[sel].tobytes() and np.array_equal(len_s[:k], want_len[sel]), key
        assert out_s[k:].tobytes() == b"\xa5" * (9 * bt.PKTOUT_DTYPE.itemsize) and (len_s[k:] == 0xA5A5A5A5).all(), key


@pytest.mark.parametrize("clk_div,clk_phase", [(625, 346), (4096, 1234)])
def test_decode_hits_piconet_phase(cap, cut, clk_div, clk_phase):
    """every packet's clock is clkn + (offset + phase) / clk_div in Python integers, reduced to 32 bits as the header says"""
    lib = bt.lib()
    entry = sv.entry_state(0x2A5)
    want_len = np.array([len(s) for s in cut.syms], np.uint32)

    def run(c, rows, far, ctx):
        n = len(rows)
        hits = _hit_array(rows, far)
        d_h = _dev(hits)
        d_out = _filled((n + 1) * bt.PKTOUT_DTYPE.itemsize)                 # (zeros where the call decodes: see _decode_hits_far)
        d_out[:n * bt.PKTOUT_DTYPE.itemsize] = 0
        d_len = _filled((n + 1) * 4)
        bt.check(lib.btbbx_decode_hits_piconet_phase_device(c.ptr, c.n_words, c.pitch, d_h.data_ptr(), None, n, entry.ctypes.data_as(C.c_void_p),
                                                            clk_div, clk_phase, bt.MAX_SYMBOLS, d_out.data_ptr(), d_len.data_ptr(), None), "piconet_phase")
        _sync()
        pin = np.repeat(entry, n)
        pin["clkn"] = [(0x2A5 + (int(o) + clk_phase) // clk_div) & 0xFFFFFFFF for o in hits["offset"]]
        want = tl.oracle_decode(_libs.oracle(), [cut.syms[r] for r in rows_index(rows)], pin)
        out, lens = _host(d_out, bt.PKTOUT_DTYPE, n + 1), _host(d_len, np.uint32, n + 1)
        _fields_equal(out[:n], want, rows, cut.lat, (clk_div, clk_phase, ctx))
        assert np.array_equal(lens[:n], want_len[rows_index(rows)]), ctx
        assert out[n:].tobytes() == b"\xa5" * bt.PKTOUT_DTYPE.itemsize and lens[n] == 0xA5A5A5A5, ctx
        return pin

    where = {id(r): i for i, r in enumerate(cut.rows)}

    def rows_index(rows):
        return [where[id(r)] for r in rows]

    pin = run(cap, cut.rows, True, "far")
    assert len(set((pin["clkn"] & 63).tolist())) > 20
    for key, sel in _short_sets(cut.rows):                 # the short references: the clock follows the untranslated offset
        run(_short_cap(*key), [cut.rows[i] for i in sel], False, key)


# ---- LE ----------------------------------------------------------------------------------------------------------------
def _le_decode_far(cap, hits, crc_init, d_phys):
    import torch
    n = len(hits)
    d_h, d_c = _dev(hits), _dev(np.array([n, 0], np.uint32))
    d_out = _filled((n + 1) * bt.LE_PKT_DTYPE.itemsize)
    bt.check(bt.lib().btbbx_le_decode_hits_device(cap.ptr, cap.n_words, cap.pitch, d_h.data_ptr(), d_c.data_ptr(), n, d_phys.data_ptr(), crc_init,
                                                  d_out.data_ptr(), None), "le_decode_hits")
    _sync()
    out = _host(d_out, bt.LE_PKT_DTYPE, n + 1)
    assert out[n:].tobytes() == b"\xa5" * bt.LE_PKT_DTYPE.itemsize
    return out[:n]


def test_le_scan_and_decode(cap):
    """btbbx_le_scan_device over both streams for the advertising access address, then btbbx_le_decode_hits_device on the ordered
    list, against _le.match_all and _le.decode on the short references"""
    import torch
    lib = bt.lib()
    want = _far.union(lambda s, ends: _far.le_matches(s, ends))
    bits = 64 * cap.n_words - 39
    hit_cap = len(want) + 64
    d_h, d_c = _filled(hit_cap * 16), torch.zeros(4, dtype=torch.int32, device="cuda")
    bt.check(lib.btbbx_le_scan_device(cap.ptr, cap.n_words, cap.pitch, 2, bits, _le.ADV_AA, _far.LE_SCAN_ERRORS, d_h.data_ptr(), hit_cap,
                                      d_c.data_ptr(), None), "le_scan")
    _sync()
    cnt = int(d_c[0].item())
    recs = _host(d_h, bt.HIT_DTYPE, hit_cap)
    assert cnt == len(want) and recs[cnt:].tobytes() == b"\xa5" * (16 * (hit_cap - cnt))
    _same(sorted(_tuples(recs[:cnt])), want, "le_scan")
    assert sum(s == 1 and o >= 1 << 32 for s, o, _, _ in want) >= 16 and len({e for _, _, _, e in want}) == 3
    # search_bits that ends between the two packets at the end of the last copy, 79 bits apart and above bit 2^35
    near = [(x, y) for x, y in zip(want, want[1:]) if x[0] == y[0] == 1 and x[1] >= 1 << 35 and y[1] - x[1] == 79]
    assert len(near) == 1
    cut = near[0][0][1] + 1
    d_h2, d_c2 = _filled(hit_cap * 16), torch.zeros(4, dtype=torch.int32, device="cuda")
    bt.check(lib.btbbx_le_scan_device(cap.ptr, cap.n_words, cap.pitch, 2, cut, _le.ADV_AA, _far.LE_SCAN_ERRORS, d_h2.data_ptr(), hit_cap,
                                      d_c2.data_ptr(), None), "le_scan")
    _sync()
    cnt2 = int(d_c2[0].item())
    assert cnt2 == sum(w[1] < cut for w in want) and cut % 32
    _same(sorted(_tuples(_host(d_h2, bt.HIT_DTYPE, hit_cap)[:cnt2])), [w for w in want if w[1] < cut], "le_scan, cut")
    hits = np.zeros(cnt, bt.HIT_DTYPE)
    for i, (s, o, aa, e) in enumerate(want):
        hits[i] = (o, aa, e, 0, s)
    d_phys = _dev(np.array(_far.MHZ, np.uint16))
    got = _le_decode_far(cap, hits, _le.ADV_CRC_INIT, d_phys)
    model = []
    for s in (0, 1):
        for c in _far.copies_of(s):
            w = _far.ref_words(s, c.ends)
            for o, aa, e in _far.le_matches(s, c.ends):
                d = _le.decode(w, len(w), s, o, e, _far.MHZ[s], _le.ADV_CRC_INIT)
                d["offset"] = _far.moved(o, c)
                model.append(d)
    model.sort(key=lambda d: (d["stream"], d["offset"]))
    _le.compare(got, model, _far.MHZ)
    assert sum(d["crc_ok"] for d in model) >= 12 and sum(d["truncated"] for d in model) >= 1
    # the short references
    for s, ends in ((1, False), (1, True)):
        w = _far.ref_words(s, ends)
        short = bt.le_scan(w, 64 * len(w) - 39, _far.MHZ[s], max_errors=_far.LE_SCAN_ERRORS)
        _le.compare(short, [_le.decode(w, len(w), 0, o, e, _far.MHZ[s], _le.ADV_CRC_INIT) for o, aa, e in _far.le_matches(s, ends)], [_far.MHZ[s]])


@pytest.mark.parametrize("max_len", [27, 255])
def test_le_discover_scan_and_group(cap, max_len):
    """btbbx_le_discover_scan_device against _le_discover.candidates moved; btbbx_le_discover_group_device on that scan's own
    output, its count left on the device, against _le_discover.group of the moved candidates; every CRCInit found gives a good
    CRC in btbbx_le_decode_hits_device."""
    import torch
    lib = bt.lib()
    model = _far.far_candidates(max_len)
    want_conns, want_cands = ld.group(model, 2)
    cand_cap, conn_cap = len(model) + 32, len(want_conns) + 8
    d_phys = _dev(np.array(_far.MHZ, np.uint16))
    d_cands, d_conns = _filled(cand_cap * CAND.itemsize), _filled(conn_cap * CONN.itemsize)
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    bt.check(lib.btbbx_le_discover_scan_device(cap.ptr, cap.n_words, cap.pitch, 2, 64 * cap.n_words - 39, d_phys.data_ptr(), max_len,
                                               d_cands.data_ptr(), cand_cap, d_cnt.data_ptr(), None), "le_discover_scan")
    _sync()
    n = int(d_cnt[0].item())
    recs = _host(d_cands, CAND, cand_cap)
    assert n == len(model), (n, len(model))
    _same(sorted(ld.cand_tuples(recs[:n])), sorted(model), ("candidates", max_len))
    assert recs[n:].tobytes() == b"\xa5" * (CAND.itemsize * (cand_cap - n))
    if max_len == 255:                                  # (the first of the two has 37 octets)
        # search_bits that ends between two candidates 79 bits apart above bit 2^32 (the end of the copy across it): rule 6
        order = sorted(model, key=lambda c: (c.stream, c.offset))
        near = [x for x, y in zip(order, order[1:]) if x.stream == y.stream and x.offset >= 1 << 32 and y.offset - x.offset == 79]
        assert len(near) == 1 and (near[0].offset + 1) % 32
        d_cands2, d_cnt2 = _filled(cand_cap * CAND.itemsize), torch.zeros(4, dtype=torch.int32, device="cuda")
        bt.check(lib.btbbx_le_discover_scan_device(cap.ptr, cap.n_words, cap.pitch, 2, near[0].offset + 1, d_phys.data_ptr(), max_len,
                                                   d_cands2.data_ptr(), cand_cap, d_cnt2.data_ptr(), None), "le_discover_scan")
        _sync()
        below = sorted(c for c in model if c.offset <= near[0].offset)
        assert int(d_cnt2[0].item()) == len(below) < len(model)
        _same(sorted(ld.cand_tuples(_host(d_cands2, CAND, cand_cap)[:len(below)])), below, ("candidates, cut", max_len))
    scratch = lib.btbbx_le_discover_scratch_bytes(cand_cap)
    d_scr = torch.zeros(scratch // 8 + 2, dtype=torch.int64, device="cuda")
    bt.check(lib.btbbx_le_discover_group_device(d_cands.data_ptr(), d_cnt.data_ptr(), cand_cap, 2, d_conns.data_ptr(), conn_cap,
                                                d_cnt.data_ptr() + 4, d_scr.data_ptr(), scratch, None), "le_discover_group")
    _sync()
    assert (int(d_cnt[0].item()), int(d_cnt[1].item())) == (n, len(want_conns))
    got_conns, got_cands = _host(d_conns, CONN, conn_cap), _host(d_cands, CAND, cand_cap)
    assert got_cands[:n].tobytes() == ld.cand_array(want_cands, CAND).tobytes()
    assert got_conns[:len(want_conns)].tobytes() == ld.conn_array(want_conns, CONN).tobytes()
    assert got_conns[len(want_conns):].tobytes() == b"\xa5" * (8 * CONN.itemsize) and got_cands[n:].tobytes() == b"\xa5" * (32 * CAND.itemsize)
    planted = {p.meta["conn"] for p in cap.far.plants[0] if p.kind == "le" and p.meta["length"] <= max_len}
    assert len(want_conns) >= len(planted) == 2 and max(c.n_packets for c in want_conns) >= 20 and sum(c.offset >= 1 << 35 for c in model) >= 8
    by_init = collections.defaultdict(list)
    for c in model:
        by_init[c.crc_init].append(c)
    for init, members in by_init.items():
        hits = np.zeros(len(members), bt.HIT_DTYPE)
        for i, c in enumerate(members):
            hits[i] = (c.offset, c.access_address, 0, 0, c.stream)
        for c, o in zip(members, _le_decode_far(cap, hits, init, d_phys)):
            assert (int(o["pdu_bytes"]), int(o["access_address"]), int(o["crc_ok"]), int(o["offset"])) == (2 + c.length, c.access_address, 1, c.offset), c
    for st in (0, 1):                                  # the short references, both streams
        for ends in (False, True):
            w = _far.ref_words(st, ends)
            conns, cands = bt.le_discover(w, 64 * len(w) - 39, _far.MHZ[st], max_len=max_len)
            sc, sk = ld.group(list(_far.le_candidates(st, ends, max_len)), 2)
            assert cands.tobytes() == ld.cand_array(sk, CAND).tobytes() and conns.tobytes() == ld.conn_array(sc, CONN).tobytes(), (st, ends)


# ---- survey, clock jobs, batch reversal, follow ----------------------------------------------------------------------
class _Line:
    """what tests/_survey.py and tests/_follow.py read of a capture: one stream's symbols"""
    channels, clk_div, n_streams = None, 625, 1

    def __init__(self, words):
        self.sym = [np.ascontiguousarray(bt.synth.unpack_bits(words))]


def _chain_far(ptr, n_words, hits, entry, clk_phase, sentinel=0xA5):
    """survey -> clock-job builder -> batch reversal -> follow on device buffers, over ONE stream at ptr, as bt.run_follow_hits chains
    them for a capture in host memory.  Every table and every count starts as `sentinel` bytes and comes back WHOLE (one entry per
    hit), so that what a call did not write, or wrote behind its count, shows; only the records of d_out that the follow decodes
    start as zeros (see _decode_hits_far).  The scratch buffers are left as they are allocated."""
    import torch
    lib, n = bt.lib(), len(hits)
    JOB, RES = bt.CLOCK_JOB_DTYPE, bt.CLOCK_RESULT_DTYPE

    def fill(nbytes):
        return _filled(nbytes, sentinel)
    d_h = _dev(hits)
    scratch = lib.btbbx_survey_scratch_bytes(n)
    d_scr = torch.empty(scratch // 8 + 2, dtype=torch.int64, device="cuda")
    d_recs, d_cand, d_nrec = fill(n * 64), fill(n * 128), fill(8)
    d_jobs, d_jrec, d_off, d_ch, d_oh, d_n = fill(n * JOB.itemsize), fill(n * 4), fill(n * 4), fill(n), fill(n * 4), fill(8)
    sb = lib.btbbx_hop_reversal_batch_scratch_bytes(n, 0)
    d_bs, d_res = torch.empty(sb // 8 + 2, dtype=torch.int64, device="cuda"), fill(n * RES.itemsize)
    ep = entry.ctypes.data_as(C.c_void_p)
    bt.check(lib.btbbx_survey_hits_device(ptr, n_words, n_words, 1, d_h.data_ptr(), None, n, None, ep, 625, clk_phase, bt.MAX_SYMBOLS,
                                          d_recs.data_ptr(), n, d_nrec.data_ptr(), d_cand.data_ptr(), d_scr.data_ptr(), scratch, None), "survey")
    bt.check(lib.btbbx_survey_clock_jobs_device(d_recs.data_ptr(), d_nrec.data_ptr(), n, d_scr.data_ptr(), scratch, n, None, 1, 0, 1024,
                                                d_jobs.data_ptr(), n, d_n.data_ptr(), d_jrec.data_ptr(), d_off.data_ptr(), d_ch.data_ptr(),
                                                d_oh.data_ptr(), n, d_n.data_ptr() + 4, None), "clock_jobs")
    bt.check(lib.btbbx_hop_reversal_batch_device(d_jobs.data_ptr(), d_n.data_ptr(), n, d_off.data_ptr(), d_ch.data_ptr(), n, d_res.data_ptr(),
                                                 None, 0, d_bs.data_ptr(), sb, None), "batch reversal")
    d_in, d_fol, d_len, d_sums = fill(n * 16), fill(n * 16), fill((n + 1) * 4), fill(n * 32)
    d_out = fill((n + 1) * bt.PKTOUT_DTYPE.itemsize)
    d_out[:n * bt.PKTOUT_DTYPE.itemsize] = 0
    bt.check(lib.btbbx_follow_hits_device(ptr, n_words, n_words, 1, d_h.data_ptr(), None, n, d_recs.data_ptr(), d_nrec.data_ptr(), n,
                                          d_jobs.data_ptr(), d_jrec.data_ptr(), d_res.data_ptr(), d_n.data_ptr(), n, None, ep, 625, clk_phase,
                                          bt.MAX_SYMBOLS, d_in.data_ptr(), d_fol.data_ptr(), d_out.data_ptr(), d_len.data_ptr(), d_sums.data_ptr(),
                                          None), "follow")
    _sync()
    n_recs = int(_host(d_nrec, np.uint32, 2)[0])
    n_jobs, n_obs = (int(x) for x in _host(d_n, np.uint32, 2))
    assert _host(d_nrec, np.uint32, 2)[1] == 0xA5A5A5A5
    return dict(n_recs=n_recs, recs=_host(d_recs, bt.SURVEY_DTYPE, n), cand=_host(d_cand, np.int16, n * 64).reshape(n, 64),
                n_jobs=n_jobs, n_obs=n_obs, jobs=_host(d_jobs, JOB, n), job_rec=_host(d_jrec, np.uint32, n), results=_host(d_res, RES, n),
                offsets=_host(d_off, np.int32, n), channels=_host(d_ch, np.uint8, n), obs_hits=_host(d_oh, np.uint32, n),
                pkt_in=_host(d_in, bt.PKTIN_DTYPE, n), follow=_host(d_fol, bt.FOLLOW_PKT_DTYPE, n), pkt_out=_host(d_out, bt.PKTOUT_DTYPE, n + 1),
                lengths=_host(d_len, np.uint32, n + 1), sums=_host(d_sums, bt.FOLLOW_SUM_DTYPE, n))


M27 = (1 << 27) - 1


def _reversal_model(recs, built):
    """What btbbx_hop_reversal_batch_device must leave for the jobs of aq.model (include/btbbx.h, 'batch reversal'), from the
    oracle port's whole hop pattern of every job's piconet in plain numpy: the initial list = the clocks with the job's CLK1-6
    whose channel is the first observation's (checked against orc_init_hop_reversal's own count); channel_winnow over the
    observations in order, observation 0 included, stopping after the first one that leaves at most one candidate."""
    orc = _libs.oracle()
    out = np.zeros(len(built["jobs"]), bt.CLOCK_RESULT_DTYPE)
    for j, job in enumerate(built["jobs"]):
        rec = recs[built["job_rec"][j]]
        lo, n = int(job["obs_first"]), int(job["n_obs"])
        off, ch = built["offsets"][lo:lo + n].astype(np.int64), built["channels"][lo:lo + n]
        pn, seq = _hop.orc_pattern(orc, int(rec["lap"]), int(rec["uap"]), None)
        c = pn.contents
        c.first_pkt_time, c.clk_offset = int(rec["first_pkt_time"]), int(rec["clk_offset"])
        c.pattern_indices[0], c.pattern_channels[0] = int(off[0]), int(ch[0])
        c.packets_observed = 1
        cand = np.arange(int(job["clk6"]), 1 << 27, 64, dtype=np.int64)
        cand = cand[seq[cand] == ch[0]]
        assert int(job["clk6"]) == (int(rec["clk_offset"]) + int(rec["first_pkt_time"])) & 63 and len(cand) == orc.orc_init_hop_reversal(0, pn)
        n_initial, stop = len(cand), n
        for i in range(n):
            cand = cand[seq[(cand + off[i]) & M27] == ch[i]]
            if len(cand) <= 1:
                stop = i
                break
        out[j] = (0, n_initial, stop, len(cand), int(cand[0]) if len(cand) else 0, 0)
        orc.orc_piconet_free(pn)
        orc.orc_hop_cache_clear()
    return out


@pytest.fixture(scope="module")
def chain():
    """The models of the chain on the two short references of stream 1 -- survey records and candidates, the builder's tables, the
    reversal's results -- computed once (the oracle port's hop patterns take about half a second per job) and never changed."""
    sp = _far.survey_plant()
    hits0 = sv.capture_single()[0].hits()
    assert len(hits0) > 100
    clkn_s, phase_s = _far.survey_clock(_far.PAD)
    short_hits = hits0.copy()
    short_hits["offset"] += 64 * _far.PAD + sp.offset
    made = {}
    for ends in (False, True):
        line = _Line(_far.ref_words(1, ends))
        recs, cand = sv.expected(sv.OracleEngine(), line, short_hits, clkn_s, phase_s)
        built = aq.model(sv.OracleEngine(), line, short_hits, recs, clkn_s, phase_s)
        if made and all(built[k].tobytes() == made[False].built[k].tobytes() for k in ("jobs", "job_rec", "offsets", "channels")) \
                and recs.tobytes() == made[False].recs.tobytes():
            results = made[False].results                       # (the same jobs for the same piconets: the same patterns)
        else:
            results = _reversal_model(recs, built)
        made[ends] = collections.namedtuple("Chain", "line recs cand built results")(line, recs, cand, built, results)
    assert made[False].built["n_jobs"] >= 4
    return collections.namedtuple("Chains", "sp hits0 short_hits clkn_s phase_s made")(sp, hits0, short_hits, clkn_s, phase_s, made)


def _check_chain(out, m, recs, hits, ch, ctx):
    """one run of _chain_far against the models: `recs` = the model's records as this run must report them (first_offset moved),
    `hits` = the run's own list; everything else is the short reference's (no other table holds an offset)"""
    n, n_recs, nj = len(hits), len(m.recs), len(m.built["jobs"])
    assert out["n_recs"] == n_recs, (ctx, out["n_recs"], n_recs)
    sv.assert_records_equal(out["recs"][:n_recs], out["cand"][:n_recs], recs, m.cand, ctx)
    assert (out["recs"][n_recs:].view(np.uint8) == 0xA5).all() and (out["cand"][n_recs:].view(np.uint8) == 0xA5).all(), ctx
    aq.assert_builder_equals(out, m.built, 0xA5, ctx)
    got = out["results"]
    bad = [j for j in range(nj) if got[j].tobytes() != m.results[j].tobytes()]
    assert not bad, (ctx, "results", [(j, got[j], m.results[j]) for j in bad[:4]])
    assert (got[nj:].view(np.uint8) == 0xA5).all(), (ctx, "results written past", nj)
    # the follow, from the MODELS' tables (and the hop selection of the job's own cfg, pinned to the oracle by test_gpu_hop.py)
    pin, fol, stage_job = fw.model(ch.short_hits, m.recs, m.built["job_rec"], m.results, m.built["jobs"], None, 1, sv.entry_state(ch.clkn_s), 625,
                                   ch.phase_s, fw.gpu_hops(m.built["jobs"]))
    decoded = fw.oracle_decode(m.line, ch.short_hits, pin)
    fw.assert_follow_equals(out, pin, fol, fw.sums(n_recs, stage_job, fol, decoded), 0xA5, n_recs=n_recs, ctx=ctx)
    fw.assert_out_equals(out["pkt_out"][:n], out["lengths"][:n], decoded, m.line, ch.short_hits, ctx=ctx)
    assert (fol["stage"] >= 1).sum() >= 20


@pytest.mark.parametrize("name", ["B1", "C1"])
def test_survey_jobs_reversal_follow(cap, chain, name):
    """One copy of capture_single at a time -- the one across bit 2^32, the one across bit 2^35: the chain over its hit list moved
    by the copy's base equals the models on the short reference -- _survey.expected, _acquire.model, the reversal from the oracle
    port's hop patterns, _follow.model -- with the clock moved by base_bits / 625 and first_offset by the base; the same chain on
    the short reference on the GPU equals the unmoved models."""
    c = [x for x in cap.far.copies if x.name == name][0]
    m = chain.made[c.ends]
    # the far run: stream 1 of the far capture as a capture of one stream; the clock of its first bit is what makes slot k of the
    # planted capture carry the clock it was built with
    clkn, phase = _far.survey_clock(c.base)
    assert (chain.phase_s - phase) % 625 == (-64 * _far.PAD) % 625      # (64 words are no whole number of slots: the phase takes the rest)
    hits = chain.hits0.copy()
    hits["offset"] += 64 * c.base + chain.sp.offset
    assert (hits["offset"] >= (1 << 32 if name == "B1" else 1 << 35)).sum() >= (40 if name == "B1" else len(hits))
    moved = m.recs.copy()
    moved["first_offset"] += np.uint64(64 * (c.base - _far.PAD))
    assert (moved["settled_by"] == 2).sum() >= 3 and (moved["settled_by"] == 1).sum() >= 1
    far = _chain_far(cap.ptr + 8 * cap.pitch, cap.n_words, hits, sv.entry_state(clkn), phase)
    _check_chain(far, m, moved, hits, chain, name)
    # the short reference: the same clocks with the stream beginning 64 words in front of S
    d_w = _dev(_far.ref_words(1, c.ends))
    short = _chain_far(d_w.data_ptr(), len(_far.ref_words(1, c.ends)), chain.short_hits, sv.entry_state(chain.clkn_s), chain.phase_s)
    _check_chain(short, m, m.recs, chain.short_hits, chain, name + " short")


# ---- documented limits ---------------------------------------------------------------------------------------------------
def test_scan_first_just_inside_and_outside_2_to_the_32(cap):
    """btbbx_scan_first_device packs the offset into 32 bits: search_bits 2^32 - 1 is accepted and finds a first hit in the last 64
    offsets (a 512 MiB sub-range of the far capture that ends in copy C0); 2^32 is an error and launches nothing."""
    import torch
    lib = bt.lib()
    c = [x for x in cap.far.copies if x.name == "C0"][0]
    first = _far.find_all(0, True, bt.LAP_ANY, 2)[0]
    h0 = first[0] - 64 * _far.PAD                            # the first hit of S0, in bits of S0
    w0 = c.base + (h0 + 65) // 64 - (1 << 26)
    rel = 64 * (c.base - w0) + h0
    bits = (1 << 32) - 1
    assert bits - 64 <= rel < bits and w0 > (1 << 26) + (1 << 20)
    d_first = torch.full((2,), -1, dtype=torch.int64, device="cuda")
    bt.check(lib.btbbx_scan_first_device(cap.ptr + 8 * w0, (1 << 26) + 1, bits, bt.LAP_ANY, 2, d_first.data_ptr(), None), "scan_first")
    _sync()
    got = int(d_first[0].item()) & 0xFFFFFFFFFFFFFFFF
    assert got == (rel << 32 | first[1] << 8 | first[2]), (hex(got), rel, first)
    d_first.fill_(-1)
    assert lib.btbbx_scan_first_device(cap.ptr + 8 * w0, (1 << 26) + 1, 1 << 32, bt.LAP_ANY, 2, d_first.data_ptr(), None) == -3
    _sync()
    assert int(d_first[0].item()) == -1
    short = _short_cap(0, True)                             # the same entry on the short reference: the untranslated offset
    bt.check(lib.btbbx_scan_first_device(short.ptr, short.n_words, short.bits, bt.LAP_ANY, 2, d_first.data_ptr(), None), "scan_first")
    _sync()
    assert int(d_first[0].item()) & 0xFFFFFFFFFFFFFFFF == (first[0] << 32 | first[1] << 8 | first[2])


def test_scan_argument_check_at_2_to_the_40_words(cap):
    """check_scan_args precedes every launch: a stream of 2^40 words (offsets below 2^46) is accepted -- searched here over copy A
    only, so nothing behind it is read -- and one of 2^40 + 1 words is an error that launches nothing."""
    import torch
    lib = bt.lib()
    a = cap.far.copies[0]
    bits = 64 * (a.base + len(cap.far.words[0]) + 32)
    want = [(0, _far.moved(o, a), l, e) for o, l, e in _far.find_all(0, False, bt.LAP_ANY, 2)]
    # n_words and the pitch claim 2^40 words over an allocation of 8 GiB.  What keeps every load inside it: launch_scan takes the
    # tile count from search_bits alone (tiles_per_stream = ceil(ceil(search_bits / 64) / TILE_WORDS)), there is one stream (the pitch
    # is never multiplied: the cursor ends at stream 1), and load_pair of scan_slide_kernel reads TILE_WORDS + 2 words from a tile's
    # first word at the most -- n_words can only shorten that.  So nothing behind word tiles_per_stream * 756 + 2 is read, a few
    # thousand words into the allocation.  A kernel that came to read ahead by n_words instead would make this call a read out of
    # bounds: this test must then search a stream of the length it really has.
    assert ((bits + 63) // 64 + 755) // 756 * 756 + 2 < cap.n_words
    cnt, got, clean, _ = _scan(cap.ptr, 1 << 40, 1 << 40, 1, bits, bt.LAP_ANY, 2, len(want), "plain")
    assert cnt == len(want) and clean
    _same(sorted(got), want, "2^40 words")
    d_h, d_c = _filled(64 * 16), torch.zeros(4, dtype=torch.int32, device="cuda")
    for call in (lambda: lib.btbbx_scan_device(cap.ptr, (1 << 40) + 1, (1 << 40) + 1, 1, bits, bt.LAP_ANY, 2, d_h.data_ptr(), 64, d_c.data_ptr(), None),
                 lambda: lib.btbbx_le_scan_device(cap.ptr, (1 << 40) + 1, (1 << 40) + 1, 1, bits, _le.ADV_AA, 2, d_h.data_ptr(), 64, d_c.data_ptr(), None)):
        assert call() == -3
    _sync()
    assert int(d_c[0].item()) == 0 and d_h.cpu().numpy().tobytes() == b"\xa5" * len(d_h)


def test_survey_and_follow_argument_check_at_2_to_the_34_words(cap, chain):
    """survey_check_args precedes every launch of the survey and of the follow: a stream of 2^34 words (offsets below 2^40) is
    accepted and gives what the real length gives, one of 2^34 + 1 words is an error that launches nothing."""
    lib = bt.lib()
    c = [x for x in cap.far.copies if x.name == "B1"][0]
    m = chain.made[False]
    clkn, phase = _far.survey_clock(c.base)
    hits = chain.hits0.copy()
    hits["offset"] += 64 * c.base + chain.sp.offset
    moved = m.recs.copy()
    moved["first_offset"] += np.uint64(64 * (c.base - _far.PAD))
    # n_words claims 2^34 words of stream 1, which has 2^29: the survey and the follow read a stream only where a hit of the list
    # lies -- the words of its packet, max_length symbols from its offset at the most, n_words can only shorten that (gather_kernel,
    # decode_hits_kernel) -- and every hit lies in the copy across word 2^26.  n_words also sets the number of radix passes.
    assert int(hits["offset"].max()) + bt.MAX_SYMBOLS + 128 < 64 * cap.n_words
    out = _chain_far(cap.ptr + 8 * cap.pitch, 1 << 34, hits, sv.entry_state(clkn), phase)
    _check_chain(out, m, moved, hits, chain, "2^34 words")
    n = len(hits)
    d_h, d_x, d_n = _dev(hits), _filled(n * bt.PKTOUT_DTYPE.itemsize), _filled(16)
    ep = sv.entry_state(clkn).ctypes.data_as(C.c_void_p)
    scratch = lib.btbbx_survey_scratch_bytes(n)
    d_scr = _filled(scratch)
    ptr, nw, x = cap.ptr + 8 * cap.pitch, (1 << 34) + 1, d_x.data_ptr()
    assert lib.btbbx_survey_hits_device(ptr, nw, nw, 1, d_h.data_ptr(), None, n, None, ep, 625, phase, bt.MAX_SYMBOLS, x, n, d_n.data_ptr(),
                                        None, d_scr.data_ptr(), scratch, None) == -3
    assert b"2^40" in lib.btbbx_last_error()
    assert lib.btbbx_follow_hits_device(ptr, nw, nw, 1, d_h.data_ptr(), None, n, x, d_n.data_ptr(), n, None, None, None, None, 0, None, ep, 625,
                                        phase, bt.MAX_SYMBOLS, x, x, x, None, x, None) == -3
    assert b"2^40" in lib.btbbx_last_error() and b"follow" in lib.btbbx_last_error()
    _sync()
    for t in (d_x, d_n, d_scr):
        assert bool((t == 0xA5).all())


# ---- streaming ingest past 2^32 symbols ---------------------------------------------------------------------------------
def test_streaming_ingest_past_2_to_the_32_symbols():
    """66 chunks of 2^26 symbols: the second half of a seam stream, zeros, its first half -- a sync word straddles every join, the
    one at symbol 2^32 included.  By quietness and translation (test_far_model.py) the hits of a period are the oracle port's on the
    seam stream between zeros, moved; the first chunk's head and the last chunk's tail come from the oracle on the two ends."""
    lib = bt.lib()
    N, n_chunks = 1 << 26, 66
    b = _far._Builder(_libs.seed(7003), 64 * 600)
    for j in range(40):
        b.sync(64 * 15 * j + (j * 37) % 640, j, must=False)
    half = 64 * 300
    b.sync(half - 30, 1, must=False)                                # ... and one across the join
    sym = b.bits
    h1, h2 = sym[:half], sym[half:]
    z = np.zeros(4096, np.uint8)
    mid = _libs.orc_find_all(np.concatenate([z, sym, z]), len(sym) + 8192 - 63, _libs.LAP_ANY, 2)
    mid = [(o - 4096 - half, l, e) for o, l, e in mid]              # relative to the join
    assert any(-64 < o < 0 for o, _, _ in mid) and len(mid) > 30
    head = _libs.orc_find_all(np.concatenate([h2, z]), len(h2) + 4096 - 63, _libs.LAP_ANY, 2)
    tail = [(o - 4096 - half, l, e) for o, l, e in _libs.orc_find_all(np.concatenate([z, h1]), 4096 + half - 63, _libs.LAP_ANY, 2)]
    want = list(head)
    for k in range(1, n_chunks):
        want += [(k * N + o, l, e) for o, l, e in mid]
    want += [(n_chunks * N + o, l, e) for o, l, e in tail]
    chunk = np.zeros(N // 64, np.uint64)
    chunk[:len(h2) // 64] = bt.synth.pack_bits(h2)
    chunk[-(half // 64):] = bt.synth.pack_bits(h1)
    h = lib.btbbx_stream_open(bt.LAP_ANY, 2, N, 0)
    assert h, lib.btbbx_last_error()
    buf = np.zeros(1 << 12, bt.HIT_DTYPE)
    got = []
    try:
        for k in range(n_chunks):
            n = bt.check(lib.btbbx_stream_feed(h, chunk.ctypes.data, N, buf.ctypes.data, len(buf)), "feed")
            got += [(int(x["offset"]), int(x["lap"]), int(x["ac_errors"])) for x in buf[:n]]
        n = bt.check(lib.btbbx_stream_flush(h, buf.ctypes.data, len(buf)), "flush")
        got += [(int(x["offset"]), int(x["lap"]), int(x["ac_errors"])) for x in buf[:n]]
    finally:
        lib.btbbx_stream_close(h)

    def period(lst, k):
        return [x for x in lst if x[0] // N == k]
    assert [len(period(got, k)) for k in range(n_chunks)] == [len(period(want, k)) for k in range(n_chunks)]
    for k in (0, 1, 63, 64, 65):
        _same(sorted(period(got, k)), period(want, k), ("period", k))
    assert sorted(got) == want and any((1 << 32) - 64 < o < 1 << 32 for o, _, _ in want)
