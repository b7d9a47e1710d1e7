"""Keyed LE following (libbtbb_amd/csrc/le_keyed.h) on the GPU: the worlds of tests/_le_keyed.py run through btbbx_le_track_device,
btbbx_le_seed_device and the two keyed entries with hand-written data_pkts / crypt / crypt_pkts records, and held against the model,
every byte of every output; equality (a), device against device; lists from elsewhere; refused arguments; and the chain -- a
capture with a pairing, an encryption start and encrypted updates through btbbx_le_keyed_span_host and le_crack_span.  Output
buffers start as 0xA5 and are one record (one connection's span records) longer than their caps, so a byte a kernel leaves unwritten,
or writes where it should not, shows."""
import ctypes as C

import numpy as np
import pytest

import _le_crypt as cm
import _le_data as dm
import _le_discover as ld
import _le_follow as lf
import _le_keyed as lk
import _le_span as ls
import _le_track as lt
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu

CAND, CONN, TRACK, PKT, ADV = bt.LE_CAND_DTYPE, bt.LE_CONN_DTYPE, bt.LE_TRACK_DTYPE, bt.LE_TRACK_PKT_DTYPE, bt.LE_PKT_DTYPE
SEED, FOLLOW, FPKT = bt.LE_SEED_DTYPE, bt.LE_FOLLOW_DTYPE, bt.LE_FOLLOW_PKT_DTYPE
SPAN, SPKT, REC = bt.LE_SPAN_DTYPE, bt.LE_SPAN_PKT_DTYPE, bt.LE_SPAN_REC_DTYPE
DPKT, CRYPT, CPKT = bt.LE_DATA_PKT_DTYPE, bt.LE_CRYPT_DTYPE, bt.LE_CRYPT_PKT_DTYPE
E_ARG = -3


@pytest.fixture(scope="module", autouse=True)
def _init():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    bt.init(2)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    pad = (-a.nbytes) % 16
    raw = np.frombuffer(a.tobytes() + bytes(pad), np.int64).copy() if a.nbytes else np.zeros(2, np.int64)
    return torch.from_numpy(raw).cuda()


def _filled(nbytes):
    import torch
    return torch.full(((nbytes + 15) // 16 * 16 + 16,), 0xA5, dtype=torch.uint8, device="cuda")


def _records(buf, n, dtype):
    return buf.cpu().numpy()[:n * dtype.itemsize].view(dtype)


def _keyed_arrays(b):
    return dm.dpkt_array(b.dpkts, DPKT), cm.crypt_array(b.crypt, CRYPT), cm.cpkt_array(b.cpkts, CPKT)


def _device(b, max_updates, arrays, unkeyed=False):
    """Tracking and seed stage, then both keyed entries (and, unkeyed, both unkeyed ones) over the same records in one run
    -> dict of whole output arrays, each one record longer than its cap."""
    import torch
    lib = bt.lib()
    n, k, m = len(b.cands), len(b.conns), len(b.adv)
    per = max_updates + 1
    n_streams = len(b.words)
    d_cands, d_conns = _dev(ld.cand_array(b.cands, CAND)), _dev(ld.conn_array(b.conns, CONN))
    d_phys, d_words, d_adv = _dev(np.asarray(lt.LATTICE_MHZ, np.uint16)), _dev(np.asarray(b.words).reshape(-1)), _dev(lf.adv_array(b.adv, ADV))
    d_dpkts, d_crypt, d_cpkts = (_dev(a) for a in arrays)
    d_tracks, d_pkts, d_seeds = _filled((k + 1) * TRACK.itemsize), _filled((n + 1) * PKT.itemsize), _filled((k + 1) * SEED.itemsize)
    d_cnt = torch.from_numpy(np.array([n, k, m], np.int64).astype(np.uint32).view(np.int32)).cuda()
    p = d_cnt.data_ptr()
    tscratch = lib.btbbx_le_track_scratch_bytes(n, k)
    d_tscr = _filled(tscratch)
    bt.check(lib.btbbx_le_track_device(d_cands.data_ptr(), p, n, d_conns.data_ptr(), p + 4, k, d_phys.data_ptr(), n_streams, b.unit, b.ifs,
                                       b.jitter, lt.REMAP, d_tracks.data_ptr(), d_pkts.data_ptr(), d_tscr.data_ptr(), tscratch, None),
             "btbbx_le_track_device")
    bt.check(lib.btbbx_le_seed_device(d_adv.data_ptr(), p + 8, m, d_conns.data_ptr(), p + 4, k, d_tracks.data_ptr(), b.unit, d_seeds.data_ptr(),
                                      None), "btbbx_le_seed_device")
    front = (d_words.data_ptr(), b.n_words, b.n_words, n_streams, d_phys.data_ptr(), d_cands.data_ptr(), p, n, d_conns.data_ptr(), p + 4, k,
             d_tracks.data_ptr(), d_pkts.data_ptr(), d_seeds.data_ptr())
    keyed = (d_dpkts.data_ptr(), d_crypt.data_ptr(), d_cpkts.data_ptr())
    bufs, scratches = {}, []

    def run(name, entry, size, mid, tail, shapes):
        d_scr = _filled(size)
        scratches.append((d_scr, size))
        outs = [_filled((count + extra) * dtype.itemsize) for count, extra, dtype in shapes]
        bt.check(getattr(lib, entry)(*front, *mid, b.unit, b.jitter, *tail, *(o.data_ptr() for o in outs), d_scr.data_ptr(), size, None), entry)
        bufs[name] = [(o, count + extra, dtype) for o, (count, extra, dtype) in zip(outs, shapes)]

    f_shapes = [(k, 1, FOLLOW), (n, 1, FPKT)]
    s_shapes = [(k, 1, SPAN), (n, 1, SPKT), (k * per, per, REC)]
    run("follow", "btbbx_le_keyed_epoch_device", lib.btbbx_le_keyed_epoch_scratch_bytes(n, k), keyed, (), f_shapes)
    run("span", "btbbx_le_keyed_span_device", lib.btbbx_le_keyed_span_scratch_bytes(n, k, max_updates), keyed, (max_updates,), s_shapes)
    if unkeyed:
        run("follow0", "btbbx_le_epoch_device", lib.btbbx_le_epoch_scratch_bytes(n, k), (), (), f_shapes)
        run("span0", "btbbx_le_span_device", lib.btbbx_le_span_scratch_bytes(n, k, max_updates), (), (max_updates,), s_shapes)
    torch.cuda.synchronize()
    for d_scr, size in scratches:
        assert set(d_scr.cpu().numpy()[size:].tolist()) == {0xA5}                # nothing behind the scratch
    out = {name: [_records(o, count, dtype) for o, count, dtype in v] for name, v in bufs.items()}
    out["seeds"] = _records(d_seeds, k + 1, SEED)
    for name, a in zip(("dpkts", "crypt", "cpkts"), arrays):                       # the input is not changed
        d = {"dpkts": d_dpkts, "crypt": d_crypt, "cpkts": d_cpkts}[name]
        assert d.cpu().numpy().view(np.uint8)[:a.nbytes].tobytes() == a.tobytes(), name
    return out


def _same(got, want, kept, what, names=None, per=1):
    want = want.reshape(-1)
    if got[:kept].tobytes() != want.tobytes():
        bad = [g for g in range(kept) if got[g].tobytes() != want[g].tobytes()]
        raise AssertionError("%s %d (%s): %s, model %s (%d differ)" % (what, bad[0], names[bad[0] // per] if names else "", got[bad[0]],
                                                                       want[bad[0]], len(bad)))
    assert got[kept:].tobytes() == b"\xa5" * (got.dtype.itemsize * (len(got) - kept)), what


def _check(b, max_updates, want_follow, want_span, arrays=None, out=None):
    """Both keyed entries on the device against the model's (seeds, follows, fpkts) and (seeds, spans, spkts, recs)."""
    n, k, per = len(b.cands), len(b.conns), max_updates + 1
    out = out or _device(b, max_updates, arrays or _keyed_arrays(b))
    _same(out["seeds"], lf.seed_array(want_follow[0], SEED), k, "seed", b.names)
    _same(out["follow"][0], lf.follow_array(want_follow[1], FOLLOW), k, "follow record", b.names)
    _same(out["follow"][1], lf.fpkt_array(want_follow[2], FPKT), n, "follow packet")
    _same(out["span"][0], ls.span_array(want_span[1], SPAN), k, "span record", b.names)
    _same(out["span"][1], ls.spkt_array(want_span[2], SPKT), n, "span packet")
    _same(out["span"][2], ls.rec_array(want_span[3], REC, max_updates), k * per, "span rec", b.names, per)
    return out


# ---- 1. the lattice ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_updates", [0, 1, 2])
def test_the_lattice(max_updates):
    b, want = lk.lattice(), lk.lattice_models()
    out = _check(b, max_updates, want["follow"], want[max_updates])
    spans = out["span"][0][:len(b.conns)]
    readable = {b.cands[i].channel for i, p in b.sent if p.state == cm.VERIFIED}
    assert sum(bool(f & lk.DECRYPTED) for f in spans["flags"]) >= 42 and len(readable) > 42
    by = dict(zip(b.names, spans))
    for name in ("planted: FAILED map update is not read", "planted: not KEYED", "planted: role UNKNOWN", "planted: VERIFIED without a start",
                 "planted: VERIFIED in front of the start", "planted: never encrypts"):
        assert not by[name]["flags"] & lk.DECRYPTED, name
    print("lattice, max_updates %d: %d connections, %d candidates, %d READABLE PDUs" % (max_updates, len(b.conns), len(b.cands), len(b.sent)))


# ---- 2. the stream's end ----------------------------------------------------------------------------------------------------------
def test_updates_across_the_streams_end():
    b = lk.end_world()
    out = _check(b, 2, lk.model_follow(b), lk.model_span(b, 2))
    spkts = out["span"][1]
    kinds = {b.names[b.cands[i].channel]: int(spkts[i]["kind"]) for i, p in b.sent}
    # inside the stream the update is one
    assert kinds["map update ending -104 bits from the end"] == lf.MAP_UPDATE and kinds["param update ending -104 bits from the end"] == lf.PARAM_UPDATE
    assert len(kinds) == 36
    # behind the end the kernels' reads cross it: the plaintext is the keystream over zeros there, and the device reads what the model reads
    want = ls.spkt_array(lk.model_span(b, 2)[2], SPKT)
    end, crossing = 64 * b.n_words, 0
    for i, p in b.sent:
        c, name = b.cands[i], b.names[b.cands[i].channel]
        d = int(name.split()[3])
        last = c.offset + 56 + 8 * (c.length - 4)
        assert last - end == d, name
        if d > 0:
            crossing += 1
            assert spkts[i].tobytes() == want[i].tobytes() and spkts[i]["kind"] != lf.OPAQUE, name
    assert crossing == 6                                   # +1, +8 and +40, a map and a parameter update each


# ---- 3. the crowd -----------------------------------------------------------------------------------------------------------------
def test_a_crowd_of_session_keys():
    b = lk.crowd_world()
    assert len(b.conns) == 600 and len(b.cands) > 2048 and len({bytes(c.session_key) for c in b.crypt}) == 600
    out = _check(b, 1, lk.model_follow(b), lk.model_span(b, 1))
    follows = out["follow"][0][:600]
    assert int((follows["flags"] & lk.DECRYPTED != 0).sum()) == 400 and int(follows["n_off"].sum()) == 0
    assert int((follows["n_map_updates"] == 1).sum()) == 400 and int(follows["n_map_updates"].sum()) == 400


# ---- 4. spans ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_updates", [0, 2])
def test_an_encrypted_parameter_update_opens_a_span(max_updates):
    b = lk.span_world()
    want = lk.model_span(b, max_updates)
    out = _check(b, max_updates, lk.model_follow(b), want)
    g = b.names.index("planted: encrypted update, map update in span 1, TERMINATE, map update")
    r = b.names.index("refused: encrypted update, interval 5")
    s = out["span"][0]
    assert s[g]["flags"] & lk.DECRYPTED and s[g]["flags"] & lf.TERMINATED and s[r]["flags"] & lk.DECRYPTED
    if max_updates:
        assert (s[g]["n_spans"], s[g]["n_off"], s[g]["n_beyond"], s[g]["n_map_updates"], s[g]["interval"]) == (2, 0, 0, 2, 9)
        assert s[r]["flags"] & ls.REFUSED and s[r]["n_spans"] == 1
        assert ls.check_planted(b, *want) > 30
    else:
        assert s[g]["flags"] & ls.CAPPED and s[g]["n_beyond"] > 0


def test_encrypted_updates_next_to_counter_65536():
    b = lk.wrap_world()
    want = lk.model_span(b, 2)
    out = _check(b, 2, lk.model_follow(b), want)
    g = b.names.index("planted: encrypted updates next to 65536")
    s = out["span"][0][g]
    assert (s["n_spans"], s["n_off"], s["n_beyond"], s["n_map_updates"], s["n_param_updates"]) == (2, 0, 0, 1, 1) and s["flags"] & lk.DECRYPTED
    assert ls.check_planted(b, *want) == 20


# ---- 5. equality (a) --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", ["follow lattice", "span lattice", "keyed lattice"])
@pytest.mark.parametrize("how", ["all CLEAR", "VERIFIED, not KEYED"])
def test_without_a_readable_member_the_keyed_entries_are_the_unkeyed_ones(world, how):
    b = {"follow lattice": lf.lattice, "span lattice": ls.lattice, "keyed lattice": lk.lattice}[world]()
    n, k = len(b.cands), len(b.conns)
    dpkts = dm.dpkt_array([dm.DPkt(lk.NONE, 0, i & 1, 0, 0) for i in range(n)], DPKT)
    key = cm.Crypt(bytes(range(16)), bytes(range(8)), 0, 0, 0, 0, 0, 0, 0, 0, 0, cm.F_ARMED | (cm.F_KEYED if how == "all CLEAR" else 0))
    state = cm.CLEAR if how == "all CLEAR" else cm.VERIFIED
    arrays = dpkts, cm.crypt_array([key] * k, CRYPT), cm.cpkt_array([cm.CPkt(i, i, state, 0, 0xFF, 0) for i in range(n)], CPKT)
    out = _device(b, 2, arrays, unkeyed=True)
    for keyed, plain in (("follow", "follow0"), ("span", "span0")):
        for x, y in zip(out[keyed], out[plain]):
            assert x.tobytes() == y.tobytes(), (keyed, x.dtype.names)
    assert (out["follow"][0][:k]["flags"] & lf.ENCRYPTED).any()


# ---- 6. lists from elsewhere ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["every member VERIFIED", "every role UNKNOWN"])
def test_lists_from_elsewhere(how):
    """Records the decryption stage would not write: VERIFIED on members with L < 5, on the start itself, in front of it and in
    connections without one; or no sender known anywhere.  Rule 1 holds member by member, and nothing is written out of bounds."""
    b = lk.lattice()
    if how == "every member VERIFIED":
        c = b._replace(cpkts=[None if p is None else (p if p.state == cm.VERIFIED else p._replace(state=cm.VERIFIED)) for p in b.cpkts])
        short = [i for i, x in enumerate(b.cands) if b.pkts[i] is not None and (x.header0 & 3) == 3 and 1 <= x.length < 5]
        assert len(short) > 50
    else:
        c = b._replace(dpkts=[None if p is None else p._replace(role=lk.UNKNOWN) for p in b.dpkts])
    want_f, want_s = lk.model_follow(c), lk.model_span(c, 2)
    out = _check(c, 2, want_f, want_s)
    flags = out["span"][0][:len(b.conns)]["flags"]
    if how == "every role UNKNOWN":
        assert not (flags & lk.DECRYPTED).any()
        assert want_s[1:] == tuple(ls.model(b, 2)[1:])
    else:                                                   # (the FAILED, SKIPPED and SHORT members are READABLE now, nothing else is)
        assert int((flags & lk.DECRYPTED != 0).sum()) > sum(bool(s and s.flags & lk.DECRYPTED) for s in lk.lattice_models()[2][1])
        by = dict(zip(b.names, want_s[1]))
        assert not by["planted: VERIFIED in front of the start"].flags & lk.DECRYPTED and by["planted: FAILED map update is not read"].flags & lk.DECRYPTED


# ---- 7. bad arguments -------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_before_any_launch():
    lib = bt.lib()
    n, k = 64, 4
    bufs = {name: _filled(size) for name, size in dict(words=8 * 64, phys=80, cands=n * 24, cnt=16, conns=k * 32, tracks=k * 48, pkts=n * 16,
                                                       seeds=k * 56, dpkts=n * 12, crypt=k * 56, cpkts=n * 16, a=k * 56, b=n * 16, c=k * 3 * 40).items()}
    size = lib.btbbx_le_keyed_span_scratch_bytes(n, k, 2)
    assert size >= lib.btbbx_le_span_scratch_bytes(n, k, 2) + 16 * n
    assert lib.btbbx_le_keyed_epoch_scratch_bytes(n, k) >= lib.btbbx_le_epoch_scratch_bytes(n, k) + 16 * n
    esize = lib.btbbx_le_keyed_epoch_scratch_bytes(n, k)
    scr = _filled(size)
    p = {name: t.data_ptr() for name, t in bufs.items()}

    def span(**kw):
        a = dict(p, n_words=64, pitch=64, streams=1, unit=1250, jitter=50, max_updates=2, size=size, scr=scr.data_ptr(), cand_cap=n, conn_cap=k)
        a.update(kw)
        return lib.btbbx_le_keyed_span_device(a["words"], a["n_words"], a["pitch"], a["streams"], a["phys"], a["cands"], a["cnt"], a["cand_cap"],
                                              a["conns"], a["cnt"] + 4, a["conn_cap"], a["tracks"], a["pkts"], a["seeds"], a["dpkts"], a["crypt"],
                                              a["cpkts"], a["unit"], a["jitter"], a["max_updates"], a["a"], a["b"], a["c"], a["scr"], a["size"], None)

    def epoch(**kw):
        a = dict(p, size=esize, scr=scr.data_ptr())
        a.update(kw)
        if kw.get("size") is not None:
            a["size"] = esize - 1
        return lib.btbbx_le_keyed_epoch_device(a["words"], 64, 64, 1, a["phys"], a["cands"], a["cnt"], n, a["conns"], a["cnt"] + 4, k, a["tracks"],
                                               a["pkts"], a["seeds"], a["dpkts"], a["crypt"], a["cpkts"], 1250, 50, a["a"], a["b"], a["scr"],
                                               a["size"], None)

    bad = [dict(dpkts=None), dict(crypt=None), dict(cpkts=None), dict(dpkts=p["dpkts"] + 2), dict(crypt=p["crypt"] + 4), dict(cpkts=p["cpkts"] + 8),
           dict(size=size - 1), dict(scr=None), dict(words=None), dict(seeds=None)]
    for kw in bad:
        assert span(**kw) == E_ARG, kw
        assert epoch(**kw) == E_ARG, kw
    for kw in (dict(max_updates=17), dict(streams=0), dict(unit=1), dict(jitter=625), dict(n_words=0), dict(a=None), dict(c=p["c"] + 4)):
        assert span(**kw) == E_ARG, kw
    assert span(cand_cap=0) == 0 and span(conn_cap=0) == 0
    import torch
    torch.cuda.synchronize()
    for name in ("a", "b", "c"):                            # nothing was launched, nothing written
        assert set(bufs[name].cpu().numpy().tolist()) == {0xA5}, name


# ---- 8. the chain -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain():
    ch = lk.chain_capture()
    cap = ch.cap
    kw = dict(min_count=2, n_streams=len(cap.mhz), pitch_words=cap.pitch_words, n_words=cap.n_words, unit_bits=dm.UNIT, ifs_bits=dm.IFS,
              jitter_bits=dm.JITTER)
    keyed = bt.le_span_keyed(cap.words, cap.search_bits, cap.mhz, [ch.stk], max_updates=4, **kw)
    plain = bt.le_span(cap.words, cap.search_bits, cap.mhz, max_updates=4, **kw)
    return ch, kw, keyed, plain


def _chain_conns(ch, conns):
    by = {(p.aa, p.crc_init): p.name for p in ch.cap.planted}
    names = [by.get((int(c["access_address"]), int(c["crc_init"]))) for c in conns]
    return names.index(lk.CHAIN_NAME), names.index(lk.CHAIN_PLAIN)


def _followed(ch, spans, recs, g):
    s = spans[g]
    assert (int(s["n_off"]), int(s["n_beyond"]), int(s["n_on"])) == (0, 0, lk.CHAIN_EVENTS), s
    assert s["flags"] & lk.DECRYPTED and s["flags"] & lf.ENCRYPTED and not s["flags"] & (ls.CAPPED | ls.REFUSED)
    assert (int(s["n_spans"]), int(s["n_map_updates"]), int(s["n_param_updates"]), int(s["interval"])) == (2, 1, 1, lk.CHAIN_INTERVAL)
    assert int(s["map"]) == lk.NINE
    r0, r1 = recs[g][0], recs[g][1]
    assert (int(r0["origin"]), int(r0["base"]), int(r0["first_event"]), int(r0["n_events"]), int(r0["interval"])) == (
        ch.t0[lk.CHAIN_NAME], 0, 0, lk.CHAIN_PARAM_AT, dm.INTERVAL)
    # the planted window: the old grid at the instant, WinOffset units on (the events lie 7 bits behind their grid)
    origin = ch.t0[lk.CHAIN_NAME] + lk.CHAIN_PARAM_AT * dm.INTERVAL * dm.UNIT + lk.CHAIN_WIN_OFFSET * dm.UNIT + 7
    assert (int(r1["origin"]), int(r1["base"]), int(r1["first_event"]), int(r1["n_events"]), int(r1["interval"]), int(r1["win_offset"]),
            int(r1["flags"])) == (origin, lk.CHAIN_PARAM_AT, lk.CHAIN_PARAM_AT, lk.CHAIN_EVENTS - lk.CHAIN_PARAM_AT, lk.CHAIN_INTERVAL,
                                  lk.CHAIN_WIN_OFFSET, 1)
    assert not recs[g][2]["flags"]


def test_the_chain_follows_what_the_unkeyed_chain_loses(chain):
    ch, kw, keyed, plain = chain
    conns, cands, tracks, pkts, seeds, crypt, cpkts, spans, spkts, recs = keyed
    g, other = _chain_conns(ch, conns)
    assert crypt[g]["flags"] & cm.F_KEYED and int(crypt[g]["n_verified"]) == 4 and int(crypt[g]["n_failed"]) == 0
    _followed(ch, spans, recs, g)
    mine = np.flatnonzero(cands["conn"] == g)
    assert (spkts["on_hop"][mine] == 1).all() and sorted(set(spkts["counter"][mine].tolist())) == list(range(lk.CHAIN_EVENTS))
    kinds = spkts["kind"][mine].tolist()
    assert kinds.count(lf.MAP_UPDATE) == 1 and kinds.count(lf.PARAM_UPDATE) == 1 and kinds.count(lf.ENC_START) == 1 and lf.OPAQUE not in kinds
    assert int(spkts["applied"][mine].sum()) == 1
    # the unkeyed chain on the same capture: the map update is never read, so behind its instant the connection is off its hop
    p_spans, p_spkts = plain[5], plain[6]
    assert plain[0].tobytes() == conns.tobytes() and plain[1].tobytes() == cands.tobytes()
    assert int(p_spans[g]["n_off"]) > 0 and int(p_spans[g]["n_spans"]) == 1 and not p_spans[g]["flags"] & lk.DECRYPTED
    behind = mine[p_spkts["counter"][mine] >= lk.CHAIN_MAP_AT]
    assert (p_spkts["on_hop"][behind] == 0).sum() > 0 and (p_spkts["on_hop"][mine[p_spkts["counter"][mine] < lk.CHAIN_MAP_AT]] == 1).all()
    assert (p_spkts["kind"][mine] == lf.OPAQUE).sum() == 4
    # the connection that never encrypts: identical records
    assert p_spans[other].tobytes() == spans[other].tobytes() and plain[7][other].tobytes() == recs[other].tobytes()
    theirs = np.flatnonzero(cands["conn"] == other)
    assert p_spkts[theirs].tobytes() == spkts[theirs].tobytes() and int(spans[other]["n_off"]) == 0 and int(spans[other]["n_map_updates"]) == 1


def test_le_crack_span_needs_no_key(chain):
    ch, kw, keyed, plain = chain
    pair, cracked = bt.le_crack_span(ch.cap.words, ch.cap.search_bits, ch.cap.mhz, tk_limit=1, max_updates=4, **kw)
    assert pair[7] == 1 and pair[6][0].tobytes() == ch.stk
    for x, y in zip(cracked, keyed):
        assert x.tobytes() == y.tobytes()
    g, _ = _chain_conns(ch, cracked[0])
    _followed(ch, cracked[7], cracked[9], g)
    # no key within reach: the pairs alone
    pair, none = bt.le_crack_span(ch.cap.words, ch.cap.search_bits, ch.cap.mhz, tk_limit=0, **kw)
    assert none is None and pair[7] == 0


# ---- 9. the wrapper against its neighbours ----------------------------------------------------------------------------------------
def test_the_wrapper_shares_its_outputs_with_the_crypt_and_span_wrappers(chain):
    ch, kw, keyed, plain = chain
    cap = ch.cap
    conns, cands, tracks, pkts, seeds, crypt, cpkts, spans, spkts, recs = keyed
    for x, y in zip((conns, cands, tracks, pkts, seeds), plain[:5]):
        assert x.tobytes() == y.tobytes()
    dec = bt.le_decrypt(cap.words, cap.search_bits, cap.mhz, [ch.stk], msg_cap=0, byte_cap=0, truncate=True, **kw)
    assert dec[0].tobytes() == conns.tobytes() and dec[1].tobytes() == cands.tobytes() and dec[3].tobytes() == pkts.tobytes()
    assert dec[8].tobytes() == crypt.tobytes() and dec[9].tobytes() == cpkts.tobytes()
    # a key that is not the connection's: nothing is READABLE and the wrapper gives the unkeyed wrapper's records
    wrong = bt.le_span_keyed(cap.words, cap.search_bits, cap.mhz, [bytes(16)], max_updates=4, **kw)
    assert wrong[7].tobytes() == plain[5].tobytes() and wrong[8].tobytes() == plain[6].tobytes() and wrong[9].tobytes() == plain[7].tobytes()
    # refusals: the span wrapper's and the crypt wrapper's
    lib = bt.lib()
    w = np.ascontiguousarray(cap.words).reshape(-1)
    phys = np.ascontiguousarray(cap.mhz, np.uint16)
    keys = np.frombuffer(ch.stk, np.uint8).copy()
    bufs = [np.zeros(4, d) for d in (CONN, CAND, TRACK, PKT, SEED, CRYPT, CPKT, SPAN, SPKT)] + [np.zeros(20, REC)]
    ptr = [b.ctypes.data for b in bufs]

    def call(n_keys=1, window=8, max_updates=4, keys_p=keys.ctypes.data, crypt_p=ptr[5], spans_p=ptr[7], adv_errors=0):
        return lib.btbbx_le_keyed_span_host(w.ctypes.data, cap.n_words, cap.pitch_words, len(cap.mhz), cap.search_bits, phys.ctypes.data, 27, 2,
                                            ptr[0], 4, ptr[1], 4, None, dm.UNIT, dm.IFS, dm.JITTER, lt.REMAP, adv_errors, ptr[2], ptr[3], ptr[4],
                                            keys_p, n_keys, window, crypt_p, ptr[6], max_updates, spans_p, ptr[8], ptr[9])

    for kw2 in (dict(n_keys=0), dict(n_keys=65), dict(window=0), dict(window=33), dict(max_updates=17), dict(keys_p=None), dict(crypt_p=None),
                dict(spans_p=None), dict(adv_errors=5)):
        assert call(**kw2) == E_ARG, kw2
    assert call() == 2
