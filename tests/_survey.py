"""Helpers of the piconet-survey tests (no test in here): synthetic multi-piconet captures and the records the
reference's survey loop leaves for them, computed two ways -- over the oracle port and over the compiled reference.

The loop (bluetooth_piconet.c:851-858), per LAP, packets in ascending (offset, stream), on a piconet fresh from
btbb_piconet_new + btbb_init_piconet:

    btbb_piconet_set_channel_seen(pn, channel)
    if btbb_header_present(pkt) and not flag(pn, BTBB_UAP_VALID):
        btbb_uap_from_header(pkt, pn)
"""
import ctypes as C
import os
import tempfile

import numpy as np

import _libs
import libbtbb_amd as bt
from libbtbb_amd import synth

UAP_VALID, LAP_VALID, CLK6_VALID, GOT_FIRST = 2, 3, 4, 10
_libc = C.CDLL(None)


# ---- captures ---------------------------------------------------------------------------------------------------

class Capture:
    """n_streams lines of n_words packed words, pitch_words apart; sym[s] = the symbols of stream s."""

    def __init__(self, seed, n_streams, n_symbols, clk_div=625, pitch_extra=0, channels=None):
        assert n_symbols % 64 == 0
        self.rng = np.random.default_rng(_libs.seed(seed))
        self.n_streams, self.n_words, self.clk_div = n_streams, n_symbols // 64, clk_div
        self.pitch_words = self.n_words + pitch_extra
        self.sym = [self.rng.integers(0, 2, n_symbols, dtype=np.uint8) for _ in range(n_streams)]
        self.channels = None if channels is None else np.asarray(channels, dtype=np.uint8)
        self.search_bits = n_symbols - 63
        self.used = set()

    def put(self, stream, slot, symbols, errors=0):
        s = np.array(symbols, dtype=np.uint8)
        for _ in range(errors):                        # symbol errors the FEC 1/3 of the header corrects
            s[68 + 3 * int(self.rng.integers(0, 18)) + int(self.rng.integers(0, 3))] ^= 1
        at = slot * self.clk_div
        assert at + len(s) <= len(self.sym[stream]) and (stream, slot) not in self.used
        self.used.add((stream, slot))
        self.sym[stream][at:at + len(s)] = s

    def words(self):
        w = np.zeros((self.n_streams, self.pitch_words), dtype=np.uint64)
        for s in range(self.n_streams):
            w[s, :self.n_words] = synth.pack_bits(self.sym[s])
        return w

    def hits(self, max_ac_errors=2):
        """The hit list: orc_find_all per stream, in (stream, offset) order."""
        out = []
        for s in range(self.n_streams):
            for off, lap, err in _libs.orc_find_all(np.ascontiguousarray(self.sym[s]), self.search_bits, _libs.LAP_ANY, max_ac_errors):
                out.append((off, lap, err, 0, s))
        return np.array(out, dtype=bt.HIT_DTYPE) if out else np.zeros(0, dtype=bt.HIT_DTYPE)


def _pkt(lap, uap, clk6, ptype, rng):
    body = b""
    if ptype in (synth.TYPE_DM1, synth.TYPE_DH1):
        body = rng.integers(0, 256, int(rng.integers(1, 17)), dtype=np.uint8).tobytes()
    elif ptype == synth.TYPE_HV1:
        body = rng.integers(0, 256, 10, dtype=np.uint8).tobytes()
    if ptype == synth.TYPE_FHS:
        return synth.build_packet(lap, uap=uap, clk6=clk6, ptype=ptype, fhs_bits=synth.fhs_payload(lap, uap, 0x1234, 0, rng))
    return synth.build_packet(lap, uap=uap, clk6=clk6, ptype=ptype, lt_addr=int(rng.integers(1, 8)), flags=int(rng.integers(0, 8)),
                              body=body)


def populate(cap, clkn0, clk_phase=0, n_crc=5, n_elim=3, n_reset=3, n_open=3, n_id=25, n_twins=1, span=None):
    """Piconets of every kind on free (stream, slot) places of `cap` (slots of clk_div symbols; the packet of slot k
    starts at symbol k * clk_div and carries the clock clkn0 + (k * clk_div + clk_phase) // clk_div).
    Returns the list of (lap, kind)."""
    rng = cap.rng
    slots_per_stream = (len(cap.sym[0]) - 700) // cap.clk_div if span is None else span
    made = []

    late = slots_per_stream * 7 // 8                   # the last eighth is kept for packets that must come behind the others

    def free_place(tail=False):
        while True:
            st = int(rng.integers(0, cap.n_streams))
            sl = int(rng.integers(late, slots_per_stream)) if tail else int(rng.integers(0, late - 1))
            if (st, sl) not in cap.used and (st, sl - 1) not in cap.used and (st, sl + 1) not in cap.used:
                return st, sl

    def send(lap, uap, off6, ptype, place=None, errors=None):
        st, sl = place or free_place()
        clkn = (clkn0 + (sl * cap.clk_div + clk_phase) // cap.clk_div) & 0xFFFFFFFF
        cap.put(st, sl, _pkt(lap, uap, (clkn + off6) & 63, ptype, rng), errors=int(rng.integers(0, 2)) if errors is None else errors)
        return st, sl

    def ident():
        return int(rng.integers(1, 1 << 24)), int(rng.integers(1, 256)), int(rng.integers(0, 64))

    quiet = (synth.TYPE_NULL, synth.TYPE_POLL, synth.TYPE_HV1)
    loud = (synth.TYPE_DM1, synth.TYPE_DH1, synth.TYPE_FHS)
    for k in range(n_crc):                             # a few headers without CRC, then one with
        lap, uap, off6 = ident()
        for j in range(k % 3):
            send(lap, uap, off6, quiet[j % 3])
        for j in range(1 + k % 2):
            send(lap, uap, off6, loud[(k + j) % 3])
        send(lap, uap, off6, synth.TYPE_POLL)          # later packets only mark channels
        made.append((lap, "crc"))
    for k in range(n_elim):                            # no CRC anywhere: candidates go by UAP disagreement
        lap, uap, off6 = ident()
        for j in range(14):
            send(lap, uap, off6, quiet[(j + k) % 2])
        made.append((lap, "elim"))
    for k in range(n_reset):                           # two devices under one LAP: nothing stays consistent
        lap, uap, off6 = ident()
        for j in range(6):
            send(lap, (uap + 0x5b * (j & 1)) & 0xff or 1, off6 + 7 * (j & 1), synth.TYPE_POLL, errors=0)
        # ... and behind them two packets with a CRC: the first settles the piconet or resets it once more (whichever
        # device opened the last attempt), the second settles it then -- a piconet that was reset before, stale candidates
        for j in range(2):
            send(lap, uap, off6, synth.TYPE_DM1, place=free_place(tail=True), errors=0)
        made.append((lap, "reset"))
    for k in range(n_open):                            # one or two headers without CRC: several candidates stay
        lap, uap, off6 = ident()
        for j in range(1 + k % 2):
            send(lap, uap, off6, synth.TYPE_POLL)
        made.append((lap, "open"))
    for k in range(n_id):                              # ID packets: an access code and nothing behind it
        lap = int(rng.integers(1, 1 << 24))
        st, sl = free_place()
        cap.put(st, sl, synth.build_packet(lap))
        made.append((lap, "id"))
    for k in range(n_twins if cap.n_streams > 1 else 0):   # the same packet at the same time on two streams
        lap, uap, off6 = ident()
        while True:
            st, sl = free_place()
            st2 = (st + 1 + int(rng.integers(0, cap.n_streams - 1))) % cap.n_streams
            if all((st2, sl + d) not in cap.used for d in (-1, 0, 1)):
                break
        send(lap, uap, off6, synth.TYPE_POLL, place=(st, sl), errors=0)
        send(lap, uap, off6, synth.TYPE_POLL, place=(st2, sl), errors=0)
        send(lap, uap, off6, synth.TYPE_POLL)
        made.append((lap, "twin"))
    return made


def capture_single(seed=11, clkn0=77):
    cap = Capture(seed, 1, 64 * 4096)
    populate(cap, clkn0)
    return cap, dict(clkn0=clkn0, clk_phase=0)


def capture_multi(seed=12, clkn0=(1 << 27) - 50, clk_phase=624, n_streams=8):
    """pitch > n_words, channels not the stream index, a clock that passes 2^27 inside the capture"""
    channels = (np.arange(n_streams) * 37 + 5) % 79
    cap = Capture(seed, n_streams, 64 * 2048, pitch_extra=3, channels=channels)
    populate(cap, clkn0, clk_phase=clk_phase, n_id=40, n_twins=3)
    return cap, dict(clkn0=clkn0, clk_phase=clk_phase)


def capture_oops(seed=13, clkn0=5, n_same=1030, clk_div=4):
    """One piconet sending the same POLL every 64 slots (slots of clk_div symbols): every candidate keeps implying the UAP it
    implied before and no type it implies has a CRC to fail, so nothing is eliminated and the pattern memory fills."""
    n_sym = -(-(n_same * 64 * clk_div + 4096) // 64) * 64
    cap = Capture(seed, 1, n_sym, clk_div=clk_div)
    lap, uap, off6 = 0x3A71C5, 0x9D, 21
    one = synth.build_packet(lap, uap=uap, clk6=(clkn0 + off6) & 63, ptype=synth.TYPE_POLL, lt_addr=2, flags=1)
    tail = cap.rng.integers(0, 2, 120, dtype=np.uint8)             # the same symbols behind every copy
    for k in range(n_same):
        cap.put(0, 64 * k, np.concatenate([one, tail]))
    # (captured length 246: every copy is the same 246 symbols; with more, the multi-slot types some candidates imply would
    # read into the following copies and the noise between them)
    return cap, dict(clkn0=clkn0, clk_phase=0, max_length=len(one) + len(tail))


FIXTURES = {"single": capture_single, "multi": capture_multi, "oops": capture_oops}


# ---- the loop over the oracle and over the compiled reference ----------------------------------------------------

class _Stdout:
    """What C code prints to stdout between mark() and text(): the only place the reference says HOW it settled."""

    def __enter__(self):
        _libc.fflush(None)
        self.saved = os.dup(1)
        self.tmp = tempfile.TemporaryFile()
        os.dup2(self.tmp.fileno(), 1)
        self.pos = 0
        return self

    def text(self):
        _libc.fflush(None)
        self.tmp.seek(self.pos)
        out = self.tmp.read()
        self.pos += len(out)
        return out

    def __exit__(self, *exc):
        _libc.fflush(None)
        os.dup2(self.saved, 1)
        os.close(self.saved)
        self.tmp.close()


class OracleEngine:
    name = "oracle"

    def __init__(self):
        self.lib = _libs.oracle()
        self.lib.orc_init(2)

    def piconet(self, lap):
        pn = self.lib.orc_piconet_new()
        self.lib.orc_init_piconet(pn, lap)
        return pn

    def packet(self, lap, ac_errors, sym, channel, clkn):
        p = self.lib.orc_packet_new()
        self.lib.orc_packet_init_found(p, lap, ac_errors)
        self.lib.orc_packet_set_data(p, _libs.ptr(sym), len(sym), channel, 0)
        p.contents.clkn = clkn
        return p

    def free_packet(self, p):
        self.lib.orc_packet_free(p)

    def free_piconet(self, pn):
        self.lib.orc_piconet_free(pn)

    def channel_seen(self, pn, ch):
        c = pn.contents
        if not c.afh_map[ch // 8] & (1 << (ch % 8)):
            c.afh_map[ch // 8] |= 1 << (ch % 8)
            c.used_channels += 1

    def header_present(self, p):
        return self.lib.orc_header_present(p)

    def uap_from_header(self, p, pn):
        return self.lib.orc_uap_from_header(p, pn)

    def flag(self, pn, f):
        return self.lib.orc_piconet_get_flag(pn, f)

    def settled_by(self, said, pn, lap, h, sym, clkn):
        """The port prints nothing: the settling candidate's own trial says whether a CRC proved it (2) or it was the last
        one standing (1)."""
        c = pn.contents
        first = (int(c.clk_offset) + int(c.first_pkt_time)) & 63
        clock = (first + clkn - int(c.first_pkt_time)) & 63
        p = self.packet(lap, int(h["ac_errors"]), sym, 0, clkn)
        self.lib.orc_try_clock(clock, p)
        verdict = self.lib.orc_crc_check(clock, p)
        self.free_packet(p)
        return 1 if verdict in (1, 2) else 2

    def state(self, pn):
        c = pn.contents
        return dict(flags=int(c.flags), uap=int(c.UAP), clk_offset=int(c.clk_offset) & 0xff, used_channels=int(c.used_channels),
                    afh_map=bytes(c.afh_map), packets_observed=int(c.packets_observed), total=int(c.total_packets_observed),
                    first_pkt_time=int(c.first_pkt_time), cand=np.array(c.clock6_candidates[:], dtype=np.int16))


class ReferenceEngine:
    name = "reference"

    def __init__(self):
        self.lib = _libs.ref()
        assert self.lib is not None, "compiled reference missing (oracle/_ref)"
        self.lib.btbb_init(2)
        self.lib.btbb_piconet_get_afh_map.restype = C.c_void_p
        self.lib.btbb_piconet_get_afh_map.argtypes = [C.c_void_p]
        self.view = None

    def piconet(self, lap):
        pn = C.c_void_p(self.lib.btbb_piconet_new())
        self.lib.btbb_init_piconet(pn, lap)
        return pn

    def packet(self, lap, ac_errors, sym, channel, clkn):
        p = C.c_void_p(self.lib.btbb_packet_new())
        if self.view is None:
            v = _libs.RefPacketView(self.lib, p.value)
            self.view = {f: v._off(f) for f in ("LAP", "ac_errors", "flags", "clkn")}
        C.c_uint32.from_address(p.value + self.view["LAP"]).value = lap             # init_packet (static in the reference)
        C.c_uint8.from_address(p.value + self.view["ac_errors"]).value = ac_errors
        C.c_uint32.from_address(p.value + self.view["flags"]).value = 0
        self.lib.btbb_packet_set_flag(p, 0, 1)
        self.lib.btbb_packet_set_data(p, _libs.ptr(sym), len(sym), channel, 0)
        C.c_uint32.from_address(p.value + self.view["clkn"]).value = clkn
        return p

    def free_packet(self, p):
        self.lib.btbb_packet_unref(p)

    def free_piconet(self, pn):
        self.lib.btbb_piconet_unref(pn)

    def channel_seen(self, pn, ch):
        self.lib.btbb_piconet_set_channel_seen(pn, ch)

    def header_present(self, p):
        return self.lib.btbb_header_present(p)

    def uap_from_header(self, p, pn):
        return self.lib.btbb_uap_from_header(p, pn)

    def flag(self, pn, f):
        return self.lib.btbb_piconet_get_flag(pn, f)

    def settled_by(self, said, pn, lap, h, sym, clkn):
        assert b"UAP = " in said, said
        return 2 if b"Correct CRC!" in said else 1

    def state(self, pn):
        lib = self.lib
        cand = (C.c_int * 64)()
        lib.refint_piconet_candidates(pn, cand)
        amap = bytes((C.c_uint8 * 10).from_address(lib.btbb_piconet_get_afh_map(pn)))
        return dict(flags=int(lib.refint_piconet_flags(pn)), uap=int(lib.btbb_piconet_get_uap(pn)),
                    clk_offset=int(lib.btbb_piconet_get_clk_offset(pn)) & 0xff,
                    used_channels=sum(bin(b).count("1") for b in amap), afh_map=amap,
                    packets_observed=int(lib.refint_piconet_packets_observed(pn)),
                    total=int(lib.refint_piconet_total_packets_observed(pn)),
                    first_pkt_time=int(lib.refint_piconet_first_pkt_time(pn)), cand=np.array(cand[:], dtype=np.int16))


def packet_symbols(cap, hit, max_length=bt.MAX_SYMBOLS):
    """what btbbx_gather_packets_device cuts out for a hit"""
    line = cap.sym[int(hit["stream"])]
    off = int(hit["offset"])
    n = min(max_length, bt.MAX_SYMBOLS, max(len(line) - off, 0))
    return np.ascontiguousarray(line[off:off + n])


def expected(engine, cap, hits, clkn0, clk_phase=0, max_length=bt.MAX_SYMBOLS, only_laps=None, stats=None):
    """(records, candidates) of the survey loop over `hits` (any order), ascending LAP.  stats (a dict) collects what the
    fixtures are asked to reach: packets skipped for header_present == 0, ..."""
    hits = np.asarray(hits)
    order = np.lexsort((hits["stream"], hits["offset"], hits["lap"]))
    recs, cands = [], []
    with _Stdout() as out:
        i = 0
        while i < len(order):
            j = i
            lap = int(hits["lap"][order[i]])
            while j < len(order) and int(hits["lap"][order[j]]) == lap:
                j += 1
            group, i = order[i:j], j
            if only_laps is not None and lap not in only_laps:
                continue
            pn = engine.piconet(lap)
            r = np.zeros(1, dtype=bt.SURVEY_DTYPE)[0]
            r["lap"], r["n_packets"], r["settled_hit"] = lap, len(group), 0xFFFFFFFF
            r["first_offset"], r["first_stream"] = hits["offset"][group[0]], hits["stream"][group[0]]
            for k in group:
                h = hits[k]
                st = int(h["stream"])
                ch = st if cap.channels is None else int(cap.channels[st])
                engine.channel_seen(pn, ch)
                if engine.flag(pn, UAP_VALID):
                    continue
                clkn = (clkn0 + (int(h["offset"]) + clk_phase) // cap.clk_div) & 0xFFFFFFFF
                p = engine.packet(lap, int(h["ac_errors"]), packet_symbols(cap, h, max_length), ch, clkn)
                if not engine.header_present(p):
                    if stats is not None:
                        stats["no_header"] = stats.get("no_header", 0) + 1
                    engine.free_packet(p)
                    continue
                total_before = engine.state(pn)["total"]
                rv = engine.uap_from_header(p, pn)
                said = out.text()
                engine.free_packet(p)
                r["n_walked"] += 1
                if rv:
                    r["settled_by"] = engine.settled_by(said, pn, lap, h, packet_symbols(cap, h, max_length), clkn)
                    r["settled_after"] = total_before + 1
                    r["settled_hit"] = k
                elif engine.state(pn)["packets_observed"] == 0:       # counted packets leave it >= 1: this call reset
                    r["n_resets"] += 1
                    if stats is not None and b"Oops" in said:
                        stats["oops"] = stats.get("oops", 0) + 1
            s = engine.state(pn)
            r["flags"], r["uap"], r["clk_offset"], r["used_channels"] = s["flags"], s["uap"], s["clk_offset"], s["used_channels"]
            r["afh_map"] = np.frombuffer(s["afh_map"], dtype=np.uint8)
            r["packets_observed"], r["total_packets_observed"], r["first_pkt_time"] = s["packets_observed"], s["total"], s["first_pkt_time"]
            recs.append(r)
            cands.append(s["cand"])
            engine.free_piconet(pn)
    return (np.array(recs, dtype=bt.SURVEY_DTYPE) if recs else np.zeros(0, dtype=bt.SURVEY_DTYPE),
            np.array(cands, dtype=np.int16).reshape(-1, 64))


def assert_records_equal(got, got_cand, want, want_cand, ctx=""):
    assert len(got) == len(want), (ctx, len(got), len(want))
    for name in bt.SURVEY_DTYPE.names:
        a, b = got[name], want[name]
        bad = np.nonzero((a != b).reshape(len(got), -1).any(axis=1))[0]
        assert len(bad) == 0, (ctx, name, [(hex(int(want["lap"][i])), a[i].tolist(), b[i].tolist()) for i in bad[:4]])
    if got_cand is not None:
        bad = np.nonzero((np.asarray(got_cand) != np.asarray(want_cand)).any(axis=1))[0]
        assert len(bad) == 0, (ctx, "candidates", [(hex(int(want["lap"][i])), got_cand[i].tolist(), want_cand[i].tolist()) for i in bad[:2]])


def entry_state(clkn0):
    """what btbb_find_ac + btbb_packet_set_data leave: whitened, nothing else known"""
    e = np.zeros(1, dtype=bt.PKTIN_DTYPE)
    e["clkn"], e["flags"] = clkn0, 1 << bt.BTBB_WHITENED
    return e
