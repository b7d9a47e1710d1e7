"""A deterministic lattice of packets on the branch points of the 64-clock trials and the decoders.

Random draws (tests/_pkt.py) hit the reference's length checks rarely or never; this module builds
every packet on purpose, one per boundary, so that a kernel whose boundary moves by one symbol, byte
or FEC block disagrees with the oracle on a named packet.  The boundaries (bluetooth_packet.c):

* every legal payload length of every type with a payload, the length field of the payload header at
  the reference's maximum and one above it (decode_payload_header's caps, :860-890);
* each packet cut where its capture could end: full with a random tail, at the last symbol of the
  packet and one before it, at the end of the payload header and one before it, where DM / DH / DV
  stop asking `bitlength > size` (:940-997) and one before it, where EV4's block loop first reaches
  the CRC (it tests byte counts one block late, :1044-1097) and one before it, at 122 / 121
  (`length < 122`, :1380), and at exactly 3125 symbols with the packet at the front (:472);
* two symbol errors inside one FEC 2/3 block -- the first block, the last two blocks of the payload
  and the block behind it -- of FHS, DM*, DV, HV2 and EV4;
* exactly 3 and exactly 4 header triples that disagree (unfec13's `be < length / 4`, :566), each with
  a majority that is still right and one that is wrong;
* EV4 packets whose CRC register is zero after the first byte (UAP 0, first byte 0): the reference's
  scan counts from two bytes on;
* entry state: packet_type over 0..15, 16 and 255, random UAP, llid 0..3, flow 0..1, the WHITENED
  flag with and against what is on air, and the other flag bits.

build() returns a Lattice; tables() the oracle's 64-clock table of every packet, computed once per
process (oracle/btbb_oracle.c: orc_trial_table).
"""
import ctypes as C
import functools
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import _libs
import libbtbb_amd as bt
from libbtbb_amd import synth

F_WHITENED, F_UAP_VALID, F_CLK6_VALID, F_HAS_PAYLOAD = 1 << 0, 1 << 2, 1 << 4, 1 << 7

NAMES = {synth.TYPE_NULL: "NULL", synth.TYPE_POLL: "POLL", synth.TYPE_FHS: "FHS", synth.TYPE_DM1: "DM1",
         synth.TYPE_DH1: "DH1", synth.TYPE_HV1: "HV1", synth.TYPE_HV2: "HV2", 7: "EV3", synth.TYPE_DV: "DV",
         synth.TYPE_AUX1: "AUX1", synth.TYPE_DM3: "DM3", synth.TYPE_DH3: "DH3", synth.TYPE_EV4: "EV4",
         synth.TYPE_EV5: "EV5", synth.TYPE_DM5: "DM5", synth.TYPE_DH5: "DH5"}
HV3_AS = "HV3"                                   # type 7 with a 30-byte voice body

# legal body lengths (payload without payload header and CRC)
MAXBODY = {synth.TYPE_DM1: 17, synth.TYPE_DH1: 27, synth.TYPE_AUX1: 29, 7: 30, synth.TYPE_DM3: 121,
           synth.TYPE_DH3: 183, synth.TYPE_DM5: 224, synth.TYPE_DH5: 339, synth.TYPE_EV4: 120,
           synth.TYPE_EV5: 180, synth.TYPE_DV: 9}
# decode_payload_header's max_length per type (bluetooth_packet.c:860-890); the payload header's
# length field is payload_length - 3 (one-byte header) or - 4 (two bytes)
REF_CAP = {synth.TYPE_DM1: 20, synth.TYPE_DH1: 30, synth.TYPE_DV: 12, synth.TYPE_DM3: 125,
           synth.TYPE_DH3: 187, synth.TYPE_DM5: 228, synth.TYPE_DH5: 343}
TWO_BYTE = {synth.TYPE_DM3, synth.TYPE_DH3, synth.TYPE_DM5, synth.TYPE_DH5}
FEC23 = {synth.TYPE_FHS, synth.TYPE_DM1, synth.TYPE_DM3, synth.TYPE_DM5, synth.TYPE_DV, synth.TYPE_HV2,
         synth.TYPE_EV4}
WITH_CRC = {synth.TYPE_DM1, synth.TYPE_DH1, synth.TYPE_DM3, synth.TYPE_DH3, synth.TYPE_DM5,
            synth.TYPE_DH5, synth.TYPE_DV}
ENTRY_TYPES = list(range(16)) + [16, 255]

# syms: symbol arrays; pin: btbbx_pkt_in entry states; tags: (type name, boundary, body bytes) per packet;
# clk6 / uap: the clock and UAP the packet was built with; air_white: whitened on air; words: packed rows
Lattice = namedtuple("Lattice", "syms pin tags clk6 uap air_white words")


def fec_tail(rng, blocks):
    """`blocks` FEC 2/3 blocks that decode, of random data."""
    return synth.fec23(rng.integers(0, 2, 10 * blocks, dtype=np.uint8))


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(_libs.seed(seed))
        self.syms, self.tags, self.clk6, self.uap, self.air_white = [], [], [], [], []

    def add(self, sym, tag, clk6, uap, whitened=True):
        sym = np.ascontiguousarray(np.asarray(sym, dtype=np.uint8)[:bt.MAX_SYMBOLS])
        self.syms.append(sym)
        self.tags.append(tag)
        self.clk6.append(clk6)
        self.uap.append(uap)
        self.air_white.append(whitened)

    def packet(self, t, n, uap=None, whitened=True, body=None, ev3=False):
        """One packet of type t with an n-byte body -> (symbols, geometry).  geometry: off (the DV data field
        starts 80 symbols behind the header), ph (symbols of the payload header), bits (payload_length * 8 as the
        reference counts it, None where it does not), blocks (FEC 2/3 blocks of the payload), L (bytes the CRC
        covers, CRC included)."""
        rng = self.rng
        lap = int(rng.integers(0, 1 << 24))
        uap = int(rng.integers(0, 256)) if uap is None else uap
        clk6 = int(rng.integers(0, 64))
        if body is None:
            body = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        kw = dict(lt_addr=int(rng.integers(0, 8)), flags=int(rng.integers(0, 8)), llid=int(rng.integers(0, 4)),
                  flow=int(rng.integers(0, 2)), whitened=whitened)
        g = dict(off=0, ph=None, bits=None, blocks=None, L=None)
        if t == 7 and ev3:
            # EV3 on air: body + CRC; synth builds type 7 as HV3 and sends `body` as it is
            crc = synth.crc16(synth.bytes_to_bits(body), uap)
            sym = synth.build_packet(lap, uap, clk6, 7, body=body + bytes([crc & 0xff, crc >> 8]), **kw)
            g["L"] = n + 2
        elif t == synth.TYPE_FHS:
            sym = synth.build_packet(lap, uap, clk6, t, fhs_bits=synth.fhs_payload(lap, uap, int(rng.integers(0, 1 << 16)),
                                                                                  int(rng.integers(0, 1 << 26)), rng), **kw)
            g.update(blocks=16, L=20)
        elif t in (synth.TYPE_HV1, synth.TYPE_HV2, synth.TYPE_HV3):
            sym = synth.build_packet(lap, uap, clk6, t, body=body, **kw)
            if t == synth.TYPE_HV2:
                g["blocks"] = 16
        elif t in (synth.TYPE_NULL, synth.TYPE_POLL):
            sym = synth.build_packet(lap, uap, clk6, t, **kw)
        else:
            sym = synth.build_packet(lap, uap, clk6, t, body=body,
                                     voice=rng.integers(0, 256, 10, dtype=np.uint8).tobytes(), **kw)
            hb = 2 if t in TWO_BYTE else 1
            if t in (synth.TYPE_EV4, synth.TYPE_EV5):
                g["L"] = n + 2
                if t == synth.TYPE_EV4:
                    g["blocks"] = (8 * (n + 2) + 9) // 10
            else:
                g["off"] = 80 if t == synth.TYPE_DV else 0
                g["ph"] = (15 * hb if t in FEC23 else 8 * hb)
                g["L"] = n + hb + (2 if t in WITH_CRC else 0)
                if t in WITH_CRC:
                    g["bits"] = 8 * g["L"]
                if t in FEC23:
                    g["blocks"] = (8 * g["L"] + 9) // 10
        return np.asarray(sym, np.uint8), g, clk6, uap

    def cuts(self, name, t, n, sym, g, clk6, uap, whitened=True, prefix=""):
        """The packet at every length where a check of the reference flips (coinciding lengths: one packet, the
        boundary names joined with '+')."""
        rng = self.rng
        E = len(sym)
        at = {}

        def put(length, what):
            if 0 < length <= bt.MAX_SYMBOLS:
                at.setdefault(length, []).append(what)
        put(E, "end")
        put(E - 1, "end-1")
        if g["ph"] is not None:
            put(122 + g["off"] + g["ph"], "ph_end")
            put(122 + g["off"] + g["ph"] - 1, "ph_end-1")
        if g["bits"] is not None:
            put(122 + g["off"] + g["bits"], "bitlen")
            put(122 + g["off"] + g["bits"] - 1, "bitlen-1")
        put(122, "122")
        put(121, "121")
        for length, what in sorted(at.items()):
            s = sym[:length]
            if length > E:                                  # behind the packet: what the capture holds there
                s = np.concatenate([sym, rng.integers(0, 2, length - E, dtype=np.uint8)])
            self.add(s, (name, prefix + "+".join(what), n), clk6, uap, whitened)
        tail = rng.integers(0, 2, int(rng.integers(0, 400)), dtype=np.uint8)
        self.add(np.concatenate([sym, tail]), (name, prefix + "full", n), clk6, uap, whitened)
        if E < bt.MAX_SYMBOLS:
            self.add(np.concatenate([sym, rng.integers(0, 2, bt.MAX_SYMBOLS - E, dtype=np.uint8)]),
                     (name, prefix + "3125", n), clk6, uap, whitened)
        if t == synth.TYPE_EV4:
            # the reference tests byte count L once the block AFTER the one that completes it has decoded
            need = 122 + 15 * (g["blocks"] + 1)
            ext = np.concatenate([sym, fec_tail(rng, 2), rng.integers(0, 2, 20, dtype=np.uint8)])
            for length, what in ((need, "ev4_need"), (need - 1, "ev4_need-1")):
                self.add(ext[:length], (name, prefix + what, n), clk6, uap, whitened)


def _flip_block(rng, sym, first, k):
    s = sym.copy()
    pos = first + 15 * k + rng.choice(15, 2, replace=False)
    s[pos] ^= 1
    return s


def _flip_triples(rng, sym, n_dis, wrong):
    """n_dis header triples that disagree; with `wrong`, one of them holds two flipped symbols (majority wrong)."""
    s = sym.copy()
    tri = rng.choice(18, n_dis, replace=False)
    for j, k in enumerate(tri):
        if wrong and j == 0:
            s[68 + 3 * k + rng.choice(3, 2, replace=False)] ^= 1
        else:
            s[68 + 3 * k + int(rng.integers(0, 3))] ^= 1
    return s


def build(seed=211):
    b = _Builder(seed)
    rng = b.rng
    with_payload = [synth.TYPE_DM1, synth.TYPE_DH1, synth.TYPE_AUX1, 7, synth.TYPE_DM3, synth.TYPE_DH3,
                    synth.TYPE_DM5, synth.TYPE_DH5, synth.TYPE_EV4, synth.TYPE_EV5, synth.TYPE_DV]
    hdr_subjects = []
    fec_subjects = []
    # every legal body length, and the payload header's length field at the reference's maximum + 1
    for t in with_payload:
        lengths = list(range(MAXBODY[t] + 1))
        over = []
        if t in REF_CAP:
            # a body of n bytes is length field n, payload_length n + header + CRC: the field's maximum is the
            # body's, one above it is the first length the reference clamps to max_length
            over = [REF_CAP[t] - (4 if t in TWO_BYTE else 3) + 1]
        if t == synth.TYPE_AUX1:
            over = [30]
        for n in lengths + over:
            name = NAMES[t]
            sym, g, clk6, uap = b.packet(t, n, ev3=name == "EV3")
            b.cuts(name, t, n, sym, g, clk6, uap, prefix="" if n <= MAXBODY[t] else "field_max+1:")
            if n == MAXBODY[t]:
                b.add(np.concatenate([sym, rng.integers(0, 2, 40, dtype=np.uint8)]), (name, "field_max", n), clk6, uap)
            if t in FEC23 and n <= MAXBODY[t]:
                fec_subjects.append((name, n, sym, g, clk6, uap))
            if n in (0, 1, MAXBODY[t] // 2, MAXBODY[t]):
                hdr_subjects.append((name, n, sym, g, clk6, uap))
    # fixed-size payloads and no payload
    for t, reps in ((synth.TYPE_HV1, 24), (synth.TYPE_HV2, 24), (synth.TYPE_HV3, 24), (synth.TYPE_FHS, 40),
                    (synth.TYPE_NULL, 8), (synth.TYPE_POLL, 8)):
        size = {synth.TYPE_HV1: 10, synth.TYPE_HV2: 20, synth.TYPE_HV3: 30}.get(t, 0)
        for r in range(reps):
            sym, g, clk6, uap = b.packet(t, size)
            name = HV3_AS if t == synth.TYPE_HV3 else NAMES[t]
            b.cuts(name, t, size, sym, g, clk6, uap)
            if t in FEC23:
                fec_subjects.append((name, size, sym, g, clk6, uap))
            if r < 2:
                hdr_subjects.append((name, size, sym, g, clk6, uap))
    # two symbol errors in one FEC 2/3 block: first, last two of the payload, the one behind it
    for name, n, sym, g, clk6, uap in fec_subjects:
        ext = np.concatenate([sym, fec_tail(rng, 3), rng.integers(0, 2, 30, dtype=np.uint8)])
        first = 122 + g["off"]
        nb = g["blocks"]
        b.add(ext, (name, "fec_clean", n), clk6, uap)
        for k, what in ((0, "fec@first"), (nb - 2, "fec@last-1"), (nb - 1, "fec@last"), (nb, "fec@after")):
            if k < 0 or (k == 0 and what != "fec@first"):
                continue
            b.add(_flip_block(rng, ext, first, k), (name, what, n), clk6, uap)
    # 3 and 4 disagreeing header triples, majority right and wrong
    for name, n, sym, g, clk6, uap in hdr_subjects:
        ext = np.concatenate([sym, fec_tail(rng, 3), rng.integers(0, 2, 30, dtype=np.uint8)])
        for n_dis in (3, 4):
            for wrong in (False, True):
                what = "hdr%d_%s" % (n_dis, "wrong" if wrong else "right")
                b.add(_flip_triples(rng, ext, n_dis, wrong), (name, what, n), clk6, uap)
    # EV4: register zero after one byte (UAP 0 seeds 0, first byte 0), not again before the capture ends
    for k in range(24):
        n = 3 + 4 * k
        body = bytes([0, 1 + int(rng.integers(0, 255))]) + rng.integers(0, 256, n - 2, dtype=np.uint8).tobytes()
        sym, g, clk6, uap = b.packet(synth.TYPE_EV4, n, uap=0, body=body)
        for blocks in (2, 3, 4 + k % 5):
            b.add(sym[:122 + 15 * blocks], ("EV4", "reg1_zero", n), clk6, uap)
    # not whitened on air: every type at a few lengths, full and cut one short
    for t, name in [(t, NAMES[t]) for t in with_payload] + [(synth.TYPE_HV1, "HV1"), (synth.TYPE_HV2, "HV2"),
                                                            (synth.TYPE_HV3, HV3_AS), (synth.TYPE_FHS, "FHS"),
                                                            (synth.TYPE_NULL, "NULL"), (synth.TYPE_POLL, "POLL")]:
        fixed = {"HV1": 10, "HV2": 20, "HV3": 30}
        lengths = [fixed.get(name, 0)] * 3 if name in ("HV1", "HV2", "HV3", "FHS", "NULL", "POLL") else \
            sorted({0, 1, MAXBODY[t] // 3, MAXBODY[t]})
        for n in lengths:
            sym, g, clk6, uap = b.packet(t, n, whitened=False, ev3=name == "EV3")
            b.add(np.concatenate([sym, fec_tail(rng, 2)]), (name, "nowh:full", n), clk6, uap, whitened=False)
            b.add(sym[:len(sym) - 1], (name, "nowh:end-1", n), clk6, uap, whitened=False)

    n = len(b.syms)
    words, lengths = bt.packets_to_words(b.syms)
    pin = np.zeros(n, bt.PKTIN_DTYPE)
    pin["length"] = lengths
    air_white = np.array(b.air_white, bool)
    idx = np.arange(n)
    white = air_white.copy()
    against = idx % 13 == 5                                 # the WHITENED flag against what is on air
    white[against] = ~white[against]
    other = rng.integers(0, 8, n)
    pin["flags"] = white.astype(np.uint32) | np.where(other & 1, F_UAP_VALID, 0) \
        | np.where(other & 2, F_CLK6_VALID, 0) | np.where(other & 4, F_HAS_PAYLOAD, 0)
    pin["uap"] = rng.integers(0, 256, n)
    pin["type"] = np.array(ENTRY_TYPES)[idx % len(ENTRY_TYPES)]
    pin["llid"] = idx % 4
    pin["flow"] = (idx // 4) % 2
    # a header whose FEC 1/3 fails leaves the entry's type and UAP to crc_check: now and then the packet's own
    for i, tag in enumerate(b.tags):
        if tag[1].startswith("hdr4") and i % 3 == 0:
            t = [k for k, v in NAMES.items() if v == tag[0]]
            pin["type"][i] = 7 if tag[0] == HV3_AS else t[0]
            pin["uap"][i] = b.uap[i]
    return Lattice(b.syms, pin, b.tags, np.array(b.clk6, np.uint32), np.array(b.uap, np.uint8), air_white, words)


@functools.lru_cache(maxsize=None)
def lattice():
    return build()


def oracle_table(orc, sym, entry):
    """The oracle's 64-clock table of one packet from a btbbx_pkt_in entry state (TRIAL_DTYPE[64])."""
    out = np.zeros(64, np.uint32)
    sym = np.ascontiguousarray(sym, dtype=np.uint8)
    orc.orc_trial_table(_libs.ptr(sym), len(sym), int(entry["flags"]), int(entry["uap"]), int(entry["type"]),
                        int(entry["llid"]), int(entry["flow"]), _libs.ptr(out))
    return out.view(bt.TRIAL_DTYPE)


@functools.lru_cache(maxsize=None)
def tables():
    """[n, 64] TRIAL_DTYPE: the oracle's table of every lattice packet from its entry state."""
    lat, orc = lattice(), _libs.oracle()
    out = np.zeros((len(lat.syms), 64), bt.TRIAL_DTYPE)

    def work(i):
        out[i] = oracle_table(orc, lat.syms[i], lat.pin[i])
    # (ctypes lets go of the GIL for the call; the oracle's tables are read-only once built)
    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(work, range(len(lat.syms)), chunksize=256))
    return out


@functools.lru_cache(maxsize=None)
def header_fec_ok():
    """Per packet: does the header's FEC 1/3 hold (fewer than 4 disagreeing triples)?"""
    lat, orc = lattice(), _libs.oracle()
    out = np.zeros(len(lat.syms), bool)
    buf = np.zeros(18, np.uint8)
    for i, s in enumerate(lat.syms):
        if len(s) >= 122:
            out[i] = bool(orc.orc_unfec13(_libs.ptr(s[68:122].copy()), _libs.ptr(buf), 18))
        else:
            hdr = np.zeros(54, np.uint8)
            hdr[:max(0, len(s) - 68)] = s[68:]
            out[i] = bool(orc.orc_unfec13(_libs.ptr(hdr), _libs.ptr(buf), 18))
    return out


def by_tag(lat, pred):
    """Indices of the packets whose tag satisfies pred(type_name, boundary, L)."""
    return np.array([i for i, t in enumerate(lat.tags) if pred(*t)], dtype=np.int64)


def has(boundary, name):
    return name in boundary.split(":")[-1].split("+")


_PAYLOAD_OFF = _libs.OrcPacket.payload.offset
_PH_OFF = _libs.OrcPacket.payload_header.offset


def oracle_decode(orc, syms, pin):
    """header_present + decode_header + decode_payload of the oracle for every packet from its btbbx_pkt_in entry
    state (flags, UAP, type, llid, flow, clkn), as btbbx_pkt_out records of a zeroed output."""
    out = np.zeros(len(syms), bt.PKTOUT_DTYPE)
    for i, s in enumerate(syms):
        e = pin[i]
        s = np.ascontiguousarray(s, dtype=np.uint8)
        p = orc.orc_packet_new()
        orc.orc_packet_init_found(p, 0, 0)
        orc.orc_packet_set_data(p, _libs.ptr(s), len(s), 0, int(e["clkn"]) << 1)
        c = p.contents
        c.flags, c.UAP, c.packet_type = int(e["flags"]), int(e["uap"]), int(e["type"])
        c.payload_llid, c.payload_flow = int(e["llid"]), int(e["flow"])
        o = out[i]
        o["header_present"] = orc.orc_header_present(p)
        o["header_rv"] = h = orc.orc_decode_header(p)
        o["payload_rv"] = orc.orc_decode_payload(p) if h else 0
        base = C.addressof(c)
        pay = np.frombuffer((C.c_uint8 * 2744).from_address(base + _PAYLOAD_OFF), dtype=np.uint8)
        o["payload"] = np.concatenate([np.packbits(pay, bitorder="little"), np.zeros(1, np.uint8)]).view("<u8")
        ph = np.frombuffer((C.c_uint8 * 16).from_address(base + _PH_OFF), dtype=np.uint8)
        o["payload_header"] = int(np.packbits(ph, bitorder="little").view("<u2")[0])
        o["payload_length"], o["payload_header_length"] = c.payload_length, c.payload_header_length
        o["flags"], o["header_packed"] = c.flags, orc.orc_packet_header_packed(p)
        o["type"], o["lt_addr"], o["hdr_flags"], o["hec"] = c.packet_type, c.packet_lt_addr, c.packet_flags, c.packet_hec
        o["llid"], o["flow"], o["uap"] = c.payload_llid, c.payload_flow, c.UAP
        orc.orc_packet_free(p)
    return out
