"""Worlds that pin LE data extraction (libbtbb_amd/csrc/le_data.h) where the planted world and the lists of tests/_le_data.py leave it
free, for tests/test_le_data_lattice_model.py (CPU) and tests/test_gpu_le_data_lattice.py (GPU):

* sequence_world: every short sequence of member states as a connection of its own -- the scan operators' `combine` over every pair
  and triple of neighbours --, with planted L2CAP headers so that COMPLETE and OVERRUN occur
* product_list: the gather's full product of source residue mod 64, destination residue mod 8 and length, the channels cycling;
  end_list: fragments and headers that end at every distance -72..72 bits from the streams' end, rows abutting
* far_world: more than 2^32 octets, built and expected in closed form with numpy (the closed form is held against the model at a
  small size)
* LATTICE_VARIANTS: wrong models that these worlds tell from the right one (the planted world of _le_data.py need not)
"""
import collections
import functools
import itertools

import numpy as np

import _le
import _le_data as dm
import _le_discover as ld
import _le_track as lt

LATTICE_VARIANTS = dict(unknown_sets_sn=dict(unknown_sets_sn=True), empty_breaks=dict(empty_breaks=True), retx_joins=dict(retx_joins=True),
                        end_reads_on=dict(end_reads_on=True), whiten_period_128=dict(whiten_period_128=True),
                        offset_mod_2_32=dict(offset_mod_2_32=True))
RULE_VARIANTS = ("unknown_sets_sn", "empty_breaks", "retx_joins")            # told apart by the sequence world
ALL_VARIANTS = dict(dm.VARIANTS, **LATTICE_VARIANTS)
N_WORDS = 64
N_STREAMS = 37


def _plant(words, stream, bit, octets):
    """Writes `octets` as a payload at stream bit `bit` (the packet's offset + 56), whitened with channel `stream`'s sequence
    behind the two header octets."""
    bits = np.unpackbits(words[stream].view(np.uint8), bitorder="little")
    n = 8 * len(octets)
    bits[bit:bit + n] = _le.octet_bits(octets) ^ _le._whitening_2080(stream)[16:16 + n]
    words[stream] = _le.pack(bits)


# ---- A. the sequence world -----------------------------------------------------------------------------------------------------------
SAME, HEAD, TAIL = 0, 1, 2                                          # a member's step: same event / a new counter / a tail
BODIES = ((1, 0), (1, 3), (2, 5), (3, 2))                           # (llid, L): EMPTY, a continuation, a START, CONTROL
ODD_BODIES = ((0, 2), (2, 0))                                       # IGNORED
PLACES = ((200, 1), (1301, 0), (2722, 4))                           # (a START's offset, the l2cap_len planted there)


def _symbols(steps, bodies):
    return [(step, llid, L, sn) for step in steps for llid, L in bodies for sn in (0, 1)]


FULL = _symbols((SAME, HEAD, TAIL), BODIES)                         # 24
PLAIN = _symbols((SAME, HEAD), BODIES[:3])                          # 12: no tail, no control
WIDE = _symbols((SAME, HEAD, TAIL), BODIES + ODD_BODIES)            # 36
LONG = 2500


def _sequences(alphabet, n):
    """Every sequence of n symbols; the first member lies in event 0 whatever its step, so it takes the SAME symbols only."""
    return itertools.product([s for s in alphabet if s[0] == SAME], *([alphabet] * (n - 1)))


def sequence_set(n_sampled=6000, seed=17):
    seqs = list(_sequences(FULL, 1)) + list(_sequences(WIDE, 2)) + list(_sequences(FULL, 3)) + list(_sequences(PLAIN, 4))
    rng = np.random.default_rng(seed)
    first = [k for k, s in enumerate(PLAIN) if s[0] == SAME]
    for row in rng.integers(0, len(PLAIN), (n_sampled, 6)).tolist():
        seqs.append(tuple([PLAIN[first[row[0] % len(first)]]] + [PLAIN[k] for k in row[1:]]))
    seqs = [seqs[i] for i in rng.permutation(len(seqs))]
    # one connection of LONG members between them: whole waves of one connection, in which every tally counts some lanes and not all
    row = rng.integers(0, len(FULL), LONG).tolist()
    seqs.insert(len(seqs) // 2, tuple([FULL[row[0] % 8]] + [FULL[k] for k in row[1:]]))
    return seqs


def _sequence_members(g, seq):
    members, event, counter = [], 0, 0
    for j, (step, llid, L, sn) in enumerate(seq):
        if j and step != SAME:
            event += 1
            counter += step == HEAD
        h0 = llid | ((g + j) & 1) << 2 | sn << 3 | ((g >> 2) & 1) << 4
        offset = PLACES[(g + j // 7) % 3][0] if (llid, L) == (2, 5) else (g * 131 + j * 977) % 4000
        members.append(dm.H(event, counter, h0, L, offset, (g + 5 * j) % N_STREAMS))
    return members


@functools.lru_cache(maxsize=None)
def sequence_world():
    seqs = sequence_set()
    words = np.random.default_rng(23).integers(0, 1 << 64, (N_STREAMS, N_WORDS), dtype=np.uint64)
    rng = np.random.default_rng(29)
    for c in range(N_STREAMS):
        for offset, claim in PLACES:
            _plant(words, c, offset + 56, bytes([claim, 0]) + bytes(rng.integers(0, 256, 3, dtype=np.uint8).tolist()))
    words.flags.writeable = False
    gaps = [1 if g % 7 == 3 else 0 for g in range(len(seqs))]
    return dm.hand_built([_sequence_members(g, s) for g, s in enumerate(seqs)], N_WORDS, n_streams=N_STREAMS, seed=31, gap=gaps, words=words)


@functools.lru_cache(maxsize=None)
def sequence_model(variant=None, msg_cap=1 << 20, byte_cap=1 << 30):
    rules = dm.MODEL if variant is None else dm.Rules(**ALL_VARIANTS[variant])
    return dm.built_model(sequence_world(), msg_cap, byte_cap, rules)


# ---- B. the gather's lattices ----------------------------------------------------------------------------------------------------------
PRODUCT_LENGTHS = tuple(range(1, 18)) + (23, 24, 25, 31, 32, 33, 63, 64, 65, 127, 128, 251, 255)


class _Line:
    """One connection, one member per event (every member CENTRAL, every event HEAD), the SN toggling (every member NEW)."""

    def __init__(self):
        self.members, self.total = [], 0

    def add(self, llid, L, offset, stream):
        e = len(self.members)
        self.members.append(dm.H(e, e & 0xFFFF, llid | (e & 1) << 3, L, offset, stream))
        self.total += L

    def cell(self, head, L, offset, stream, start_offset):
        """A CONTINUATION of L octets whose destination is `head` mod 8: behind a START of 1 to 8 octets."""
        self.add(2, (head - self.total - 1) % 8 + 1, start_offset, stream)
        assert self.total % 8 == head
        self.add(1, L, offset, stream)


@functools.lru_cache(maxsize=None)
def product_list():
    """Source residue (offset + 56) mod 64 x head x PRODUCT_LENGTHS as continuations, the streams cycling over all channels; then a
    START of exactly four octets at every source residue on every channel (the header read)."""
    line, cell = _Line(), 0
    for L in PRODUCT_LENGTHS:
        rows = (64 * N_WORDS - 56 - 8 * L - 63) // 64 + 1            # offsets 64 k + r with the payload inside the stream
        for head in range(8):
            for res in range(64):
                line.cell(head, L, 64 * (cell % rows) + (res - 56) % 64, cell % N_STREAMS, (cell * 29) % 3900)
                cell += 1
    for c in range(N_STREAMS):
        for res in range(64):
            line.add(2, 4, 64 * ((c * 64 + res) % 60) + (res - 56) % 64, c)
    return dm.hand_built([line.members], N_WORDS, n_streams=N_STREAMS, seed=37, gap=2)


END_LENGTHS = (1, 8, 9, 17)
END_D = tuple(range(-72, 73))


@functools.lru_cache(maxsize=None)
def end_list(pad):
    """Rows of N_WORDS words, `pad` words (all ones) between them; odd rows all ones, even rows random, so that a read across a row's
    end shows whichever row it is.  Continuations of END_LENGTHS that end at 64 N_WORDS + d bits for every d of END_D and every
    head, and a START of four octets per d."""
    end = 64 * N_WORDS
    words = np.full((N_STREAMS, N_WORDS + pad), 0xFFFFFFFFFFFFFFFF, np.uint64)
    words[::2, :N_WORDS] = np.random.default_rng(43).integers(0, 1 << 64, ((N_STREAMS + 1) // 2, N_WORDS), dtype=np.uint64)
    words.flags.writeable = False
    line, cell = _Line(), 0
    for L in END_LENGTHS:
        for d in END_D:
            for head in range(8):
                line.cell(head, L, end + d - 56 - 8 * L, (cell + cell // 296) % N_STREAMS, (cell * 13) % 3000)
                cell += 1
    for k, d in enumerate(END_D):
        line.add(2, 4, end + d - 56 - 32, (36 - k) % N_STREAMS)
    return dm.hand_built([line.members], N_WORDS, n_streams=N_STREAMS, seed=47, gap=1, words=words)


def fragment_cells(b, out):
    """From the MODEL's records and the candidates, not from the builder: per fragment (source residue, head, L, kind, list index)."""
    cells = []
    for i, d in enumerate(out.dpkts):
        if d is not None and d.kind <= dm.CONTINUATION:
            c = b.cands[i]
            cells.append(((c.offset + 56) % 64, (out.msgs[d.msg].byte_offset + d.pos) % 8, c.length, d.kind, i))
    return cells


# ---- C. the far world ------------------------------------------------------------------------------------------------------------------
FAR_COUNTS, FAR_FRAGS = (100, 65600, 150, 50), 257
FAR_L = 255
FAR_PLACES = 61
Far = collections.namedtuple("Far", "cands conns pkts words counts frags first n_words")


def _far_index(counts, frags, first, M, j):
    """The list index of fragment j of message M (numpy arrays or numbers)."""
    counts = np.asarray(counts, np.int64)
    before = np.concatenate([[0], np.cumsum(counts)])
    g = np.searchsorted(before, M, side="right") - 1
    rank = (M - before[g]) * frags + j
    return first[g] + np.where((rank | 3) < counts[g] * frags, rank ^ 3, rank), g, rank


def far_world(msgs_per_conn, frags, dtypes, seed=53):
    """Connections of msgs_per_conn messages, each a START and frags - 1 CONTINUATIONs of 255 octets, one member per event: all
    CENTRAL, HEAD and NEW.  Message M (over all connections) lies on channel M mod 37, its START at offset 33 (M mod 61), where the
    stream holds l2cap_len = 255 frags - 4: every message is COMPLETE.  Members overlap in the 64-word streams.  One non-member
    leads the list; within a connection the list order swaps ranks in fours (rank ^ 3).  dtypes: the candidate, connection and
    tracking-packet record types.  -> Far, records as arrays."""
    cand_t, conn_t, pkt_t = dtypes
    counts = np.asarray(msgs_per_conn, np.int64)
    assert 4 <= frags * FAR_L - 4 <= 0xFFFF
    members = counts * frags
    first = 1 + np.concatenate([[0], np.cumsum(members)[:-1]])
    n = 1 + int(members.sum())
    idx = np.arange(n - 1, dtype=np.int64)
    M, j = idx // frags, idx % frags
    at, g, rank = _far_index(counts, frags, first, M, j)
    cands, pkts = np.zeros(n, cand_t), np.zeros(n, pkt_t)
    pkts.view(np.uint8)[:pkt_t.itemsize] = 0xFF
    cands[0] = (77, 0x11110000, 7, 0, 1, 0, ld.NO_CONN)
    cands["offset"][at] = np.where(j == 0, 33 * (M % FAR_PLACES), (33 * (M % FAR_PLACES) + 17 * j) % 1999)
    cands["access_address"][at] = 0x50000000 + g
    cands["crc_init"][at] = 0x100 + g
    cands["stream"][at] = M % N_STREAMS
    cands["header0"][at] = np.where(j == 0, 2, 1) | (rank & 1) << 3
    cands["length"][at] = FAR_L
    cands["conn"][at] = g
    pkts["rank"][at] = pkts["event"][at] = pkts["counter"][at] = rank
    pkts["channel"][at] = M % N_STREAMS
    pkts["unmapped"][at] = pkts["expected"][at] = 0xFF
    conns = np.zeros(len(counts), conn_t)
    conns["access_address"], conns["crc_init"] = 0x50000000 + np.arange(len(counts)), 0x100 + np.arange(len(counts))
    conns["n_packets"], conns["channel_mask"], conns["first"] = members, (1 << 37) - 1, first
    words = np.random.default_rng(seed).integers(0, 1 << 64, (N_STREAMS, N_WORDS), dtype=np.uint64)
    claim = frags * FAR_L - 4
    for c in range(N_STREAMS):
        for k in range(FAR_PLACES):
            _plant(words, c, 33 * k + 56, bytes([claim & 0xFF, claim >> 8]))
    words.flags.writeable = False
    return Far(cands, conns, pkts, words, counts, frags, first, N_WORDS)


def far_offsets(msgs_per_conn, frags, rules=dm.MODEL):
    """byte_offset of every message, in closed form."""
    off = np.arange(int(np.sum(msgs_per_conn)), dtype=np.uint64) * np.uint64(frags * FAR_L)
    return off & np.uint64(0xFFFFFFFF) if rules.offset_mod_2_32 else off


def far_expected(w, dtypes, msg_cap, byte_cap, rules=dm.MODEL, fixed=None):
    """The four outputs' records in closed form -> (data, dpkts, msgs, n_msgs, n_bytes); dtypes: the connection-data, data-packet
    and message record types; fixed: far_fixed's, which no cap changes, where the caller kept them."""
    counts, size = w.counts, w.frags * FAR_L
    data, dpkts = fixed if fixed is not None else far_fixed(w, dtypes[:2])
    return data, dpkts, far_msgs(w, dtypes[2], msg_cap, byte_cap, rules), int(counts.sum()), int(counts.sum()) * size


def far_fixed(w, dtypes):
    """The connection and data-packet records in closed form."""
    data_t, dpkt_t = dtypes
    counts, frags = w.counts, w.frags
    size = frags * FAR_L
    before = np.concatenate([[0], np.cumsum(counts)])
    data = np.zeros(len(counts), data_t)
    data["bytes"], data["first_msg"], data["n_msgs"] = counts * size, before[:-1], counts
    data["n_complete"], data["n_central"] = counts, counts * frags
    n = len(w.cands)
    idx = np.arange(n - 1, dtype=np.int64)
    at, g, rank = _far_index(counts, frags, w.first, idx // frags, idx % frags)
    dpkts = np.zeros(n, dpkt_t)
    dpkts.view(np.uint8)[:dpkt_t.itemsize] = 0xFF
    dpkts["msg"][at], dpkts["pos"][at] = idx // frags, FAR_L * (idx % frags)
    dpkts["kind"][at], dpkts["bits"][at] = idx % frags != 0, rank & 1
    return data, dpkts


def far_msgs(w, msg_t, msg_cap, byte_cap, rules=dm.MODEL):
    """The first msg_cap message records in closed form."""
    counts, frags = w.counts, w.frags
    size = frags * FAR_L
    M = np.arange(min(int(counts.sum()), msg_cap), dtype=np.int64)
    cid = np.zeros((N_STREAMS, FAR_PLACES), np.uint16)                  # octets 2 and 3 behind the planted length
    for c in range(N_STREAMS):
        for k in range(FAR_PLACES):
            o = dm.payload_octets(w.words[c], w.n_words, 33 * k, 4, c)
            assert o[0] | o[1] << 8 == size - 4
            cid[c, k] = o[2] | o[3] << 8
    msgs = np.zeros(len(M), msg_t)
    full = far_offsets(counts, frags)[:len(M)]
    msgs["byte_offset"] = far_offsets(counts, frags, rules)[:len(M)]
    msgs["start"], msgs["conn"], _ = _far_index(counts, frags, w.first, M, 0)
    msgs["n_fragments"], msgs["bytes"], msgs["l2cap_len"] = frags, size, size - 4
    msgs["cid"] = cid[M % N_STREAMS, M % FAR_PLACES]
    msgs["flags"] = dm.COMPLETE | np.where(full + np.uint64(size) <= np.uint64(byte_cap), dm.STORED, 0)
    return msgs


def far_octets(w, M):
    """The octets of message M, from the streams."""
    out = bytearray()
    for j in range(w.frags):
        c = w.cands[int(_far_index(w.counts, w.frags, w.first, M, j)[0])]
        out += dm.payload_octets(w.words[int(c["stream"])], w.n_words, int(c["offset"]), int(c["length"]), int(c["stream"]))
    return bytes(out)


def far_tuples(w):
    """The far world's records as the tuples the model reads -> (conns, cands, pkts)."""
    pkts = [None if int(p["rank"]) == dm.NONE else lt.Pkt(*(int(p[k]) for k in lt.Pkt._fields)) for p in w.pkts]
    return [ld.Conn(*(int(c[k]) for k in ld.Conn._fields)) for c in w.conns], ld.cand_tuples(w.cands), pkts
