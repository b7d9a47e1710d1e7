"""The worlds of tests/_le_data_lattice.py on their own, without a GPU: each holds what it was built for -- read off the MODEL's
output, not the builder's intent --, the model keeps its invariants on them, the far world's closed forms are the model's at a small
size, and every wrong variant is told apart by the world that owns it."""
import collections

import numpy as np
import pytest

import _le_data as dm
import _le_data_lattice as dl
import libbtbb_amd as bt

BIG = (1 << 20, 1 << 30)
IN_TYPES = (bt.LE_CAND_DTYPE, bt.LE_CONN_DTYPE, bt.LE_TRACK_PKT_DTYPE)
OUT_TYPES = (bt.LE_DATA_DTYPE, bt.LE_DATA_PKT_DTYPE, bt.LE_MSG_DTYPE)


def _differs(a, b):
    return (a.data, a.dpkts, a.msgs, a.payload) != (b.data, b.dpkts, b.msgs, b.payload)


# ---- A -----------------------------------------------------------------------------------------------------------------------------
def test_the_sequence_set_is_exhaustive():
    seqs = dl.sequence_set()
    by_len = collections.Counter(len(s) for s in seqs)
    assert (len(dl.FULL), len(dl.PLAIN), len(dl.WIDE)) == (24, 12, 36)
    assert by_len[1] == 8 and by_len[2] == 12 * 36 and by_len[3] == 8 * 24 * 24 and by_len[4] == 6 * 12 ** 3 and by_len[6] >= 5000
    have = set(seqs)
    firsts = [s for s in dl.FULL if s[0] == dl.SAME]
    assert all((a, b, c) in have for a in firsts for b in dl.FULL for c in dl.FULL)
    # the issue's example: a RETRANSMIT directly behind an UNKNOWN member, in front of a CONTINUATION of the other role
    assert ((dl.SAME, 2, 5, 0), (dl.TAIL, 1, 3, 1), (dl.HEAD, 2, 5, 0)) in have


def test_the_sequence_world():
    b, out = dl.sequence_world(), dl.sequence_model()
    dm.check_invariants(out, b.conns, b.cands, b.pkts, *BIG)
    assert len(b.conns) >= 21000 and sum(c.n_packets for c in b.conns) >= 90000
    assert 0 < sum(c.channel == dm.ld.NO_CONN for c in b.cands) < len(b.conns) // 4
    kinds = collections.Counter(d.kind for d in out.dpkts if d is not None)
    assert set(kinds) == set(range(8)) and min(kinds.values()) >= 100, kinds
    flags = collections.Counter(m.flags for m in out.msgs)
    assert set(flags) == {dm.STORED, dm.STORED | dm.COMPLETE, dm.STORED | dm.OVERRUN} and min(flags.values()) >= 100, flags
    assert {m.n_fragments for m in out.msgs} >= {1, 2, 3, 4}
    # a four-octet header means COMPLETE only through a continuation: 5 + 3 = 4 + 4
    assert sum(m.flags & dm.COMPLETE and m.l2cap_len == 4 and m.n_fragments == 2 for m in out.msgs) >= 100
    # the long connection: whole waves of one connection in which each of the eight tallies counts some members and not all
    g = max(range(len(b.conns)), key=lambda x: b.conns[x].n_packets)
    assert b.conns[g].n_packets == dl.LONG and all(1 <= t <= dl.LONG - 64 for t in out.data[g][3:]), out.data[g]
    assert {m.l2cap_len for m in out.msgs} == {0, 1, 4} and {b.cands[m.start].offset % 64 for m in out.msgs} == {8, 21, 34}
    print("sequence world: %d connections, %d candidates, %d messages, %d octets; kinds %s" %
          (len(b.conns), len(b.cands), out.n_msgs, out.n_bytes, sorted(kinds.items())))


def test_the_sequence_world_under_caps():
    b, whole = dl.sequence_world(), dl.sequence_model()
    caps = sequence_caps(whole)
    out = dl.sequence_model(None, *caps)
    dm.check_invariants(out, b.conns, b.cands, b.pkts, *caps)
    stored = sum(bool(m.flags & dm.STORED) for m in out.msgs)
    assert 0 < stored < len(out.msgs) == caps[0] < whole.n_msgs
    cut = out.msgs[stored]
    assert cut.byte_offset < caps[1] < cut.byte_offset + cut.bytes and cut.n_fragments >= 2     # byte_cap cuts inside a message


def sequence_caps(whole):
    """msg_cap = half the messages; byte_cap inside the first message of two or more fragments behind a third of them."""
    m = [m for m in whole.msgs[whole.n_msgs // 3:] if m.n_fragments >= 2][0]
    return whole.n_msgs // 2, m.byte_offset + m.bytes - 2


@pytest.mark.parametrize("name", sorted(dm.VARIANTS) + list(dl.RULE_VARIANTS))
def test_a_wrong_rule_differs_on_the_sequence_world(name):
    right, wrong = dl.sequence_model(), dl.sequence_model(name)
    n = sum(x != y for x, y in zip(right.dpkts, wrong.dpkts))
    print("%s: %d packet records differ" % (name, n))
    assert _differs(right, wrong)
    if name in dl.RULE_VARIANTS:
        assert n >= 100


# ---- B -----------------------------------------------------------------------------------------------------------------------------
def test_the_product_lattice_is_complete():
    b = dl.product_list()
    out = dm.built_model(b)
    dm.check_invariants(out, b.conns, b.cands, b.pkts, *BIG)
    cells = dl.fragment_cells(b, out)
    have = {(res, head, L) for res, head, L, kind, i in cells if kind == dm.CONTINUATION}
    assert have == {(res, head, L) for res in range(64) for head in range(8) for L in dl.PRODUCT_LENGTHS} and len(have) == 15360
    # ldt_read64's unshifted branch for a fragment's first word, under every head
    assert {head for res, head, L, kind, i in cells if (res - 8 * head) % 64 == 0} == set(range(8))
    # the header read: a START of exactly four octets at every source residue on every channel
    four = {(res, b.cands[i].stream) for res, head, L, kind, i in cells if kind == dm.START and L == 4 and out.msgs[out.dpkts[i].msg].bytes == 4}
    assert four >= {(res, c) for res in range(64) for c in range(37)}
    # every channel's whitening under every length
    assert {(b.cands[i].stream, L) for res, head, L, kind, i in cells} >= {(c, L) for c in range(37) for L in dl.PRODUCT_LENGTHS}
    assert _differs(out, dm.built_model(b, rules=dm.Rules(**dl.LATTICE_VARIANTS["whiten_period_128"])))
    assert not _differs(out, dm.built_model(b, rules=dm.Rules(**dl.LATTICE_VARIANTS["end_reads_on"])))     # nothing here reads beyond an end


@pytest.mark.parametrize("pad", [0, 1])
def test_the_end_lattice(pad):
    b = dl.end_list(pad)
    out = dm.built_model(b)
    dm.check_invariants(out, b.conns, b.cands, b.pkts, *BIG)
    end = 64 * b.n_words
    cells = dl.fragment_cells(b, out)
    have = {(b.cands[i].offset + 56 + 8 * L - end, head, L) for res, head, L, kind, i in cells if kind == dm.CONTINUATION}
    assert have == {(d, head, L) for d in dl.END_D for head in range(8) for L in dl.END_LENGTHS}
    assert {b.cands[i].offset + 56 + 32 - end for res, head, L, kind, i in cells if kind == dm.START and L == 4} >= set(dl.END_D)
    # a fragment across the end of an even row, of an odd row and of the last row
    across = {b.cands[i].stream for res, head, L, kind, i in cells if b.cands[i].offset + 56 < end < b.cands[i].offset + 56 + 8 * L}
    assert 36 in across and {s & 1 for s in across} == {0, 1}
    assert np.asarray(b.words).shape == (37, 64 + pad) and (np.asarray(b.words)[1::2] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()
    wrong = dm.built_model(b, rules=dm.Rules(**dl.LATTICE_VARIANTS["end_reads_on"]))
    assert _differs(out, wrong)
    assert sum(x != y for x, y in zip(out.msgs, wrong.msgs)) >= 30                     # the header read as well as the gather
    # the pad word changes nothing of the right model
    assert tuple(out) == tuple(dm.built_model(dl.end_list(0)))


# ---- C -----------------------------------------------------------------------------------------------------------------------------
def test_the_far_world_closed_forms_are_the_model_at_a_small_size():
    counts, frags = (3, 40, 5, 2), 5
    w = dl.far_world(counts, frags, IN_TYPES)
    conns, cands, pkts = dl.far_tuples(w)
    n_msgs, n_bytes = sum(counts), sum(counts) * frags * 255
    for msg_cap, byte_cap in (BIG, (0, 0), (n_msgs, n_bytes), (17, 1 << 30), (1 << 20, 10 * frags * 255 + 7)):
        want = dm.data(conns, cands, pkts, w.words, w.n_words, msg_cap, byte_cap)
        dm.check_invariants(want, conns, cands, pkts, msg_cap, byte_cap)
        data, dpkts, msgs, got_msgs, got_bytes = dl.far_expected(w, OUT_TYPES, msg_cap, byte_cap)
        assert (got_msgs, got_bytes) == (want.n_msgs, want.n_bytes) == (n_msgs, n_bytes)
        assert data.tobytes() == dm.data_array(want.data, OUT_TYPES[0]).tobytes()
        assert dpkts.tobytes() == dm.dpkt_array(want.dpkts, OUT_TYPES[1]).tobytes()
        assert msgs.tobytes() == dm.msg_array(want.msgs, OUT_TYPES[2]).tobytes()
        stored = sum(bool(m.flags & dm.STORED) for m in want.msgs)
        assert b"".join(dl.far_octets(w, M) for M in range(stored)) == want.payload
    assert all(m.flags & dm.COMPLETE for m in want.msgs) and {d.role for d in want.dpkts if d is not None} == {dm.CENTRAL}
    assert [c.first for c in conns] == sorted(c.first for c in conns) and conns[0].first == 1
    # kept modulo 2^32 the offsets are the same at this size: only the full size tells
    wrong = dm.data(conns, cands, pkts, w.words, w.n_words, *BIG, rules=dm.Rules(**dl.LATTICE_VARIANTS["offset_mod_2_32"]))
    assert tuple(wrong) == tuple(dm.data(conns, cands, pkts, w.words, w.n_words, *BIG))
    assert (dl.far_offsets(counts, frags) == dl.far_offsets(counts, frags, dm.Rules(offset_mod_2_32=True))).all()


def test_the_far_world_arithmetic_at_full_size():
    counts, frags = dl.FAR_COUNTS, dl.FAR_FRAGS
    size = frags * dl.FAR_L
    assert size == 65535 == 4 + 65531
    off = dl.far_offsets(counts, frags)
    assert off.dtype == np.uint64 and len(off) == 65900 and sum(counts) * frags == 16936300
    assert int(off[65537]) == (1 << 32) - 1                                # the crossing inside the first word of a START
    assert int(off[65536]) + size < 1 << 32 < int(off[65537]) + 8
    assert counts[1] * size > 1 << 32                                      # one connection's octets need 64 bits
    assert counts[0] + counts[1] > 65537 and 65537 - counts[0] < counts[1]          # the crossing lies inside the second connection
    assert int(off[counts[0] + counts[1]]) > 1 << 32                      # two whole connections behind it
    assert sum(counts) * size == 4318756500 > 1 << 32
    assert (1 << 32) // 255 < sum(counts) * frags                          # the 32-bit running octet sums wrap
    wrong = dl.far_offsets(counts, frags, dm.Rules(**dl.LATTICE_VARIANTS["offset_mod_2_32"]))
    assert (wrong[:65537] == off[:65537]).all() and (wrong[65538:] != off[65538:]).all() and int(wrong[65538]) == size - 1


def test_every_lattice_variant_has_an_owner():
    assert set(dl.LATTICE_VARIANTS) == set(dl.RULE_VARIANTS) | {"end_reads_on", "whiten_period_128", "offset_mod_2_32"}
    assert not set(dl.LATTICE_VARIANTS) & set(dm.VARIANTS)
