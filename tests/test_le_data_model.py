"""The model of LE data extraction (tests/_le_data.py) on its own, without a GPU: on the planted world it returns exactly what was
planted -- every seen packet's role, every message of either direction octet for octet --, its outputs keep what rules 6 and 7
promise, and each deliberately wrong variant differs from it on the lattice the GPU tests run, so that lattice has teeth."""
import pytest

import _le_data as dm
import _le_discover as ld

BIG = (1 << 20, 1 << 30)


def test_the_planted_world_holds_what_the_issue_lists():
    b = dm.planted_world()
    out = dm.planted_model()
    by = dict(zip(b.names, out.data))
    kinds = {(b.names[b.cands[i].channel], d.kind) for i, d in enumerate(out.dpkts) if d is not None}
    assert {len([i for i, c in enumerate(b.cands) if c.channel == 0 and b.pkts[i].event == e]) for e in range(6)} >= {1, 2, 3, 4, 5}
    assert by["planted: retransmissions"].n_retransmit == 2 and by["planted: retransmissions"].n_control == 1
    assert by["planted: a lost packet"].n_unknown == 2 and by["planted: not timed"].n_unknown == 2
    assert by["planted: odd messages"].n_orphan == 2 and ("planted: odd messages", dm.IGNORED) in kinds
    flags = [m.flags for m in out.msgs if b.names[m.conn] == "planted: odd messages"]
    assert flags.count(dm.RUNT | dm.STORED) == 2 and dm.OVERRUN | dm.STORED in flags and dm.STORED in flags     # (cut short: neither)
    assert not b.tracks[b.names.index("planted: not timed")].flags & 1
    assert sum(c.channel == ld.NO_CONN for c in b.cands) >= 40


def test_planted_truth():
    b = dm.planted_world()
    out = dm.planted_model()
    assert dm.check_planted(b, out) == out.n_msgs == 116
    dm.check_invariants(out, b.conns, b.cands, b.pkts, *BIG)
    # the fragments of a message lie behind each other in the buffer, and a two-fragment message crosses two events
    two = [m for m in out.msgs if m.n_fragments == 2]
    assert two and any(len({b.pkts[i].event for i, d in enumerate(out.dpkts) if d is not None and d.msg == M}) == 2
                       for M, m in enumerate(out.msgs) if m.n_fragments == 2)


@pytest.mark.parametrize("which", ["align", "long", "crowd", "both"])
def test_invariants_on_the_hand_made_lists(which):
    b = dm.align_list() if which == "align" else dm.seam_list(which)
    out = dm.built_model(b)
    dm.check_invariants(out, b.conns, b.cands, b.pkts, *BIG)
    if which == "align":
        assert {m.byte_offset % 8 for m in out.msgs} == set(range(8)) and {b.cands[m.start].length for m in out.msgs} == set(dm.ALIGN_LENGTHS)
        assert {b.cands[i].offset % 64 for i, d in enumerate(out.dpkts) if d is not None and d.kind <= dm.CONTINUATION} == set(range(64))
        end = 64 * b.n_words
        assert any(c.offset + 56 < end < c.offset + 56 + 8 * c.length for c in b.cands) and any(c.offset + 56 >= end for c in b.cands)
    if which in ("long", "both"):
        g = max(range(len(b.conns)), key=lambda x: b.conns[x].n_packets)
        first, d = b.conns[g].first, out.data[g]
        assert first % 64 and d.n_retransmit >= 3 * 40 and d.n_msgs >= 2 * 40
        seen = dm.check_seams(b, out)                           # in slot space: the kernels' seams, not multiples of a rank
        assert seen[64] >= 44 and seen[256] >= 11 and seen[2048] == 1, seen
        tile = [s for s in range(2048, first + b.conns[g].n_packets, 2048) if s > first][0]
        assert {2048: which == "long", 4096: which == "both"}[tile]


@pytest.mark.parametrize("caps", [(0, 0), (3, 1 << 30), (1 << 20, 100), (1 << 20, 104), (7, 105)])
def test_caps_cut_a_prefix(caps):
    b = dm.planted_world()
    whole, out = dm.planted_model(), dm.planted_model(*caps)
    dm.check_invariants(out, b.conns, b.cands, b.pkts, *caps)
    assert (out.n_msgs, out.n_bytes, out.data, out.dpkts) == (whole.n_msgs, whole.n_bytes, whole.data, whole.dpkts)
    assert whole.payload.startswith(out.payload) and len(out.msgs) == min(caps[0], whole.n_msgs)


@pytest.mark.parametrize("name", sorted(dm.VARIANTS))
def test_a_wrong_variant_differs_on_the_lattice(name):
    rules = dm.Rules(**dm.VARIANTS[name])
    b = dm.planted_world()
    right, wrong = dm.planted_model(), dm.planted_model(rules=rules)
    assert (wrong.dpkts, wrong.msgs, wrong.payload) != (right.dpkts, right.msgs, right.payload)
    a = dm.align_list()
    if name in ("whiten_restart", "role_flip", "order_by_index"):                        # the hand-made list tells these as well
        assert tuple(dm.built_model(a, rules=rules)) != tuple(dm.built_model(a))
    assert b.names.count(None) == 0
