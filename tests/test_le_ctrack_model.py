"""The model of the LE Coded connection tracking (tests/_le_ctrack.py) against the models it stands on, without a GPU: its restated
tracking rules against tests/_le_track.py, its durations against the discovery's and the decoder's models, the wrong variants
against the shared lists, and what the chain capture holds -- among it the statement of the feature: on coded connections the 1M
duration doubles the events and times nothing."""
import numpy as np
import pytest

import _le
import _le_cfind as f
import _le_coded as c
import _le_csa2 as c2
import _le_ctrack as m
import _le_discover as ld
import _le_track as lt


def _both(conns, cands, flags):
    want = lt.track(cands, len(conns), lt.LATTICE_MHZ, lt.N_STREAMS, m.UNIT, m.IFS, m.JITTER, flags)
    got = m.track(cands, len(conns), lt.LATTICE_MHZ, lt.N_STREAMS, m.UNIT, m.IFS, m.JITTER, flags, m.one_m_durations(cands))
    return want, got


@pytest.mark.parametrize("flags", [0, lt.REMAP])
def test_one_m_durations_give_the_tracking_model_on_the_lattice(flags):
    for min_count in (1, 2):
        conns, cands, _ = lt.lattice_list(min_count)
        want, got = _both(conns, cands, flags)
        assert got == want and len(conns) >= 50
    conns, cands, _ = lt.lattice_list()
    for unit, ifs, jitter in ((2, lt.IFS, 0), (1250, 0, 0), (625, 150, 312 - 1)):        # (unit 2: the gcd beyond 32 bits)
        assert m.track(cands, len(conns), lt.LATTICE_MHZ, lt.N_STREAMS, unit, ifs, jitter, flags, m.one_m_durations(cands)) == \
            lt.track(cands, len(conns), lt.LATTICE_MHZ, lt.N_STREAMS, unit, ifs, jitter, flags)


@pytest.mark.parametrize("name", ["seam", "align A", "align B", "crowd", "long events"])
def test_one_m_durations_give_the_tracking_model_on_the_large_lists(name):
    conns, cands = {"seam": lt.seam_list, "align A": lambda: lt.align_list("A"), "align B": lambda: lt.align_list("B"), "crowd": lt.crowd_list,
                    "long events": lt.long_event_list}[name]()[:2]
    want, got = _both(conns, cands, lt.REMAP)
    assert got == want


def test_durations_equal_the_discovery_models_info():
    cap, _ = f.chain_capture()
    found = cap.candidates(27, 16)
    assert len(found) >= 40
    got = m.symbols(cap.words, cap.n_words, [cd for cd, _ in found], len(cap.mhz))
    assert got == [i.symbols for _, i in found] and len(set(got)) > 10
    cap = f.lattice(True)
    found = list(f.lattice_model(True, 255, 63))
    got = m.symbols(cap.words, cap.n_words, [cd for cd, _ in found], len(cap.mhz))
    assert got == [i.symbols for _, i in found] and {i.s for _, i in found} == {2, 8} and max(got) == 17040


def test_durations_equal_the_decoders_info_for_planted_packets():
    rng = np.random.default_rng(5)
    line = rng.integers(0, 2, 64 * 120, dtype=np.uint8)
    at, hits = 21, []
    for s, ci, length in ((8, None, 0), (2, None, 0), (8, None, 9), (2, None, 31), (8, 2, 4), (2, 3, 4), (2, 2, 0)):
        sym = c.coded_symbols(0x5A3C96E1, 17, _le.make_pdu(2 if length else 1, bytes(rng.integers(0, 256, length, dtype=np.uint8))), 0x1A2B3C, s, ci=ci)
        line[at:at + len(sym)] = sym
        hits.append((at, length))
        at += len(sym) + 13
    assert at < len(line)
    words = _le.pack(line)
    infos = [c.decode(words, len(words), 0, o, 0, 2440, 0x1A2B3C)[1] for o, _ in hits]
    got = m.symbols(words.reshape(1, -1), len(words), [ld.Cand(o, 0, 0, 0, 0, n, 17) for o, n in hits], 1)
    assert got == [i["symbols"] for i in infos] and sorted(i["ci"] for i in infos) == [0, 0, 1, 1, 2, 2, 3]
    assert got[:4] == [720, 462, 376 + 8 * 115, 376 + 2 * 291] and got[4:] == [376] * 3


def test_the_lattice_holds_what_it_was_built_to_hold():
    words, cands, notes = m.symbols_lattice()
    got = m.symbols(words, m.SYM_WORDS, cands, 1)
    placed = [cd for cd, n in zip(cands, notes) if n.startswith("residue")]
    assert {cd.offset % 64 for cd in placed} == set(range(64)) and {cd.length for cd in placed} == {0, 1, 27, 255}
    by_note = dict(zip(notes, got))
    assert all(by_note["ci %d sent at S = %d" % (ci, s)] == 376 for ci in (2, 3) for s in (8, 2))
    assert by_note["stream == n_streams"] == 0 and by_note["stream 65535"] == 0
    # a block 1 of zeros decodes to ci 0
    assert by_note["an offset beyond the stream"] == by_note["an offset far beyond the stream"] == 720
    clean = [(cd, g) for cd, n, g in zip(cands, notes, got) if n.startswith("residue")]
    assert all(g == m.coded_duration((8, 2)[k & 1], cd.length) for k, (cd, g) in enumerate(clean))
    # symbol errors in the CI: the model decides; some of them move the duration, the trellis corrects the others
    noisy = [(n, cd, g) for cd, n, g in zip(cands, notes, got) if "errors" in n]
    sent = [m.coded_duration((8, 2)[k & 1], cd.length) for k, (_, cd, _) in enumerate(noisy[:12])]
    assert len(noisy) == 18 and [g for _, _, g in noisy[:12]] == sent
    ends = [m.symbols(w, nw, cs, 1) for w, nw, cs in m.end_cases()]
    assert [e[0] for e in ends] == [720, 462, 720, 720] and len(ends) == 4


@pytest.mark.parametrize("variant", m.SYMBOL_VARIANTS)
def test_the_lattice_tells_the_duration_from_wrong_variants(variant):
    words, cands, _ = m.symbols_lattice()
    assert m.symbols(words, m.SYM_WORDS, cands, 1, m.Rules(**m.VARIANTS[variant])) != m.symbols(words, m.SYM_WORDS, cands, 1)


@pytest.mark.parametrize("variant", m.TRACK_VARIANTS)
def test_the_flag_list_tells_rule_3_from_wrong_variants(variant):
    conns, cands, durations, names = m.flag_list()
    args = (cands, len(conns), lt.LATTICE_MHZ, lt.N_STREAMS, m.UNIT, m.IFS, m.JITTER, lt.REMAP, durations)
    assert m.track(*args, rules=m.Rules(**m.VARIANTS[variant])) != m.track(*args)


def test_the_flag_list_holds_what_it_was_built_to_hold():
    conns, cands, durations, names = m.flag_list()
    tracks, pkts = m.track(cands, len(conns), lt.LATTICE_MHZ, lt.N_STREAMS, m.UNIT, m.IFS, m.JITTER, lt.REMAP, durations)
    by_name = dict(zip(names, tracks))
    events = {n: t.n_events for n, t in by_name.items()}
    assert events["gap of ifs: one event"] == 2 and events["gap of ifs + 1: two events"] == 3
    assert events["duration 0, gap of ifs"] == 2 and events["duration 0, gap of ifs + 1"] == 3
    assert events["17040 symbols reach past the next start"] == 3 and events["17040 symbols, gap of ifs and of ifs + 1"] == 3
    assert events["channel change inside the gap"] == 3 and events["a non-member between two members"] == 2
    assert events["end carries across 2^32"] == 4 and events["end reaches 2^32 exactly"] == 2
    for n, count in (("wave a", 40), ("wave b", 30), ("tile a", 1100), ("tile b", 1000)):
        assert events[n] == count and by_name[n].flags == lt.TIMED | lt.HOPPING
    # the slots on both sides of the seams: the tracking lays the members out by connection, then by time
    slot_of, slot = {}, 0
    for g in range(len(conns)):
        members = sorted((i for i, cd in enumerate(cands) if cd.channel == g and pkts[i] is not None), key=lambda i: pkts[i].rank)
        for i in members:
            slot_of[slot] = i
            slot += 1
    kind = lambda j: "request" if cands[slot_of[j]].length == 0 else "reply"          # noqa: E731
    assert [kind(j) for j in (63, 64, 127, 128, 2047, 2048, 4095, 4096)] == ["reply", "request", "request", "reply", "request", "reply", "reply", "request"]
    assert all(cands[slot_of[j]].channel == cands[slot_of[j + 1]].channel for j in (63, 127, 2047, 4095))
    assert sum(p is None for p in pkts) == 2


def test_the_chain_capture_and_what_the_feature_changes():
    cap, planted = m.chain_capture()
    conns, cands, info, durations, tracks, pkts, sels, sel_pkts = m.chain_model()
    assert len(conns) == 2 and cap.n_words == 1600 and len(cap.mhz) == 8
    assert durations == [info[(cd.stream, cd.offset)].symbols for cd in cands] and set(durations) >= {720, 510}
    one_m, _ = lt.track(cands, len(conns), cap.mhz, len(cap.mhz), m.UNIT, m.IFS, m.JITTER, lt.REMAP)
    for p in planted:
        g = next(k for k, x in enumerate(conns) if (x.access_address, x.crc_init) == (p.aa, p.crc_init))
        assert conns[g].n_packets == 2 * m.CHAIN_EVENTS
        # the tracking as it stands: every reply an event of its own, nothing on the 1.25 ms grid
        assert one_m[g].n_events == 2 * m.CHAIN_EVENTS and one_m[g].flags == 0 and one_m[g].n_fit == 0
        t, s = tracks[g], sels[g]
        assert t.n_events == m.CHAIN_EVENTS >= 12 and t.interval == p.interval == 6 and t.flags & lt.TIMED and t.map_mask == m.CHAIN_MAP
        if p.algorithm == 1:
            assert t.flags & lt.HOPPING and (t.hop_increment, t.first_unmapped) == (p.hop, p.u0) and t.n_on_hop == m.CHAIN_EVENTS
        else:
            assert s.flags == c2.EVALUATED | c2.UNIQUE | c2.PREFERRED and s.counter0 == p.counter0 and s.n_on == m.CHAIN_EVENTS
    assert sorted(p.algorithm for p in planted) == [1, 2]
