"""The test-side model of the LE channel selection #2 stage (tests/_le_csa2.py) on the CPU: the specification's sample data, the
numpy form against the plain one, the hand-built lattice against every deliberately wrong variant of the model, and how often the
rules recover a planted event counter.  No GPU, no library."""
import numpy as np
import pytest

import _le_csa2 as lc
import _le_discover as ld
import _le_track as lt

SAMPLE_AA = 0x8E89BED6                    # Core v5.x Vol 6 Part C 3: channel identifier 0x305F


def test_specification_sample_data():
    assert lc.channel_id(SAMPLE_AA) == 0x305F
    all37 = {0: (56857, 25), 1: (1685, 20), 2: (38301, 6), 3: (27475, 21)}
    for counter, (prn, channel) in all37.items():
        assert lc.csa2_steps(SAMPLE_AA, counter, lc.FULL_MAP) == (prn, prn % 37, None, channel) and prn % 37 == channel
        assert lc.predict(counter, 0x305F, lc.FULL_MAP, lc.REMAP) == (prn, channel, channel)
        assert lc.predict(counter, 0x305F, lc.FULL_MAP, 0) == (prn, channel, channel)
    nine = {6: (10975, 23, None, 23), 7: (5490, 14, 0, 9), 8: (46970, 17, 6, 34)}
    assert lc.NINE_MAP == sum(1 << c for c in (9, 10, 21, 22, 23, 33, 34, 35, 36))
    for counter, (prn, unmapped, index, channel) in nine.items():
        assert lc.csa2_steps(SAMPLE_AA, counter, lc.NINE_MAP) == (prn, unmapped, index, channel)
        assert lc.predict(counter, 0x305F, lc.NINE_MAP, lc.REMAP) == (prn, unmapped, channel)
        assert lc.predict(counter, 0x305F, lc.NINE_MAP, 0) == (prn, unmapped, channel if index is None else 0xFF)
    table = lc.expected_table(SAMPLE_AA, lc.NINE_MAP, lc.REMAP)
    assert [int(table[c]) for c in (6, 7, 8)] == [23, 9, 34]


def test_forward_and_model_agree_on_random_counters():
    rng = np.random.default_rng(2)
    for _ in range(300):
        aa, c, chmap = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 16)), lt.random_map(rng, int(rng.integers(1, 38)))
        prn, unmapped, _, channel = lc.csa2_steps(aa, c, chmap)
        assert lc.predict(c, lc.channel_id(aa), chmap, lc.REMAP) == (prn, unmapped, channel)
        assert int(lc.expected_table(aa, chmap, lc.REMAP)[c]) == channel


@pytest.mark.parametrize("flags", [lc.REMAP, 0])
def test_numpy_form_equals_the_plain_model_on_the_lattice(flags):
    """Without REMAP on the cases where an unknown prediction matters and a few others; with it on all of them."""
    conns, cands, names = lc.lattice_list()
    tracks, pkts, want = lc.lattice_model(flags)
    keep = None if flags else {"map of 9", "map of 2", "two packets per event, map of 9", "events off the prediction", "both algorithms", "wrap inside",
                               "2 events", "not TIMED: interval 5", "no members"}
    calls = []

    def core(aa, events, map_mask, f, n_on_hop, rules):
        calls.append(aa)
        g = [c.access_address for c in conns].index(aa)
        if keep is not None and names[g] not in keep:
            return want[0][g]
        return lc.evaluate(aa, events, map_mask, f, n_on_hop, rules)

    assert lc.select(conns, cands, tracks, pkts, flags, core=core) == want
    assert len(calls) == sum(t.flags & lt.TIMED for t in tracks) >= 20


def test_the_lattice_holds_what_it_names():
    conns, cands, names = lc.lattice_list()
    assert len(set(names)) == len(names) == len(lc.lattice()) and None not in names
    for flags in (0, lc.REMAP):
        tracks, pkts, (sels, sel_pkts) = lc.lattice_model(flags)
        by, tby = dict(zip(names, sels)), dict(zip(names, tracks))
        assert [tby["%d events" % n].n_events for n in (2, 3, 8, 40)] == [2, 3, 8, 40]
        for c0 in (0, 1, 65535):
            assert (by["counter0 %d" % c0].counter0, by["counter0 %d" % c0].n_on, by["counter0 %d" % c0].flags) == (c0, 12, 7)
        assert (by["wrap inside"].counter0, by["wrap inside"].n_on) == (65530, 12)
        assert (by["n_e beyond 2^16"].counter0, by["n_e beyond 2^32"].counter0) == (40000, 123)
        assert [tby["map of %d" % n].n_used <= n for n in (37, 36, 9, 2, 1)] == [True] * 5 and tby["map of 1"].n_used == 1
        assert tby["two packets per event"].n_events == 9 and by["two packets per event"].n_on == 9
        assert not by["not TIMED: interval 5"].flags and not by["not TIMED: one event"].flags and not by["no members"].flags
        assert tby["no members"].n_events == 0 and by["no members"].channel_id
        assert tby["algorithm #1"].flags == lt.TIMED | lt.HOPPING and not by["algorithm #1"].flags & lc.PREFERRED
        assert not by["algorithm #1, map of 5"].flags & lc.PREFERRED
        assert by["40 events"].flags == 7 and tby["40 events"].n_on_hop < by["40 events"].n_on == 40
        assert by["events off the prediction"].n_off >= 2 and by["events off the prediction"].n_on == 17
        g = names.index("n_e beyond 2^32")
        mine = [i for i, c in enumerate(cands) if c.channel == g]
        assert sorted(pkts[i].counter for i in mine) == sorted(n % (1 << 32) for n in lc.BEYOND_32)
        assert sorted(sel_pkts[i].counter for i in mine) == sorted((123 + n) % 65536 for n in lc.BEYOND_32)
        assert all(sel_pkts[i].on_hop for i in mine)
        assert sum(p is None for p in sel_pkts) >= 40 + 2 and sel_pkts.count(None) == pkts.count(None)
    # the forced ties (REMAP): exactly two hypotheses share the best score, in two blocks of 1024 and inside one
    tracks, pkts, (sels, _) = lc.lattice_model(lc.REMAP)
    for name, (aa, c0, n), same_block in (("tie across two blocks", lc.TIE_ACROSS, False), ("tie inside one block", lc.TIE_INSIDE, True)):
        g = names.index(name)
        events = sorted({(p.counter, p.channel, 1) for i, p in enumerate(pkts) if p is not None and cands[i].channel == g})
        scores, _ = lc.scores_np(aa, events, tracks[g].map_mask, lc.REMAP)
        winners = np.flatnonzero(scores == scores.max()).tolist()
        assert len(events) == n and len(winners) == 2 and winners[0] == c0 == sels[g].counter0, (name, winners)
        assert (winners[0] // 1024 == winners[1] // 1024) == same_block
        assert (sels[g].n_on, sels[g].n_second, sels[g].flags) == (n, n, lc.EVALUATED)
    # both algorithms explain seven events each (no REMAP): UNIQUE, and PREFERRED only if the comparison let equality pass
    g = names.index("both algorithms")
    tracks, _, (sels, _) = lc.lattice_model(0)
    assert sels[g].flags == lc.EVALUATED | lc.UNIQUE and sels[g].n_on == tracks[g].n_on_hop == 7


@pytest.mark.parametrize("variant", sorted(lc.VARIANTS))
def test_the_lattice_tells_the_model_from_each_wrong_variant(variant):
    conns, cands, names = lc.lattice_list()
    rules = lc.Rules(**lc.VARIANTS[variant])
    told = []
    for flags in (0, lc.REMAP):
        tracks, pkts, want = lc.lattice_model(flags)
        got = lc.select(conns, cands, tracks, pkts, flags, rules=rules)
        told += [(flags, names[g]) for g in range(len(conns)) if got[0][g] != want[0][g]]
        told += [(flags, "packet %d" % i) for i in range(len(cands)) if got[1][i] != want[1][i]][:3]
    print(variant, told[:8])
    assert told, variant
    expect = dict(no_wrap="wrap inside", tie_largest="tie across two blocks", second_below="tie inside one block",
                  count_packets="two packets per event", preferred_ge="both algorithms", remap_prn_mod="map of 9",
                  remap_unmapped_mod="map of 9")
    if variant in expect:
        assert expect[variant] in [name for _, name in told], told


# ---- how often the rules recover a planted counter ----------------------------------------------------------------------
CELLS = [(12, 37, 0.0), (120, 20, 0.0), (60, 5, 0.0), (60, 2, 0.0), (30, 3, 0.0), (24, 37, 0.3), (40, 9, 0.2)]


@pytest.mark.parametrize("cell", CELLS, ids=lambda c: "%d events, %d channels, loss %.1f" % c)
def test_recovery_sweep(cell):
    """200 draws of a random access address, counter and map per cell, REMAP on the OBSERVED map.  Every draw whose observed map is
    the planted one (with all 37 channels in use: every draw, an event's unmapped channel is then its channel whatever the observed
    map is) must come out with the planted counter, UNIQUE and with every event on the prediction; at least 150 draws of a cell
    count."""
    n_events, n_used, loss = cell
    rng = np.random.default_rng(1000 + n_events + n_used)
    counted = 0
    for _ in range(200):
        aa, c0, chmap = int(rng.integers(0, 1 << 32)), int(rng.integers(0, 1 << 16)), lt.random_map(rng, n_used)
        seen = [n for n in range(n_events) if not (loss and rng.random() < loss)]
        if len(seen) < 2:
            continue
        events = [(n - seen[0], lc.csa2(aa, c0 + n, chmap), 1) for n in seen]
        observed = lc.mask_of(ch for _, ch, _ in events)
        if observed != chmap and n_used != 37:
            continue
        counted += 1
        sel = lc.evaluate_np(aa, events, observed, lc.REMAP, 0)
        assert (sel.counter0, sel.n_on, sel.n_off, sel.flags & lc.UNIQUE) == ((c0 + seen[0]) % 65536, len(events), 0, lc.UNIQUE), (aa, c0, chmap, sel)
    print("%d events, %d channels, loss %.1f: %d draws counted" % (n_events, n_used, loss, counted))
    assert counted >= 150


def test_the_two_algorithms_are_told_apart():
    """A connection planted with algorithm #1 is not PREFERRED; one planted with #2, run through the tracking, has fewer events on
    the #1 hop than #2 gives it."""
    rng = np.random.default_rng(8)
    for k in range(6):
        aa, ci = ld.good_aa(rng), 0x100 + k
        one, _ = lt.synth(rng, 30, lc.FULL_MAP if k % 2 else lc.FIVE_MAP, 8, 5 + 2 * k, 3 * k, aa=aa, crc_init=ci)
        two = lc.plant(aa ^ 0x10000, ci, int(rng.integers(0, 1 << 16)), range(30), lc.FULL_MAP if k % 2 else lc.FIVE_MAP, interval=8)
        conns, cands = ld.group([c._replace(channel=c.stream) for c in one] + two, 2)
        assert [c.access_address for c in conns] == sorted((aa, aa ^ 0x10000))
        tracks, pkts = lc.tracked(conns, cands, lc.REMAP)
        sels, _ = lc.select(conns, cands, tracks, pkts, lc.REMAP, core=lc.evaluate_np)
        for c, t, s in zip(conns, tracks, sels):
            if c.access_address == aa:
                assert t.flags == lt.TIMED | lt.HOPPING and t.n_on_hop == 30 and not s.flags & lc.PREFERRED, (t, s)
            else:
                assert s.flags == 7 and s.n_on == 30 and t.n_on_hop < s.n_on, (t, s)
