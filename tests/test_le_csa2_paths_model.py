"""The path model of the LE channel selection #2 stage (tests/_le_csa2_paths.py) and the lists built for it (pair_list and
wide_list of tests/_le_csa2.py): the constants the model reads out of the sources, the tags every run of RUNS carries --
tests/test_gpu_le_csa2.py runs the same RUNS on the device --, the connections the lists were built around, each checked from the
model's own numbering, and the tags the older lists do NOT carry.  No GPU."""
import numpy as np
import pytest

import _le_csa2 as lc
import _le_csa2_paths as lp
import _le_track as lt


def test_constants_are_the_ones_the_lists_speak_of():
    """A moved constant asks for a second look at the builders of tests/_le_csa2.py (at(): 1024 hypotheses per block, 4 per lane;
    511 .. 1 025 events; gaps to 3071 .. 3073) and at the tag names (thread 255, lane 63)."""
    assert (lp.LC_BLOCKS, lp.LC_PER_LANE, lp.LC_TILE, lp.LC_SPAN, lp.LC_BASE_ROUND, lp.LE_THREADS) == (64, 4, 512, 3072, 2048, 256)
    assert lp.PER_BLOCK == 1024 and lp.LC_BLOCKS * lp.PER_BLOCK == 65536 and lp.N_WAVES == 4
    p = lp.place(lc.at(58, 152, 0))
    assert (p.c0, p.block, p.j, p.thread, p.wave, p.lane, p.r) == (60000, 58, 608, 152, 2, 24, 0)      # (the winner of seam_list's "large")
    assert lp.place(65535)[1:] == (63, 1023, 255, 3, 63, 3) and lp.place(64512)[1:] == (63, 0, 0, 0, 0, 0)
    assert lp.window_byte(lc.at(7, 255, 3), 39) == 1062


def test_tiles_of_the_1025_event_connection():
    """range(511) + [3072] + [3073 ..]: d_last on the cut in the first tile, a third tile of one event and span 0."""
    t = lp.tiles(list(range(511)) + [3072] + [3073 + i for i in range(513)])
    assert [(x.t0, x.m, x.n_first, x.d_last, x.span, x.pad, int(x.near.sum())) for x in t] == [
        (0, 512, 0, 3072, 3072, 0, 512), (512, 512, 3073, 511, 511, 0, 512), (1024, 1, 3585, 0, 0, 3, 1)]
    t = lp.tiles([65000, 65001, 400, 500, 64999])                           # d_last wraps to 65535: the cut; the events beyond it are far
    assert (t[0].d_last, t[0].span, t[0].near.tolist(), t[0].d.tolist()) == (65535, 3072, [True, True, True, True, False], [0, 1, 936, 1036, 65535])


@pytest.mark.parametrize("run", lp.RUNS, ids=[r.name for r in lp.RUNS])
def test_run_carries_the_tags_it_was_built_for(run):
    got = lp.run_tags(run)
    print(run.name, sorted(got))
    assert set(run.tags) <= got, sorted(set(run.tags) - got)


def test_the_lists_cover_every_tag():
    carried = set()
    for run in lp.RUNS:
        assert set(run.tags) <= set(lp.TAGS)
        carried |= set(run.tags) & lp.run_tags(run)
    for tag, names in lp.BETWEEN_RUNS.items():                              # facts of single connections, from the runs named
        between = set().union(*(lp.run_facts(r) for r in lp.RUNS if r.name in names))
        assert tag not in carried and lp.TAGS[tag][1] <= between, sorted(lp.TAGS[tag][1] - between)
        carried.add(tag)
    assert carried == set(lp.TAGS), sorted(set(lp.TAGS) - carried)


@pytest.mark.parametrize("flags", [0, lc.REMAP])
def test_pairs_score_what_was_planted(flags):
    """Every pair: A and B with the planted scores, every third hypothesis at least 2 below B; through the tracking and the
    selection's model the record says the same, and A and B lie where the pair's name says."""
    conns, cands, names = lc.pair_list()
    tracks, pkts, (sels, _) = lc.list_model("pair_list", None, flags)
    plan = lc.pair_plan()
    assert len(conns) == len(plan) == len(lc.PAIRS) >= 33 and len({c.access_address for c in conns}) == 1      # (more work items than the grid has workgroups)
    assert sum(c.channel == 0xFFFFFFFF for c in cands) == 20
    events = lp.conn_events(conns, cands, tracks, pkts)
    for g, name in enumerate(names):
        a, b, tie, seed, planted = plan[name]
        n_a = lc.PAIR_EVENTS // 2 if tie else lc.PAIR_EVENTS // 2 + 2
        assert tracks[g].flags & lt.TIMED and events[g] == list(planted) and len(planted) == lc.PAIR_EVENTS, name
        assert any(n1 - n0 == 1 for (n0, _), (n1, _) in zip(planted, planted[1:]))
        v = lp.view(name, lc.PAIR_AA, events[g], tracks[g].map_mask, flags)
        third = v.scores.copy()
        third[[a, b]] = 0
        assert (v.scores[a], v.scores[b]) == (n_a, lc.PAIR_EVENTS - n_a) and third.max() <= lc.PAIR_EVENTS - n_a - 2, (name, seed)
        s = sels[g]
        assert (s.counter0, s.n_on, s.n_second, s.flags & 3) == (min(a, b) if tie else a, n_a, lc.PAIR_EVENTS - n_a, 1 if tie else 3), (name, s)
        assert v.winner == s.counter0 and v.runners.tolist() == [max(a, b) if tie else b]


def test_plain_model_equals_the_numpy_form_on_two_pairs():
    conns, cands, names = lc.pair_list()
    tracks, pkts, (sels, _) = lc.list_model("pair_list", None, lc.REMAP)
    events = lp.conn_events(conns, cands, tracks, pkts)
    for name in ("same lane, runner-up at the smaller r", "tie in blocks 0 and 63"):
        g = names.index(name)
        assert lc.evaluate(lc.PAIR_AA, [(n, ch, 1) for n, ch in events[g]], tracks[g].map_mask, lc.REMAP, tracks[g].n_on_hop) == sels[g]


@pytest.mark.parametrize("group", ["windows", "counts"])
def test_wide_connections_come_through_the_tracking_as_planted(group):
    conns, cands, names = lc.wide_list(group)
    planted = {w.name: w for w in (lc.WINDOWS if group == "windows" else lc.COUNTS)}
    assert sorted(names) == sorted(planted)
    for flags in (0, lc.REMAP):
        tracks, pkts, (sels, _) = lc.list_model("wide_list", group, flags)
        events = lp.conn_events(conns, cands, tracks, pkts)
        for g, name in enumerate(names):
            w = planted[name]
            assert tracks[g].flags & lt.TIMED and tracks[g].interval == 6 and [n for n, _ in events[g]] == list(w.counters), name
            assert (tracks[g].map_mask == w.chmap or len(w.counters) < 500) and any(n1 - n0 == 1 for n0, n1 in zip(w.counters, w.counters[1:]))
            assert sels[g].counter0 == w.counter0 and sels[g].flags == 7, (name, sels[g])
            if w.b is None and (flags or w.chmap == lc.FULL_MAP):
                assert (sels[g].n_on, sels[g].n_off) == (len(w.counters) - len(w.moved), len(w.moved)), (name, sels[g])
    by = dict(zip(names, lc.list_model("wide_list", group, lc.REMAP)[2][0]))
    if group == "counts":
        assert 511 <= min(len(w.counters) for w in lc.COUNTS) and max(len(w.counters) for w in lc.COUNTS) == 1025
        assert (by["1025 events"].n_on, by["1025 events"].n_off, by["1025 events"].counter0) == (1019, 6, 1023)
        s = lc.list_model("wide_list", group, 0)[2][0][names.index("map of 20, last event off")]
        assert (s.n_off, s.flags) == (3, 7) and s.n_on < 400                # (without REMAP: three known and off, some 270 unknown)
    else:
        assert (by["tile spans 2^16"].n_on, by["tile spans 2^16"].counter0) == (600, 65535)


def test_cutting_the_last_connection_leaves_the_others_alone():
    conns, cands, _ = lc.wide_list("windows")
    tracks, pkts, want = lc.list_model("wide_list", "windows", lc.REMAP)
    k = len(conns) - 1
    cut_tracks, cut_pkts = lc.tracked(conns, cands, lc.REMAP, kept=k)
    assert lc.select(conns[:k], cands, cut_tracks, cut_pkts, lc.REMAP) == lc.without_last_connection(conns, cands, want)


def _facts_of(conns, cands, names, flags, tracks=None, pkts=None):
    if tracks is None:
        tracks, pkts = lc.tracked(conns, cands, flags)
    return lp.facts(lp.views(conns, cands, names, tracks, pkts, flags), flags)


def test_tags_tell_the_older_lists_that_hide_a_mistake():
    """The gaps the new lists close: the lattice and the seam list carry none of these.  (An off event behind event 63, a winner at
    j = 1023 of a tile with span >= 1024, a UNIQUE runner-up in the winner's lane, one in another wave of its block.)"""
    gaps = {"off_behind_63", "tail_wide", "tail_cut", "second_same_lane_smaller_r", "second_same_lane_larger_r", "second_other_wave_0_3",
            "second_other_wave_3_0", "second_other_wave_1_2", "second_only_in_tile_two", "far_decides_thread_0", "far_decides_thread_255",
            "cut_near_and_far", "tile_spans_2_16", "n_e_wraps_in_tile", "block_63_j_0", "block_63_j_1023", "count_512", "count_513", "count_1025"}
    conns, cands, names = lc.lattice_list()
    got = set()
    for flags in (0, lc.REMAP):
        tracks, pkts, _ = lc.lattice_model(flags)
        got |= _facts_of(conns, cands, names, flags, tracks, pkts)
    conns, cands, names = lc.seam_list()
    got |= _facts_of(conns, cands, names, lc.REMAP)
    print(sorted(got))
    assert not got & gaps, sorted(got & gaps)
    assert not lp.tags_of(got) & {"off_behind_63", "winner_at_window_tail", "second_same_lane", "second_other_wave", "second_same_wave",
                                  "second_across_lane_63_64", "second_other_block", "far_decides", "span_cut", "tile_counts", "winner_across_wave_seam"}
