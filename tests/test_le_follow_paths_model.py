"""The path model of LE following (tests/_le_follow_paths.py) and the worlds built for it (crowd_world, byte_world and tally_world
of tests/_le_follow.py): the constants the numbering reads out of the sources, the tags every run of RUNS carries --
tests/test_gpu_le_follow.py runs the same worlds on the device --, the tags the older worlds do NOT carry, the planted connections
against the forward selections, and the short cut through which the cuts of crowd_world get their model.  No GPU."""
import pytest

import _le_follow as lf
import _le_follow_paths as lp


def test_constants_are_the_ones_the_worlds_speak_of():
    """A moved constant asks for a second look at the builders of tests/_le_follow.py (crowd_world counts packets up to seams of
    2 048, tally_world lays 330 events out lane by lane in waves of 64) and at the tag names (threads 63, 64 and 255, lane 63)."""
    assert (lp.LE_THREADS, lp.LT_TILE, lp.RADIX_SORT_TILE, lp.WAVE) == (256, 2048, 4096, 64)
    assert lf.CROWD_TILE == lp.LT_TILE and lp.SCAN_THREADS == (63, 64, 255)
    assert lp.place(2048 + 256 + 64)[1:] == (1, 1, 64, 1, 0) and lp.place(4095)[1:] == (1, 7, 255, 3, 63)
    assert {"update_at_thread_%d_behind_one_in_its_round" % t for t in (63, 64, 255)} < set(lp.TAGS) and len(lp.TAGS) == 34


def test_numbering_of_the_tally_world():
    """The layout tally_world's docstring promises, from the model's own records."""
    b, (seeds, follows, fpkts, trace) = lp.world("tally")
    nb = lp.numbering(b, seeds, fpkts, trace)
    assert [c.first for c in b.conns[:6]] == [0, 4, 63, 134, 144, 149] and [c.first for c in b.conns[22:]] == [240, 256, 320, 330]
    assert (nb.n, nb.k) == (372, 26) and (nb.slot[342:] == -1).all() and (nb.econn[342:] == -1).all()
    assert nb.econn[62:65].tolist() == [1, 2, 2] and nb.econn[141:145].tolist() == [3, -1, -1, 4]
    assert nb.state[4:7].tolist() == [lf.ST_BEFORE, lf.ST_BEFORE, lf.ST_COUNTED] and nb.state[126:130].tolist() == [0, 0, lf.ST_BEYOND, lf.ST_BEYOND]
    assert (nb.state[144:149] == -1).all() and (nb.state[256:320] == -1).all() and (nb.econn[256:320] == 23).all()
    assert nb.front[1] == (1 << 33) + 3 and nb.front[3] - nb.front[2] == 70 and nb.lo == [0] * 3 + [2] * 3 + [3] * 19 + [4]
    assert follows[25].n_map_updates == 0 and follows[25].n_control == 1 and follows[25].n_on == 12
    assert [(x.u, x.q, x.g, x.instant, x.sorted_at) for x in nb.updates] == [(0, 64, 2, 10, 0), (1, 66, 2, 67, 1), (2, 150, 5, 5, 2), (3, 321, 24, 4, 3)]
    big = follows[2]
    assert (big.n_on, big.n_beyond, big.map, big.stop, big.n_map_updates) == (65, 6, lf.NINE, 65, 2)


@pytest.mark.parametrize("run", lp.RUNS, ids=[r.name for r in lp.RUNS])
def test_run_carries_the_tags_it_was_built_for(run):
    got = lp.run_tags(run)
    print(run.name, sorted(got))
    assert set(run.tags) <= got, sorted(set(run.tags) - got)


def test_the_worlds_cover_every_tag():
    carried = set()
    for run in lp.RUNS:
        assert set(run.tags) <= set(lp.TAGS)
        carried |= set(run.tags) & lp.run_tags(run)
    assert carried == set(lp.TAGS), sorted(set(lp.TAGS) - carried)


def test_the_older_worlds_carry_none_of_the_five():
    """The gaps the new worlds close: no update behind a tile that holds one, none behind an empty tile, no list beyond one radix
    tile, no order that the connection's second byte or an instant's third decides."""
    got = set()
    for build in (lf.lattice, lf.seam_world, lf.wrap_world):
        b, trace = build(), {}
        seeds, _, fpkts = lf.model(b, trace=trace)
        got |= lp.facts(lp.numbering(b, seeds, fpkts, trace))
    print(sorted(got))
    assert set(lp.OLD_WORLDS_LACK) < set(lp.TAGS) and not got & set(lp.OLD_WORLDS_LACK), sorted(got & set(lp.OLD_WORLDS_LACK))


def test_the_model_predicts_the_planted_channels_of_the_new_worlds():
    b, (seeds, follows, fpkts, _) = lp.world("crowd")
    n_seeded = sum(s is not None for s in seeds)
    assert len(b.conns) == lf.CROWD_CONNS and b.names == ["planted: crowd %d" % k for k in range(lf.CROWD_CONNS)]
    assert 0.78 * len(b.conns) < n_seeded < 0.82 * len(b.conns) and sum(c.channel == 0xFFFFFFFF for c in b.cands) == lf.CROWD_NOISE
    with_updates = [f for f in follows if f is not None and f.n_map_updates]
    assert all(f.n_map_updates == 4 for f in with_updates) and len(with_updates) * 4 > lp.RADIX_SORT_TILE
    assert sum(g >= 256 for g, f in enumerate(follows) if f is not None and f.n_map_updates) > 700
    assert all(f is None or (f.n_off, f.n_before, f.n_beyond) == (0, 0, 0) for f in follows)
    # every packet of a seeded connection is on the prediction
    assert lf.check_planted(b, seeds, follows, fpkts) == sum(c.n_packets for c, s in zip(b.conns, seeds) if s is not None) > 14000
    b, (seeds, follows, fpkts, _) = lp.world("byte")
    assert lf.check_planted(b, seeds, follows, fpkts) == sum(len(i.counters) for i in b.info) == 19
    assert [(f.n_map_updates, f.n_off, f.map) for f in follows] == [(2, 0, lf.M36)] * 2
    b, (seeds, follows, fpkts, _) = lp.world("tally")
    planted = [g for g, name in enumerate(b.names) if name.startswith("planted") and seeds[g] is not None]
    assert len(planted) == 23 and all(follows[g].n_off == 0 for g in planted)
    assert lf.check_planted(b, seeds, follows, fpkts) == sum(follows[g].n_on for g in planted) + 1 == 203   # (one second packet of a counted event)


def test_cut_model_equals_model_cut_on_the_cuts_of_the_crowd():
    """The GPU test's three cuts, through the whole-list models once: the short cut gives the same records."""
    b, full = lp.world("crowd")
    n, k = len(b.cands), len(b.conns)
    for kw in (dict(work=lp.ragged_count(b, full)), dict(work=n - 5), dict(kept=k - 1)):
        _, seeds, follows, fpkts, _ = lf.cut_model(b, full, full[3], **kw)
        assert (seeds, follows, fpkts) == lf.model_cut(b, **kw)[2:], kw
    assert b.conns[-1].first < n - 5 and lp.ragged_count(b, full) % lp.LE_THREADS
