"""The path model of the LE connection tracking (tests/_le_track_paths.py) and the lists built for it (align_list and
long_event_list of tests/_le_track.py): the constants the model reads out of the sources, the tags every run of RUNS carries --
tests/test_gpu_le_track.py runs the same RUNS on the device --, and the connections the lists were built around, each checked
from the model's own numbering.  No GPU."""
import numpy as np
import pytest

import _le_track as lt
import _le_track_paths as lp


def test_constants_are_the_ones_the_tags_speak_of():
    """A moved constant asks for a second look at the builders' sizes (63 .. 3071 events, 40 trains of 13 300 packets) and at the
    tag names (lane 63, thread 255)."""
    assert (lp.LT_TILE, lp.LT_SCORE_TILE, lp.RADIX_SORT_TILE, lp.LE_THREADS) == (2048, 1024, 4096, 256)
    assert lt.LT_SCORE_ALIGN == lp.LT_SCORE_TILE and lp.PREFIX_ROUND * lp.LT_TILE == 524288


def test_closed_form_of_the_channel_selection():
    rng = np.random.default_rng(5)
    for chmap in (lt.FULL_MAP, lt.FIVE_MAP, lt.random_map(rng, 20), 1 << 9):
        for h, u0 in ((5, 0), (16, 36), (11, 17)):
            assert all(lt.csa1_at(u0, h, n, chmap) == lt.csa1(u0, h, n, chmap) for n in range(80))
    assert (1 << 32) % 37 == 7 and lt.csa1_at(29, 7, (1 << 32) + 5, lt.FULL_MAP) == (29 + 7 * (7 + 5)) % 37


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
    assert carried == set(lp.TAGS), sorted(set(lp.TAGS) - carried)


def _align(variant, flags):
    run = [r for r in lp.RUNS if (r.build, r.arg, r.flags, r.kw) == ("align_list", variant, flags, {})][0]
    conns, cands, names = lp.run_list(run)
    tracks, pkts = lp.run_model(run)
    return conns, cands, names, tracks, pkts, lp.numbering(cands, len(conns), tracks, pkts)


def test_align_list_holds_what_it_was_built_to_hold():
    conns, cands, names, tracks, pkts, nb = _align("A", lt.REMAP)
    by = {n: (g, tracks[g]) for g, n in enumerate(names) if n != "filler"}
    assert 18000 <= len(cands) <= 40000 and sum(c.channel == 0xFFFFFFFF for c in cands) == 5 and sum(p is None for p in pkts) == 7
    for n in (63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 3071, 1):
        assert by["%d events" % n][1].n_events == n
    assert [(int(nb.ev0[by["%d events" % n][0]]) % 64, int(nb.ev1[by["%d events" % n][0]]) % 64) for n in (127, 128, 129)] == [(0, 63), (0, 0), (0, 1)]
    assert sum(t.n_events == 2 for t in tracks) >= 4 and int(nb.ev1[-1]) % lp.LT_SCORE_TILE == 0
    # counters beyond 2^32, and every later connection behind their sum
    g, t = by["beyond 2^32"]
    assert g == 0 and (t.interval, t.hop_increment, t.first_unmapped, t.flags, t.n_off_hop) == (6, 7, 29, lt.TIMED | lt.HOPPING, 0)
    assert sorted(p.counter for c, p in zip(cands, pkts) if c.channel == 0) == [0, 1, 2, 3, 5, 6, 7, 9]
    # three waves: from a multiple of 64, every merge needed
    g, t = by["three waves"]
    assert nb.ev0[g] % 64 == 0 and (t.n_events, t.n_fit, t.interval, t.flags) == (193, 192, 6, lt.TIMED | lt.HOPPING)
    # the pairs at lane 63 and at thread 255
    for name, at in (("lane 63", 63), ("thread 255", 255)):
        g, t = by[name]
        a = nb.anchor[nb.ev0[g]:nb.ev1[g]]
        q = np.round(np.diff(a) / lt.UNIT).astype(int)
        assert nb.ev0[g] % 256 == 0 and t.interval == 6 and t.n_fit == len(q) and t.n_events > at + 1
        assert q[at] == 18 and (np.delete(q, at) == 12).all()
    # the planted events off the hop: waves of slots of the connection alone with five, one and none; its first and last wave shared
    g, t = by["off hop"]
    planted = lt.off_hop_plan(int(nb.slot0[g]))
    assert 8 <= len(planted) <= 9 and (t.n_off_hop, t.n_events, t.n_on_hop, t.hop_increment, t.first_unmapped, t.flags) == (
        len(planted), 400, 400 - len(planted), 10, 17, lt.TIMED | lt.HOPPING)
    first, last = int(nb.slot0[g]), int(nb.slot0[g]) + 799
    assert first % 64 and (last + 1) % 64
    per_wave = np.bincount(np.flatnonzero(nb.s_off & (nb.s_conn == g)) // 64 - first // 64, minlength=last // 64 - first // 64 + 1)
    assert per_wave.tolist() == [1, 5, 1] + [0] * (len(per_wave) - 4) + [len(planted) - 7], per_wave
    # the second variant: one event more
    _, _, names_b, tracks_b, _, nb_b = _align("B", lt.REMAP)
    assert names_b[:-1] == names and tracks_b[:-1] == tracks and names_b[-1] == "one more" and int(nb_b.ev1[-1]) % lp.LT_SCORE_TILE == 1


def test_cut_run_ends_mid_wave_inside_the_off_hop_connection():
    run = [r for r in lp.RUNS if r.kw.get("count") == "cut"][0]
    conns, cands, names = lp.run_list(run)
    count = lp.run_kw(run)["count"]
    tracks, pkts = lp.run_model(run)
    g = names.index("off hop")
    assert cands[count - 1].channel == g == cands[count].channel and sum(p is not None for p in pkts) % 64
    assert 0 < tracks[g].n_events < 400 and tracks[g].n_off_hop and all(t.n_events == 0 for t in tracks[g + 1:])


def test_long_event_list_holds_what_it_was_built_to_hold():
    conns, cands, names, fields = lt.long_event_list()
    run = [r for r in lp.RUNS if r.build == "long_event_list"][0]
    tracks, pkts = lp.run_model(run)
    assert names == ["trains", "behind a", "behind b", "behind c"] and conns[0].n_packets == 532000 > lp.PREFIX_ROUND * lp.LT_TILE
    assert (tracks[0].n_events, tracks[0].interval, tracks[0].hop_increment, tracks[0].first_unmapped, tracks[0].flags) == (
        40, 3200, 6, 5, lt.TIMED | lt.HOPPING)
    assert [t.n_events for t in tracks[1:]] == [30, 5, 5]
    assert fields.shape == (len(cands), 7) and [tuple(r) for r in fields[[0, 7, len(cands) // 2, -1]].tolist()] == [
        tuple(cands[i]) for i in (0, 7, len(cands) // 2, -1)]


def test_tags_tell_a_list_that_hides_a_mistake():
    """The sensitivity conditions: the seam list of tests/test_gpu_le_track.py drives the wave-uniform tally and the merge over
    many waves only with values that cannot tell right from wrong, and carries neither tag."""
    conns, cands = lt.seam_list()
    tracks, pkts = lt.track(cands, len(conns), lt.LATTICE_MHZ, lt.N_STREAMS, lt.UNIT, lt.IFS, lt.JITTER, lt.REMAP)
    got = lp.tags(cands, len(conns), tracks, pkts, lt.REMAP)
    print(sorted(got))
    assert not got & {"off_hop_wave_uniform", "gcd_needs_every_wave", "gcd_pair_at_lane_63", "gcd_pair_at_thread_255",
                      "sum_beyond_32_bits_crosses_tile", "prefix_second_round", "conn_index_three_passes", "score_one_remap"}
