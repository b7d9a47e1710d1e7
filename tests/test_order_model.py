"""CPU checks of tests/_order_model.py: the lattice of the hit ordering drives every branch it claims, the model's geometry
agrees with the facts sort.hip states about itself, and the slot-side tags see what they are meant to see.  No GPU: a case
that stops driving its branch after a constant in sort.hip changed fails here, not silently on the device."""
import numpy as np
import pytest

import _libs
import _order_model as om


@pytest.fixture(scope="module")
def lists():
    return {c.name: c.build() for c in om.LATTICE}


def primary_run(case):
    return "loose" if case.form == "bounds" else case.form


@pytest.mark.parametrize("case", om.LATTICE, ids=lambda c: c.name)
def test_every_case_carries_the_tags_it_exists_for(case, lists):
    hits = lists[case.name]
    cap, count = om.case_numbers(case, hits)
    got = om.run_tags(case, hits, primary_run(case))
    assert case.tags <= om.ORDER_TAGS
    assert case.tags <= got, (case.name, sorted(case.tags - got))
    # the same list again gives the same tags (the builders are seeded)
    assert np.array_equal(case.build(), hits)
    assert len(hits) <= om.MAX_RECORDS
    assert cap <= om.MAX_RECORDS or case.name in om.BIG_CAP_CASES       # (a capacity is a hit buffer and scratch of that size)
    # inside the documented contract, and inside both kinds of bounds the device test gives
    assert int(hits["offset"].max()) < om.OFFSET_LIMIT
    for loose in (False, True):
        ns, bits = om.case_bounds(case, hits, loose)
        assert int(hits["stream"].max()) < ns and int(hits["offset"].max()) < bits and ns * bits < 1 << 64


def test_the_lattice_covers_every_tag(lists):
    seen = set()
    for case in om.LATTICE:
        seen |= case.tags
    assert seen == om.ORDER_TAGS, sorted(om.ORDER_TAGS - seen)
    assert len({c.name for c in om.LATTICE}) == len(om.LATTICE)
    # the sort entry (one number for count, cap and length) runs the cases on both population edges
    sortable = [c for c in om.LATTICE if om.case_numbers(c, lists[c.name])[0] == om.case_numbers(c, lists[c.name])[1] == len(lists[c.name])]
    edge = set()
    for c in sortable:
        edge |= om.run_tags(c, lists[c.name], "sort")
    assert {"shared_at_48", "pairs_at_49", "pairs_at_4096", "bitmap_at_4097", "offset_limit"} <= edge


def test_constants_are_the_ones_the_tags_are_named_after():
    """The tag names say 48 / 49, 4096 / 4097, 2^20 and 2^22: when sort.hip moves one of them the lattice moves with it (the
    builders use the constants), and this test says that the names in ISSUE / DESIGN need another look."""
    assert (om.ORDER_SMALL, om.ORDER_PAIRS, om.ORDER_BIG_BITS, om.K["SCAN_FEW_LOG2"]) == (48, 4096, 20, 22)
    assert (om.K["SCAN_FEW"], om.K["SCAN_MANY"], om.K["NB_MIN_LOG2"], om.WINDOW_SPAN) == (4, 16, 8, 65535)
    assert (om.SLOT_N, om.SLOT_BLOCK, om.SLOT_PER) == (2, 1024, 8)


def test_geometry_against_what_the_code_says_about_itself():
    # "the key space of n_streams x mul keys seldom fills a power of two (79 streams: 62 % of one)"
    mul = 1 << 26
    assert abs(79 * mul / (1 << om.key_bits(79 * mul)) - 0.62) < 0.01
    for nb_log2_fine in (12, 17, 22):
        nb = om.order_fine_buckets(79, mul, nb_log2_fine)
        assert (1 << (nb_log2_fine - 1)) < nb <= 1 << nb_log2_fine and abs(nb / (1 << nb_log2_fine) - 0.62) < 0.01
    # as many buckets as the list can have records, 2^8 .. 2^ORDER_MAX_LOG2; the scans of the counts never need more than 1024 workgroups
    caps = [2, 3, 255, 256, 257, 4096, 4097, (1 << 18) + 1, (1 << 21) - 3, (1 << 21) + 1, 1 << 22, (1 << 22) + 1, (1 << 23) + 5, 1 << 24,
            (1 << 24) + 3, 1 << 31, (1 << 32) - 1]
    for cap in caps:
        l = om.order_nb_log2(cap)
        assert 8 <= l <= om.ORDER_MAX_LOG2 and ((1 << l) >= cap or l == om.ORDER_MAX_LOG2) and (l == 8 or (1 << (l - 1)) < cap)
        for ns, bits in ((1, 1), (1, 5), (79, 1 << 26), (3, 1000003), (65536, 1 << 47), (1 << 20, 1 << 50), (7, (1 << 35) + 12345)):
            g = om.geometry(None, cap, cap, "bounds", ns, bits)
            assert 1 <= g.nb <= 1 << om.ORDER_MAX_LOG2 and om.scan_blocks(g.nb) <= om.K["SCAN_BLOCKS_MAX"]
            assert g.nb_log2 == min(l + 1, om.ORDER_MAX_LOG2)
            # every key has a bucket, and the last bucket in use is the last key's
            if ns * bits < 1 << 64:
                assert (ns * bits - 1) >> g.shift == g.nb - 1 or g.nb == 1 << g.nb_log2
                assert (ns * bits - 1) >> g.shift < g.nb
    assert om.scan_items(1 << 22) == 4 and om.scan_items((1 << 22) + 1) == 16 and om.scan_blocks(1 << 22) == 1024 == om.scan_blocks(1 << 24)
    # the bit count of the key space: exact powers of two, one more, products that do not fit 64 bits
    assert [om.key_bits(t) for t in (0, 1, 2, 3, 4, 5, 1 << 40, (1 << 40) + 1, (1 << 64) - 1, 1 << 64, 1 << 70)] == [0, 0, 1, 2, 2, 3, 40, 41, 64, 64, 64]
    assert om.order_shift(1, 500, 10) == 0 and om.order_shift(65536, 1 << 47, 8) == 55


def test_expected_and_comparison():
    h = om.records([1, 0, 0, 1, 0], np.array([5, 9, 3, 5, 3], np.uint64), 3)
    want = om.expected(h, 5, 5)
    assert list(zip(want["stream"], want["offset"])) == [(0, 3), (0, 3), (0, 9), (1, 5), (1, 5)]
    assert om.has_repeats(h, 5, 5) and om.same_list(want, want, False)
    swapped = want.copy()
    swapped[[0, 1]] = want[[1, 0]]                          # equal keys the other way round: the same list
    assert om.same_list(swapped, want, False) and (not om.same_list(swapped, want, True) or want[0] == want[1])
    wrong = want.copy()
    wrong[[1, 2]] = want[[2, 1]]
    assert not om.same_list(wrong, want, False)
    assert len(om.expected(h, 9, 3)) == 3 and len(om.expected(h, 2, 5)) == 2


# ---- segment slots ---------------------------------------------------------------------------------------------------------------

def test_slot_geometry():
    g = om.slot_geometry(4032 * 12 * 3 + 1, 3, om.LAP_ANY)
    assert (g.seg_offsets, g.tile_words, g.segs_per_tile, g.segs_per_stream, g.n_segs) == (4032, 756, 12, 48, 144)
    g = om.slot_geometry(4096 * 8 * 3, 5, 0x9E8B33)
    assert (g.seg_offsets, g.tile_words, g.segs_per_tile, g.segs_per_stream, g.n_segs, g.n_blocks) == (4096, 512, 8, 24, 120, 1)
    assert om.slot_geometry(4096 * 8193, 1, 0x9E8B33).n_blocks == 2 and om.slot_geometry(4096 * 8192, 1, 0x9E8B33).n_blocks == 1
    assert om.slot_header_offset(1000) == 1024 and om.slot_header_offset(1024) == 1024
    assert om.slot_header(np.array([3, 1, 7, 7, 99], np.uint32)) == (3, 1, 7, 7)


def test_slot_tags_on_small_lists():
    bits, lap = 4032 * 12 * 3, om.LAP_ANY                  # three tiles a stream, 36 segments, 3 streams: 108 segments (ragged)
    keys = sorted([(0, 0), (0, 4031), (0, 4032), (0, 4040), (0, 3 * 4032 + 1), (0, 3 * 4032 + 2), (0, 3 * 4032 + 3)]
                  + [(0, bits - 5)] + [(1, 7)] + [(1, 5 * 4032 + 10 * k) for k in range(9)])
    t = om.slot_tags(keys, bits, 3, lap, 100)
    assert {"seg_0", "seg_1", "seg_2", "seg_3", "seg_many", "seg_first_offset", "seg_last_offset", "stream_seam", "n_segs_ragged",
            "overflow_fits"} <= t
    assert not t & {"two_place_workgroups", "cut_between_slots", "cut_in_overflow", "overflow_full"}
    # cuts: record `cap` is the first one left out
    assert "cut_between_slots" in om.slot_tags(keys, bits, 3, lap, 3)          # (0, 4032) kept, (0, 4040) not
    assert "cut_in_overflow" in om.slot_tags(keys, bits, 3, lap, 4 + 2 + 4 + 3)  # inside the nine hits of one segment of stream 1
    assert "cut_in_overflow" not in om.slot_tags(keys, bits, 3, lap, 6)        # the third hit of a segment is cut off: nothing of the overflow kept
    assert "overflow_full" in om.slot_tags(keys, bits, 3, lap, 7)              # 1 + 7 overflow records
    assert "n_segs_ragged" not in om.slot_tags(keys[:8], bits, 2, lap, 100)
    assert "n_segs_ragged" not in om.slot_tags([(0, 5)], 4096 * 8 * 3, 3, 0x9E8B33, 10)   # known LAP: always whole eights
    far = sorted(keys[:8] + [(0, 4096 * 9000)])
    assert "two_place_workgroups" in om.slot_tags(far, 4096 * 9001, 1, 0x9E8B33, 100)


# ---- the streams of the scan-counted path, order_single_kernel and the compaction ------------------------------------------------

@pytest.fixture(scope="module")
def oracle():
    orc = _libs.oracle()
    orc.orc_reset_syndrome_map()
    orc.orc_init(2)
    yield orc
    orc.orc_reset_syndrome_map()


@pytest.mark.parametrize("lap", om.STREAM_LAPS)
def test_burst_streams_fill_shared_and_crowded_buckets(lap, oracle):
    """The "scan" source of the geometry on the oracle's list of the burst streams: 2048-key buckets with up to 48 mates for a
    capacity of 600, 4096-key buckets with more than 48 for 300 -- and every hit fits both capacities."""
    words, bits, want = om.burst_stream(lap)
    assert len(words) == om.BURST_WORDS and 260 <= len(want) <= 300 and want == sorted(want)
    first = 756 * 10 * 64 if lap == om.LAP_ANY else 512 * 20 * 64           # the burst starts on a tile of its scan kernel
    burst = [o for (_, o, _, _) in want if first <= o < first + 64 * 260]
    assert len(burst) >= 200
    for cap, tag in om.BURST_CASES:
        g = om.geometry(None, len(want), cap, "scan", 1, bits)
        assert 1 << g.shift == (2048 if tag == "shared" else 4096) and g.nb >= 2 * cap - 2
        tags = om.classify(om.as_records(want), len(want), cap, "scan", 1, bits)
        assert {tag, "alone", "count_lt_cap"} <= tags and ("pairs" in tags) == (tag == "pairs")
    if lap == om.LAP_ANY:            # more hits in the 63 words of one wave than a candidate ring of 64 holds
        assert sum(first <= o < first + 4032 for o in burst) > 64
    else:                            # hits in all four 32-offset chains of the lanes of the wave that owns words 0 .. 127 of the tile
        chains = [sum(1 for o in burst if o < first + 128 * 64 and (o - first) % 128 // 32 == c) for c in range(4)]
        assert all(chains) and sum(chains) - chains[3] > 64, chains


@pytest.mark.parametrize("lap", om.STREAM_LAPS)
def test_slot_streams_carry_every_slot_tag(lap, oracle):
    words, n_words, pitch, bits, want, _ = om.slot_stream(lap)
    keys = [(s, o) for (s, o, _, _) in want]
    geo = om.slot_geometry(bits, 3, lap)
    assert geo.n_segs > om.SLOT_BLOCK * om.SLOT_PER and geo.n_blocks == 2 and len(words) == 3 * pitch
    assert 3.9 < 3 * n_words * 8 / 2 ** 20 < 4.3 and 500 <= len(want) <= 2000
    caps = om.slot_caps(want, bits, lap)
    need = set(om.SLOT_NEED) | ({"n_segs_ragged"} if lap == om.LAP_ANY else set())
    assert need <= om.slot_tags(keys, bits, 3, lap, caps["overflow_fits"])
    for tag in ("cut_between_slots", "cut_in_overflow"):
        assert {tag, "overflow_fits"} <= om.slot_tags(keys, bits, 3, lap, caps[tag]) and caps[tag] < len(want)
    assert "overflow_full" in om.slot_tags(keys, bits, 3, lap, caps["overflow_full"])


def test_the_streams_cover_every_slot_tag():
    assert om.SLOT_TAGS == om.SLOT_NEED | {"n_segs_ragged", "cut_between_slots", "cut_in_overflow", "overflow_full"}
