"""What the captures of tests/_le_coded_frames.py hold, shown on the CPU from the models and the frames' geometry alone: that they
reach the tile walk, the rings, the decoder's stride, the host wrapper's second pass and the far offsets that
tests/test_gpu_le_coded_frames.py runs the kernels through, and that the simplest wrong variants of the expectation -- a cursor
that stays in its first stream, a ring that drops its 129th entry, an offset or a byte address kept in 32 bits -- give another
list.  No kernel is involved.  The GPU test repeats the geometry assertions with the device's own CU count."""
import numpy as np
import pytest

import _le
import _le_cfind as f
import _le_coded as c
import _le_coded_frames as fr

CUS = (256, 64)                            # the geometry is a function of the CU count: two counts, the larger an MI355X's


# ---- 1. more tiles than workgroups -------------------------------------------------------------------------------------
def test_addresses_and_content_counts():
    assert _le.data_offenses(fr.AA_A) == 0 and _le.data_offenses(fr.AA_B) == 0 and fr.AA_A != fr.AA_B
    for n_words, k in fr._K.items():
        assert k >= 17 and all(k % q for q in range(2, k)), k
        words, planted = fr.walk_contents(n_words)
        assert len(words) == k and len({w.tobytes() for w in words}) == k
        assert len(fr._PLACES[n_words]) >= k                                # every content holds a place


def _model_offsets(n_words, limit=fr.MAX_ERRORS):
    """offsets of the hits of either address in any content"""
    out = set()
    for counts, _, _ in fr.walk_content_models(n_words):
        for aa in (fr.AA_A, fr.AA_B):
            out |= set(np.nonzero(counts[aa] <= limit)[0].tolist())
    return out


def test_the_plants_reach_every_seam_and_the_last_window():
    """Where the existing coded tests put a pattern, some content has a hit: beginning on a seam, one symbol before and behind it,
    and with the window's last symbol on either side of it -- lane seams in both forms, wave and tile seams in the long one --
    and a window that ends on the stream's last symbol, for both addresses."""
    short, long_ = _model_offsets(12), _model_offsets(1030)
    for offs, seams in ((short, (fr.LANE,)), (long_, (fr.LANE, fr.WAVE, fr.TILE))):
        for seam in seams:
            for what, hit in (("on", lambda o: o % seam == 0), ("before", lambda o: o % seam == seam - 1), ("behind", lambda o: o % seam == 1),
                              ("ends against", lambda o: (o + c.PATTERN) % seam == 0), ("ends across", lambda o: (o + c.PATTERN) % seam == 1)):
                if seam == fr.LANE and offs is short and what.startswith("ends"):
                    continue                                                # (the short form's only such windows begin below 0)
                assert any(hit(o) and o > 0 for o in offs), (seam, what)
    assert {2 * fr.TILE - 1, 2 * fr.TILE, 2 * fr.TILE + 1} <= long_         # the ragged third tile's seam
    for n_words in (12, 1030):
        last = 64 * n_words - c.PATTERN
        for aa in (fr.AA_A, fr.AA_B):
            assert any(counts[aa][last] <= fr.MAX_ERRORS for counts, _, _ in fr.walk_content_models(n_words)), (n_words, hex(aa))
        # limits 0 and 16 find different lists, and every data content but the bare ones holds a whole packet that is a candidate
        assert len(_model_offsets(n_words, 0)) < len(_model_offsets(n_words, 16))
        _, planted = fr.walk_contents(n_words)
        for p in planted:
            if p.note != "bare pattern":
                assert p.offset + fr.packet_symbols(p.s, p.length) <= 64 * n_words, p
        cands = [{x.offset for x, _ in cd} for _, _, cd in fr.walk_content_models(n_words)]
        clean = [p for p in planted if p.note != "bare pattern" and len(p.flips) == 0]
        assert len(clean) >= 5 and all(p.offset in cands[p.stream] for p in clean if p.offset < 64 * n_words - 335)


@pytest.mark.parametrize("cus", CUS)
def test_walk_geometry_and_the_cursor_variant(cus):
    # one ragged tile per stream
    w = fr.walk(12, cus)
    g = w.geometry()
    assert w.pitch_words > w.n_words and w.tps == 1 and w.grid == 8 * cus and w.n_streams == 2 * w.grid + 37
    assert g["min_trips"] >= 2 and g["max_trips"] == 3 and g["cursor_steps"] == w.grid and g["prefetch_past_the_end"]
    # three tiles per stream
    w3 = fr.walk(1030, cus)
    g3 = w3.geometry()
    assert w3.pitch_words > w3.n_words and w3.tps == 3 and w3.n_tiles > 2 * w3.grid and w3.grid % 3 != 0
    assert g3["min_trips"] >= 2 and g3["streams_differ"] and g3["tiles_differ"] and g3["prefetch_past_the_end"]
    for cap in (w, w3):
        assert len(set(cap.content_of.tolist())) == cap.K and 0.2 < cap.is_adv.mean() < 0.4
        a, b = cap.skip_and_work()
        assert a >= 50 and b >= 50, (a, b)
        for aa in (fr.AA_A, fr.AA_B):
            for limit in (0, 16):
                want = cap.coded_hits(aa, limit)
                assert len(want) > 100 and fr.first_trip_only(want, cap.tile_of, cap.grid) != want
        cands, pre = cap.cfind()
        assert len(cands) > 100 and not any(cap.is_adv[x.stream] for x, _ in cands)
        flat = [(x.stream, x.offset) for x, _ in cands]
        assert fr.first_trip_only(flat, cap.tile_of, cap.grid) != flat
        pre_so = [(s, o, b) for o, s, b in pre]
        assert fr.first_trip_only(pre_so, cap.tile_of, cap.grid) != pre_so and len(pre) >= len(cands)


# ---- 2. dense rings ----------------------------------------------------------------------------------------------------
def test_the_periodic_stream_matches_at_every_eighth_offset():
    err = c.mismatch_counts(fr.periodic(40, False), fr.DENSE_AA, 2000)
    assert (err[0::8] == 12).all() and err.reshape(-1, 8)[:, 1:].min() >= 90
    assert (c.pattern_symbols(fr.DENSE_AA)[:80] == np.tile(fr.PERIOD, 10)).all()


def test_dense_streams_exercise_the_ring():
    clean, flipped = fr.dense_stream(False), fr.dense_stream(True)
    assert len(fr.dense_hits(False, fr.DENSE_AA, 11)) == 0                  # one below the periodic content's 12: nothing
    for limit in (12, 16, 63):
        offs = [h[1] for h in fr.dense_hits(False, fr.DENSE_AA, limit)]
        per = fr.wave_tile_counts(offs)
        assert per.max() == 1024 > 2 * fr.RING
    # a wave whose 64 lanes read the same symbols: sixteen full ballots, flushes inside stage, a drain behind the tile, a wrap
    per = fr.wave_tile_counts([h[1] for h in fr.dense_hits(False, fr.DENSE_AA, 12)])
    full = int(np.argmax(per == 1024))
    sym = np.unpackbits(clean[0].view(np.uint8), bitorder="little")
    assert fr.lanes_alike(sym, full)
    in_stage, drain, top, left = fr.ring_trace([64] * 16)
    assert in_stage >= 1 and drain >= 1 and top > fr.RING and left == 0
    # the flipped stream: partial ballots, tails on no multiple of 64
    for limit in (12, 16, 63):
        per = fr.wave_tile_counts([h[1] for h in fr.dense_hits(True, fr.DENSE_AA, limit)])
        assert (per % fr.FLUSH != 0).any(), limit
    per16 = fr.wave_tile_counts([h[1] for h in fr.dense_hits(True, fr.DENSE_AA, 16)])
    assert per16.max() > 2 * fr.RING and 650 < per16[:8].min() and per16[:8].max() < 900
    assert not fr.lanes_alike(np.unpackbits(flipped[0].view(np.uint8), bitorder="little"), 0)
    # the ring variant tells itself from the model on every dense list
    for flip in (False, True):
        for limit in (16, 63) if flip else (12, 16, 63):                   # (at limit 12 the flipped stream keeps a wave below 128)
            want = fr.dense_hits(flip, fr.DENSE_AA, limit)
            assert fr.drop_129th(want) != want and len(fr.drop_129th(want)) < len(want)
    # the sparse search in the same stream: the planted patterns and nothing else
    for flip in (False, True):
        got = [(h[1], h[3]) for h in fr.dense_hits(flip, fr.AA_B, 16)]
        assert got == sorted(fr.DENSE_SPARSE)
        assert fr.drop_129th(fr.dense_hits(flip, fr.AA_B, 16)) == fr.dense_hits(flip, fr.AA_B, 16)


def test_caps_fall_inside_a_flush():
    """hit_cap 1 lies strictly inside the flush that gets base 0 whatever the order of the atomics, and count // 2 + 13 lies behind
    some flush's base and before the count: a flush has base < cap <= base + 64."""
    want = fr.dense_hits(True, fr.DENSE_AA, 16)
    per = fr.wave_tile_counts([h[1] for h in want])
    assert (per % fr.FLUSH != 1).all() and per.min() >= 2 and not fr.possible_bases(per, 1)
    assert 64 < len(want) // 2 + 13 < len(want) - 64
    cap = fr.dense_cfind(*fr.DENSE_CFIND)
    cands, pre = fr.dense_cfind_model(*fr.DENSE_CFIND)
    per = fr.wave_tile_counts([p[0] for p in pre])
    assert per.max() > 2 * fr.RING and (per % fr.FLUSH != 0).any() and not fr.possible_bases(per, 1)
    assert len(cands) >= fr.DENSE_CFIND[1] and {x.offset for x, _ in cands} >= {p[0] for p in cap.planted}
    assert len(cands) // 2 + 13 < len(cands)                               # cand_cap below the count


def test_the_decoders_stride_capture():
    """2 * 32 * CUs + 300 words of the flipped content leave more pre-records than one trip of the whole grid takes (8 per workgroup):
    the stride runs in more than half of the workgroups, and the candidates lie on both sides of it.  (Every workgroup would need
    16 * 32 * CUs pre-records, 2400 fewer than the stream has offsets that are 0 mod 8; the 40 packets take more than that.)"""
    cus = 64
    grid = fr.DECODE_WGS_PER_CU * cus
    cap = fr.dense_cfind(fr.stride_words(cus), 40)
    cands, pre = fr.dense_cfind_model(fr.stride_words(cus), 40)
    assert cap.n_words == 2 * grid + 300 and cap.pitch_words > cap.n_words
    assert fr.decode_grid(cus, len(pre) + 64) == grid and len(pre) > fr.DECODE_RECS * grid
    assert 2 * ((len(pre) - fr.DECODE_RECS * grid) // fr.DECODE_RECS) > grid                # more than half of the workgroups take a second trip
    assert {(p[3], p[4]) for p in cap.planted} == {(s, n) for s in (2, 8) for n in (0, 5, 27)}
    assert {x.offset for x, _ in cands} >= {p[0] for p in cap.planted} and all(_le.data_offenses(p[1]) == 0 for p in cap.planted)
    # the periodic content itself: a pre-record at (nearly) every eighth offset and no candidate of its own
    quiet = fr.dense_cfind(200, 0)
    assert len(f.pre_records(quiet.model, quiet.search_bits, fr.MAX_ERRORS)) > 0.95 * quiet.search_bits / 8
    assert f.candidates(quiet.model, quiet.search_bits, 255, fr.MAX_ERRORS) == []


def test_the_host_wrappers_first_guess_is_short():
    w = fr.second_pass_stream()
    offs, errs = fr.second_pass_hits()
    search_bits = 64 * len(w) - (c.PATTERN - 1)
    assert len(w) == fr.SECOND_PASS_WORDS and len(offs) > search_bits // 1024 * 1 + 4096
    lengths = fr.second_pass_lengths()
    assert len(lengths) == 40 and min(lengths, key=lambda m: (lengths[m], m)) == fr.SECOND_PASS_MHZ and lengths[fr.SECOND_PASS_MHZ] == 0


# ---- 3. far offsets ----------------------------------------------------------------------------------------------------
def test_an_all_zero_window_is_168_mismatches_from_any_pattern():
    rng = np.random.default_rng(1)
    for aa in [fr.AA_A, fr.AA_B, fr.DENSE_AA, 0, _le.ADV_AA] + [int(a) for a in rng.integers(0, 1 << 32, 50, dtype=np.uint64)]:
        assert int(c.pattern_symbols(aa).sum()) == 168
    assert (c.mismatch_counts(np.zeros(1000, np.uint8), fr.AA_A, 600) == 168).all()
    quiet = f.StreamModel(np.zeros(64, np.uint64), 64, fr.FAR_MHZ[0], 0)
    assert f.pre_records(quiet, 64 * 64 - 335, 63) == [] and f.candidates(quiet, 64 * 64 - 335, 255, 63) == []


def test_the_far_placement():
    F = fr.far()
    bad = [k for k, v in fr.far_crossings().items() if not v]
    assert not bad, bad
    assert F.pitch_words == F.n_words + 37 and (1 << 29) < F.n_words < (1 << 29) + (1 << 13)
    # the sparse capture is the short references laid at the copies' bases, and nothing else
    for cp in F.copies:
        behind = 0 if cp.ends else fr.PAD_BEHIND
        got = F.read(cp.stream, cp.base - fr.PAD_FRONT, cp.base + fr.R_WORDS + behind)
        assert np.array_equal(got, F.ref(cp.stream, cp.ends)), cp
    assert not F.read(0, F.n_words, F.pitch_words).any() and not F.read(1, 5000, 6000).any()
    assert not np.array_equal(F.R[0], F.R[1])
    kinds = {(p.s, p.length) for p in F.plants if p.s}
    assert {s for s, _ in kinds} == {2, 8} and {n for _, n in kinds} >= {0, 27, 255} and any(p.flips for p in F.plants)


def test_the_models_do_not_see_zero_words_around_a_reference():
    """What the translation rests on: more zero words in front of R_in or behind it move the models' results and change nothing."""
    F = fr.far()
    for s in (0, 1):
        base, more = F.ref(s, False), F.ref(s, False, front=fr.PAD_FRONT + 135, behind=fr.PAD_BEHIND + 410)
        shift = 64 * 135
        for aa in fr.FAR_AAS:
            a, b = fr.ref_coded_hits(base, aa), fr.ref_coded_hits(more, aa)
            assert len(a) > 5 and [(o + shift, x, e) for o, x, e in a] == b
        hits = sorted(h for aa in fr.FAR_AAS for h in fr.ref_coded_hits(base, aa))
        a = fr.ref_decode(base, s, hits, fr.FAR_MHZ[s])
        b = fr.ref_decode(more, s, [(o + shift, x, e) for o, x, e in hits], fr.FAR_MHZ[s])
        assert [(o + shift, dict(p, offset=o + shift), i) for o, p, i in a] == b
        (ca, pa), (cb, pb) = fr.ref_cfind(base, s, fr.FAR_MHZ[s]), fr.ref_cfind(more, s, fr.FAR_MHZ[s])
        assert len(ca) >= 8 and [(o + shift, x._replace(offset=o + shift), i) for o, x, i in ca] == cb
        assert [(o + shift, bound) for o, bound in pa] == pb


def test_what_the_far_lists_hold():
    F = fr.far()
    for aa in fr.FAR_AAS:
        hits = fr.far_coded_hits(aa)
        assert sum(h[1] >= 1 << 32 for h in hits) >= 8 and sum(h[1] >= 1 << 35 for h in hits) >= 4
        assert fr.offsets_32bit(hits) != sorted(hits)                       # an offset kept in 32 bits
    assert (1, F.search_bits - 1, fr.AA_A, 0) in fr.far_coded_hits(fr.AA_A)  # stream 1's last searchable offset
    above = [h for h in fr.far_coded_hits(fr.DENSE_AA) if h[1] >= 1 << 35]
    assert any(b[0] == a[0] and b[1] - a[1] <= 128 and (a[1] + 1) % 32 for a, b in zip(above, above[1:]))      # a place to end search_bits
    dec = fr.far_decoded()
    assert any(o >= 1 << 35 and p["crc_ok"] for _, o, p, _ in dec) and any(o >= 1 << 35 and p["truncated"] for _, o, p, _ in dec)
    assert {i["s"] for _, _, _, i in dec} >= {2, 8}
    cands, pre = fr.far_cfind()
    assert sum(x.offset >= 1 << 32 for x, _ in cands) >= 8 and sum(x.offset >= 1 << 35 for x, _ in cands) >= 4
    assert fr.offsets_32bit([tuple(x) for x, _ in cands], 0) != sorted(tuple(x) for x, _ in cands)
    # C0's last packet is cut by the stream's end: no candidate there, though copy A (the stream goes on) has it; C1's last packet
    # ends on the last symbol and is one
    cut = next(p for p in F.plants if p.note == "the stream ends inside its block 2")
    a, c0, c1 = F.copies[0], F.copies[2], F.copies[3]
    where = {(x.stream, x.offset) for x, _ in cands}
    assert (0, 64 * a.base + cut.offset) in where and (0, 64 * c0.base + cut.offset) not in where
    last = next(p for p in F.plants if p.note == "ends on the stream's last symbol")
    assert (1, 64 * c1.base + last.offset) in where and 64 * c1.base + last.offset + fr.packet_symbols(last.s, last.length) == 64 * F.n_words
    assert any(p["truncated"] and (s, o) == (0, 64 * c0.base + cut.offset) for s, o, p, _ in dec)
    assert any(not p["truncated"] and (s, o) == (1, 64 * c1.base + last.offset) for s, o, p, _ in dec)
    durations = fr.far_durations([x for x, _ in cands])
    assert durations == [i.symbols for _, i in cands] and len(set(durations)) >= 6


def test_a_byte_address_kept_in_32_bits_reads_other_words():
    """Every copy but A lies beyond byte 2^32 of the buffer -- stream 1 as a whole.  Read with the byte address cut to 32 bits, each of
    them shows other words, and the models find another list there."""
    F = fr.far()
    assert 8 * F.pitch_words > 1 << 32
    for cp in F.copies:
        behind = 0 if cp.ends else fr.PAD_BEHIND
        w0, w1 = cp.base - fr.PAD_FRONT, cp.base + fr.R_WORDS + behind
        true, cut = F.read(cp.stream, w0, w1), F.read(cp.stream, w0, w1, byte_bits=32)
        if cp.name == "A":
            assert np.array_equal(true, cut)
            continue
        assert 8 * (cp.stream * F.pitch_words + w1) > 1 << 32 and not np.array_equal(true, cut), cp
        assert fr.ref_coded_hits(cut, fr.AA_A) != fr.ref_coded_hits(true, fr.AA_A), cp
        assert fr.ref_cfind(cut, cp.stream, fr.FAR_MHZ[cp.stream])[0] != fr.ref_cfind(true, cp.stream, fr.FAR_MHZ[cp.stream])[0], cp
