"""CPU checks of the LE lattice (tests/_le_lattice.py): that it holds what it says it holds, that the model's lell fields on
it equal the compiled reference's (oracle/_ref/libbtbb_ref.so; skipped when it is not built), and that it tells a subtly
wrong decoder from the right one: each mutant below is the model (tests/_le.py) with one rule changed, and its records
must differ from the true ones in at least one hit of the lattice."""
import pytest

import _le
import _le_lattice as ll
import _libs

CRC_INITS = (0x555555, 0x000000, 0xFFFFFF, 0x7B31C9, 0xAB123456)        # (the GPU test's launches; the last one has bits above 24)


@pytest.fixture(scope="module")
def lat():
    return ll.decode_lattice()


@pytest.fixture(scope="module")
def want():
    return ll.expected()


def test_builders_are_deterministic():
    ll.decode_lattice.cache_clear()
    a = ll.decode_lattice(tight=True)
    ll.decode_lattice.cache_clear()
    b = ll.decode_lattice(tight=True)
    assert a.words is not b.words and a.words.tobytes() == b.words.tobytes() and a.hits.tobytes() == b.hits.tobytes()
    assert a.tags == b.tags
    ll.scan_lattice.cache_clear()
    c = ll.scan_lattice()
    ll.scan_lattice.cache_clear()
    d = ll.scan_lattice()
    assert all(x.words.tobytes() == y.words.tobytes() and x.planted == y.planted and x.aa == y.aa for x, y in zip(c, d))
    assert len(c) == len(d)


def test_decode_lattice_composition(lat, want):
    tags, hits = lat.tags, lat.hits
    assert len(hits) == len(tags) == len(want) < 15000 and lat.words.size * 64 < 4 << 20
    assert (hits["offset"] + 40 <= 64 * lat.n_words).all()
    assert lat.pitch_words > lat.n_words and (lat.words[:, lat.n_words:] != 0).all()
    tight = ll.decode_lattice(tight=True)
    assert tight.pitch_words == tight.n_words == lat.n_words and tight.hits.tobytes() == hits.tobytes()
    assert (tight.words == lat.words[:, :lat.n_words]).all()
    for s in range(lat.n_streams):                      # a packet at offset 0 of every stream
        assert ((hits["stream"] == s) & (hits["offset"] == 0)).any(), s
    # the model reads the AA and the length each hit was built with, on the channel kind it was built for
    for t, h, r in zip(tags, hits, want):
        assert r["access_address"] == int(h["lap"]) and r["aa_errors"] == int(h["ac_errors"])
        assert r["is_data"] == (t.kind == "data")
        inside = int(h["offset"]) + 56 <= 64 * lat.n_words
        if inside:
            assert r["pdu_bytes"] == 2 + t.L, t
            assert r["length"] == t.L & (0x1F if t.kind == "data" else 0x3F)
        assert r["truncated"] == int((t.dist or 0) > 0)
        assert r["crc_ok"] == int(t.flip is None and not r["truncated"]), t
    # lengths, flips, phases, ends
    for kind in ("data", "adv"):
        got = sorted(t.L for t in tags if t.axis == "lengths" and t.kind == kind)
        assert got == list(range(256))
        assert {t.flip for t in tags if t.axis == "lengths" and t.kind == kind} == set(ll.FLIPS) | {None}
    for size, ok in (("short", lambda L: L + 5 <= 8), ("long", lambda L: L >= 100)):
        ph = sorted(int(h["offset"]) % 64 for t, h in zip(tags, hits) if t.axis == "phase" and t.detail[1] == size and ok(t.L))
        assert ph == list(range(64)), size
    for L in ll.END_LENGTHS:
        for kind in ("data", "adv"):
            have = {int(h["offset"]) + 40 + 8 * (L + 5) - 64 * lat.n_words for t, h in zip(tags, hits)
                    if t.axis == "end" and t.kind == kind and t.L == L}
            assert have == set(ll.end_distances(L)), (L, kind)
            assert {0, 1, 7, 8, 9, 23, 24, 25} <= have
            assert {8 * (L + 5) - 16, 8 * (L + 5) - 8, 8 * (L + 5)} <= have       # 16, 8 and 0 header bits inside
    # MHz, seeds, streams, ac_errors
    assert sorted(set(int(m) for m in lat.mhz[:84])) == list(range(2400, 2484))
    for s in range(84):
        ok = [r for t, h, r in zip(tags, hits, want) if int(h["stream"]) == s and t.flip is None and not r["truncated"]]
        assert ok and all(r["crc_ok"] for r in ok)
        assert all(r["channel_idx"] == _le.channel_index(int(lat.mhz[s])) for r in ok)
    assert {int(r["channel_idx"]) for r in want} >= {0xFE, 0xFF} | set(range(40))
    assert int(hits["stream"].min()) == 0 and int(hits["stream"].max()) == lat.n_streams - 1
    assert set(hits["ac_errors"].tolist()) == {0, 1, 2, 3, 4}
    # access addresses
    data_aas = {int(h["lap"]) for t, h in zip(tags, hits) if t.axis == "aa"}
    assert {_le.ADV_AA} | {_le.ADV_AA ^ (1 << i) for i in range(32)} <= data_aas
    assert {b * 0x01010101 for b in range(256)} <= data_aas
    assert set(ll.run_aas()) | set(ll.TRANSITION_AAS) <= data_aas
    assert set(range(4096)) | {v << 20 for v in range(4096)} <= data_aas
    assert len([t for t in tags if t.axis == "aa" and t.detail == "random"]) == 1000
    omitted = {}
    for t, h in zip(tags, hits):
        if t.axis == "aa" and isinstance(t.detail, tuple):
            _, v, shift, flip = t.detail
            aa = int(h["lap"])
            assert (aa >> shift) & 0xFFF == (v if flip is None else v ^ (1 << flip))
            assert (aa ^ 0x55555555) & ~(0xFFF << shift) & 0xFFFFFFFF == 0
            omitted.setdefault((v, shift), set()).add(flip)
    assert set(omitted) == {(v, shift) for v in _le.OMITTED_WINDOWS for shift in range(0, 21, 4)} and len(omitted) == 38 * 6
    assert all(flips == {None} | set(range(12)) for flips in omitted.values())
    counts = {r["access_address_offenses"] for t, r in zip(tags, want) if t.kind == "data"}
    assert {0, 1, 2, 3, 4} <= counts
    adv = [(int(h["lap"]), r) for t, h, r in zip(tags, hits, want) if t.axis == "aa_adv"]
    assert {_le.ADV_AA} | {_le.ADV_AA ^ (1 << i) for i in range(32)} <= {a for a, _ in adv} and len(adv) == 233
    assert {(r["access_address_ok"], r["access_address_offenses"]) for _, r in adv} == {(1, 0), (0, 1), (0, 32)}


def test_further_crc_inits_run_on_a_thinned_lattice():
    for crc_init in CRC_INITS[1:]:
        sub = ll.decode_lattice(crc_init=crc_init, full=False)
        assert 200 <= len(sub.hits) <= 1000
        recs = ll.expected(crc_init=crc_init, full=False)
        assert all(r["crc_ok"] == int(t.flip is None and not r["truncated"]) for t, r in zip(sub.tags, recs))
        assert sum(r["crc_ok"] for r in recs) > 150


def test_scan_lattice_composition():
    cases = ll.scan_lattice()
    aas = [c.aa for c in cases]
    assert {(a & 1, a >> 24) for a in aas} >= {(b, top) for b in (0, 1) for top in ll.TOP_OCTETS}
    assert {_le.ADV_AA ^ 1, _le.ADV_AA ^ (1 << 8), _le.ADV_AA ^ (1 << 31), ll.CONN_AA} <= set(aas) and _le.ADV_AA not in aas
    assert {int(_le.bits_value(_le.preamble_bits(a))) for a in aas} == {0x55, 0xAA}         # both preamble values
    assert sum(c.dense_stream is not None for c in cases) == ll.DENSE_AAS
    assert any(int(m) == 2402 for c in cases for m in c.mhz) and all(int(c.mhz[0]) not in _le.ADV_MHZ for c in cases)
    for c in cases:
        assert c.n_words == 2 * 512 + 3 and c.words.shape[1] == c.n_words
        by_e = {}
        for p in c.planted:                             # what was planted is what the stream holds
            e, zones = ll.window_errors(c.words[p.stream], p.offset, c.aa)
            assert (e, zones) == (p.errors, tuple(sorted(p.zones))), p
            if p.offset < c.search_bits:
                by_e.setdefault(e, []).append(zones)
        for limit in range(5):
            for e in (limit, limit + 1):
                assert len(by_e[e]) >= 6, (hex(c.aa), e)
                if e:
                    assert {z for zones in by_e[e] for z in zones} == {0, 1, 2}, (hex(c.aa), e)
        assert len(by_e[6]) >= 3
        whats = {p.what for p in c.planted}
        assert whats == {"lane", "wave", "tile", "last offset", "behind the last offset", "planted"}
        seam = {"lane": 128, "wave": 8192, "tile": 32768}
        for p in c.planted:                             # a seam pattern's 40 bits lie across (or start at) its seam
            if p.what in seam:
                assert (p.offset + 39) // seam[p.what] > (p.offset - 1) // seam[p.what], p
        assert any(p.what == "last offset" and p.offset == c.search_bits - 1 for p in c.planted)
        assert any(p.what == "behind the last offset" and p.offset == c.search_bits for p in c.planted)
        if bin(c.aa ^ _le.ADV_AA).count("1") == 1:
            assert len(c.adv_packets) >= 4
            for s, o in c.adv_packets:
                assert ll.window_errors(c.words[s], o, _le.ADV_AA)[0] == 0
        else:
            assert not c.adv_packets
        if c.dense_stream is not None:
            off, err, _ = _le.match_all(c.words[c.dense_stream], c.n_words, c.search_bits, c.aa, 0)
            assert set(range(0, c.search_bits, 40)) <= set(off.tolist())
            per_wave_and_tile = [int(((off >= 8192 * k) & (off < 8192 * (k + 1))).sum()) for k in range(8)]
            assert min(per_wave_and_tile) > 128          # more than the per-wave ring holds


@pytest.fixture(scope="module")
def ref():
    r = _libs.ref()
    if r is None:
        pytest.skip("oracle/_ref/libbtbb_ref.so not built")
    return r


def test_lattice_records_against_the_compiled_reference(ref, lat, want):
    for tight, crc_init, full in [(False, ll.MAIN_CRC_INIT, True)] + [(False, c, False) for c in CRC_INITS[1:]]:
        la = ll.decode_lattice(tight, crc_init, full)
        for h, r in zip(la.hits, ll.expected(tight, crc_init, full)):
            rf = _le.ref_lell_fields(ref, r["bytes"], int(la.mhz[int(h["stream"])]))
            assert {k: r[k] for k in rf} == rf, (h, r)


# ---- sensitivity -------------------------------------------------------------------------------------------------------
def _caught(la, true, rules, axes=None, crc_init=None):
    """The hits of lattice `la` on which the model under `rules` differs from the true records."""
    out = []
    for i, t in enumerate(la.tags):
        if axes is None or t.axis in axes:
            if ll.model_record(la, i, rules, crc_init) != true[i]:
                out.append(i)
    return out


def _lell_caught(la, true, rules):
    """The same for rules that change only the lell fields (they depend on the record's bytes and the MHz alone)."""
    out = []
    for i, (h, r) in enumerate(zip(la.hits, true)):
        f = _le.lell_fields(r["bytes"], int(la.mhz[int(h["stream"])]), rules)
        if any(r[k] != v for k, v in f.items()):
            out.append(i)
    return out


GROUPS = _le.omitted_windows()


@pytest.mark.parametrize("group", range(5))
def test_mutant_run_window_exception_dropped(lat, want, group):
    bad = _lell_caught(lat, want, _le.Rules(run_windows=_le.RUN_WINDOWS | GROUPS[group]))
    assert bad
    assert all(lat.tags[i].kind == "data" for i in bad)


def test_mutant_single_omitted_window_counted(lat, want):
    data = [i for i, t in enumerate(lat.tags) if t.kind == "data"]
    aas = [int(lat.hits["lap"][i]) for i in data]
    true = [want[i]["access_address_offenses"] for i in data]
    for v in sorted(_le.OMITTED_WINDOWS):
        rules = _le.Rules(run_windows=_le.RUN_WINDOWS | {v})
        differ = sum(_le.data_offenses(a, rules) != n for a, n in zip(aas, true))
        assert differ >= 6, hex(v)                        # (at least its six positions)


def test_mutant_length_masks(lat, want):
    bad = _lell_caught(lat, want, _le.Rules(data_mask=0x3F))
    assert len(bad) > 100 and all(lat.tags[i].kind == "data" and want[i]["bytes"][5] & 0x20 for i in bad)
    bad = _lell_caught(lat, want, _le.Rules(adv_mask=0x1F))
    assert len(bad) > 100 and all(lat.tags[i].kind == "adv" and want[i]["bytes"][5] & 0x20 for i in bad)


def test_mutant_transitions_over_32_positions(lat, want):
    assert _lell_caught(lat, want, _le.Rules(transition_positions=32))


def test_mutant_truncated_at_the_bit(lat, want):
    bad = _caught(lat, want, _le.Rules(truncated_ge=True), axes=("end",))
    assert bad and all(lat.tags[i].dist == 0 for i in bad)
    assert len(bad) == 2 * len(ll.END_LENGTHS)


@pytest.mark.parametrize("tight", [False, True])
def test_mutant_reads_behind_the_end(tight):
    la, true = ll.decode_lattice(tight=tight), ll.expected(tight=tight)
    bad = _caught(la, true, _le.Rules(read_past_end=True), axes=("end",))
    assert len(bad) >= 20
    assert all(la.tags[i].dist > 0 for i in bad)
    assert {la.tags[i].kind for i in bad} == {"data", "adv"}


def test_mutant_second_word_one_phase_late(lat, want):
    bad = _caught(lat, want, _le.Rules(second_word_above=57), axes=("phase",))
    assert bad and all(int(lat.hits["offset"][i]) % 8 == 1 for i in bad)
    assert {lat.tags[i].detail[1] for i in bad} == {"short", "long"}


def test_mutant_crc_init_not_masked():
    crc_init = CRC_INITS[-1]
    assert crc_init >> 24
    la, true = ll.decode_lattice(crc_init=crc_init, full=False), ll.expected(crc_init=crc_init, full=False)
    bad = _caught(la, true, _le.Rules(crc_init_mask=False))
    assert len(bad) > len(la.hits) // 2
    # (with a CRCInit of 24 bits the mutant is the model: only this launch can tell)
    sub = ll.decode_lattice(crc_init=CRC_INITS[1], full=False)
    assert not _caught(sub, ll.expected(crc_init=CRC_INITS[1], full=False), _le.Rules(crc_init_mask=False), axes=("end", "head"))


def test_mutant_channel_index_without_the_unsigned_char(lat, want):
    bad = _caught(lat, want, _le.Rules(uchar_wrap=False), axes=("head",))
    assert sorted(int(lat.mhz[int(lat.hits["stream"][i])]) for i in bad) == [2400, 2401]


def test_mutant_whitening_seed_not_masked(lat, want):
    bad = _caught(lat, want, _le.Rules(seed_mask=False), axes=("head",))
    assert sorted(int(lat.mhz[int(lat.hits["stream"][i])]) for i in bad) == [2400, 2401]
    assert all(want[i]["crc_ok"] for i in bad)
