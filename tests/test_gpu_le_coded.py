"""The LE Coded PHY kernels (libbtbb_amd/csrc/le_coded.h) against the model (tests/_le_coded.py): every byte of the hit list,
of both record arrays and the counts.  Output buffers start as 0xA5 and are longer than their caps, so a byte a kernel leaves
unwritten, or writes where it should not, shows.  The scan's streams are 1100 words (two tiles of 512 and a ragged one); the
decoder's inputs are _le_coded.decode_cases(), which tests/test_le_coded_model.py shows to tell every wrong variant apart."""
import numpy as np
import pytest

import _le
import _le_coded as m
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu

REC, INFO, HIT = bt.LE_PKT_DTYPE.itemsize, bt.LE_CODED_INFO_DTYPE.itemsize, bt.HIT_DTYPE.itemsize
OTHER_AA = 0x5A3C96E1
N_WORDS, N_STREAMS = 1100, 3
LIMITS = (0, 1, 16, 63)


@pytest.fixture(scope="module", autouse=True)
def _init():
    torch = pytest.importorskip("torch")
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    bt.init(2)


# ---- the scan ----------------------------------------------------------------------------------------------------------
def _plants(aa, rng):
    """(fixed offset or None, residue mod 64 or None, symbols) of every planted pattern of one access address."""
    pat = m.pattern_symbols(aa)
    out = []
    # every offset residue mod 64, clean
    for r in range(64):
        out.append((None, r, pat))
    # exactly E - 1, E, E + 1 mismatches, confined in turn to the preamble, each quarter of the AA, the pairs the pre-filter reads
    # (one symbol of k distinct pairs: the filter's count equals the mismatches) and, two at a time, both symbols of a pair (the
    # filter sees nothing of them); the sixteen symbols the filter does not read carry what they can
    regions = [np.arange(0, 80)] + [np.arange(80 + 64 * q, 144 + 64 * q) for q in range(4)]
    pair_firsts = np.array([k for k in range(320) if k % 4 < 2])
    for e in sorted({max(E + d, 0) for E in LIMITS for d in (-1, 0, 1)}):
        for reg in regions:
            out.append((None, None, m.flip(pat, rng.choice(reg, e, replace=False))))
        firsts = rng.choice(pair_firsts, e, replace=False)
        out.append((None, None, m.flip(pat, firsts + 2 * rng.integers(0, 2, e))))
        both = rng.choice(pair_firsts, e // 2, replace=False)
        out.append((None, None, m.flip(pat, np.concatenate([both, both + 2, [333] * (e % 2)]).astype(np.int64))))
        if e <= 16:
            out.append((None, None, m.flip(pat, rng.choice(np.arange(320, 336), e, replace=False))))
    return out


def _capture(seed=31):
    """Three streams of noise with the plants of two access addresses: across lane (128 symbols), wave (8192) and tile (32768)
    seams, back to back, and one whose window ends on the stream's last symbol."""
    rng = np.random.default_rng(seed)
    total = 64 * N_WORDS
    lines = rng.integers(0, 2, (N_STREAMS, total), dtype=np.uint8)
    used = np.zeros((N_STREAMS, total), bool)

    def put(s, o, sym):
        assert o + len(sym) <= total and not used[s, o:o + len(sym)].any(), (s, o)
        lines[s, o:o + len(sym)] = sym
        used[s, o:o + len(sym)] = True

    for i, aa in enumerate((_le.ADV_AA, OTHER_AA)):
        pat = m.pattern_symbols(aa)
        s = i                                           # fixed places: streams 0 and 1
        for o in (128 * 9 - 100, 128 * 14, 8192 - 200, 8192 * 2, 8192 * 3 - 1, 32768 - 170, 65536 - 336, 65536 + 64, total - 336):
            put(s, o, pat)
        for o in (32768, 8192 * 5 - 335) if i == 0 else (65536, 8192 * 6 - 1):     # stream 2: on and against the seams
            put(2, o, pat)
        put(s, 40000, pat)                              # back to back
        put(s, 40336, pat)
        put(s, 40672, m.flip(pat, [5, 100, 300]))
    for i, aa in enumerate((_le.ADV_AA, OTHER_AA)):
        cursor = [0] * N_STREAMS
        for k, (_, residue, sym) in enumerate(_plants(aa, rng)):
            s = (k + i) % N_STREAMS
            o = cursor[s] + int(rng.integers(1, 30))
            while True:
                if residue is not None:
                    o += (residue - o) % 64
                if not used[s, o:o + 336 + 8].any() and not used[s, max(o - 8, 0):o].any():
                    break
                o += 1
            put(s, o, sym)
            cursor[s] = o + 336
    return lines


@pytest.fixture(scope="module")
def capture():
    lines = _capture()
    counts = {aa: [m.mismatch_counts(lines[s], aa, 64 * N_WORDS - 335) for s in range(N_STREAMS)] for aa in (_le.ADV_AA, OTHER_AA)}
    return lines, counts


def _expected_hits(counts, aa, limit, search_bits):
    want = []
    for s, err in enumerate(counts[aa]):
        for o in np.nonzero(err[:search_bits] <= limit)[0]:
            want.append((s, int(o), aa, int(err[o])))
    return want


def _device_scan(lines, pitch, search_bits, aa, limit, hit_cap, alloc):
    import torch
    words = np.zeros((N_STREAMS, pitch), np.uint64)
    words[:, N_WORDS:] = np.uint64(0xFFFFFFFFFFFFFFFF)  # (what lies between the streams is not part of them)
    for s in range(N_STREAMS):
        words[s, :N_WORDS] = _le.pack(lines[s])
    d_words = torch.from_numpy(words.reshape(-1).view(np.int64).copy()).cuda()
    d_hits = torch.full((alloc * HIT,), 0xA5, dtype=torch.uint8, device="cuda")
    d_cnt = torch.zeros(4, dtype=torch.int32, device="cuda")
    bt.check(bt.lib().btbbx_le_coded_scan_device(d_words.data_ptr(), N_WORDS, pitch, N_STREAMS, search_bits, aa, limit, d_hits.data_ptr(),
                                                 hit_cap, d_cnt.data_ptr(), None), "btbbx_le_coded_scan_device")
    torch.cuda.synchronize()
    cnt = d_cnt.cpu().numpy()
    assert not cnt[1:].any()
    return int(cnt[0]), d_hits.cpu().numpy().view(bt.HIT_DTYPE)


@pytest.mark.parametrize("aa", [_le.ADV_AA, OTHER_AA])
@pytest.mark.parametrize("limit", LIMITS)
def test_scan_equals_the_model(capture, aa, limit):
    lines, counts = capture
    search_bits = 64 * N_WORDS - 335                    # the last window ends on the stream's last symbol
    want = _expected_hits(counts, aa, limit, search_bits)
    assert len(want) > 80 and any(w[1] == search_bits - 1 for w in want)
    for pitch in (N_WORDS, N_WORDS + 37):
        alloc = len(want) + 9
        count, hits = _device_scan(lines, pitch, search_bits, aa, limit, alloc - 1, alloc)
        assert count == len(want)
        got = sorted((int(h["stream"]), int(h["offset"]), int(h["lap"]), int(h["ac_errors"])) for h in hits[:count])
        assert got == sorted(want)
        assert not hits["reserved"][:count].any() and hits[count:].tobytes() == b"\xa5" * HIT * (alloc - count)


def test_scan_search_bits_cut_and_hit_cap(capture):
    lines, counts = capture
    # a search that ends inside the second tile, on no word boundary
    search_bits = 40336 + 1
    want = _expected_hits(counts, _le.ADV_AA, 16, search_bits)
    count, hits = _device_scan(lines, N_WORDS, search_bits, _le.ADV_AA, 16, len(want) + 4, len(want) + 5)
    got = sorted((int(h["stream"]), int(h["offset"]), int(h["lap"]), int(h["ac_errors"])) for h in hits[:count])
    assert got == sorted(want) and max(w[1] for w in want) == 40336
    # hit_cap below the count: the count is the whole number, hit_cap distinct true records are written and nothing behind them
    full = _expected_hits(counts, _le.ADV_AA, 63, 64 * N_WORDS - 335)
    cap = len(full) // 2
    count, hits = _device_scan(lines, N_WORDS, 64 * N_WORDS - 335, _le.ADV_AA, 63, cap, cap + 7)
    got = [(int(h["stream"]), int(h["offset"]), int(h["lap"]), int(h["ac_errors"])) for h in hits[:cap]]
    assert count == len(full) and len(set(got)) == cap and set(got) <= set(full)
    assert hits[cap:].tobytes() == b"\xa5" * HIT * 7
    # search_bits 0: nothing happens
    count, hits = _device_scan(lines, N_WORDS, 0, _le.ADV_AA, 63, 4, 4)
    assert count == 0 and hits.tobytes() == b"\xa5" * HIT * 4


# ---- the decoder -------------------------------------------------------------------------------------------------------
def _arrays(pairs):
    pk, inf = np.zeros(len(pairs), bt.LE_PKT_DTYPE), np.zeros(len(pairs), bt.LE_CODED_INFO_DTYPE)
    for i, (r, f) in enumerate(pairs):
        for k in _le.FIELDS:
            pk[k][i] = r[k]
        pk["bytes"][i] = np.frombuffer(r["bytes"], np.uint8)
        for k in m.INFO_FIELDS:
            inf[k][i] = f[k]
    return pk, inf


def _device_decode(words, n_words, pitch, hits, mhz, crc_init, count=None, cap=None):
    """One launch -> (records, info) of buffers that were 0xA5 and are two records longer than cap."""
    import torch
    count = len(hits) if count is None else count
    cap = len(hits) if cap is None else cap
    alloc = cap + 2
    d_words = torch.from_numpy(np.ascontiguousarray(words).reshape(-1).view(np.int64).copy()).cuda()
    d_hits = torch.from_numpy(np.frombuffer(hits.tobytes() + bytes(16), np.int64).copy()).cuda()
    d_phys = torch.from_numpy(np.asarray(mhz, np.uint16).astype(np.int16).reshape(-1).copy()).cuda()
    d_cnt = torch.from_numpy(np.array([count, 0, 0, 0], np.uint32).view(np.int32)).cuda()
    d_out = torch.full((alloc * REC,), 0xA5, dtype=torch.uint8, device="cuda")
    d_info = torch.full((alloc * INFO,), 0xA5, dtype=torch.uint8, device="cuda")
    bt.check(bt.lib().btbbx_le_coded_decode_hits_device(d_words.data_ptr(), n_words, pitch, d_hits.data_ptr(), d_cnt.data_ptr(), cap,
                                                        d_phys.data_ptr(), crc_init, d_out.data_ptr(), d_info.data_ptr(), None, 0, None),
             "btbbx_le_coded_decode_hits_device")
    torch.cuda.synchronize()
    assert int(d_cnt.cpu().numpy().view(np.uint32)[0]) == count
    return d_out.cpu().numpy().view(bt.LE_PKT_DTYPE), d_info.cpu().numpy().view(bt.LE_CODED_INFO_DTYPE)


def _hits(pairs, stream=0):
    h = np.zeros(len(pairs), bt.HIT_DTYPE)
    for i, (o, e) in enumerate(pairs):
        h["offset"][i], h["ac_errors"][i], h["lap"][i], h["stream"][i] = o, e, 0xDEADBEEF, stream
    return h


def _same(got, want, n, itemsize, what):
    bad = [i for i in range(n) if got[i].tobytes() != want[i].tobytes()]
    assert not bad, (what, len(bad), [(i, got[i], want[i]) for i in bad[:3]])
    assert got[n:].tobytes() == b"\xa5" * itemsize * (len(got) - n), what


@pytest.fixture(scope="module")
def cases():
    out = []
    for c in m.decode_cases():
        offs, errs = [o for o, _ in c["hits"]], [e for _, e in c["hits"]]
        out.append((c, _arrays(m.decode_many(c["words"], c["n_words"], 0, offs, errs, c["mhz"], c["crc_init"]))))
    return out


def test_decoder_equals_the_model_on_every_case(cases):
    ok = moved = rfu = cut = 0
    for c, (want_pk, want_info) in cases:
        n = len(c["hits"])
        pk, info = _device_decode(c["words"], c["n_words"], c["n_words"], _hits(c["hits"]), [c["mhz"]], c["crc_init"])
        _same(pk, want_pk, n, REC, c["note"])
        _same(info, want_info, n, INFO, c["note"])
        ok += int(pk["crc_ok"][:n].sum())
        moved += int(info["header_moved"][:n].sum())
        rfu += int((info["s"][:n] == 0).sum())
        cut += int(pk["truncated"][:n].sum())
    assert ok > 90 and moved >= 1 and rfu == 2 and cut >= 10


def test_decoder_two_streams_pitch_above_n_words(cases):
    c, _ = cases[0]
    nw, pitch = c["n_words"], c["n_words"] + 7
    words = np.full((2, pitch), np.uint64(0xFFFFFFFFFFFFFFFF))
    words[:, :nw] = c["words"][:nw]
    mhz = [2402, 2440]
    hits = np.concatenate([_hits(c["hits"], 1), _hits(c["hits"], 0)])
    want = []
    for s in (1, 0):
        for o, e in c["hits"]:
            want.append(m.decode(words[s], nw, s, o, e, mhz[s], c["crc_init"]))
    want_pk, want_info = _arrays(want)
    pk, info = _device_decode(words, nw, pitch, hits, mhz, c["crc_init"])
    _same(pk, want_pk, len(hits), REC, "two streams")
    _same(info, want_info, len(hits), INFO, "two streams")


@pytest.mark.parametrize("cap,count", [(0, 65), (1, 65), (7, 65), (8, 65), (9, 65), (65, 65), (9, 1000), (65, 40)])
def test_decoder_caps_and_counts(cases, cap, count):
    """Groups of eight lanes per hit, eight hits per wave: caps on both sides of a wave, a count above the cap and one below it."""
    c, (want_pk, want_info) = next(x for x in cases if x[0]["note"] == "phases")
    pairs = c["hits"] + c["hits"][:1]
    want_pk, want_info = np.concatenate([want_pk, want_pk[:1]]), np.concatenate([want_info, want_info[:1]])
    assert len(pairs) == 65
    pk, info = _device_decode(c["words"], c["n_words"], c["n_words"], _hits(pairs), [c["mhz"]], c["crc_init"], count=count, cap=cap)
    n = min(cap, count)
    _same(pk, want_pk, n, REC, (cap, count))
    _same(info, want_info, n, INFO, (cap, count))


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_le_coded_scan_end_to_end():
    """Three advertising channels, both S values, a few symbol errors in every packet: le_coded_scan against match_all + decode_many."""
    rng = np.random.default_rng(77)
    mhz = _le.ADV_MHZ
    nw = 600
    lines = rng.integers(0, 2, (3, 64 * nw), dtype=np.uint8)
    for s in range(3):
        at = 50 + 13 * s
        for k in range(5):
            sym = m.coded_symbols(_le.ADV_AA, _le.channel_index(mhz[s]), m.pdu_of(rng, int(rng.integers(0, 38))), _le.ADV_CRC_INIT, (2, 8)[(k + s) & 1])
            sym = m.flip(sym, np.concatenate([rng.choice(376, 4, replace=False), 376 + rng.choice(len(sym) - 376, 2, replace=False)]))
            lines[s, at:at + len(sym)] = sym
            at += len(sym) + int(rng.integers(100, 900))
        assert at < 64 * nw
    words = np.stack([_le.pack(lines[s]) for s in range(3)])
    search_bits = 64 * nw - 335
    want = []
    for s in range(3):
        offs, errs = m.match_all(words[s], nw, search_bits, _le.ADV_AA, 16)
        want += m.decode_many(words[s], nw, s, offs, errs, mhz[s], _le.ADV_CRC_INIT)
    want_pk, want_info = _arrays(want)
    assert len(want) == 15 and want_pk["crc_ok"].all() and set(want_info["s"]) == {2, 8}
    pk, info = bt.le_coded_scan(words, search_bits, mhz, n_streams=3)
    assert pk.tobytes() == want_pk.tobytes() and info.tobytes() == want_info.tobytes()
    pk, info = bt.le_coded_scan(words, search_bits, mhz, n_streams=3, cap=4, truncate=True)
    assert pk.tobytes() == want_pk[:4].tobytes() and info.tobytes() == want_info[:4].tobytes()
    with pytest.raises(bt.BtbbError):
        bt.le_coded_scan(words, search_bits, mhz, n_streams=3, cap=4)
