"""The 64-clock trial kernels, the UAP table and the decoders on the boundary lattice of tests/_trial_lattice.py:
every result against the oracle's, at every batch geometry of btbbx_trials_device (one-workgroup-per-trial kernel
up to 256 packets, the persistent batch kernel above: last batch full or ragged, several passes of its grid) and in
batches that hold one kind of packet only."""
import numpy as np
import pytest

import _libs
import _trial_lattice as tl
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def ready():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    bt.init(2)
    _libs.oracle().orc_init(2)


@pytest.fixture(scope="module")
def lat():
    return tl.lattice()


@pytest.fixture(scope="module")
def tables():
    return tl.tables()


def _check(got, want, tags, what):
    """[n, 64] TRIAL_DTYPE against the oracle's; a few failures with their tags on a mismatch."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    rows = np.nonzero(bad.any(axis=1))[0]
    assert not len(rows), (what, "%d of %d packets differ" % (len(rows), len(got)),
                           [(int(r), tags[r], [(int(c), got[r, c].tolist(), want[r, c].tolist())
                                               for c in np.nonzero(bad[r])[0][:3]]) for r in rows[:5]])
    return got.size


def _run(lat, tables, idx, what, pin=None, want=None):
    idx = np.asarray(idx, dtype=np.int64)
    pin = lat.pin[idx] if pin is None else pin
    got = bt.run_trials(np.ascontiguousarray(lat.words[idx]), np.ascontiguousarray(pin))
    return _check(got, tables[idx] if want is None else want, [lat.tags[i] for i in idx], what), got


def test_trials_at_every_batch_geometry(lat, tables):
    import torch
    n_all = len(lat.syms)
    rng = np.random.default_rng(_libs.seed(401))
    order = rng.permutation(n_all)
    for n in (1, 2, 255, 256, 257, 288, 289):           # wide kernel up to 256; 257 / 289 leave a batch of one
        _run(lat, tables, order[:n], ("n", n))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 3 * 32 * 2 * cus + 17                           # three passes of the persistent grid, a ragged last batch
    _run(lat, tables, rng.integers(0, n_all, n), ("grid passes", n))
    _run(lat, tables, np.arange(n_all), "lattice in order")        # types grouped: batches of one type
    _run(lat, tables, order, "lattice permuted")


def _fixed_unwhitened(lat):
    return [i for i, t in enumerate(lat.tags) if not lat.air_white[i] and not int(lat.pin["flags"][i]) & 1]


def test_trials_in_batches_of_one_kind(lat, tables):
    """Batches of 32 (the persistent kernel's batch) that hold one kind of packet only: the per-batch slot layout
    (type_base / pk_sort) with no varying packet, with every packet of one type, with entry types 16 / 255."""
    orc = _libs.oracle()
    rng = np.random.default_rng(_libs.seed(403))
    fixed = _fixed_unwhitened(lat)
    hdr4 = [i for i, t in enumerate(lat.tags) if t[1].startswith("hdr4")]
    dm3 = [i for i, t in enumerate(lat.tags) if t[:2] == ("DM3", "full") and lat.air_white[i] and int(lat.pin["flags"][i]) & 1]
    plain = [i for i, t in enumerate(lat.tags) if t[1] == "full" and lat.air_white[i] and int(lat.pin["flags"][i]) & 1]
    assert len(fixed) >= 64 and len(hdr4) >= 32 and len(dm3) >= 32
    batches = []
    for entry in (3, 16):                                # unwhitened packets, one entry type for all
        b = list(rng.choice(fixed, 32, replace=False))
        batches.append((b, dict(type=entry)))
    b = list(rng.choice(hdr4, 32, replace=False))        # header FEC 1/3 fails: entry types 0..15, 16, 255
    batches.append((b, dict(type=np.array(tl.ENTRY_TYPES * 2)[:32])))
    batches.append((list(rng.choice(hdr4, 32, replace=False)), dict(type=255)))
    batches.append((list(rng.choice(dm3, 32, replace=False)), {}))        # whitened, all of one true type
    alt = [int(x) for pair in zip(rng.choice(fixed + hdr4, 16, replace=False), rng.choice(plain, 16, replace=False))
           for x in pair]
    batches.append((alt, {}))                            # fixed and varying alternating
    batches.append((list(rng.choice(plain, 32, replace=False)), {}))      # filler: the call must take > 256 packets
    batches.append((list(rng.choice(plain, 32, replace=False)), {}))
    batches.append((list(rng.choice(plain, 32, replace=False)), {}))
    idx = np.concatenate([np.array(b, dtype=np.int64) for b, _ in batches])
    pin = lat.pin[idx].copy()
    for k, (_, over) in enumerate(batches):
        for f, v in over.items():
            pin[f][32 * k:32 * k + 32] = v
    want = np.stack([tl.oracle_table(orc, lat.syms[i], pin[j]) for j, i in enumerate(idx)])
    assert len(idx) == 288 and (want["rv"][:64] == want["rv"][:64, :1]).all()   # fixed type: one verdict per packet
    _, linear = _run(lat, tables, idx, "one kind per batch", pin=pin, want=want)
    wide = np.concatenate([bt.run_trials(np.ascontiguousarray(lat.words[idx[k:k + 96]]), pin[k:k + 96])
                           for k in range(0, len(idx), 96)])
    assert np.array_equal(wide, linear)


def test_wide_and_linear_kernels_agree_on_the_lattice(lat, tables):
    """The same packets through trials_wide_kernel (calls of 256) and trials_linear_kernel (one call): identical."""
    n = len(lat.syms)
    linear = bt.run_trials(lat.words, lat.pin)
    wide = np.concatenate([bt.run_trials(np.ascontiguousarray(lat.words[k:k + 256]), lat.pin[k:k + 256])
                           for k in range(0, n, 256)])
    assert np.array_equal(wide, linear)
    _check(wide, tables, lat.tags, "wide kernel, lattice")


def test_uap_table_on_the_lattice(lat, tables):
    """btbbx_uap_table_device = try_clock's return | type << 8 where the header's FEC 1/3 holds, 0 where it fails;
    equal to the trial tables there."""
    ok = tl.header_fec_ok()
    n_all = len(lat.syms)
    want_all = np.where(ok[:, None], tables["uap"].astype(np.uint16) | tables["type"].astype(np.uint16) << 8, 0)
    for n in (1, 63, 65, 257, n_all, n_all + 1):
        idx = np.arange(n) % n_all
        got = bt.run_uap_table(np.ascontiguousarray(lat.words[idx]), np.ascontiguousarray(lat.pin[idx]))
        bad = np.nonzero((got != want_all[idx]).any(axis=1))[0]
        assert not len(bad), (n, len(bad), [(lat.tags[idx[r]], got[r][:4], want_all[idx[r]][:4]) for r in bad[:5]])
    assert 100 < (~ok).sum() < n_all // 4


def _decode_entries(lat, wrong):
    rng = np.random.default_rng(_libs.seed(409 + wrong))
    n = len(lat.syms)
    pin = lat.pin.copy()
    clk = lat.clk6.astype(np.uint32)
    if wrong:
        clk = clk ^ rng.integers(1, 64, n).astype(np.uint32)
    pin["clkn"] = clk | (rng.integers(0, 1 << 20, n).astype(np.uint32) << 6)
    pin["uap"] = lat.uap
    pin["flags"] |= tl.F_UAP_VALID | tl.F_CLK6_VALID
    return pin


@pytest.mark.parametrize("wrong", [0, 1])
def test_decode_on_the_lattice(lat, wrong):
    """btbbx_decode_device at the clock each packet was built with and at a wrong one (CLK6 valid, UAP given, the
    lattice's entry type / llid / flow / flags) against the oracle, every field of the record; the oracle against
    the compiled reference on a sample."""
    from test_gpu_packets import _both_decode
    orc = _libs.oracle()
    pin = _decode_entries(lat, wrong)
    got = bt.run_decode(lat.words, pin)
    want = tl.oracle_decode(orc, lat.syms, pin)
    for f in bt.PKTOUT_DTYPE.names:
        bad = np.nonzero((got[f] != want[f]).reshape(len(got), -1).any(axis=1))[0]
        assert not len(bad), (f, len(bad), [(int(r), lat.tags[r], got[f][r].tolist() if f != "payload" else "",
                                             want[f][r].tolist() if f != "payload" else "") for r in bad[:5]])
    rv = got["payload_rv"]
    if not wrong:
        assert (rv == 10).sum() > 3000 and (rv == 1000).sum() > 100 and (rv == 0).sum() > 200
    # the oracle port against the compiled reference (whitened entries: _both_decode's packets are)
    for i in range(wrong, len(lat.syms), 29):
        if int(pin["flags"][i]) & 1:
            present, h, r, st = _both_decode(orc, lat.syms[i], int(pin["clkn"][i]), int(pin["uap"][i]), ctx=lat.tags[i])
            assert (present, h) == (int(want[i]["header_present"]), int(want[i]["header_rv"])), lat.tags[i]
            if h:
                assert r == int(want[i]["payload_rv"]), lat.tags[i]


def test_decode_from_the_streams_on_the_lattice(lat):
    """The lattice laid end to end into packed streams: btbbx_decode_hits_device equals gather + btbbx_decode_device
    byte for byte (each packet's window runs on into the next one, as in a capture)."""
    rng = np.random.default_rng(_libs.seed(411))
    n = len(lat.syms)
    n_streams = 4
    pin = _decode_entries(lat, 0)
    rows, parts, pos = [], [[] for _ in range(n_streams)], [64] * n_streams
    for st in range(n_streams):
        parts[st].append(rng.integers(0, 2, 64, dtype=np.uint8))
    for i in range(n):
        st = i % n_streams
        gap = rng.integers(0, 2, int(rng.integers(0, 48)), dtype=np.uint8)
        parts[st] += [lat.syms[i], gap]
        rows.append((st, pos[st]))
        pos[st] += len(lat.syms[i]) + len(gap)
    n_words = (max(pos) + 64 * 8) // 64
    words = np.zeros((n_streams, n_words), np.uint64)
    for st in range(n_streams):
        w = bt.synth.pack_bits(np.concatenate(parts[st]))
        words[st, :len(w)] = w
    hits = np.zeros(n, bt.HIT_DTYPE)
    hits["stream"] = [r[0] for r in rows]
    hits["offset"] = [r[1] for r in rows]
    direct, len_d = bt.run_decode_hits(words, hits, pin)
    two_step, len_g = bt.run_decode_hits(words, hits, pin, via_gather=True)
    assert np.array_equal(len_d, len_g)
    bad = [i for i in range(n) if direct[i].tobytes() != two_step[i].tobytes()]
    assert not bad, (len(bad), [(i, lat.tags[i]) for i in bad[:5]])
    assert (direct["payload_rv"] == 10).sum() > 2500
