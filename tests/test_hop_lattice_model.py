"""The hop lattice on the CPU (tests/_hop_lattice.py): its numpy model against the oracle's whole patterns and its reversal, the
frozen reversal scenarios and the selection points against what their tags claim -- the condition that keeps
tests/test_gpu_hop_lattice.py honest -- and a set of deliberately wrong models, each of which some lattice point tells apart."""
import ctypes as C

import numpy as np
import pytest

import _hop
import _hop_lattice as hl
import _libs


@pytest.fixture(scope="module")
def orc():
    o = _libs.oracle()
    o.orc_init(2)
    yield o
    o.orc_hop_cache_clear()


def _amap(cfg):
    return None if cfg.afh_map is None else np.array(cfg.afh_map, np.uint8)


PATTERN_KINDS = (("none", 7), ("u1", 0), ("u2", 0), ("u32", 0), ("u78", 1), ("u79", 1))


def _pattern_clocks():
    rng = np.random.default_rng(_libs.seed(8101))
    return np.concatenate([rng.integers(0, hl.SEQ_LEN, 1 << 20), np.arange(1 << 16), np.arange(hl.SEQ_LEN - 4096, hl.SEQ_LEN)])


def test_model_matches_oracle_patterns(orc, capfd):
    cfgs = [hl.config_by_kind(kind, nth) for kind, nth in PATTERN_KINDS]
    fields = [hl.address_fields(c.address) for c in cfgs]
    assert len({f[1] for f in fields}) == len(cfgs) and len({f[4] for f in fields}) == len(cfgs)     # b and e differ in each
    clocks = _pattern_clocks()
    for cfg in cfgs:
        lap, uap = hl.lap_uap(cfg)
        pn, want = _hop.orc_pattern(orc, lap, uap, _amap(cfg))
        c = pn.contents
        assert (c.a1, c.b, c.c1, c.d1, c.e) == hl.address_fields(cfg.address), cfg.tag
        got = hl.model_hops(cfg.address, cfg.afh_map, clocks)
        bad = np.nonzero(got != want[clocks])[0]
        assert len(bad) == 0, (cfg.tag, len(bad), int(clocks[bad[0]]))
        orc.orc_piconet_free(pn)
        orc.orc_hop_cache_clear()                                   # a pattern is 128 MiB: gone before the next
    capfd.readouterr()
    # the same against the compiled reference, where it is at hand (its pattern cache cannot be emptied: two patterns only)
    ref = _libs.ref()
    for cfg in (cfgs[0], cfgs[4]) if ref is not None else ():
        lap, uap = hl.lap_uap(cfg)
        r = C.c_void_p(ref.btbb_piconet_new())
        ref.btbb_init_piconet(r, lap)
        ref.btbb_piconet_set_uap(r, uap)
        if cfg.afh_map is not None:
            ref.btbb_piconet_set_flag(r, _hop.F_IS_AFH, 1)
            ref.btbb_piconet_set_afh_map(r, _libs.ptr(_amap(cfg)))
        else:
            ref.btbb_piconet_set_channel_seen(r, 0)                 # the reference divides by used_channels, see _hop.orc_pattern
            ref.get_hop_pattern(r)
        want = _hop.seq_view(ref.refint_piconet_sequence(r))
        got = hl.model_hops(cfg.address, cfg.afh_map, clocks)
        assert np.array_equal(got, want[clocks]), cfg.tag
    capfd.readouterr()


def test_model_matches_oracle_reversal(orc, capfd):
    """model_candidates and model_winnow against orc_init_hop_reversal and orc_winnow, call by call; candidate counts the
    reference's own array holds (basic hopping and maps of 30 channels and more)"""
    rng = np.random.default_rng(_libs.seed(8102))
    for rep, (kind, nth, alias) in enumerate((("none", 3, 0), ("none", 4, 1), ("u63", 0, 0), ("u32", 0, 1))):
        cfg = hl.config_by_kind(kind, nth)
        lap, uap = hl.lap_uap(cfg)
        pn, seq = _hop.orc_pattern(orc, lap, uap, _amap(cfg))
        c0, t0 = int(rng.integers(0, hl.SEQ_LEN)), int(rng.integers(0, 1 << 27))
        c = pn.contents
        c.first_pkt_time, c.clk_offset, c.aliased = t0, ((c0 & 63) - (t0 & 63)) & 63, alias
        obs = _hop.observations(rng, seq, c0, 30, alias=bool(alias), max_gap=2000)
        if rep == 1:
            obs[2] = (obs[2][0], _hop.aliased((seq[(c0 + obs[2][0]) % hl.SEQ_LEN] + 7) % 79))      # a contradiction
        c.pattern_indices[0], c.pattern_channels[0] = obs[0]
        c.packets_observed = 1
        n = orc.orc_init_hop_reversal(alias, pn)
        cur = hl.model_candidates(cfg.address, cfg.afh_map, c0 & 63, obs[0][1], alias)
        assert n == len(cur) and n > 0
        assert np.array_equal(cur, np.ctypeslib.as_array(c.clock_candidates, (n,))), cfg.tag
        k = 1
        for step in [1, 1, 3, 1, 2] + [1] * 40:
            if k >= len(obs) or not (c.flags >> _hop.F_HOP_INIT & 1):
                break
            for idx, ch in obs[k:k + step]:
                c.pattern_indices[c.packets_observed], c.pattern_channels[c.packets_observed] = idx, ch
                c.packets_observed += 1
            k += step
            w0 = c.winnowed
            offs = [c.pattern_indices[i] for i in range(w0, c.packets_observed)]
            chans = [c.pattern_channels[i] for i in range(w0, c.packets_observed)]
            rv = orc.orc_winnow(pn)
            stop, count, cand0, cur = hl.model_winnow(cur, offs, chans, cfg.address, cfg.afh_map, alias)
            assert count == rv == len(cur), (cfg.tag, k)
            if rv:
                assert w0 + stop == c.winnowed
                assert np.array_equal(cur, np.ctypeslib.as_array(c.clock_candidates, (rv,))) and cand0 == cur[0], (cfg.tag, k)
            if rv <= 1:
                break
        if rep == 1:
            assert len(cur) == 0 or cur[0] != c0
        else:
            assert cur.tolist() == [c0], cfg.tag
        orc.orc_piconet_free(pn)
        orc.orc_hop_cache_clear()
    capfd.readouterr()


# ---- the frozen tables ---------------------------------------------------------------------------------------------------

def test_selection_points_cover_what_they_claim():
    cfgs = hl.configs()
    fields = [hl.address_fields(c.address) for c in cfgs]
    basic = [f for c, f in zip(cfgs, fields) if c.afh_map is None]
    afh = [f for c, f in zip(cfgs, fields) if c.afh_map is not None]
    assert {f[1] for f in basic} == {f[1] for f in afh} == set(range(16))                  # every b, under both
    assert {f[4] for f in fields} == set(hl.E_VALUES)
    for k, name in ((0, "a1"), (2, "c1")):
        assert {0, 31} <= {f[k] for f in fields} and len({f[k] for f in fields}) > 4, name
    assert {0, 511} <= {f[3] for f in fields}
    mods = {hl.bank_of(c.afh_map)[1] for c in cfgs if c.afh_map is not None}
    assert mods == {1, 2, 3, 31, 32, 33, 63, 64, 65, 77, 78, 79}
    two = {tuple(hl.bank_of(c.afh_map)[0].tolist()) for c in cfgs if c.afh_map is not None and hl.bank_of(c.afh_map)[1] == 2}
    assert (40, 42) in two and (0, 77) in two and len(two) >= 3
    # the window start K = e + f over the clock sets: every K & 3 with every e, and the top of the table: K + 63 = 268
    groups = np.array(hl.edge_groups(), np.int64)
    assert {int(16 * t % 79) for t in groups} >= {0, 78} and {0, hl.N_GROUPS - 1} <= set(groups.tolist())
    top = 0
    n_clocks = 0
    for i, (c, f) in enumerate(zip(cfgs, fields)):
        clocks = hl.clock_set(i)
        n_clocks += len(clocks)
        assert (clocks >= hl.SEQ_LEN).sum() > 60000                                       # 32-bit values: most are above 2^27
        t = (clocks.astype(np.int64) & hl.M27) >> 6
        fk = 16 * t % 79
        mod = hl.bank_of(c.afh_map)[1]
        if c.afh_map is not None:
            fk = fk % mod
        assert {int(v) for v in np.unique((f[4] + fk) & 3)} == ({0, 1, 2, 3} if mod >= 4 else {(f[4] + j) & 3 for j in range(mod)}), c.tag
        top = max(top, int(f[4] + fk.max()) + 63)
    assert top == 268
    e127 = [c for c, f in zip(cfgs, fields) if f[4] == 127 and hl.bank_of(c.afh_map)[1] == 79]
    assert e127, "e = 127 on 79 channels: the only way to entry 268"
    # every count and every kind of first, and all their pairs over the configurations
    pairs = {(kind, count) for i in range(len(cfgs)) for kind, first, count in hl.slices(i)}
    assert pairs == {(k, 64 * g) for k in hl.SLICE_FIRSTS for g in hl.SLICE_GROUPS}
    for i in range(len(cfgs)):
        for kind, first, count in hl.slices(i):
            assert first % 64 == 0 and first + count <= hl.SEQ_LEN
            assert {"zero": first == 0, "odd64": (first >> 6) & 1 == 1, "f78": 16 * (first >> 6) % 79 == 78,
                    "end": first + count == hl.SEQ_LEN}[kind]
    n_slices = sum(len(hl.slices(i)) for i in range(len(cfgs)))
    print("\nhop lattice: %d configurations, %d clocks, %d slices, %d reversal scenarios" % (len(cfgs), n_clocks, n_slices, len(hl.SCENARIOS)))
    assert 55 <= len(cfgs) <= 70


def test_reversal_scenarios_are_what_their_tags_claim():
    """Every frozen scenario recomputed with the model: the list lengths, stops and counts written into the table, and over
    the table every point of the issue's list."""
    lens, per_call, facts = {}, set(), set()
    for s in hl.SCENARIOS:
        opened, calls = hl.replayed(s["tag"])
        assert len(opened) == s["n_open"], s["tag"]
        assert [c[:3] for c in calls] == [tuple(c) for c in s["calls"]], s["tag"]
        off, ch = hl.expand(s)
        assert len(off) == sum(s["cuts"])
        facts.add("aliased" if s["aliased"] else "plain")
        facts.update("channel-%d" % v for v in (79, 128, 255) if v in ch.tolist())
        facts.update({0: "group-0", hl.N_GROUPS - 1: "group-last"}.get(s["c0"] >> 6, "group-mid").split())
        at = 0
        for n, (n_before, stop, count, cand0, left) in zip(s["cuts"], calls):
            lens.setdefault(n_before, (s["tag"], n))
            per_call.add(n)
            path = "small" if n_before <= 16384 else "large"
            if n_before > 1:
                facts.add("%d-obs-%s" % (n, path))
                if stop == n:
                    facts.add("never")
                    facts.update(["two-left"] if count == 2 else [])
                else:
                    facts.add("stop-first" if stop == 0 else "stop-last" if stop == n - 1 else "stop-middle")
                    facts.update(["contradiction"] if count == 0 else [])
                    if count == 1 and not any(v in ch[:at + stop + 1].tolist() for v in (79, 128, 255)):
                        assert cand0 == s["c0"], s["tag"]                       # built to end with one: it is the true clock
            elif n_before == 1:
                facts.add("call-on-one")
            else:
                facts.add("call-on-none")
                assert (stop, count) == (0, 0)
            if path == "large":
                facts.add("large-mod64-%d" % (n_before % 64))
                facts.add("per-%d" % min(((n_before + 63) // 64 + 1023) // 1024, 3))
            if path == "small" and n_before > 1024 and count > 1:
                where = np.searchsorted(opened if at == 0 else prev, left)
                if where.min() < 1024 and where.max() >= (n_before - 1) // 1024 * 1024:
                    facts.add("first-and-last-block")
            if len(left) and int(left.max()) + int(off[:at + n].max()) >= hl.SEQ_LEN:
                facts.add("passes-2^27")
            prev, at = left, at + n
    for n in (1, 2, 1023, 1024, 1025, 16384, 16385, 1 << 21):
        assert n in lens, n
    print("\nthe kernel switch: a call begins with 16384 candidates in %s and with 16385 in %s" % (lens[16384][0], lens[16385][0]))
    assert per_call >= {1, 2, 255, 256, 257, 1023, 1024}
    want = {"aliased", "plain", "channel-79", "channel-128", "channel-255", "group-0", "group-last", "never", "two-left", "stop-first",
            "stop-middle", "stop-last", "contradiction", "call-on-one", "call-on-none", "large-mod64-0", "large-mod64-1",
            "large-mod64-63", "per-1", "per-2", "1024-obs-small", "1024-obs-large", "first-and-last-block", "passes-2^27"}
    assert want <= facts, sorted(want - facts)
    assert 18 <= len(hl.SCENARIOS) <= 24


# ---- wrong variants --------------------------------------------------------------------------------------------------------

def test_every_wrong_hop_variant_is_told_apart():
    """each deliberate mistake in the selection changes the hop at some clock of the lattice's clock sets"""
    cfgs = hl.configs()
    found = {}
    for i, c in enumerate(cfgs):
        clocks = hl.clock_set(i)[-64 * len(hl.edge_groups()) - 4096:]             # the edge groups and 4096 random clocks
        true = hl.model_hops(c.address, c.afh_map, clocks)
        for v in hl.WRONG_HOP_VARIANTS:
            if v in found or (v == "mod+1" and c.afh_map is None):                # (mod + 1 = 80 leaves the bank)
                continue
            bad = np.nonzero(hl.model_hops(c.address, c.afh_map, clocks, v) != true)[0]
            if len(bad):
                found[v] = (c.tag, int(clocks[bad[0]]))
        if len(found) == len(hl.WRONG_HOP_VARIANTS):
            break
    assert set(found) == set(hl.WRONG_HOP_VARIANTS), sorted(set(hl.WRONG_HOP_VARIANTS) - set(found))
    # a table that ends at entry 256 shows only where e is large
    assert hl.address_fields([c for c in cfgs if c.tag == found["tab256"][0]][0].address)[4] >= 124
    print("\nwrong selection variants and the lattice point that tells each apart:", found)


def test_every_wrong_reversal_variant_is_told_apart():
    found = {}
    for v, tag in (("alias+1", "aliased/basic/stop-mid-257"), ("stop<1", "basic/stop-last-of-1023/top"), ("block-order", "u2/n63/n1025")):
        s = hl.scenario(tag)
        opened, calls = hl.replayed(tag)
        wrong_open, wrong_calls = hl.replay(s, v)
        for k, (a, b) in enumerate(zip(calls, wrong_calls)):
            if a[:4] != b[:4] or not np.array_equal(a[4], b[4]):
                found[v] = (tag, "call %d" % k)
                break
        if v == "alias+1" and not np.array_equal(opened, wrong_open):
            found[v] = (tag, "open")
    assert set(found) == set(hl.WRONG_REVERSAL_VARIANTS), found
    print("\nwrong reversal variants and the scenario that tells each apart:", found)
