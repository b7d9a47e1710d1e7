"""The model of LE following through connection parameter updates (tests/_le_span.py) on the CPU: on every planted world every event
the model leaves COUNTED carries its planted counter and lies on the planted channel; the two equivalences with the follow
stage's model; the record invariants of rule 7; and every deliberately wrong variant of the model differs from it somewhere on
the lattice -- so a device that made that mistake would not pass tests/test_gpu_le_span.py."""
import pytest

import _le_follow as lf
import _le_span as ls


@pytest.mark.parametrize("name, max_updates", [("lattice", 0), ("lattice", 1), ("lattice", 4), ("lattice", 16), ("chain", 0), ("chain", 1),
                                               ("chain", 2), ("chain", 3), ("chain", 16), ("wrap", 4), ("crowd", 2), ("seam", 8), ("end", 4)])
def test_planted_events_carry_their_counters(name, max_updates):
    b = ls.WORLDS[name]()
    seeds, spans, spkts, recs = ls.world_model(name, max_updates)
    n = ls.check_planted(b, seeds, spans, spkts)
    planted = [g for g, nm in enumerate(b.names) if nm in b.by_anchor and nm.startswith("planted") and seeds[g] is not None]
    assert n > 0 and planted
    if name in ("chain", "wrap", "crowd", "seam") and max_updates >= 3 or name == "crowd":
        # every update is followed: nothing is off the prediction, BEYOND or -- but for the crowd's one stray packet -- in a GAP
        for g in planted:
            s = spans[g]
            assert (s.n_off, s.n_beyond, s.n_before) == (0, 0, 0) and s.n_gap <= (name == "crowd"), (b.names[g], s)
        inside = set(planted)
        assert n == sum(c.channel in inside for c in b.cands) - sum(spans[g].n_gap for g in planted)      # (a GAP event here is one packet)


def _invariants(b, spans, spkts, recs, max_updates):
    for g, s in enumerate(spans):
        mine = [i for i, c in enumerate(b.cands) if c.channel == g and spkts[i] is not None]
        if s is None:
            assert recs[g] == [None] * (max_updates + 1) and all(spkts[i][:3] == (0, 0, 0) and spkts[i][5:] == (0xFF, 0, 0, 0) for i in mine)
            continue
        events = {b.pkts[i].event for i in mine}
        assert s.n_before + s.n_gap + s.n_on + s.n_off + s.n_beyond == len(events), (b.names[g], s)
        there = [r for r in recs[g] if r is not None]
        assert len(recs[g]) == max_updates + 1 and recs[g][:len(there)] == there and len(there) == s.n_spans
        assert sum(r.n_events for r in there) == s.n_on + s.n_off and there[-1].interval == s.interval
        assert there[0].pdu == ls.NONE and [spkts[r.pdu].applied for r in there[1:]] == [1] * (s.n_spans - 1)
        assert sum(spkts[i].applied for i in mine) == s.n_spans - 1
        assert s.n_param_updates == sum(spkts[i].kind == lf.PARAM_UPDATE for i in mine)
        assert s.n_map_updates == sum(spkts[i].kind == lf.MAP_UPDATE for i in mine)
        assert bool(s.flags & lf.STOPPED) == bool(s.flags & (ls.CAPPED | ls.REFUSED)) and (s.flags & (ls.CAPPED | ls.REFUSED)) != ls.CAPPED | ls.REFUSED
        counters = [(b.pkts[i].event, spkts[i].span, spkts[i].counter) for i in mine if spkts[i].state in (lf.ST_COUNTED, lf.ST_BEYOND)]
        ordered = sorted(set(counters))
        assert [sp for _, sp, _ in ordered] == sorted(sp for _, sp, _ in ordered)               # spans rise with the events
        for x in there[1:]:
            assert all(c >= x.base for _, sp, c in ordered if sp == there.index(x)) or x.base > 0xFFFF0000


@pytest.mark.parametrize("name, max_updates", [("lattice", 0), ("lattice", 4), ("chain", 2), ("chain", 16), ("wrap", 4), ("crowd", 2)])
def test_record_invariants(name, max_updates):
    _invariants(ls.WORLDS[name](), *ls.world_model(name, max_updates)[1:], max_updates)


def _equivalent(b, max_updates):
    seeds, follows, fpkts = lf.model(b)
    _, spans, spkts, _ = ls.model(b, max_updates)
    n = 0
    for g, (f, s) in enumerate(zip(follows, spans)):
        assert (f is None) == (s is None)
        if f is not None and max_updates == 0:
            assert (s.map, s.counter_first, s.stop, s.n_before, s.n_on, s.n_off, s.n_beyond, s.n_control, s.n_map_updates, s.algorithm) == \
                (f.map, f.counter_first, f.stop, f.n_before, f.n_on, f.n_off, f.n_beyond, f.n_control, f.n_map_updates, f.algorithm), b.names[g]
            assert s.flags & ~(ls.CAPPED | ls.REFUSED) == f.flags and (s.n_gap, s.n_spans) == (0, 1)
    for i, (p, q) in enumerate(zip(fpkts, spkts)):
        assert (p is None) == (q is None)
        if p is None:
            continue
        shared = (q.counter, q.epoch, q.kind, q.opcode, q.expected, q.on_hop, q.state)
        if max_updates == 0:
            assert shared == tuple(p) and (q.span, q.applied) == (0, 0), (i, p, q)
        elif follows[b.cands[i].channel] is not None and p.state == lf.ST_COUNTED:
            same_alg = follows[b.cands[i].channel].algorithm == spans[b.cands[i].channel].algorithm
            assert q.span == 0 and (shared if same_alg else shared[:4] + shared[6:]) == (tuple(p) if same_alg else tuple(p)[:4] + tuple(p)[6:])
            n += 1
    return n


@pytest.mark.parametrize("world", ["follow lattice", "follow wrap", "lattice", "chain", "wrap"])
@pytest.mark.parametrize("max_updates", [0, 4])
def test_equivalence_with_the_follow_model(world, max_updates):
    b = {"follow lattice": lf.lattice, "follow wrap": lf.wrap_world, "lattice": ls.lattice, "chain": ls.chain_world, "wrap": ls.wrap_world}[world]()
    assert _equivalent(b, max_updates) > 20 or max_updates == 0


def _differs(name, rules, max_updates):
    return ls.model(ls.WORLDS[name](), max_updates, rules)[1:] != ls.world_model(name, max_updates)[1:]


@pytest.mark.parametrize("variant", sorted(ls.VARIANTS))
def test_every_wrong_variant_differs_on_the_lattice(variant):
    rules = ls.Rules(**ls.VARIANTS[variant])
    assert _differs("lattice", rules, 1 if variant.startswith("cap_") else 4), variant


def test_the_variants_cover_the_issue_list():
    assert len(ls.VARIANTS) == 24 and all(vars(ls.Rules(**kw)) != vars(ls.MODEL) for kw in ls.VARIANTS.values())
