"""The test-side model of keyed LE following (tests/_le_keyed.py) against what does not share its code: the twin capture, in which
every READABLE PDU stands as the plaintext the world planted, read by the UNKEYED models; the planted connections' own hopping;
and a list of deliberately wrong rules, each of which the shared lattice must tell from the right ones."""
import pytest

import _le_crypt as cm
import _le_follow as lf
import _le_keyed as lk
import _le_span as ls

WORLDS = dict(lattice=lk.lattice, end=lk.end_world, crowd=lk.crowd_world, span=lk.span_world, wrap=lk.wrap_world)


@pytest.mark.parametrize("world", sorted(WORLDS))
def test_the_keyed_model_on_s_is_the_unkeyed_model_on_the_twin(world):
    b = WORLDS[world]()
    assert any(p.state == cm.VERIFIED for _, p in b.sent)
    n = lk.same_as_twin(b, lk.model_follow(b)[1:], lk.twin_follow(b)[1:])
    for max_updates in (0, 1, 2):
        assert lk.same_as_twin(b, lk.model_span(b, max_updates)[1:], lk.twin_span(b, max_updates)[1:]) == n
    assert n > 15


@pytest.mark.parametrize("world", ["lattice", "crowd", "span", "wrap"])
def test_planted_connections_are_on_their_channels_with_their_counters(world):
    """Every planted connection that sends its updates encrypted is on its planted channel at every counted event and carries the
    planted counters across parameter updates: nothing is off the hop, nothing BEYOND."""
    b = WORLDS[world]()
    seeds, spans, spkts, recs = lk.model_span(b, 2)
    assert ls.check_planted(b, seeds, spans, spkts) > 15
    decrypted = 0
    for name, s in zip(b.names, spans):
        if name and name.startswith("planted") and s is not None:
            assert s.n_off == 0 and s.n_beyond == 0, (name, s)
            decrypted += bool(s.flags & lk.DECRYPTED)
    assert decrypted >= 1
    follows = lk.model_follow(b)[1]
    for name, f, s in zip(b.names, follows, spans):                    # (the follow stage stops where a parameter update applies)
        if name and name.startswith("planted") and f is not None and s.n_spans == 1:
            assert f.n_off == 0 and f.n_beyond == 0 and f.flags == s.flags, (name, f)


def test_the_unkeyed_model_loses_what_the_keyed_one_follows():
    """What the feature is for: the same lists through the unkeyed model leave the connections that changed their map or their
    interval behind the start off their hop sequence."""
    b = lk.span_world()
    keyed, plain = lk.model_span(b, 2)[1], ls.model(b, 2)[1]
    g = b.names.index("planted: encrypted update, map update in span 1, TERMINATE, map update")
    assert keyed[g].n_off == 0 and keyed[g].n_spans == 2 and keyed[g].n_map_updates == 2 and keyed[g].flags & lf.TERMINATED
    assert keyed[g].flags & lk.DECRYPTED and keyed[g].flags & lf.ENCRYPTED
    assert plain[g].n_off > 10 and plain[g].n_spans == 1 and not plain[g].flags & (lk.DECRYPTED | lf.TERMINATED)
    r = b.names.index("refused: encrypted update, interval 5")
    assert keyed[r].flags & ls.REFUSED and keyed[r].n_beyond > 0 and not plain[r].flags & ls.REFUSED


def test_equality_a_without_a_readable_member():
    """Contract 5 (a): with every crypt_pkts state CLEAR, or with no connection KEYED, the keyed model is the unkeyed one."""
    b = lk.lattice()
    clear = [None if p is None else cm.CPkt(0, 0, cm.CLEAR, 0, 0xFF, 0) for p in b.cpkts]
    unkeyed = [c._replace(flags=c.flags & ~cm.F_KEYED) for c in b.crypt]
    for cpkts, crypt in ((clear, b.crypt), (b.cpkts, unkeyed)):
        c = b._replace(cpkts=cpkts, crypt=crypt)
        assert lk.model_follow(c)[1:] == tuple(lf.model(b)[1:])
        for max_updates in (0, 2):
            got, want = lk.model_span(c, max_updates)[1:], ls.model(b, max_updates)[1:]
            assert (got[0], got[1], got[2]) == (want[0], want[1], want[2])


def test_equality_b_span_stage_and_follow_stage():
    """Contract 5 (b): with max_updates 0 every field the keyed span records share with the keyed follow records equals it."""
    b = lk.lattice()
    follows, fpkts = lk.model_follow(b)[1:]
    spans, spkts = lk.model_span(b, 0)[1:3]
    for f, s in zip(follows, spans):
        assert (f is None) == (s is None)
        if f is not None:
            assert all(getattr(f, k) == getattr(s, k) for k in f._fields if k != "flags") and f.flags == s.flags & ~(ls.CAPPED | ls.REFUSED)
    for f, s in zip(fpkts, spkts):
        assert (f is None) == (s is None) and (f is None or all(getattr(f, k) == getattr(s, k) for k in f._fields))


@pytest.mark.parametrize("variant", sorted(lk.VARIANTS))
def test_the_lattice_tells_a_wrong_rule_from_the_right_one(variant):
    b = lk.lattice()
    rules = lk.Rules(**lk.VARIANTS[variant])
    right = lk.lattice_models()
    wrong_follow = lk.model_follow(b, rules)
    wrong_span = lk.model_span(b, 2, rules)
    assert wrong_follow[1:] != right["follow"][1:], variant
    assert wrong_span[1:] != right[2][1:], variant
    bad = [name for name, x, y in zip(b.names, wrong_span[1], right[2][1]) if x != y]
    assert bad, variant
    print(variant, "fails on", len(bad), "connections, the first:", bad[0])
