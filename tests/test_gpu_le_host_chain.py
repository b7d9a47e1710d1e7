"""The host wrappers of the six LE stages (libbtbb_amd/csrc/le_host.h) against each other: they share one chain -- discovery, tracking,
copy-out, the fill when no connection was stored --, so on one capture with the same arguments they agree in everything they have in
common, they all take the same way out when nothing is stored, and a call leaves nothing behind that a later call on the same thread
could read.  What each stage computes is checked against the models in its own module; here the capture is tests/_le_span.py's, the
smallest one planted for a host wrapper (three connections, 40 streams of 4 600 words)."""
import re

import numpy as np
import pytest

import libbtbb_amd as bt
import _le_span as ls

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _init():
    import torch                                             # (a torch that does not import fails these tests, it does not skip them)
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    bt.init(2)


@pytest.fixture(scope="module")
def cap():
    return ls.span_capture()[0]


def _kw(cap, **more):
    kw = dict(max_len=27, min_count=2, n_streams=len(cap.mhz), pitch_words=cap.pitch_words, n_words=cap.n_words)
    kw.update(more)
    return kw


TIMING = dict(unit_bits=1250, ifs_bits=200, jitter_bits=50)
# name -> (the call, its keywords beyond the discovery's, the positions of its per-candidate arrays beyond cands)
WRAPPERS = {
    "discover": (bt.le_discover, {}, ()),
    "track": (bt.le_track, TIMING, (3,)),
    "csa2": (bt.le_csa2, TIMING, (3, 5)),
    "epoch": (bt.le_follow, TIMING, (3, 6)),
    "span0": (bt.le_span, dict(TIMING, max_updates=0), (3, 6)),
    "span4": (bt.le_span, dict(TIMING, max_updates=4), (3, 6)),
    "data": (bt.le_data, TIMING, (3, 5)),
}


def _call(cap, name, **more):
    fn, own, _ = WRAPPERS[name]
    return fn(cap.words, cap.search_bits, cap.mhz, **_kw(cap, **dict(own, **more)))


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def alone(cap):
    """every wrapper called once, on its own"""
    return {name: _call(cap, name) for name in WRAPPERS}


def test_the_wrappers_agree_in_what_they_share(alone):
    conns, cands = alone["discover"]
    assert len(conns) == 3 and len(cands) > len(conns)
    for name, got in alone.items():                          # (the lengths are the return value and n_cands)
        assert _same(got[0], conns) and _same(got[1], cands), name
    tracks, pkts = alone["track"][2:4]
    assert (pkts["rank"] != 0xFFFFFFFF).any()
    for name in ("csa2", "epoch", "span0", "span4", "data"):
        assert _same(alone[name][2], tracks) and _same(alone[name][3], pkts), name
    seeds = alone["epoch"][4]
    assert len(seeds) == 3 and _same(alone["span0"][4], seeds) and _same(alone["span4"][4], seeds)


def _counts_refused(cap, name, **more):
    """(connections found, candidates found) as the wrapper returned them, read from the refusal of buffers that are too small"""
    with pytest.raises(bt.BtbbError) as e:
        _call(cap, name, **more)
    m = re.search(r"(\d+) connections > \d+,? (?:or )?(\d+) candidates > \d+", str(e.value))
    assert m, str(e.value)
    return int(m.group(1)), int(m.group(2))


@pytest.mark.parametrize("how", ["min_count", "conn_cap"])
def test_no_connection_stored(cap, alone, how):
    more = dict(min_count=1000) if how == "min_count" else dict(conn_cap=0, truncate=True)
    conns, cands = _call(cap, "discover", **more)
    assert len(conns) == 0 and len(cands) == len(alone["discover"][1])
    if how == "conn_cap":                                    # three connections are found, none can be stored
        assert _counts_refused(cap, "discover", conn_cap=0) == (3, len(cands))
    for name, (_, _, per_cand) in WRAPPERS.items():
        got = _call(cap, name, **more)
        assert len(got[0]) == 0 and _same(got[1], cands), name
        if how == "conn_cap":
            assert _counts_refused(cap, name, conn_cap=0) == (3, len(cands)), name
        for at in per_cand:
            assert len(got[at]) == len(cands) and got[at].tobytes() == b"\xff" * (len(cands) * got[at].dtype.itemsize), (name, at)
        for at in range(2, len(got)):                        # and nothing per connection, no message, no octet
            assert at in per_cand or len(got[at]) == 0, (name, at)


def test_back_to_back_calls_on_one_thread_equal_the_calls_alone(cap, alone):
    small = dict(msg_cap=2, byte_cap=16, truncate=True)
    data_alone = _call(cap, "data", **small)
    assert len(data_alone[6]) <= 2 and len(data_alone[7]) <= 16
    runs = [("span4", {}, alone["span4"]), ("epoch", {}, alone["epoch"]), ("data", small, data_alone), ("span0", {}, alone["span0"])]
    for name, more, want in runs:
        got = _call(cap, name, **more)
        assert len(got) == len(want)
        for at, (g, w) in enumerate(zip(got, want)):
            assert _same(g, w), (name, at)
