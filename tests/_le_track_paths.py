"""A plain model of what DECIDES the path of the LE connection tracking (libbtbb_amd/csrc/le_track.h), and the runs that drive
its paths.

The rules of the tracking have their model in tests/_le_track.py.  The kernels decompose the work by position: a wave of 64 slots
or events, a workgroup of LE_THREADS, a score tile of LT_SCORE_TILE events, a scan tile of LT_TILE slots or events, rounds of
LE_THREADS tiles in the tile prefix, one radix pass per eight bits of the connection capacity.  Which of these a list drives
follows from where its connections begin: the tracking lays the slots (the members in time order) and the events of connection 0,
1, 2 ... back to back, non-members behind them, so the model's own records (rank and event of every packet, the events of every
connection) give every slot and event number.  This module ports that numbering and the branch conditions -- not the kernels --
so that

* every path has a NAMED tag, and a tag holds only where the path runs with a value that a mistake would change (its
  sensitivity condition, in TAGS below);
* tests/test_le_track_paths_model.py asserts on the CPU that the runs of RUNS carry the tags they were built for, and all of
  TAGS between them, and fails when a constant of the headers moves;
* tests/test_gpu_le_track.py runs the same RUNS on the device against the model, byte for byte.

The constants are read out of the sources by regular expression, each found exactly once.
"""
import collections
import functools
import math
import os
import re

import numpy as np

import _le_track as lt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libbtbb_amd", "csrc")


def read_constants():
    """The numbers the model rests on, each found exactly once in its file."""
    k = {}
    for name, file in (("LT_TILE", "le_track.h"), ("LT_SCORE_TILE", "le_track.h"), ("RADIX_SORT_TILE", "radix_sort.h"), ("LE_THREADS", "le.hip")):
        with open(os.path.join(CSRC, file)) as f:
            found = re.findall(r"^#define\s+%s\s+(\d+)u?\b" % name, f.read(), re.M)
        assert len(found) == 1, "%s: #define %s found %d times" % (file, name, len(found))
        k[name] = int(found[0])
    return k


K = read_constants()
WAVE = 64
LT_TILE, LT_SCORE_TILE, RADIX_SORT_TILE, LE_THREADS = K["LT_TILE"], K["LT_SCORE_TILE"], K["RADIX_SORT_TILE"], K["LE_THREADS"]
UNITS = (("wave", WAVE), ("workgroup", LE_THREADS), ("score_tile", LT_SCORE_TILE), ("scan_tile", LT_TILE))
PREFIX_ROUND = LE_THREADS                  # tiles per round of le_track_prefix_kernel / le_track_prefix64_kernel
THREE_PASSES = 1 << 16                     # connection capacities from here on sort the connection index in three radix passes
LARGE_IN_TILE = 200

# tag -> when it holds
TAGS = {
    "off_hop_wave_uniform": "a wave of 64 slots of one connection holds >= 2 slots that open an event off the hop, and a second packet of such an event",
    "off_hop_wave_mixed": "a wave of slots of several connections, of non-members or of the list's tail holds a slot that opens an event off the hop",
    "off_hop_unknown": "flags 0: an event whose unmapped channel is unused, neither on nor off the hop",
    "gcd_needs_every_wave": "a connection's fitting pairs lie in >= 3 waves of pairs, and every two of these waves have a gcd above the interval",
    "gcd_pair_at_lane_63": "the pair whose first event is at lane 63 is the only one that brings its connection's gcd down to the interval",
    "gcd_pair_at_thread_255": "the same for the pair at the last thread of a workgroup",
    "gcd_wave_of_several": "a wave of pairs holds fitting pairs of >= 3 connections, one of them with a gcd that is not the smallest of its q",
    "score_one_remap": "REMAP: a whole score tile inside one TIMED connection whose map has <= 36 channels",
    "score_tile_of_two_large": "a score tile holds >= 200 events each of two TIMED connections",
    "events_end_on_score_tile": "the number of events is a multiple of LT_SCORE_TILE",
    "events_end_one_past": "the number of events is one more than a multiple of LT_SCORE_TILE",
    "slots_decoupled": "a connection begins at another lane as a slot than as an event",
    "sum_beyond_32_bits_crosses_tile": "the step sum that enters a scan tile is >= 2^32, and a connection that begins in or behind that tile straddles a scan tile boundary",
    "prefix_second_round": "more than 256 scan tiles hold slots, and a tile beyond the 256th opens an event",
    "tile_opens_no_event": "a whole scan tile of member slots opens no event",
    "conn_index_three_passes": "conn_cap >= 65536",
    "conn_index_third_byte": "members of a connection with an index >= 65536 lie, in time, between those of the connection 65536 below it",
    "non_members_behind": "candidates that are no members follow the last member slot in its wave",
}
for _side in ("begins", "ends"):
    for _unit, _ in UNITS:
        for _at, _what in (("", "on"), ("_plus_1", "one behind"), ("_minus_1", "one before")):
            TAGS["conn_%s_at_%s%s" % (_side, _unit, _at)] = "a connection %s %s a multiple of a %s of events" % (_side, _what, _unit)
assert len(TAGS) == 18 + 24

Numbering = collections.namedtuple("Numbering", "n n_members slot0 ev0 ev1 s_conn s_event s_open s_off e_conn anchor")


def numbering(cands, n_conns, tracks, pkts):
    """Slot and event numbers as the kernels have them, from the model's records of the candidates worked on.
    slot0 / ev0 / ev1 per connection; per slot its connection, event (numbered through all connections), whether it opens the event
    and whether that event is off the hop; per event its connection and anchor."""
    n_mem = [0] * n_conns
    for c, p in zip(cands, pkts):
        if p is not None:
            n_mem[c.channel] += 1
    slot0 = np.concatenate([[0], np.cumsum(n_mem)]).astype(np.int64)
    ev0 = np.concatenate([[0], np.cumsum([t.n_events for t in tracks])]).astype(np.int64)
    n_members, n_events = int(slot0[-1]), int(ev0[-1])
    s_conn = np.full(n_members, -1, np.int64)
    s_event = np.zeros(n_members, np.int64)
    s_offset = np.zeros(n_members, np.int64)
    s_off = np.zeros(n_members, bool)
    for c, p in zip(cands, pkts):
        if p is not None:
            j = slot0[c.channel] + p.rank
            assert s_conn[j] == -1                               # (ranks are a permutation of a connection's members)
            s_conn[j], s_event[j], s_offset[j] = c.channel, ev0[c.channel] + p.event, c.offset
            s_off[j] = tracks[c.channel].flags & lt.TIMED and p.expected != 0xFF and not p.on_hop
    assert (s_conn >= 0).all() and (np.diff(s_conn) >= 0).all() and (np.diff(s_event) >= 0).all() and (np.diff(s_event) <= 1).all()
    s_open = np.concatenate([[True], np.diff(s_event) == 1]) if n_members else np.zeros(0, bool)
    assert int(s_open.sum()) == n_events
    return Numbering(len(cands), n_members, slot0[:-1], ev0[:-1], ev0[1:], s_conn, s_event, s_open, s_off & s_open, s_conn[s_open], s_offset[s_open])


def _gcd(values):
    return functools.reduce(math.gcd, values)


def tags(cands, n_conns, tracks, pkts, flags, unit=lt.UNIT, jitter=lt.JITTER, conn_cap=None):
    """The tags a run carries.  cands: the candidates worked on (cut to the count and the capacity), tracks and pkts: the model's."""
    nb = numbering(cands, n_conns, tracks, pkts)
    out = set()
    n_events = len(nb.e_conn)
    timed = np.array([bool(t.flags & lt.TIMED) for t in tracks], bool)
    # ---- le_track_pkt_kernel: waves of slots; non-members (-2) behind the members, the tail of the last wave (-3)
    lanes = np.concatenate([nb.s_conn, np.full(nb.n - nb.n_members, -2), np.full(-nb.n % WAVE, -3)]).reshape(-1, WAVE)
    off = np.concatenate([nb.s_off, np.zeros(lanes.size - nb.n_members, bool)]).reshape(-1, WAVE)
    uniform = (lanes == lanes[:, :1]).all(axis=1) & (lanes[:, 0] >= 0)
    if (off.any(axis=1) & ~uniform).any():
        out.add("off_hop_wave_mixed")
    opener = np.flatnonzero(nb.s_open)                                      # event -> its first slot
    j = np.arange(nb.n_members)
    second = ~nb.s_open & nb.s_off[opener[nb.s_event]] & (opener[nb.s_event] // WAVE == j // WAVE)
    second = np.concatenate([second, np.zeros(lanes.size - nb.n_members, bool)]).reshape(-1, WAVE)
    if (uniform & (off.sum(axis=1) >= 2) & second.any(axis=1)).any():
        out.add("off_hop_wave_uniform")
    if not flags & lt.REMAP and any(p is not None and p.unmapped != 0xFF and p.expected == 0xFF for p in pkts):
        out.add("off_hop_unknown")
    if nb.n_members % WAVE and nb.n > nb.n_members:
        out.add("non_members_behind")
    # ---- le_track_interval_kernel: q of every fitting pair (e, e + 1)
    per_wave = collections.defaultdict(dict)                                # wave of pairs -> connection -> [q]
    for g in range(n_conns):
        a = [int(x) for x in nb.anchor[nb.ev0[g]:nb.ev1[g]]]
        fit = []
        for i in range(len(a) - 1):
            d = a[i + 1] - a[i]
            q = (d + unit // 2) // unit
            if q >= 1 and abs(d - q * unit) <= jitter:
                fit.append((int(nb.ev0[g]) + i, q))
        assert len(fit) == tracks[g].n_fit
        if not fit:
            continue
        whole = _gcd(q for _, q in fit)
        assert min(whole, 0xFFFFFFFF) == tracks[g].interval
        waves = collections.defaultdict(list)
        for e, q in fit:
            waves[e // WAVE].append(q)
            per_wave[e // WAVE].setdefault(g, []).append(q)
        of_wave = [_gcd(v) for v in waves.values()]
        if len(of_wave) >= 3 and all(math.gcd(x, y) > whole for i, x in enumerate(of_wave) for y in of_wave[i + 1:]):
            out.add("gcd_needs_every_wave")
        for i, (e, q) in enumerate(fit):
            if e % WAVE == WAVE - 1 and len(fit) > 1 and _gcd(x for k, (_, x) in enumerate(fit) if k != i) > whole:
                out.add("gcd_pair_at_lane_63")
                if e % LE_THREADS == LE_THREADS - 1:
                    out.add("gcd_pair_at_thread_255")
    if any(len(v) >= 3 and any(_gcd(q) != min(q) for q in v.values()) for v in per_wave.values()):
        out.add("gcd_wave_of_several")
    # ---- where connections begin and end
    for g in range(n_conns):
        if nb.ev1[g] == nb.ev0[g]:
            continue
        for name, u in UNITS:
            for side, at in (("begins", int(nb.ev0[g])), ("ends", int(nb.ev1[g]))):
                if side == "begins" and at == 0:
                    continue                                                # (nothing in front of it)
                for rest, suffix in ((0, ""), (1, "_plus_1"), (u - 1, "_minus_1")):
                    if at % u == rest:
                        out.add("conn_%s_at_%s%s" % (side, name, suffix))
        if nb.slot0[g] % WAVE != nb.ev0[g] % WAVE:
            out.add("slots_decoupled")
    # ---- le_track_score_kernel
    for g in range(n_conns):
        first_tile = -(-int(nb.ev0[g]) // LT_SCORE_TILE)
        if flags & lt.REMAP and timed[g] and tracks[g].n_used <= 36 and (first_tile + 1) * LT_SCORE_TILE <= nb.ev1[g]:
            out.add("score_one_remap")
    if n_events:
        pair, count = np.unique(np.stack([np.arange(n_events) // LT_SCORE_TILE, nb.e_conn]), axis=1, return_counts=True)
        large = pair[0][(count >= LARGE_IN_TILE) & timed[pair[1]]]
        if len(np.unique(large)) < len(large):
            out.add("score_tile_of_two_large")
        if n_events % LT_SCORE_TILE == 0:
            out.add("events_end_on_score_tile")
        if n_events % LT_SCORE_TILE == 1:
            out.add("events_end_one_past")
    # ---- the 64-bit step sums: the k of every pair of a TIMED connection, as rule 5 has it
    step = [0] * n_events
    for g in range(n_conns):
        if timed[g]:
            a = [int(x) for x in nb.anchor[nb.ev0[g]:nb.ev1[g]]]
            p = tracks[g].interval * unit
            for i in range(1, len(a)):
                step[nb.ev0[g] + i] = (a[i] - a[i - 1] + p // 2) // p
    total, entering = 0, []
    for e in range(n_events):
        if e % LT_TILE == 0:
            entering.append(total)
        total += step[e]
    beyond = [t for t, s in enumerate(entering) if s >= 1 << 32]
    if beyond and any(nb.ev0[g] >= beyond[0] * LT_TILE and nb.ev1[g] > nb.ev0[g] and nb.ev0[g] // LT_TILE != (nb.ev1[g] - 1) // LT_TILE
                      for g in range(n_conns)):
        out.add("sum_beyond_32_bits_crosses_tile")
    # ---- the tiles of slots
    opens = np.add.reduceat(nb.s_open.astype(np.int64), np.arange(0, nb.n_members, LT_TILE)) if nb.n_members else np.zeros(0, np.int64)
    if -(-nb.n // LT_TILE) > PREFIX_ROUND and opens[PREFIX_ROUND:].any():
        out.add("prefix_second_round")
    if (opens[:nb.n_members // LT_TILE] == 0).any():
        out.add("tile_opens_no_event")
    if (n_conns if conn_cap is None else conn_cap) >= THREE_PASSES:
        out.add("conn_index_three_passes")
        for g in range(THREE_PASSES, min(n_conns, conn_cap or n_conns)):
            mine, below = nb.anchor[nb.ev0[g]:nb.ev1[g]], nb.anchor[nb.ev0[g - THREE_PASSES]:nb.ev1[g - THREE_PASSES]]
            if len(mine) and len(below) and ((mine > below.min()) & (mine < below.max())).any():
                out.add("conn_index_third_byte")
    assert out <= set(TAGS)
    return out


# ---- the runs ---------------------------------------------------------------------------------------------------------------------
BOUNDARIES = frozenset(t for t in TAGS if t.startswith(("conn_begins_", "conn_ends_")))
ALIGN = BOUNDARIES | {"off_hop_wave_uniform", "off_hop_wave_mixed", "gcd_needs_every_wave", "gcd_pair_at_lane_63", "gcd_pair_at_thread_255",
                      "gcd_wave_of_several", "score_tile_of_two_large", "slots_decoupled", "sum_beyond_32_bits_crosses_tile", "non_members_behind"}

# name; the list (a builder of tests/_le_track.py and its argument); flags; what the call differs in from (count, cand_cap, conn_cap) =
# (length, length, connections): numbers, or "cut" for a count that ends mid-wave inside the "off hop" connection; the tags it exists for
Run = collections.namedtuple("Run", "name build arg flags kw tags")
RUNS = (
    Run("align A", "align_list", "A", 0, {}, ALIGN | {"off_hop_unknown", "events_end_on_score_tile"}),
    Run("align A, REMAP", "align_list", "A", lt.REMAP, {}, ALIGN | {"score_one_remap", "events_end_on_score_tile"}),
    Run("align B", "align_list", "B", 0, {}, ALIGN | {"off_hop_unknown", "events_end_one_past"}),
    Run("align B, REMAP", "align_list", "B", lt.REMAP, {}, ALIGN | {"score_one_remap", "events_end_one_past"}),
    Run("align A, three passes", "align_list", "A", lt.REMAP, dict(conn_cap=70000), ALIGN | {"conn_index_three_passes"}),
    Run("align A, zeros behind", "align_list", "A", lt.REMAP, dict(cand_cap=600000), ALIGN),
    Run("align A, cut", "align_list", "A", lt.REMAP, dict(count="cut"), {"off_hop_wave_mixed", "slots_decoupled"}),
    Run("crowd", "crowd_list", None, lt.REMAP, {}, {"conn_index_three_passes", "conn_index_third_byte", "non_members_behind"}),
    Run("long events", "long_event_list", None, lt.REMAP, {}, {"prefix_second_round", "tile_opens_no_event", "non_members_behind"}),
)


def run_list(run):
    """(conns, cands, names) of a run, whole."""
    return (getattr(lt, run.build)(run.arg) if run.arg is not None else getattr(lt, run.build)())[:3]


def cut_count(conns, cands, names):
    """A count that ends inside the candidates of the "off hop" connection (a connection's candidates stand in (stream, offset)
    order: the cut takes its upper channels away) and leaves a number of members that is no multiple of 64."""
    g = names.index("off hop")
    count = conns[g].first + (conns[g].n_packets * 7 // 10)
    while sum(c.channel != 0xFFFFFFFF for c in cands[:count]) % WAVE < 8:
        count += 1
    assert conns[g].first < count < conns[g].first + conns[g].n_packets
    return count


def run_kw(run):
    """The keyword arguments of the device call of a run."""
    kw = dict(run.kw)
    if kw.get("count") == "cut":
        kw["count"] = cut_count(*run_list(run))
    return kw


@functools.lru_cache(maxsize=None)
def _model(build, arg, flags, count):
    conns, cands, _ = run_list(Run(None, build, arg, flags, {}, ()))
    return lt.track(cands[:count], len(conns), lt.LATTICE_MHZ, lt.N_STREAMS, lt.UNIT, lt.IFS, lt.JITTER, flags)


def run_model(run):
    """The model's (tracks, pkts) of the candidates a run works on (shared between the runs on one list)."""
    return _model(run.build, run.arg, run.flags, run_kw(run).get("count"))


_TAGS_OF = {}


def run_tags(run):
    """The tags a run carries (worked out once)."""
    if run.name not in _TAGS_OF:
        conns, cands, _ = run_list(run)
        kw = run_kw(run)
        tracks, pkts = run_model(run)
        _TAGS_OF[run.name] = frozenset(tags(cands[:kw.get("count")], len(conns), tracks, pkts, run.flags, conn_cap=kw.get("conn_cap")))
    return _TAGS_OF[run.name]
