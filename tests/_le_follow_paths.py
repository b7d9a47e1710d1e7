"""A plain model of what DECIDES the path of LE following from CONNECT_IND (libbtbb_amd/csrc/le_follow.h), and the runs that drive
its paths.

The rules of the stage have their model in tests/_le_follow.py.  The kernels decompose the work by position: member `rank` of
connection g stands at SLOT first + rank and its event at EVENT position first + event of two tables of N entries; the mark, list
and step kernels take a scan tile of LT_TILE positions per workgroup, LE_THREADS at a time (a round), the tile sums go through a
prefix kernel; the listed updates -- in slot order, which is (connection, rank) order -- are sorted by I over six radix passes and
by the connection over one pass per byte of conn_cap, RADIX_SORT_TILE keys per workgroup; le_epoch_predict_kernel searches the
sorted list twice per event and tallies a connection's flags per wave of 64 event positions, one run of lanes per connection.  This
module ports that NUMBERING -- not the kernels -- from the model's own records, so that every path has a named tag:

* numbering(): every member's slot and event position; per position its tile, round, thread, wave and lane (place()); every
  listed update's index u and its place in the list sorted by (connection, I, rank); the sum of steps in front of every connection;
* TAGS: tag -> which byte of which record changes when that path is wrong; facts(): the tags a run carries, each a plain
  condition on the numbering;
* tests/test_le_follow_paths_model.py asserts on the CPU that the runs of RUNS carry the tags they were built for and all of TAGS
  between them, that lattice(), seam_world() and wrap_world() carry none of the five whose gap the new worlds close, and fails when a
  constant moves; tests/test_gpu_le_follow.py runs the same worlds on the device against the model, byte for byte.

Against the list the tags were asked by: update_at_thread_0_behind_one_in_its_ROUND cannot hold -- thread 0 is the first of its
round, its exclusive scan is 0 whatever the scan does --, what thread 0 does carry is the sum of the rounds in front of it
(`carry += sum`), so its tag asks for an update in an EARLIER ROUND OF ITS TILE.  The instant tags ask, beyond the order of the two
instants, that the two maps differ and that a predicted event lies at or behind the larger instant: without that no byte shows
which of the two stands behind the other.  last_predicted_at_lane_63_with_beyond_behind asks that the map in force there is not
the request's: `last_pred` is read for the verdict's map only.  Not tagged, because no byte of a world that fits a test shows them
(DESIGN 3.8.4): bytes 3 to 5 of an instant, a connection digit above byte 1, the epoch's saturation at 65 535.

The constants are read out of the sources by regular expression, each found exactly once.

What the worlds cost on the CPU (one core, one run, while the CPU suite ran beside it): crowd_world() 3.4 s to build (1 450
connections through the grouping's and the tracking's models) and 0.5 s for the follow model, its numbering and facts 0.1 s; its
three cuts 0.04 s at most through cut_model (2.7 to 3.0 s each through model_cut, which tracks the whole list again);
tally_world() and byte_world() 0.1 s each to build, their models under 0.01 s.
"""
import collections
import os
import re

import numpy as np

import _le_follow as lf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libbtbb_amd", "csrc")


def read_constants():
    """The numbers the numbering rests on, each found exactly once in its file."""
    k = {}
    for name, file in (("LE_THREADS", "le.hip"), ("LT_TILE", "le_track.h"), ("RADIX_SORT_TILE", "radix_sort.h")):
        with open(os.path.join(CSRC, file)) as f:
            found = re.findall(r"^#define\s+%s\s+(\d+)u?\b" % name, f.read(), re.M)
        assert len(found) == 1, "%s: #define %s found %d times" % (file, name, len(found))
        k[name] = int(found[0])
    return k


K = read_constants()
WAVE = 64
LE_THREADS, LT_TILE, RADIX_SORT_TILE = K["LE_THREADS"], K["LT_TILE"], K["RADIX_SORT_TILE"]
SCAN_THREADS = (WAVE - 1, WAVE, LE_THREADS - 1)                            # the last lane of wave 0, the first of wave 1, the last thread
MANY = LE_THREADS                                                          # "many connections": more than one workgroup's worth

# ---- the numbering ------------------------------------------------------------------------------------------------------------------
Place = collections.namedtuple("Place", "q tile round thread wave lane")
Update = collections.namedtuple("Update", "u q g rank instant map cand sorted_at")
Numbering = collections.namedtuple("Numbering", "n k conns seeds trace slot econn state epoch updates lo front n_events")


def place(q):
    """Where table position q lies: scan tile, round of the tile, thread of the workgroup, wave of the workgroup, lane."""
    thread = q % LE_THREADS
    return Place(int(q), int(q // LT_TILE), int(q % LT_TILE // LE_THREADS), int(thread), int(thread // WAVE), int(q % WAVE))


def numbering(b, seeds, fpkts, trace, n=None, k=None, pkts=None):
    """The tables of one run.  b: a Built; seeds, fpkts, trace: the model's on the n candidates and k connections the run works on
    (pkts: the tracking's records of that run, b.pkts when nothing is cut).
    slot[q] / econn[q]: the candidate at slot q, the connection whose event stands at event position q (-1: none); state[q], epoch[q]:
    of the event at q where its connection is seeded (-1 elsewhere); updates: the listed updates in slot order, each with its index
    u and its place in the list sorted by (connection, I, rank); lo[g]: the entries of connections below g in that list; front[g]:
    the sum of the steps in front of connection g modulo 2^64; n_events[g]."""
    n = len(b.cands) if n is None else n
    k = len(b.conns) if k is None else k
    pkts = b.pkts if pkts is None else pkts
    slot, econn = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    state, epoch = np.full(n, -1, np.int64), np.full(n, -1, np.int64)
    n_events = [0] * k
    instants = {}
    for g, t in trace.items():
        for at, _, chmap, i in t["ups"]:
            instants[i] = (at, chmap)
    ups = []
    for i in range(n):
        g, p = b.cands[i].channel, pkts[i]
        if p is None or g >= k:
            continue
        first = b.conns[g].first
        assert first < n and p.rank < n - first and p.event < n - first       # (the grouping's promise, which lf_member checks)
        slot[first + p.rank] = i
        econn[first + p.event] = g
        n_events[g] = max(n_events[g], p.event + 1)
        if seeds[g] is not None:
            state[first + p.event], epoch[first + p.event] = fpkts[i].state, fpkts[i].epoch
        if fpkts[i].kind == lf.MAP_UPDATE:
            ups.append((first + p.rank, g, p.rank, i))
    ups.sort()
    order = sorted(range(len(ups)), key=lambda u: (ups[u][1], instants[ups[u][3]][0], ups[u][2]))
    sorted_at = {u: j for j, u in enumerate(order)}
    updates = [Update(u, q, g, rank, instants[i][0], instants[i][1], i, sorted_at[u]) for u, (q, g, rank, i) in enumerate(ups)]
    lo, front, seen, total = [], [], 0, 0
    per = collections.Counter(x.g for x in updates)
    for g in range(k):
        lo.append(seen)
        front.append(total)
        seen += per.get(g, 0)
        if g in trace and trace[g]["cnt"]:
            total = (total + max(trace[g]["cnt"].values())) % (1 << 64)       # (c_f and the k_e behind it add up to the last counter)
    return Numbering(n, k, b.conns[:k], seeds, trace, slot, econn, state, epoch, updates, lo, front, n_events)


# ---- the tags -----------------------------------------------------------------------------------------------------------------------
# tag -> which byte of which record changes if that path is wrong
TAGS = {
    # compaction (le_epoch_mark_kernel, le_track_prefix_kernel, le_epoch_list_kernel)
    "update_behind_a_tile_with_updates": "the list index u starts from the tile prefix: without it two updates share an entry, and the epoch or "
                                         "`expected` of the events of the connection that lost its entry changes",
    "update_behind_an_empty_tile": "a tile sum of 0 between two others: a sum left unwritten or skipped by the prefix moves every u behind it; "
                                   "the same bytes",
    "updates_in_two_rounds_of_a_tile": "`carry += sum` between the rounds: the second round's updates land on the first's entries; the same bytes",
    "update_at_thread_0_behind_one_in_its_tile": "thread 0 takes the carry alone (its scan is 0): a carry that left out the round in front overwrites "
                                                 "that round's first entry; the same bytes",
    "update_at_thread_%d_behind_one_in_its_round" % SCAN_THREADS[0]: "the scan's last lane of wave 0: its u is off by the updates of its wave; the same bytes",
    "update_at_thread_%d_behind_one_in_its_round" % SCAN_THREADS[1]: "the first lane of wave 1 takes wave 0's total from LDS; the same bytes",
    "update_at_thread_%d_behind_one_in_its_round" % SCAN_THREADS[2]: "the last thread takes the totals of three waves and 63 lanes; the same bytes",
    "update_in_the_last_slot_of_a_ragged_list": "slot N - 1 of a list that ends inside a round: a bound taken per round or one too early drops the "
                                                "update -- `kind` of its packet, n_map_updates, the epochs behind its instant",
    "listed_beyond_one_radix_tile": "the radix passes run over U keys in more than one tile: a pass over one tile leaves the list's tail unsorted; "
                                    "epoch, `expected` and the record's map of the connections there",
    # sorts
    "instant_order_decided_by_byte_0": "two updates of a connection listed against their instants: the epoch of the events between the two instants "
                                       "and the map (`expected`, the record's map) behind the larger",
    "instant_order_decided_by_byte_1": "the same where the low byte orders them the wrong way round: only the pass over byte 1 sets them right",
    "instant_order_decided_by_byte_2": "the same where the low sixteen bits order them the wrong way round: only the pass over byte 2 does",
    "connection_order_decided_by_byte_1": "after the pass over the connection's low byte an entry of g2 stands in front of one of g1 < g2: the searches "
                                          "of both connections and of those between run over an unsorted list -- epoch, `expected`, the maps",
    "equal_instant_in_many_connections": "one digit value in every pass, in more than one radix tile: the scatter must keep (connection, rank) order "
                                         "within the value across the tiles, or equal instants of one connection change places -- the record's map",
    # search (lf_lower, lf_upper)
    "segment_first_in_list": "lo = 0 with a nonzero epoch: a search that cannot return 0 changes the epoch",
    "segment_last_in_list": "hi = U: a search that stops one short changes the epoch and the map of the last segment's events",
    "seeded_connection_without_updates_between_two_with": "lo = hi inside the list: epoch 0, the request's map; one entry taken from a neighbour "
                                                          "changes epoch and `expected`",
    "event_in_front_of_its_segment_behind_others": "epoch 0 although lo > 0: the map is the request's, not the entry in front of lo",
    "epoch_equals_segment_length": "hi is the first entry of the next connection: an upper bound that ignores the connection runs on into it",
    # counters (le_epoch_step_kernel, the 64-bit prefix)
    "conn_first_on_a_tile_seam": "the sum in front of the connection is the last entry of the tile in front: `counter` of every event",
    "connection_over_a_tile_seam": "the events behind the seam take the tile prefix: `counter`, and with it everything behind it",
    "sum_in_front_beyond_2^32": "the sum in front does not fit 32 bits: a prefix or a difference in 32 bits changes `counter`",
    "hole_in_front_of_a_seeded_connection": "position first - 1 is no event: it must still hold the running sum, or every `counter` of the connection is off",
    # tallies (le_epoch_predict_kernel)
    "run_head_at_lane_63": "the run is lane 63 alone: n_before / n_on / n_off / n_beyond of its connection lose or gain an event",
    "run_over_a_wave_seam": "lane 0 is a head although its connection began in the wave in front: the tallies lose the second wave's events",
    "wave_within_one_connection": "one head, no head behind it: the run is all 64 lanes",
    "sixteen_runs_in_a_wave": "each run ends in front of the next head: an event counted for its neighbour changes two connections' tallies",
    "before_and_counted_in_one_run": "two flags over one run: n_before and n_on + n_off of one connection",
    "beyond_and_counted_in_one_run": "the same for n_beyond",
    "unseeded_between_seeded_in_a_wave": "lanes without a live event belong to the run in front and hold no flag: a flag there changes its tallies",
    "holes_between_runs": "the same for positions that hold no event",
    "last_predicted_at_lane_63_with_beyond_behind": "lane 63 has no neighbour to ask: without its own test last_pred stays behind and the record's "
                                                    "map is the request's",
    "wave_without_a_live_lane": "no head in the wave: every tally returns early; an atomic there lands in connection 0's record",
    # verdict
    "map_of_last_predicted_not_of_last_event": "an update comes into force among the BEYOND events: the record's map is the one at the last PREDICTED event",
}
assert len(TAGS) == 34


def facts(nb):
    """The tags a run carries (nb: its Numbering)."""
    out = set()
    ups, U = nb.updates, len(nb.updates)
    # ---- compaction
    tiles = collections.defaultdict(lambda: collections.defaultdict(list))
    for x in ups:
        p = place(x.q)
        tiles[p.tile][p.round].append(p.thread)
    with_updates = sorted(tiles)
    if len(with_updates) >= 2:
        out.add("update_behind_a_tile_with_updates")
    if any(b - a >= 2 for a, b in zip(with_updates, with_updates[1:])):
        out.add("update_behind_an_empty_tile")
    for rounds in tiles.values():
        if len(rounds) >= 2:
            out.add("updates_in_two_rounds_of_a_tile")
        for r, threads in rounds.items():
            for s in SCAN_THREADS:
                if s in threads and min(threads) < s:
                    out.add("update_at_thread_%d_behind_one_in_its_round" % s)
            if 0 in threads and min(rounds) < r:
                out.add("update_at_thread_0_behind_one_in_its_tile")
    if U and ups[-1].q == nb.n - 1 and nb.n % LE_THREADS:
        out.add("update_in_the_last_slot_of_a_ragged_list")
    if U > RADIX_SORT_TILE:
        out.add("listed_beyond_one_radix_tile")
    # ---- sorts
    per = collections.defaultdict(list)
    for x in ups:
        per[x.g].append(x)
    for g, mine in per.items():
        t = nb.trace[g]
        predicted = [c for e, c in t["cnt"].items() if t["state"][e] == lf.ST_COUNTED]
        for j, a in enumerate(mine):
            for b in mine[j + 1:]:                                          # a is listed in front of b
                if a.instant > b.instant and a.map != b.map and predicted and max(predicted) >= a.instant:
                    byte = ((a.instant ^ b.instant).bit_length() - 1) // 8
                    low = (1 << (8 * byte)) - 1
                    if byte == 0 or (a.instant & low) < (b.instant & low):
                        out.add("instant_order_decided_by_byte_%d" % byte)
    gs = np.array(sorted(per), np.int64)
    if len(gs):
        least = np.array([min(x.instant for x in per[g]) for g in gs], np.float64)
        most = np.array([max(x.instant for x in per[g]) for g in gs], np.float64)
        for j in range(len(gs)):                                            # g1 = gs[j] < g2
            behind = slice(j + 1, None)
            if (((gs[j] & 255) > (gs[behind] & 255)) & (least[behind] < most[j])).any():
                out.add("connection_order_decided_by_byte_1")
                break
    by_instant = collections.defaultdict(list)
    for x in ups:
        by_instant[x.instant].append(x)
    for xs in by_instant.values():
        if len({x.g for x in xs}) >= MANY and len({x.u // RADIX_SORT_TILE for x in xs}) >= 2:
            out.add("equal_instant_in_many_connections")
    # ---- search and counters
    for g, t in nb.trace.items():
        first, cnt = nb.conns[g].first, t["cnt"]
        if not cnt:
            continue
        mine = sorted(x.instant for x in per.get(g, ()))
        lo = nb.lo[g]
        for c in cnt.values():
            ep = sum(at <= c for at in mine)
            if mine and lo == 0 and ep:
                out.add("segment_first_in_list")
            if mine and lo + ep == U and ep:
                out.add("segment_last_in_list")
            if not mine and 0 < lo < U:
                out.add("seeded_connection_without_updates_between_two_with")
            if mine and ep == 0 and lo > 0:
                out.add("event_in_front_of_its_segment_behind_others")
            if mine and ep == len(mine) and lo + ep < U:
                out.add("epoch_equals_segment_length")
        front = nb.front[g]
        if first > 0 and first % LT_TILE == 0 and front:
            out.add("conn_first_on_a_tile_seam")
        at = sorted((first + e, c) for e, c in cnt.items())
        if any(q0 // LT_TILE != q1 // LT_TILE and c1 > c0 for (q0, c0), (q1, c1) in zip(at, at[1:])):
            out.add("connection_over_a_tile_seam")
        if front >= 1 << 32:
            out.add("sum_in_front_beyond_2^32")
        if front and first > 0 and nb.econn[first - 1] < 0 and g > 0:
            c = nb.conns[g - 1]
            if c.first + nb.n_events[g - 1] <= first - 1 < c.first + c.n_packets:
                out.add("hole_in_front_of_a_seeded_connection")
        # ---- the last predicted event
        predicted = sorted(e for e in cnt if t["state"][e] == lf.ST_COUNTED)
        if predicted:
            last, q = predicted[-1], first + predicted[-1]
            if t["in_force"][last] != t["in_force"][max(cnt)]:
                out.add("map_of_last_predicted_not_of_last_event")
            if q % WAVE == WAVE - 1 and t["state"].get(last + 1) == lf.ST_BEYOND and t["in_force"][last] != nb.seeds[g].map:
                out.add("last_predicted_at_lane_63_with_beyond_behind")
    # ---- tallies: wave by wave
    for w0 in range(0, nb.n, WAVE):
        g = np.full(WAVE, -1, np.int64)
        st = np.full(WAVE, -1, np.int64)
        m = min(WAVE, nb.n - w0)
        g[:m], st[:m] = nb.econn[w0:w0 + m], nb.state[w0:w0 + m]
        live = st >= 0
        heads = [ln for ln in range(WAVE) if live[ln] and (ln == 0 or g[ln - 1] != g[ln])]
        if not heads:
            if (g >= 0).any():
                out.add("wave_without_a_live_lane")
            continue
        if len(heads) >= 16:
            out.add("sixteen_runs_in_a_wave")
        if live.all() and len(set(g.tolist())) == 1:
            out.add("wave_within_one_connection")
        if heads[-1] == WAVE - 1:
            out.add("run_head_at_lane_63")
        if w0 and live[0] and nb.state[w0 - 1] >= 0 and nb.econn[w0 - 1] == g[0]:
            out.add("run_over_a_wave_seam")
        for h, end in zip(heads, heads[1:] + [WAVE]):
            states = set(st[h:end][live[h:end]].tolist())
            if {lf.ST_BEFORE, lf.ST_COUNTED} <= states:
                out.add("before_and_counted_in_one_run")
            if {lf.ST_BEYOND, lf.ST_COUNTED} <= states:
                out.add("beyond_and_counted_in_one_run")
            if end < WAVE:                                                  # (a run behind it)
                if (~live[h:end] & (g[h:end] >= 0)).any():
                    out.add("unseeded_between_seeded_in_a_wave")
                if (g[h:end] < 0).any():
                    out.add("holes_between_runs")
    return out & set(TAGS)


# ---- the runs ---------------------------------------------------------------------------------------------------------------------
COMPACTION = frozenset(t for t in TAGS if t.startswith("update")) - {"update_in_the_last_slot_of_a_ragged_list"}
SEARCH = frozenset({"segment_first_in_list", "segment_last_in_list", "seeded_connection_without_updates_between_two_with",
                    "event_in_front_of_its_segment_behind_others", "epoch_equals_segment_length"})
TALLIES = frozenset({"run_head_at_lane_63", "run_over_a_wave_seam", "wave_within_one_connection", "sixteen_runs_in_a_wave",
                     "before_and_counted_in_one_run", "beyond_and_counted_in_one_run", "unseeded_between_seeded_in_a_wave", "holes_between_runs",
                     "last_predicted_at_lane_63_with_beyond_behind", "wave_without_a_live_lane"})
# name; the world of tests/_le_follow.py; the cut ("count": see ragged_count); the tags it was built for
Run = collections.namedtuple("Run", "name world cut tags")
RUNS = (
    Run("crowd", "crowd", None, COMPACTION | SEARCH | {"listed_beyond_one_radix_tile", "instant_order_decided_by_byte_0", "connection_order_decided_by_byte_1",
                                                        "equal_instant_in_many_connections", "conn_first_on_a_tile_seam", "connection_over_a_tile_seam",
                                                        "hole_in_front_of_a_seeded_connection"}),
    Run("crowd, count cut", "crowd", "count", {"update_in_the_last_slot_of_a_ragged_list", "listed_beyond_one_radix_tile"}),
    Run("bytes", "byte", None, {"instant_order_decided_by_byte_1", "instant_order_decided_by_byte_2"}),
    Run("tallies", "tally", None, TALLIES | {"sum_in_front_beyond_2^32", "map_of_last_predicted_not_of_last_event"}),
)
OLD_WORLDS_LACK = ("update_behind_a_tile_with_updates", "update_behind_an_empty_tile", "listed_beyond_one_radix_tile",
                   "connection_order_decided_by_byte_1", "instant_order_decided_by_byte_2")


def world(name):
    """(Built, (seeds, follows, fpkts, trace)) of a world of tests/_le_follow.py."""
    return getattr(lf, name + "_world")(), getattr(lf, name + "_model")()


def ragged_count(b, full):
    """The largest count that is no multiple of LE_THREADS, cuts a connection's candidates short and leaves a map update PDU as the
    last of them in time: its slot is N - 1.  (That the update is valid there too is for the cut's own model to say: facts().)"""
    for c in reversed(b.conns):
        for m in range(c.n_packets - 1, 1, -1):
            n = c.first + m
            last = max(range(c.first, n), key=lambda i: (b.cands[i].offset, b.cands[i].stream, i))
            if n % LE_THREADS and full[2][last] is not None and full[2][last].kind == lf.MAP_UPDATE:
                return n
    raise AssertionError("no such count")


_CARRIED = {}


def run_numbering(run):
    b, full = world(run.world)
    if run.cut is None:
        return numbering(b, full[0], full[2], full[3])
    n = ragged_count(b, full)
    pkts, seeds, _, fpkts, trace = lf.cut_model(b, full, full[3], work=n)
    return numbering(b, seeds, fpkts, trace, n=n, pkts=pkts)


def run_tags(run):
    """The tags a run carries (worked out once)."""
    if run.name not in _CARRIED:
        _CARRIED[run.name] = frozenset(facts(run_numbering(run)))
    return _CARRIED[run.name]
