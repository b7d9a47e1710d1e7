"""A plain model of what DECIDES the path of the LE channel selection #2 stage (libbtbb_amd/csrc/le_csa2.h), and the runs that
drive its paths.

The six rules of the stage have their model in tests/_le_csa2.py.  The kernels decompose the work by position: a connection's
events come through LDS in tiles of LC_TILE; within a tile an event is NEAR (looked up in a window of 1024 + span tabulated
counters, span cut at LC_SPAN) or FAR (evaluated directly, by a second loop); the 65 536 hypotheses are LC_BLOCKS blocks of
LE_THREADS threads of LC_PER_LANE registers, folded in the lane, across the wave, across the waves of the block and, in the
verdict, across the blocks; the verdict's wave walks the events once more, 64 at a time.  This module ports that numbering and the
branch conditions -- not the kernels -- so that every path has a NAMED tag.

Of the 65 536 scores of a connection the record shows three things: the largest (n_on), where it lies (counter0) and the second
largest (n_second).  A wrong score of a losing hypothesis changes no byte.  So a tag holds only where the WINNER or the RUNNER-UP
lies where the path computes -- their locations come from lc.scores_np, the model's records hold only the scores -- and where the
event in question lies on that hypothesis' prediction: n_on and n_second are bytes of the record, so one event counted too few or
too often there shows, whatever the margin between the two is.  Where a tag speaks of a margin (far_decides, second_only_in_tile_two)
the path's contribution is more than one event and the tag asks that without it another hypothesis would take the place.

* TAGS: tag -> (when it holds, the facts it needs); facts(): the facts a run carries, each a plain condition on the numbering;
* tests/test_le_csa2_paths_model.py asserts on the CPU that the runs of RUNS carry the tags they were built for, and all of TAGS
  between them, that the older lists do not carry the tags whose gap the new ones close, and fails when a constant moves;
* tests/test_gpu_le_csa2.py runs the same RUNS on the device against the model, byte for byte.

The constants are read out of the sources by regular expression, each found exactly once.
"""
import collections
import os
import re

import numpy as np

import _le_csa2 as lc
import _le_track as lt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libbtbb_amd", "csrc")


def read_constants():
    """The numbers the model rests on, each found exactly once in its file (LC_BASE_ROUND as a multiple of LE_THREADS)."""
    k = {}
    for name, file, value in (("LC_BLOCKS", "le_csa2.h", r"(\d+)u?"), ("LC_PER_LANE", "le_csa2.h", r"(\d+)u?"), ("LC_TILE", "le_csa2.h", r"(\d+)u?"),
                              ("LC_SPAN", "le_csa2.h", r"(\d+)u?"), ("LC_BASE_ROUND", "le_csa2.h", r"\((\d+)u? \* LE_THREADS\)"),
                              ("LE_THREADS", "le.hip", r"(\d+)u?")):
        with open(os.path.join(CSRC, file)) as f:
            found = re.findall(r"^#define\s+%s\s+%s(?=\s)" % (name, value), f.read(), re.M)
        assert len(found) == 1, "%s: #define %s found %d times" % (file, name, len(found))
        k[name] = int(found[0])
    k["LC_BASE_ROUND"] *= k["LE_THREADS"]
    return k


K = read_constants()
WAVE = 64
LC_BLOCKS, LC_PER_LANE, LC_TILE, LC_SPAN, LC_BASE_ROUND, LE_THREADS = (K[n] for n in ("LC_BLOCKS", "LC_PER_LANE", "LC_TILE", "LC_SPAN", "LC_BASE_ROUND",
                                                                                     "LE_THREADS"))
PER_BLOCK = LC_PER_LANE * LE_THREADS
LAST_J, LAST_THREAD, N_WAVES = PER_BLOCK - 1, LE_THREADS - 1, LE_THREADS // WAVE
SEAM_THREADS = (0, WAVE - 1, WAVE, LAST_THREAD)
COUNTS = (LC_TILE - 1, LC_TILE, LC_TILE + 1, 2 * LC_TILE, 2 * LC_TILE + 1)
OFF_AT = (WAVE - 1, WAVE, LC_TILE - 1, LC_TILE, LC_TILE + 1)

# ---- the numbering ------------------------------------------------------------------------------------------------------------------
Place = collections.namedtuple("Place", "c0 block j thread wave lane r")
Tile = collections.namedtuple("Tile", "t0 m n_first d_last span d near pad")


def place(c0):
    """Where le_csa2_score_kernel computes S(c0): work item block, the hypothesis' number j in the block, thread, wave, lane and
    register."""
    j = c0 % PER_BLOCK
    thread = j // LC_PER_LANE
    return Place(int(c0), int(c0) // PER_BLOCK, int(j), int(thread), int(thread // WAVE), int(thread % WAVE), int(j % LC_PER_LANE))


def tiles(n16):
    """The tiles of a connection's events (n16: n_e mod 2^16 in event order): per tile its first event, m, n_first, d_last, span,
    every event's d_e, which are near, and the padding words behind the last."""
    n16 = np.asarray(n16, np.int64)
    out = []
    for t0 in range(0, len(n16), LC_TILE):
        n = n16[t0:t0 + LC_TILE]
        d = (n - n[0]) % 65536
        d_last = int(d[-1])
        span = min(d_last, LC_SPAN)
        out.append(Tile(t0, len(n), int(n[0]), d_last, span, d, d <= span, -len(n) % 4))
    return out


def window_byte(c0, d):
    """The byte of the window that hypothesis c0 reads for a near event at d_e = d (the window holds bytes 0 .. 1023 + span)."""
    return place(c0).j + int(d)


View = collections.namedtuple("View", "name n full ch tiles scores table best winner n_second runners unique tie")


def conn_events(conns, cands, tracks, pkts):
    """Per connection None (not TIMED) or (counter as the tracking stores it, channel) per event, as rule 1 gathers them."""
    events = [dict() for _ in tracks]
    for c, p in zip(cands, pkts):
        if p is not None and c.channel < len(tracks):
            events[c.channel][p.event] = (p.counter, p.channel)
    return [[ev[e] for e in sorted(ev)] if t.flags & lt.TIMED else None for ev, t in zip(events, tracks)]


def view(name, aa, events, map_mask, flags):
    """One EVALUATED connection as the kernels number it, with the LOCATIONS of the winner and of the runner-up: `runners` are the
    hypotheses other than the winner that score n_second; unique: best > n_second; tie: exactly two share the best score."""
    full = np.array([n for n, _ in events], np.int64)
    ch = np.array([c for _, c in events], np.int64)
    scores, table = lc.scores_np(aa, [(int(n), int(c), 1) for n, c in events], map_mask, flags)
    best = int(scores.max())
    winner = int(np.flatnonzero(scores == best)[0])
    others = scores.copy()
    others[winner] = -1
    n_second = int(others.max())
    runners = np.flatnonzero(others == n_second)
    return View(name, full % 65536, full, ch, tiles(full % 65536), scores, table, best, winner, n_second, runners, best > n_second,
                best == n_second and len(runners) == 1)


def on(v, c0):
    """Per event: does it lie on the prediction of hypothesis c0."""
    return v.table[(c0 + v.n) % 65536] == v.ch


def views(conns, cands, names, tracks, pkts, flags):
    return [view(name, c.access_address, ev, t.map_mask, flags)
            for name, c, t, ev in zip(names, conns, tracks, conn_events(conns, cands, tracks, pkts)) if ev is not None]


# ---- the facts ------------------------------------------------------------------------------------------------------------------------
def _placement(w, r):
    """How winner w and runner-up r (Places) lie to each other: the facts, without the second_ / tie_ in front."""
    out = set()
    if w.block != r.block:
        out.add("other_block")
        if (w.block, r.block) in ((0, LC_BLOCKS - 1), (LC_BLOCKS - 1, 0)):
            out.add("other_block_%d_%d" % (w.block, r.block))
        if r.block == w.block + 1 and (w.j, r.j) == (LAST_J, 0):
            out.add("other_block_adjacent_up")
        if r.block == w.block - 1 and (w.j, r.j) == (0, LAST_J):
            out.add("other_block_adjacent_down")
        return out
    if w.block >= LC_BLOCKS // 2:
        out.add("same_block_high")                                          # (the verdict's lanes 32 .. 63)
    if w.thread == r.thread:
        out.add("same_lane_%s_r" % ("smaller" if r.r < w.r else "larger"))
    elif w.wave == r.wave:
        if w.wave >= 1:                                                     # (thread 0 reads wave_second[k] for k >= 1)
            out.add("same_wave_runner_%s" % ("below" if r.lane < w.lane else "above"))
            if (w.lane ^ r.lane) & 32:
                out.add("same_wave_across_lane_31_32")
    else:
        out.add("other_wave_%d_%d" % (w.wave, r.wave))
        if (w.thread, r.thread) in ((WAVE - 1, WAVE), (WAVE, WAVE - 1)):
            out.add("lane_63_64_winner_%d" % w.thread)
    return out


def facts(vs, flags):
    """The facts a run carries.  vs: the views of its EVALUATED connections; flags: of the call."""
    out = set()
    seam = []                                                               # multi-tile unique winners at the seam threads
    for v in vs:
        w = place(v.winner)
        on_w = on(v, v.winner)
        on_r = np.zeros(len(v.n), bool)
        for c0 in v.runners[:64]:
            on_r |= on(v, int(c0))
        multi = len(v.tiles) > 1
        count = len(v.n)
        # ---- the window and the two loops, tile by tile
        if v.unique:
            near_score = 0
            for k, t in enumerate(v.tiles):
                mine = on_w[t.t0:t.t0 + t.m]
                near_score += int((mine & t.near).sum())
                kinds = [kind for kind, ok in (("wide", PER_BLOCK <= t.span < LC_SPAN), ("cut", t.span == LC_SPAN)) if ok]
                for kind in kinds:
                    if w.j == LAST_J and (mine & t.near & (t.d == t.span)).any():
                        out.add("tail_" + kind)                             # (the byte 1023 + span, which only thread 255 reads, in r = 3)
                    if w.j == 0 and (mine & (t.d == 0)).any():
                        out.add("head_" + kind)
                if all((mine & t.near & ~on_r[t.t0:t.t0 + t.m] & (t.d % 4 == s)).any() for s in range(4)):
                    out.add("shift_classes")
                for delta in (-1, 0, 1):
                    if t.d_last == LC_SPAN + delta:
                        out.add("d_last_cut%+d" % delta)
                if (mine & (t.d == LC_SPAN) & t.near).any() and (mine & (t.d == LC_SPAN + 1) & ~t.near).any():
                    out.add("cut_near_and_far")
                if k >= 1 and 65536 - t.n_first <= LC_TILE:
                    behind = v.n[t.t0:t.t0 + t.m] < t.n_first
                    if (mine & behind).any() and (mine & ~behind).any():
                        out.add("n_e_wraps_in_tile")
                        if (mine & behind & t.near).any() and (~t.near).any():
                            out.add("n_e_wraps_beside_far")                  # (the second loop passes over near events with n_e < n_first)
                turns = (v.full[t.t0:t.t0 + t.m] - v.full[t.t0]) >> 16      # (the tracking's counters do not wrap at 2^16)
                if turns[-1] >= 1 and (mine & t.near & (turns == 0)).any() and (mine & t.near & (turns >= 1)).any() and (mine & ~t.near).any():
                    out.add("tile_spans_2_16")
                if t.pad and multi and k == len(v.tiles) - 1 and mine.any():
                    out.add("last_tile_pad_%d" % t.pad)
            far_score = v.best - near_score
            if far_score and near_score <= v.n_second and w.thread in SEAM_THREADS:
                out.add("far_decides_thread_%d" % w.thread)                 # (without the far loop the runner-up wins, or ties)
            if count in COUNTS and on_w[-1]:
                out.add("count_%d" % count)
            if multi:
                if w.thread in SEAM_THREADS:
                    seam.append(w)
                if w.block == LC_BLOCKS - 1 and w.j in (0, LAST_J):
                    out.add("block_63_j_%d" % w.j)
        # ---- the verdict's walk over the events: off the winner's prediction, the prediction known
        expected = v.table[(v.winner + v.n) % 65536]
        off = np.flatnonzero((expected != 0xFF) & (expected != v.ch))
        if (off >= WAVE).any():
            out.add("off_behind_63")
            out |= {"off_at_%d" % e for e in OFF_AT if e in off}
            if count - 1 in off:
                out.add("off_at_last")
            if not flags & lc.REMAP and (expected[WAVE:] == 0xFF).any():
                out.add("unknown_behind_63")
        # ---- where the runner-up lies
        if len(v.runners) == 1 and (v.unique or v.tie):
            r = place(int(v.runners[0]))
            kind = "second_" if v.unique else "tie_"
            out |= {kind + p for p in _placement(w, r)}
            if v.unique and r.c0 < w.c0:
                out.add("second_at_smaller_c0")
            if v.unique and multi:
                behind_one = int(on(v, r.c0)[LC_TILE:].sum())
                rest = v.scores.copy()
                rest[[w.c0, r.c0]] = 0
                if behind_one > rest.max() and behind_one > int(on(v, r.c0)[:LC_TILE].sum()):
                    out.add("second_only_in_tile_two")                      # (tile two alone makes it the runner-up)
    for a in seam:
        out.add("seam_thread_%d" % a.thread)
        out.add("seam_r_%d" % a.r)
        if a.thread == LAST_THREAD and any(b.thread == 0 and b.block == a.block + 1 for b in seam):
            out.add("seam_255_beside_0")
    return out


# tag -> (when it holds, the facts it needs)
TAGS = {
    "winner_at_window_tail": ("the winner at j = 1023; a tile with 1024 <= span < LC_SPAN and one with span = LC_SPAN whose event at d = span lies on its prediction",
                              {"tail_wide", "tail_cut"}),
    "winner_at_window_head": ("the same with the winner at j = 0 and the tile's event at d = 0", {"head_wide", "head_cut"}),
    "winner_across_wave_seam": ("connections of several tiles with winners at threads 0, 63, 64 and 255, 255 in the block below 0's, every r among them",
                                {"seam_thread_%d" % t for t in SEAM_THREADS} | {"seam_r_%d" % r for r in range(LC_PER_LANE)} | {"seam_255_beside_0"}),
    "shift_classes": ("one tile with near events at d mod 4 = 0, 1, 2, 3 on the winner's prediction and on no runner-up's", {"shift_classes"}),
    "span_cut": ("tiles with d_last = LC_SPAN - 1, LC_SPAN, LC_SPAN + 1; events at d = LC_SPAN (near) and LC_SPAN + 1 (far) of one tile on the winner's prediction",
                 {"d_last_cut-1", "d_last_cut+0", "d_last_cut+1", "cut_near_and_far"}),
    "far_decides": ("winners at threads 0, 63, 64, 255 whose near events alone do not beat the runner-up", {"far_decides_thread_%d" % t for t in SEAM_THREADS}),
    "tile_counts": ("UNIQUE connections of 511, 512, 513, 1 024, 1 025 events, the last on the winner's prediction", {"count_%d" % n for n in COUNTS}),
    "last_tile_padded": ("connections of several tiles whose last needs 1, 2 and 3 padding words", {"last_tile_pad_%d" % p for p in (1, 2, 3)}),
    "n_e_wraps_in_tile": ("a tile behind the first with n_first within 512 of 2^16; events of the winner's on both sides of the wrap, far events in the same tile",
                          {"n_e_wraps_in_tile", "n_e_wraps_beside_far"}),
    "tile_spans_2_16": ("a tile over more than 65 536 counters: near events of the winner's before and behind the wrap, far ones between", {"tile_spans_2_16"}),
    "block_63_multi_tile": ("connections of several tiles with the winners 65535 and 64512", {"block_63_j_0", "block_63_j_%d" % LAST_J}),
    "off_behind_63": ("events off the prediction at e >= 64: at 63, 64, 511, 512, 513 and a last event; without REMAP an unknown prediction behind 63",
                      {"off_behind_63", "off_at_last", "unknown_behind_63"} | {"off_at_%d" % e for e in OFF_AT}),
    "second_same_lane": ("UNIQUE, the runner-up in the winner's lane, at a smaller and at a larger r", {"second_same_lane_smaller_r", "second_same_lane_larger_r"}),
    "second_same_wave": ("UNIQUE, both in one wave k >= 1 (wave_second[k]), the runner-up's lane below and above, and across lanes 31 | 32",
                         {"second_same_wave_runner_below", "second_same_wave_runner_above", "second_same_wave_across_lane_31_32"}),
    "second_across_lane_63_64": ("UNIQUE, winner and runner-up at threads 63 and 64, both orders", {"second_lane_63_64_winner_63", "second_lane_63_64_winner_64"}),
    "second_other_wave": ("UNIQUE, winner in wave a, runner-up in wave b of the block: (0, 3), (3, 0), (1, 2)",
                          {"second_other_wave_0_3", "second_other_wave_3_0", "second_other_wave_1_2"}),
    "second_other_block": ("UNIQUE, blocks (0, 63), (63, 0) and adjacent ones with j = 1023 beside j = 0, both orders; the runner-up at the smaller c0",
                           {"second_other_block_0_63", "second_other_block_63_0", "second_other_block_adjacent_up", "second_other_block_adjacent_down",
                            "second_at_smaller_c0"}),
    "second_same_block_high": ("UNIQUE, both in one block >= 32: a partial of the verdict's upper lanes", {"second_same_block_high"}),
    "tie_same_lane": ("exactly two share the best score, in one lane", {"tie_same_lane_larger_r"}),
    "tie_same_wave": ("... in one wave k >= 1, and across lanes 31 | 32", {"tie_same_wave_runner_above", "tie_same_wave_across_lane_31_32"}),
    "tie_across_lane_63_64": ("... at threads 63 and 64", {"tie_lane_63_64_winner_63"}),
    "tie_other_wave": ("... in waves (0, 3) and (1, 2) of one block", {"tie_other_wave_0_3", "tie_other_wave_1_2"}),
    "tie_other_block": ("... in blocks 0 and 63, and in adjacent ones at j = 1023 and j = 0", {"tie_other_block_0_63", "tie_other_block_adjacent_up"}),
    "tie_same_block_high": ("... in one block >= 32", {"tie_same_block_high"}),
    "second_only_in_tile_two": ("UNIQUE; the runner-up's events behind the first tile alone outnumber every third hypothesis' and its own of the first",
                                {"second_only_in_tile_two"}),
}


def tags_of(fs):
    return {tag for tag, (_, need) in TAGS.items() if need <= fs}


# ---- the runs ---------------------------------------------------------------------------------------------------------------------
SECOND = frozenset(t for t in TAGS if t.startswith(("second_same", "second_across", "second_other", "tie_")))
WINDOW = frozenset({"winner_at_window_tail", "winner_at_window_head", "shift_classes", "span_cut", "far_decides", "n_e_wraps_in_tile", "tile_spans_2_16",
                    "block_63_multi_tile"})
# name; the list (a builder of tests/_le_csa2.py and its argument); flags; "cut": conn_cap one below the connections; the tags
Run = collections.namedtuple("Run", "name build arg flags cut tags")
RUNS = (
    Run("pairs", "pair_list", None, 0, False, SECOND),
    Run("pairs, REMAP", "pair_list", None, lc.REMAP, False, SECOND),
    Run("windows, REMAP", "wide_list", "windows", lc.REMAP, False, WINDOW),
    Run("counts", "wide_list", "counts", 0, False, {"tile_counts", "last_tile_padded", "off_behind_63", "second_only_in_tile_two", "shift_classes"}),
    Run("counts, REMAP", "wide_list", "counts", lc.REMAP, False, {"tile_counts", "last_tile_padded", "second_only_in_tile_two", "shift_classes"}),
    Run("windows, REMAP, cut", "wide_list", "windows", lc.REMAP, True, ()),
    Run("counts, REMAP, cut", "wide_list", "counts", lc.REMAP, True, ()),
)


# a tag whose facts are properties of single connections may be carried by several runs between them: the seam threads 0 and 255
# are the windows', 63 and 64 the counts'
BETWEEN_RUNS = {"winner_across_wave_seam": ("windows, REMAP", "counts, REMAP")}


def run_list(run):
    return lc.pair_list() if run.build == "pair_list" else lc.wide_list(run.arg)


def run_model(run):
    """(tracks, pkts, (sels, sel_pkts)) of the models on a run's list, whole (shared between the runs on one list)."""
    return lc.list_model(run.build, run.arg, run.flags)


_FACTS = {}


def run_facts(run):
    """The facts a run carries (worked out once)."""
    if run.name not in _FACTS:
        conns, cands, names = run_list(run)
        tracks, pkts, _ = run_model(run)
        kept = len(conns) - 1 if run.cut else len(conns)
        _FACTS[run.name] = frozenset(facts(views(conns[:kept], cands, names, tracks[:kept], pkts, run.flags), run.flags))
    return _FACTS[run.name]


def run_tags(run):
    return tags_of(run_facts(run))
