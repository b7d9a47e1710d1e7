"""A plain model of what DECIDES the path of the hit ordering (libbtbb_amd/csrc/sort.hip), and a lattice of lists on its branches.

The ordering takes another path for almost every property of its input: how many records share a bucket (1, up to
ORDER_SMALL, up to ORDER_PAIRS, more), how wide a bucket is against the 2^ORDER_BIG_BITS keys of one presence-bitmap window,
where in the bucket the keys lie (which windows are visited, whether the span of windows is given up on), whether a key
repeats, which of the scans of the counts runs and whether the bucket count ends ragged.  This module ports those decisions --
not the kernels -- so that

* every branch has a NAMED list that drives it (LATTICE), built from the bucket geometry the code will use;
* tests/test_order_model.py fails on the CPU when a constant of sort.hip moves and a case stops driving its branch;
* tests/test_gpu_order_lattice.py runs the same lists through the device entries and compares with expected().

The constants are read out of sort.hip by regular expression (the patterns follow the spelling of the lines they name: a
refactor that rewrites such a line fails the model test with "found 0 times" and the pattern wants another look).  The builders
use the constants, so the lattice moves with them; the TAG NAMES say 48 / 4096 / 2^20 / 2^22, and test_order_model.py pins
those four values so that a change of one ends in a failing test that asks for the names to be looked at.  The segment-slot side (the compaction behind
btbbx_scan_ordered_device) has its own small model at the end: slot_geometry(), slot_tags() and the one place that knows
where the SlotHeader lies in the caller's scratch (slot_header_offset()).
"""
import functools
import os
import re
import time
from collections import namedtuple

import numpy as np

import _libs
import libbtbb_amd as bt
from libbtbb_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SORT_HIP = os.path.join(ROOT, "libbtbb_amd", "csrc", "sort.hip")

LAP_ANY = 0xFFFFFFFF
OFFSET_LIMIT = 1 << 47                     # include/btbbx.h: "Offsets must stay below 2^47"
STREAM_LIMIT = 1 << 16                     # btbbx_hit::stream is 16 bits wide


def read_constants(path=SORT_HIP):
    """The numbers the model rests on, each found exactly once in sort.hip."""
    with open(path) as f:
        src = f.read()

    def one(pattern):
        found = re.findall(pattern, src, re.M)
        assert len(found) == 1, "sort.hip: %r found %d times" % (pattern, len(found))
        return found[0]

    k = {}
    for name in ("ORDER_SMALL", "ORDER_MAX_LOG2", "ORDER_BIG_BITS", "ORDER_PAIRS", "SLOT_N", "SLOT_BLOCK", "SLOT_PER"):
        k[name] = int(one(r"^#define\s+%s\s+(\d+)u?\b" % name))
    # `if (w_last - w_first > 65535)` in order_crowded_body
    k["WINDOW_SPAN"] = int(one(r"w_last\s*-\s*w_first\s*>\s*(\d+)"))                   # more windows than this: all pairs instead
    # the launch of order_crowded_kernel in order_launch: `dim3(std::min(nb, 256u)), dim3(1024)`
    k["CROWDED_GRID"] = int(one(r"order_crowded_kernel,\s*dim3\(std::min\(nb,\s*(\d+)u\)\)"))  # workgroups of order_crowded_kernel
    # the bucket walk of order_crowded_body: `for (uint32_t first = vblock * 1024; ...`
    k["CROWDED_STEP"] = int(one(r"first\s*=\s*vblock\s*\*\s*(\d+)\s*;"))               # buckets a workgroup looks at per step
    # order_launch: `const uint32_t scan_items = nb <= (1u << 22) ? 4u : 16u;` and `if (scan_blocks > 1024)`
    items = one(r"scan_items\s*=\s*nb\s*<=\s*\(1u\s*<<\s*(\d+)\)\s*\?\s*(\d+)u\s*:\s*(\d+)u")
    k["SCAN_FEW_LOG2"], k["SCAN_FEW"], k["SCAN_MANY"] = (int(x) for x in items)
    k["SCAN_BLOCKS_MAX"] = int(one(r"if\s*\(scan_blocks\s*>\s*(\d+)\)"))
    # order_nb_log2: `uint32_t l = 8;` (the smallest bucket count)
    k["NB_MIN_LOG2"] = int(one(r"uint32_t\s+l\s*=\s*(\d+);"))
    return k


K = read_constants()
ORDER_SMALL, ORDER_MAX_LOG2, ORDER_BIG_BITS, ORDER_PAIRS = K["ORDER_SMALL"], K["ORDER_MAX_LOG2"], K["ORDER_BIG_BITS"], K["ORDER_PAIRS"]
SLOT_N, SLOT_BLOCK, SLOT_PER, WINDOW_SPAN = K["SLOT_N"], K["SLOT_BLOCK"], K["SLOT_PER"], K["WINDOW_SPAN"]

ORDER_TAGS = frozenset((
    "alone", "shared", "shared_at_48", "pairs_at_49", "pairs", "pairs_at_4096", "bitmap_at_4097", "bitmap_one_window",
    "bitmap_shift_eq_20", "bitmap_windows", "bitmap_span_exit", "bitmap_repeat_redo", "bitmap_windows_repeat_redo",
    "two_crowded_in_one_step", "crowded_in_a_later_step", "shift_zero", "nb_ragged", "nb_2p22", "items16", "nb_min",
    "count_lt_cap", "count_eq_cap", "count_gt_cap", "streams_65536", "offset_limit"))
SLOT_TAGS = frozenset((
    "seg_0", "seg_1", "seg_2", "seg_3", "seg_many", "seg_first_offset", "seg_last_offset", "stream_seam", "n_segs_ragged",
    "two_place_workgroups", "cut_between_slots", "cut_in_overflow", "overflow_fits", "overflow_full"))


# ---- geometry (host side of sort.hip) ------------------------------------------------------------------------------------------

def order_nb_log2(cap):
    l = K["NB_MIN_LOG2"]
    while l < ORDER_MAX_LOG2 and (1 << l) < cap:
        l += 1
    return l


def key_bits(total):
    """T with 2^T >= total keys; 64 when the product does not fit 64 bits."""
    if total >> 64:
        return 64
    return (total - 1).bit_length() if total > 1 else 0


def order_shift(n_streams, mul, nb_log2):
    t = key_bits(int(n_streams) * int(mul))
    return t - nb_log2 if t > nb_log2 else 0


def order_fine_buckets(n_streams, mul, nb_log2_fine):
    shift = order_shift(n_streams, mul, nb_log2_fine)
    total = int(n_streams) * int(mul)
    nbu = (total + (1 << shift) - 1) >> shift
    most = 1 << nb_log2_fine
    return (nbu or 1) if nbu < most else most


def scan_items(nb):
    return K["SCAN_FEW"] if nb <= (1 << K["SCAN_FEW_LOG2"]) else K["SCAN_MANY"]


def scan_blocks(nb):
    per = 1024 * scan_items(nb)
    return (nb + per - 1) // per


Geometry = namedtuple("Geometry", "n nb_log2 nb shift mul n_streams")

# where the parameters come from: "extent" (order_extent_kernel reads the list), "bounds" (the caller of
# btbbx_order_scan_hits_device gives them), "scan" (btbbx_scan_ordered_device: bounds and counts from the scan);
# "sort" is btbbx_sort_hits_device = extent with count == cap == the length
SOURCES = ("extent", "bounds", "scan", "sort")


def geometry(hits, count, cap, source, n_streams=0, search_bits=0):
    assert source in SOURCES and cap >= 2
    n = min(int(count), int(cap))
    nb_log2 = order_nb_log2(cap)
    if source in ("extent", "sort"):
        h = hits[:n]
        mo = int(h["offset"].max()) if n else 0
        ms = int(h["stream"].max()) if n else 0
        mul, ns = mo + 1, ms + 1
        return Geometry(n, nb_log2, 1 << nb_log2, order_shift(ns, mul, nb_log2), mul, ns)
    assert n_streams and search_bits
    nb = 1 << nb_log2
    if nb_log2 < ORDER_MAX_LOG2:
        nb_log2 += 1
        nb = order_fine_buckets(n_streams, search_bits, nb_log2)
    return Geometry(n, nb_log2, nb, order_shift(n_streams, search_bits, nb_log2), int(search_bits), int(n_streams))


def linear_keys(hits, mul):
    """stream * mul + offset as uint64 (the caller has checked that it fits)."""
    st, off = hits["stream"].astype(np.uint64), hits["offset"].astype(np.uint64)
    if len(hits):
        assert int(st.max()) * int(mul) + int(off.max()) < 1 << 64
    return st * np.uint64(mul) + off


def has_repeats(hits, count, cap):
    h = hits[:min(count, cap)]
    key = (h["stream"].astype(np.uint64) << np.uint64(48)) | h["offset"]
    return len(np.unique(key)) < len(h)


def classify(hits, count, cap, form, n_streams=0, search_bits=0):
    """The branch tags a call takes.  form: one of SOURCES."""
    if form == "sort":
        assert count == cap == len(hits), "btbbx_sort_hits_device has one number for all three"
    g = geometry(hits, count, cap, form, n_streams, search_bits)
    h = hits[:g.n]
    tags = {"count_lt_cap" if count < cap else "count_eq_cap" if count == cap else "count_gt_cap"}
    if g.shift == 0:
        tags.add("shift_zero")
    if g.nb % scan_items(g.nb):
        tags.add("nb_ragged")
    if g.nb == 1 << K["SCAN_FEW_LOG2"]:
        tags.add("nb_2p22")
    if scan_items(g.nb) == K["SCAN_MANY"]:
        tags.add("items16")
    if g.nb == 1 << K["NB_MIN_LOG2"]:
        tags.add("nb_min")
    assert g.nb <= 1 << ORDER_MAX_LOG2 and scan_blocks(g.nb) <= K["SCAN_BLOCKS_MAX"]
    if not g.n:
        return tags
    assert int(h["offset"].max()) < OFFSET_LIMIT, "outside the documented contract"
    if form in ("bounds", "scan"):
        assert int(h["stream"].max()) < n_streams and int(h["offset"].max()) < search_bits, "records outside the caller's bounds"
    last = h["stream"] == STREAM_LIMIT - 1
    if last.any():
        tags.add("streams_65536")
        if (h["offset"][last] == OFFSET_LIMIT - 1).any():
            tags.add("offset_limit")
    lin = linear_keys(h, g.mul)
    bucket = lin >> np.uint64(g.shift)
    assert int(bucket.max()) < g.nb
    ub, inv, k = np.unique(bucket, return_inverse=True, return_counts=True)
    if (k == 1).any():
        tags.add("alone")
    if ((k > 1) & (k <= ORDER_SMALL)).any():
        tags.add("shared")
    if (k == ORDER_SMALL).any():
        tags.add("shared_at_48")
    if (k == ORDER_SMALL + 1).any():
        tags.add("pairs_at_49")
    if ((k > ORDER_SMALL + 1) & (k < ORDER_PAIRS)).any():
        tags.add("pairs")
    if (k == ORDER_PAIRS).any():
        tags.add("pairs_at_4096")
    crowded = ub[k > ORDER_SMALL].astype(np.int64)
    steps = crowded // K["CROWDED_STEP"]
    if len(np.unique(steps)) < len(steps):
        tags.add("two_crowded_in_one_step")
    if (crowded >= K["CROWDED_GRID"] * K["CROWDED_STEP"]).any():
        tags.add("crowded_in_a_later_step")
    wbits = min(g.shift, ORDER_BIG_BITS)
    low_mask = np.uint64((1 << g.shift) - 1)
    for i in np.flatnonzero(k > ORDER_PAIRS):
        low = lin[inv == i] & low_mask
        wdw = (low >> np.uint64(wbits)).astype(np.int64)
        w_first, w_last = int(wdw.min()), int(wdw.max())
        if w_last - w_first > WINDOW_SPAN:
            tags.add("bitmap_span_exit")
            continue                                         # (ranked by all pairs: it carries none of the bitmap tags, 4097 members or not)
        if k[i] == ORDER_PAIRS + 1:
            tags.add("bitmap_at_4097")
        if g.shift == ORDER_BIG_BITS:
            tags.add("bitmap_shift_eq_20")
        repeat = len(np.unique(low)) < k[i]
        if w_first == w_last:
            tags.add("bitmap_one_window")
            if repeat:
                tags.add("bitmap_repeat_redo")
        else:
            if w_first > 0 and len(np.unique(wdw)) < w_last - w_first + 1:
                tags.add("bitmap_windows")
            if repeat:
                tags.add("bitmap_windows_repeat_redo")
    return tags


def expected(hits, count, cap):
    """The first min(count, cap) records in (stream, offset) order (ties stay in list order; see same_list)."""
    h = hits[:min(int(count), int(cap))]
    return h[np.lexsort((h["offset"], h["stream"]))]


FULL = ["stream", "offset", "lap", "ac_errors", "reserved"]


def same_list(got, want, unique):
    """Whole records for lists with unique keys; with repeated keys the key sequence and the multiset of records (where
    bucket-mates with equal keys land depends on an atomic cursor)."""
    if len(got) != len(want):
        return False
    if unique:
        return got.tobytes() == want.tobytes()
    return (np.array_equal(got["stream"], want["stream"]) and np.array_equal(got["offset"], want["offset"])
            and np.array_equal(np.sort(got, order=FULL), np.sort(want, order=FULL)))


# ---- the lattice ---------------------------------------------------------------------------------------------------------------

def records(streams, offsets, seed):
    """A shuffled list of hit records with these keys and random LAP / error fields."""
    rng = np.random.default_rng(seed)
    h = np.zeros(len(offsets), bt.HIT_DTYPE)
    h["offset"], h["stream"] = offsets, streams
    h["lap"] = rng.integers(0, 1 << 24, len(h))
    h["ac_errors"] = rng.integers(0, 3, len(h))
    return h[rng.permutation(len(h))]


class _Plan:
    """Keys placed bucket by bucket for a list whose extent is pinned by one record at (max_stream, max_off)."""

    def __init__(self, cap, max_off, max_stream=0, seed=0):
        self.cap, self.mul = cap, max_off + 1
        self.shift = order_shift(max_stream + 1, self.mul, order_nb_log2(cap))
        self.width = 1 << self.shift
        self.rng = np.random.default_rng(seed)
        self.lin = [np.array([max_stream * self.mul + max_off], dtype=np.uint64)]
        self.seed = seed

    def draw(self, k, below):
        """k distinct numbers below `below`."""
        if below <= 1 << 22:
            return self.rng.choice(below, k, replace=False).astype(np.uint64)
        v = np.unique(self.rng.integers(0, below, 2 * k + 16, dtype=np.uint64))
        assert len(v) >= k
        return self.rng.permutation(v)[:k]

    def put(self, b, low):
        low = np.asarray(low, dtype=np.uint64)
        assert len(low) and int(low.max()) < self.width
        self.lin.append((np.uint64(b) << np.uint64(self.shift)) + low)
        return self

    def fill(self, first_bucket, n):
        """n records, each alone in a bucket of its own from first_bucket on."""
        for b in range(first_bucket, first_bucket + n):
            self.put(b, [int(self.rng.integers(0, self.width))])
        return self

    def hits(self, length=None):
        lin = np.concatenate(self.lin)
        assert length is None or len(lin) == length, (len(lin), length)
        return records(lin // np.uint64(self.mul), lin % np.uint64(self.mul), self.seed + 1)


def _edges_small():
    # 2^8 buckets of 2^20 keys; populations on both sides of ORDER_SMALL, all in the first step of one workgroup
    p = _Plan(200, (1 << 28) - 1, seed=11)
    for b, k in ((3, 1), (5, 2), (10, ORDER_SMALL), (11, ORDER_SMALL + 1), (20, ORDER_SMALL + 12)):
        p.put(b, p.draw(k, p.width))
    used = 1 + 1 + 2 + ORDER_SMALL * 3 + 13
    return p.fill(100, 200 - used).hits(200)


def _edges_bitmap():
    # buckets exactly as wide as one bitmap window; populations on both sides of ORDER_PAIRS
    p = _Plan(8400, (1 << (ORDER_BIG_BITS + 14)) - 1, seed=12)
    assert p.shift == ORDER_BIG_BITS
    p.put(7, p.draw(ORDER_PAIRS, p.width)).put(9, p.draw(ORDER_PAIRS + 1, p.width))
    return p.fill(2000, 8400 - 2 * ORDER_PAIRS - 2).hits(8400)


def _windows(repeat):
    def build():
        # buckets of 2^6 windows: one bucket with keys in windows 3, 4 and 7 (0 .. 2 skipped, 5 and 6 empty in between), one
        # in another step with all its keys in window 9
        p = _Plan(9600, (1 << (ORDER_BIG_BITS + 6 + 14)) - 1, seed=13 + repeat)
        assert p.shift == ORDER_BIG_BITS + 6
        win = 1 << ORDER_BIG_BITS
        parts = [np.uint64(w * win) + p.draw(k, win) for w, k in ((3, 2000), (4, 1500), (7, 1500))]
        if repeat:
            parts.append(parts[0][:40])                      # forty keys of window 3 a second time
            parts.append(parts[2][-3:])
        p.put(100, np.concatenate(parts))
        one = np.uint64(9 * win) + p.draw(ORDER_PAIRS + 300, win)
        p.put(5000, np.concatenate([one, one[:25]]) if repeat else one)
        return p.hits()
    return build


def _span_exit():
    # buckets of 2^37 keys = 2^17 windows: two dense runs more than WINDOW_SPAN windows apart inside one bucket
    p = _Plan(4300, OFFSET_LIMIT - 1, max_stream=7, seed=15)
    assert p.shift - ORDER_BIG_BITS > 16
    win = 1 << ORDER_BIG_BITS
    far = np.uint64((WINDOW_SPAN + 4000) * win)
    assert int(far) + win <= p.width
    p.put(5, np.concatenate([np.uint64(3 * win) + p.draw(2100, win), far + p.draw(2000, win)]))
    return p.fill(600, 50).hits()


def _later_step():
    # 2^19 buckets: order_crowded_kernel's 256 workgroups reach the crowded bucket in their second trip
    p = _Plan((1 << 18) + 1, (1 << 30) - 1, seed=16)
    beyond = K["CROWDED_GRID"] * K["CROWDED_STEP"]
    p.put(beyond + 37000, p.draw(60, p.width)).put(beyond + 37001, p.draw(2, p.width)).put(5, p.draw(50, p.width))
    return p.fill(1000, 20).hits()


def _shift_zero():
    # 500 keys, 1024 buckets: a key is its bucket; repeated keys are the only bucket-mates there can be
    rng = np.random.default_rng(17)
    off = rng.choice(499, 300, replace=False)
    off = np.concatenate([off, np.repeat(off[:20], 2), [499]])
    return records(0, off.astype(np.uint64), 17)


def _sparse_big(seed):
    def build():
        # a short list in a huge buffer: the bucket count follows cap, the length comes from HBM.  Records all over the key space
        # (the sums of every workgroup of the scans matter), three in one bucket near the end, two in the last bucket
        rng = np.random.default_rng(seed)
        top = 1 << 35
        off = np.unique(np.concatenate([rng.integers(0, top - (1 << 14), 1500, dtype=np.uint64),
                                        np.array([top - 1, top - 77, top - (1 << 20) + 1, top - (1 << 20) + 5, top - (1 << 20) + 9], np.uint64)]))
        return records(0, off, seed)
    return build


def _ragged():
    # five streams of 1 345 682 offsets: with the caller's bounds 13 142 buckets of 2^9 keys -- no multiple of four.  The last
    # bucket holds three records, so the total behind the last counter (cnt[nb], written from a ragged end) is used
    rng = np.random.default_rng(19)
    bits = 1345682
    st = rng.integers(0, 5, 3000)
    off = rng.integers(0, bits, 3000, dtype=np.uint64)
    st = np.concatenate([st, [4, 4, 4]])
    off = np.concatenate([off, np.array([bits - 1, bits - 30, bits - 200], np.uint64)])
    key = np.unique((st.astype(np.uint64) << np.uint64(48)) | off)
    return records(key >> np.uint64(48), key & np.uint64((1 << 48) - 1), 19)


def _limits():
    # the largest key there is: stream 65535, offset 2^47 - 1
    rng = np.random.default_rng(20)
    st = np.concatenate([rng.integers(0, STREAM_LIMIT, 390), [STREAM_LIMIT - 1] * 9, [STREAM_LIMIT - 1]])
    off = np.concatenate([rng.integers(0, OFFSET_LIMIT, 390, dtype=np.uint64), rng.integers(0, OFFSET_LIMIT - 1, 9, dtype=np.uint64),
                          np.array([OFFSET_LIMIT - 1], np.uint64)])
    return records(st, off, 20)


def _three_streams(n, seed):
    def build():
        rng = np.random.default_rng(seed)
        key = np.unique((rng.integers(0, 3, n + 64).astype(np.uint64) << np.uint64(48)) | rng.integers(0, 1 << 22, n + 64, dtype=np.uint64))
        key = rng.permutation(key)[:n]
        return records(key >> np.uint64(48), key & np.uint64((1 << 48) - 1), seed)
    return build


# name; builder of the list; cap and count (None: the length of the list); the source of the parameters the case is built for;
# the tags it exists for; loose: what btbbx_order_scan_hits_device's loose form adds to the exact bounds (streams, offsets)
Case = namedtuple("Case", "name build cap count form tags loose")
LOOSE = (2, None)                                            # two more streams, a third more offsets + 12345


def _case(name, build, cap, count, form, tags, loose=LOOSE):
    return Case(name, build, cap, count, form, frozenset(tags), loose)


LATTICE = [
    _case("edges_small", _edges_small, None, None, "extent",
          ("alone", "shared", "shared_at_48", "pairs_at_49", "pairs", "two_crowded_in_one_step", "nb_min", "count_eq_cap")),
    _case("edges_bitmap", _edges_bitmap, None, None, "extent",
          ("pairs_at_4096", "bitmap_at_4097", "bitmap_one_window", "bitmap_shift_eq_20", "two_crowded_in_one_step", "count_eq_cap")),
    _case("bitmap_windows", _windows(0), 9600, None, "extent", ("bitmap_windows", "bitmap_one_window", "count_lt_cap")),
    _case("bitmap_windows_repeat", _windows(1), 9600, None, "extent",
          ("bitmap_windows", "bitmap_windows_repeat_redo", "bitmap_repeat_redo", "bitmap_one_window")),
    _case("bitmap_span_exit", _span_exit, 4300, None, "extent", ("bitmap_span_exit",)),
    _case("crowded_later_step", _later_step, (1 << 18) + 1, None, "extent", ("crowded_in_a_later_step", "pairs", "shared", "count_lt_cap")),
    _case("shift_zero", _shift_zero, 1000, None, "extent", ("shift_zero", "alone", "shared")),
    _case("nb_2p22", _sparse_big(181), 1 << K["SCAN_FEW_LOG2"], None, "extent", ("nb_2p22", "alone", "shared", "count_lt_cap")),
    _case("items16", _sparse_big(182), (1 << K["SCAN_FEW_LOG2"]) + 1, None, "extent", ("items16", "alone", "shared", "count_lt_cap")),
    _case("nb_ragged", _ragged, 5000, None, "bounds", ("nb_ragged", "alone", "shared"), loose=(0, 0)),
    _case("key_limits", _limits, None, None, "extent", ("streams_65536", "offset_limit", "count_eq_cap")),
    _case("count_gt_cap", _three_streams(3000, 21), 2000, 3000, "extent", ("count_gt_cap", "alone", "shared")),
    _case("count_short", _three_streams(3000, 22), 3000, 1000, "extent", ("count_lt_cap", "alone")),
]
MAX_RECORDS = 300_000                                        # no case is longer
BIG_CAP_CASES = ("nb_2p22", "items16")                       # ... and only these need a buffer of millions of records


def case_numbers(case, hits):
    """(cap, count) of a case with the defaults filled in."""
    n = len(hits)
    return (n if case.cap is None else case.cap), (n if case.count is None else case.count)


def case_bounds(case, hits, loose):
    """(n_streams, search_bits) for btbbx_order_scan_hits_device: exactly the extent of the whole list, or loose."""
    ns, bits = int(hits["stream"].max()) + 1, int(hits["offset"].max()) + 1
    if loose:
        more_streams, more_bits = case.loose
        ns += more_streams
        bits += bits // 3 + 12345 if more_bits is None else more_bits
    return ns, bits


# the four ways test_gpu_order_lattice.py runs a case -> the model's form
RUNS = {"extent": "extent", "exact": "bounds", "loose": "bounds", "sort": "sort"}


def run_tags(case, hits, run):
    cap, count = case_numbers(case, hits)
    if run in ("exact", "loose"):
        ns, bits = case_bounds(case, hits, run == "loose")
        return classify(hits, count, cap, "bounds", ns, bits)
    return classify(hits, count, cap, RUNS[run])


# ---- segment slots -------------------------------------------------------------------------------------------------------------
#
# The ONE place that knows the layout of the caller's scratch behind the general ordering's part (sort.hip: slot_layout, SlotHeader):
# the header lies at the first 256-byte boundary at or after btbbx_order_hits_scratch_bytes(cap); its first four dwords are
# ovf_count, irregular, total, redo_count.  A GPU test reads it from its own scratch buffer to prove which path a call took.

SlotHeader = namedtuple("SlotHeader", "ovf_count irregular total redo_count")


def slot_header_offset(order_scratch_bytes):
    return (int(order_scratch_bytes) + 255) & ~255


def slot_header(dwords):
    return SlotHeader(*(int(x) for x in dwords[:4]))


SlotGeometry = namedtuple("SlotGeometry", "seg_offsets tile_words segs_per_tile segs_per_stream n_segs n_blocks")


def slot_geometry(search_bits, n_streams, lap):
    """Segments of the ordered scan: LAP_ANY 4032 offsets (the 63 words a wave owns of a 756-word tile, 12 per tile), a known
    LAP 4096 offsets (8 per 512-word tile); a stream has whole tiles of them."""
    seg_offsets, tile_words, per_tile = (4032, 756, 12) if lap == LAP_ANY else (4096, 512, 8)
    assert tile_words * 64 == per_tile * seg_offsets
    words = (int(search_bits) + 63) // 64
    sps = (words + tile_words - 1) // tile_words * per_tile
    n_segs = sps * n_streams
    per_block = SLOT_BLOCK * SLOT_PER
    return SlotGeometry(seg_offsets, tile_words, per_tile, sps, n_segs, (n_segs + per_block - 1) // per_block)


def slot_segments(keys, geo, lap):
    """Segment of every (stream, offset) and the offset's place inside it (a tile is a whole number of segments)."""
    st = np.array([k[0] for k in keys], dtype=np.int64)
    off = np.array([k[1] for k in keys], dtype=np.int64)
    return st * geo.segs_per_stream + off // geo.seg_offsets, off % geo.seg_offsets


def slot_tags(keys, search_bits, n_streams, lap, cap):
    """Tags of the compaction for the list `keys` = sorted (stream, offset) pairs of ALL hits of the scan, and a capacity."""
    geo = slot_geometry(search_bits, n_streams, lap)
    tags = set()
    if geo.n_segs % SLOT_PER:
        tags.add("n_segs_ragged")
    if not keys:
        return tags
    assert list(keys) == sorted(keys)
    seg, pos = slot_segments(keys, geo, lap)
    assert (np.diff(seg) >= 0).all() and int(seg.max()) < geo.n_segs
    us, first, cnt = np.unique(seg, return_index=True, return_counts=True)
    if len(us) < geo.n_segs:
        tags.add("seg_0")
    for k, name in ((1, "seg_1"), (2, "seg_2"), (3, "seg_3")):
        if (cnt == k).any():
            tags.add(name)
    if (cnt > 4).any():                                      # (more than the four codes the scan's fast ranking keeps per segment)
        tags.add("seg_many")
    if (pos == 0).any():
        tags.add("seg_first_offset")
    if (pos == geo.seg_offsets - 1).any():
        tags.add("seg_last_offset")
    hit = set(int(s) for s in us)
    last_local = slot_segments([(0, int(search_bits) - 1)], geo, lap)[0][0]
    if any(s * geo.segs_per_stream + int(last_local) in hit and (s + 1) * geo.segs_per_stream in hit for s in range(n_streams - 1)):
        tags.add("stream_seam")
    per_block = SLOT_BLOCK * SLOT_PER
    if geo.n_segs > per_block and int(us.min()) < per_block <= int(us.max()):
        tags.add("two_place_workgroups")
    overflow = int(np.maximum(cnt - SLOT_N, 0).sum())
    tags.add("overflow_fits" if overflow <= cap else "overflow_full")
    if cap < len(keys):
        i = int(np.searchsorted(us, seg[cap]))               # the segment of the first record that is cut off
        rank, size = cap - int(first[i]), int(cnt[i])
        if rank == 1 and size >= 2 and SLOT_N >= 2:
            tags.add("cut_between_slots")
        if SLOT_N < rank < size:
            tags.add("cut_in_overflow")
    return tags


# ---- streams for the scan-counted path, order_single_kernel and the compaction ------------------------------------------------
#
# Built here so that tests/test_order_model.py can assert on the CPU, from the oracle's list, that each still carries its tags;
# tests/test_gpu_order_lattice.py runs the same streams on the device.  (The oracle must be initialised for two errors.)

def plant(sym, off, lap, errors=()):
    sw = synth.syncword(lap)
    for e in errors:
        sw ^= 1 << int(e)
    sym[off:off + 64] = synth.bits_lsb(sw, 64)


@functools.lru_cache(maxsize=None)
def chain_pool():
    """LAPs whose sync word may FOLLOW another one 57 symbols later: its seven lowest bits are the seven highest (barker code and LAP
    MSB) of a sync word with MSB 0 / 1.  -> {top seven bits: [lap, ...]}"""
    tops = {synth.syncword(l) >> 57 for l in (0, 1 << 23, 0x123456, 0xFEDCBA)}
    assert len(tops) == 2
    rng = np.random.default_rng(_libs.seed(57))
    pool = {t: [] for t in tops}
    for l in rng.integers(0, 1 << 24, 40000):
        low = synth.syncword(int(l)) & 0x7F
        if low in pool:
            pool[low].append(int(l))
    assert all(len(v) >= 100 for v in pool.values())
    return pool


BURST_WORDS = 1 << 16                                       # a stream of 2^22 offsets: 2048- or 4096-key buckets for caps of 600 / 300


@functools.lru_cache(maxsize=None)
def burst_stream(lap):
    """Noise with a burst of about 250 sync words that the segment slots refuse, and twenty sparse ones.
    Known LAP: back-to-back sync words from the first word of a 512-word tile, with one gap of 32 symbols behind the 60th: the wave
    that owns the tile's first 128 words then stages hits from all four of its chains (30 + 34 + 30 + 34) and finds 94 in its
    128-entry ring when 64 more may come -- scan_known.h gives up (`irregular`).  (Strictly back-to-back words fill the ring
    exactly: two chains of 64.)
    LAP_ANY: sync words 57 symbols apart, each one's seven lowest bits being the seven highest of the one before: 70 hits in the
    63 words of a wave where the candidate ring holds 64, so a hit is verified outside the drains.
    One hit per 64 (57) offsets: 32 (36) bucket-mates in buckets of 2048 keys, 64 (72) in buckets of 4096.
    -> (words, search_bits, the oracle's (stream, offset, lap, errors) list)"""
    rng = np.random.default_rng(_libs.seed(300 + (lap & 0xFF)))
    words = synth.noise_words(_libs.seed(3100) + (lap & 0xFFFF), 0, BURST_WORDS)
    sym = np.ascontiguousarray(synth.unpack_bits(words))
    if lap == LAP_ANY:
        pool = chain_pool()
        at, cur = 756 * 10 * 64, int(rng.integers(0, 1 << 24))
        for _ in range(250):
            plant(sym, at, cur)
            nxt = pool[synth.syncword(cur) >> 57]
            cur = nxt[int(rng.integers(0, len(nxt)))]
            at += 57
    else:
        first = 512 * 20 * 64
        for k in range(250):
            plant(sym, first + 64 * k + (32 if k >= 60 else 0), lap)
    for k in range(20):                                     # sparse ones: alone in their buckets
        off = (3000 + 3100 * k) * 64 + int(rng.integers(0, 64))
        plant(sym, off, lap if lap != LAP_ANY else int(rng.integers(0, 1 << 24)), rng.choice(57, k % 3, replace=False))
    bits = len(sym) - 63
    want = [(0, o, l, e) for (o, l, e) in _libs.orc_find_all(sym, bits, _libs.LAP_ANY if lap == LAP_ANY else lap, 2)]
    return synth.pack_bits(sym), bits, want


def as_records(tuples):
    h = np.zeros(len(tuples), bt.HIT_DTYPE)
    if tuples:
        a = np.array(tuples, dtype=np.uint64)
        h["stream"], h["offset"], h["lap"], h["ac_errors"] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    return h


@functools.lru_cache(maxsize=None)
def slot_stream(lap):
    """Three streams with a pitch, more than 8192 segments in all (LAP_ANY: 229 tiles of 756 words a stream = 8244 segments, no
    multiple of eight; known LAP: 342 tiles of 512 words = 8208), about 4.2 MiB of packed noise with planted sync words:
    one in every sixteenth segment or so, on both sides of segment 8192; segments with exactly 2, 3 and 20 hits; a sync word on the
    first and on the last offset of a segment; the last segment of a stream and the first of the next one both hit.
    -> (words of all streams, n_words, pitch, search_bits, the oracle's list, seconds the oracle took)"""
    any_lap = lap == LAP_ANY
    seg = 4032 if any_lap else 4096
    n_words = 229 * 756 if any_lap else 342 * 512
    pitch, n_streams = n_words + 24, 3
    bits = n_words * 64 - 63 - 11
    rng = np.random.default_rng(_libs.seed(400 + (lap & 0xFF)))
    pick = lambda: lap if not any_lap else int(rng.integers(0, 1 << 24))
    rows, want, oracle_s = [], [], 0.0
    last_seg = (bits - 1) // seg
    for ch in range(n_streams):
        sym = np.ascontiguousarray(synth.unpack_bits(synth.noise_words(_libs.seed(4100) + 77 * ch + (lap & 0xFFFF), 0, n_words)))
        dense = {100 + 400 * ch: 2, 101 + 400 * ch: 3, 103 + 400 * ch: 20, last_seg - 40 - ch: 20, last_seg - 30: 3, last_seg - 20: 2}
        for s in range(5 + ch, last_seg - 45, 16):          # one hit in every sixteenth segment
            if s not in dense and s - 1 not in dense:
                plant(sym, s * seg + int(rng.integers(70, seg - 140)), pick(), rng.choice(57, s % 3, replace=False))
        for s, k in dense.items():
            for off in np.sort(rng.choice((seg - 200) // 70, k, replace=False)) * 70 + 64:
                plant(sym, s * seg + int(off), pick(), rng.choice(57, int(off) % 3, replace=False))
        plant(sym, 300 * seg, pick())                       # the first offset of a segment
        plant(sym, 303 * seg - 1, pick())                   # the last offset of one
        plant(sym, 10, pick())                              # a stream's first segment ...
        plant(sym, bits - 1 - 64 * ch, pick())              # ... and its last (the last offset searched, in stream 0)
        t0 = time.time()
        want += [(ch, o, l, e) for (o, l, e) in _libs.orc_find_all(sym, bits, _libs.LAP_ANY if any_lap else lap, 2)]
        oracle_s += time.time() - t0
        rows.append(np.concatenate([synth.pack_bits(sym), np.zeros(pitch - n_words, np.uint64)]))
    return np.concatenate(rows), n_words, pitch, bits, want, oracle_s


def cut_caps(want, bits, lap):
    """Capacities that put the cut between a segment's two slots / inside its overflow records, as late in the list as there is such
    a segment (so that the overflow list, `cap` entries, still holds every overflow record)."""
    geo = slot_geometry(bits, 3, lap)
    seg, _ = slot_segments([(s, o) for (s, o, _, _) in want], geo, lap)
    us, first, cnt = np.unique(seg, return_index=True, return_counts=True)
    between = int(first[np.flatnonzero(cnt == 2)[-1]]) + 1
    inside = int(first[np.flatnonzero(cnt >= 10)[-1]]) + SLOT_N + 5
    return between, inside


# what the device tests run on these streams, and the tags each run exists for (asserted on the CPU from the oracle's list)
KNOWN_LAP = 0x9E8B33
STREAM_LAPS = (LAP_ANY, KNOWN_LAP)
BURST_CASES = ((600, "shared"), (300, "pairs"))             # (cap, the tag of the burst's buckets): buckets of 2048 / 4096 keys
SLOT_NEED = frozenset(("seg_0", "seg_1", "seg_2", "seg_3", "seg_many", "seg_first_offset", "seg_last_offset", "stream_seam",
                       "two_place_workgroups", "overflow_fits"))
OVERFLOW_FULL_CAP = 16


def slot_caps(want, bits, lap):
    """The capacities of the compaction test -> {tag the capacity exists for: cap}."""
    between, inside = cut_caps(want, bits, lap)
    return {"overflow_fits": len(want) + 50, "cut_between_slots": between, "cut_in_overflow": inside, "overflow_full": OVERFLOW_FULL_CAP}
