"""A numpy model of BR hop selection and of the CLK1-27 reversal, and the lattice of addresses, maps, clocks, slices and
reversal scenarios the hop kernels are pinned on (test infrastructure; tests/test_hop_lattice_model.py keeps the model and the
frozen tables honest on the CPU, tests/test_gpu_hop_lattice.py holds the kernels to them).

The model is written from the specification (vol 2 part B 2.6: the selection box, its inputs A-F, X, Y1, Y2, the PERM5 butterfly
and its control word) and from reading the reference's precalc / address_precalc / gen_hops / init_candidates / channel_winnow /
btbb_winnow.  It keeps the bits of the permuted word in five arrays and exchanges whole arrays, as the specification draws the
butterflies (once over every control word and input; the clocks then look their pair up); nothing of it follows the kernels'
table index or their byte shuffles."""
import functools
from collections import namedtuple

import numpy as np

SEQ_LEN = 1 << 27
M27 = SEQ_LEN - 1
N_GROUPS = 1 << 21                     # values of CLK7-27: groups of 64 hops
NCHAN = 79
E_ARG = -3                             # BTBBX_E_ARG

# PERM5: butterfly stage s exchanges these two wires when control bit P[s] is set (spec figure 2.17 / table 2.3)
STAGE_WIRES = ((0, 1), (2, 3), (1, 2), (3, 4), (0, 4), (1, 3), (0, 2), (3, 4), (1, 4), (0, 3), (2, 4), (1, 3), (0, 3), (1, 2))


# ---- the model ---------------------------------------------------------------------------------------------------------

def bank_of(afh_map):
    """(register bank, number of used channels): the even channels and then the odd ones, only the used ones under AFH"""
    order = [(2 * i) % NCHAN for i in range(NCHAN)]
    if afh_map is None:
        return np.array(order, np.uint8), NCHAN
    m = [int(x) for x in afh_map]
    assert len(m) == 10 and not m[9] & 0x80, "channel 79 does not exist: the reference reads behind its bank there"
    bank = [c for c in order if m[c // 8] >> (c % 8) & 1]
    return np.array(bank, np.uint8), sum(bin(x).count("1") for x in m)


def address_fields(address):
    """the selection inputs taken from the 28 address bits: (a1, b, c1, d1, e)"""
    a = int(address) & 0xFFFFFFF
    c1 = sum((a >> (2 * i) & 1) << i for i in range(5))
    e = sum((a >> (2 * i + 1) & 1) << i for i in range(7))
    return (a >> 23) & 31, (a >> 19) & 15, c1, (a >> 10) & 511, e


def make_address(a1, b, c1, d1, e):
    """an address with these inputs; address bits 11 and 13 belong to d1 AND to e, and e wins"""
    a = (a1 & 31) << 23 | (b & 15) << 19 | (d1 & 511) << 10
    for i in range(5):
        a |= (c1 >> i & 1) << (2 * i)
    for i in range(7):
        a = (a & ~(1 << (2 * i + 1))) | (e >> i & 1) << (2 * i + 1)
    assert address_fields(a)[:3] == (a1, b, c1) and address_fields(a)[4] == e
    return a


def _perm5(z, control, wires=STAGE_WIRES):
    """the 14 butterflies, stage 13 first, on the five bit arrays of z"""
    bits = [(z >> i) & 1 for i in range(5)]
    for s in range(13, -1, -1):
        u, v = wires[s]
        on = (control >> s & 1).astype(bool)
        bits[u], bits[v] = np.where(on, bits[v], bits[u]), np.where(on, bits[u], bits[v])
    return bits[0] | bits[1] << 1 | bits[2] << 2 | bits[3] << 3 | bits[4] << 4


@functools.lru_cache(maxsize=4)
def _perm_table(wires):
    """PERM5 of every (control word, input): the butterflies run once over all 2^19 pairs, the model looks the pairs up"""
    control, z = np.meshgrid(np.arange(1 << 14, dtype=np.int32), np.arange(32, dtype=np.uint8), indexing="ij")
    return _perm5(z.reshape(-1), control.reshape(-1), wires).reshape(1 << 14, 32)


def observable(ch, aliased, variant=None):
    """what a receiver that aliases the 79 channels onto 25 reports"""
    ch = np.asarray(ch).astype(np.int64)
    if not aliased:
        return ch
    return (ch + (25 if variant == "alias+1" else 24)) % 25 + 26


def model_hops(address, afh_map, clocks, variant=None):
    """the channel of every CLK1-27 value in `clocks` (any integers: masked to 27 bits) as uint8.  `variant` names one of the
    deliberate mistakes of WRONG_HOP_VARIANTS."""
    a1, b, c1, d1, e = address_fields(address)
    bank, used = bank_of(afh_map)
    afh = afh_map is not None
    mod = used if afh else NCHAN
    assert 1 <= mod <= NCHAN
    clk = (np.asarray(clocks).astype(np.int64) & M27).astype(np.int32)
    if mod == 1 and variant is None:                   # anything mod 1 is 0: every hop is the one channel
        return np.full(clk.shape, bank[0], np.uint8)
    if variant is not None and variant.startswith("b-bit"):
        b &= ~(1 << int(variant[-1]))
    y1, x, t = clk & 1, clk >> 1 & 31, clk >> 6        # (narrow integers from here on: the arrays are long)
    a = a1 ^ (t >> 14 & 31)
    c = c1 ^ (t >> 9 & 31)
    c = np.where(y1 == 1, c ^ 31, c)                   # Y1 flips C
    d = d1 ^ (t & 511)
    perm_in = (((x + a) % 32) ^ b).astype(np.uint8)
    wires = list(STAGE_WIRES)
    if variant == "stage-swap":
        wires[5], wires[6] = wires[6], wires[5]
    perm_out = _perm_table(tuple(wires))[c << 9 | d, perm_in].astype(np.int32)
    f = 16 * t % NCHAN
    if afh:
        f = 16 * t % used if variant == "fdash-single" else f % used
    index = perm_out + e + f + (0 if variant == "no-odd32" else 32 * y1)
    padded = np.zeros(NCHAN + 1, np.uint8)
    padded[:len(bank)] = bank
    if variant == "mod+1":
        return padded[index % (mod + 1)]
    out = padded[index % mod]
    if variant == "tab256":
        out = np.where(index < 256, out, 0).astype(np.uint8)
    return out


WRONG_HOP_VARIANTS = ("b-bit0", "b-bit1", "b-bit2", "b-bit3", "fdash-single", "mod+1", "stage-swap", "no-odd32", "tab256")


@functools.lru_cache(maxsize=8)
def _congruent_hops(address, afh_map, clk6):
    return model_hops(address, afh_map, clk6 + 64 * np.arange(N_GROUPS, dtype=np.int64))


def model_candidates(address, afh_map, clk6, channel, aliased, variant=None):
    """the ascending clocks clk6 + 64 j whose observable hop is `channel` (a channel above 127 never matches)"""
    clk6 &= 63
    if variant is None:
        hops = _congruent_hops(address, afh_map, clk6)
    else:
        hops = model_hops(address, afh_map, clk6 + 64 * np.arange(N_GROUPS, dtype=np.int64))
    if channel > 127:
        return np.zeros(0, np.uint32)
    j = np.nonzero(observable(hops, aliased, variant) == channel)[0]
    return (clk6 + 64 * j).astype(np.uint32)


def model_winnow(cands, offsets, channels, address, afh_map, aliased, variant=None, agreed=None):
    """(stop, count, cand0, survivors) of one winnowing call: the observations are applied in order, the walk stops at the first
    that leaves at most one candidate (stop = its index, or their number if none does), count and the ascending survivors are
    what is left then, cand0 the first of them (0 if none).  An empty list with observations gives (0, 0); no observations
    leave the list as it is.  `agreed`: a set of (offset, channel) every candidate of the list is known to agree with already
    (a caller that winnows one list call after call hands the same set in again); such an observation removes nothing and is
    not evaluated a second time."""
    cur = np.asarray(cands, dtype=np.uint32)
    first = lambda a: int(a[0]) if len(a) else 0
    n_obs = len(offsets)
    assert n_obs == len(channels)
    if n_obs == 0:
        return 0, len(cur), first(cur), cur
    if len(cur) == 0:
        return 0, 0, 0, cur
    least = 0 if variant == "stop<1" else 1
    one_channel = afh_map is not None and bank_of(afh_map)[1] == 1
    agreed = set() if agreed is None else agreed
    for k in range(n_obs):
        ch, key = int(channels[k]), (int(offsets[k]), int(channels[k]))
        if key in agreed:
            keep = np.ones(1, bool)
        elif ch > 127:
            keep = np.zeros(len(cur), bool)
        elif one_channel:                              # every clock hops on the one channel: all stay or all go
            same = int(observable(bank_of(afh_map)[0][0], aliased, variant)) == ch
            keep = np.ones(1, bool) if same else np.zeros(len(cur), bool)
        else:
            hops = model_hops(address, afh_map, cur.astype(np.int64) + int(offsets[k]))
            keep = observable(hops, aliased, variant) == ch
        agreed.add(key)
        if not keep.all():
            if variant == "block-order":               # survivors emitted per block of 1024, last block first
                blocks = [cur[i:i + 1024][keep[i:i + 1024]] for i in range(0, len(cur), 1024)]
                cur = np.concatenate(blocks[::-1])
            else:
                cur = cur[keep]
        if len(cur) <= least:
            return k, len(cur), first(cur), cur
    return n_obs, len(cur), first(cur), cur


WRONG_REVERSAL_VARIANTS = ("alias+1", "stop<1", "block-order")


# ---- selection points --------------------------------------------------------------------------------------------------

Config = namedtuple("Config", "tag address afh_map")       # afh_map: a tuple of 10 bytes, or None

E_VALUES = (0, 1, 2, 3, 124, 125, 126, 127, 41, 86)
MAP_KINDS = ("none", "u1", "u2", "u3", "u31", "u32", "u33", "u63", "u64", "u65", "u77", "u78", "u79", "u2adj", "u2ends")
ACD_KINDS = ("zeros", "ones", "random")


def map_of(channels):
    m = [0] * 10
    for c in channels:
        assert 0 <= c < NCHAN
        m[c // 8] |= 1 << (c % 8)
    return tuple(m)


def lattice_map(kind):
    if kind == "none":
        return None
    if kind == "u2adj":                                # neighbours in the bank: entries 20 and 21 of the even-then-odd order
        return map_of((40, 42))
    if kind == "u2ends":                               # the bank's first and last entries
        return map_of((0, 77))
    used = int(kind[1:])
    return map_of(np.random.default_rng(7900 + used).choice(NCHAN, size=used, replace=False).tolist())


def _config(i, kind, b, e, acd):
    rng = np.random.default_rng(5100 + i)
    a1, c1, d1 = {"zeros": (0, 0, 0), "ones": (31, 31, 511)}.get(acd) or (int(rng.integers(32)), int(rng.integers(32)), int(rng.integers(512)))
    address = make_address(a1, b, c1, d1, e)
    f = address_fields(address)
    return Config("%02d:%s/b%d/e%d/%s(a%d,c%d,d%d)" % (i, kind, b, e, acd, f[0], f[2], f[3]), address, lattice_map(kind))


@functools.lru_cache(maxsize=None)
def configs():
    """About 60 configurations: every b under basic hopping and under AFH, every e, every kind of map and of a1/c1/d1 -- each
    value of each dimension, not their product"""
    out = []
    for i in range(16):
        out.append(_config(len(out), "none", i, E_VALUES[i % 10], ACD_KINDS[i % 3]))
    for i in range(16):
        out.append(_config(len(out), MAP_KINDS[1 + i % 14], i, E_VALUES[(i + 5) % 10], ACD_KINDS[(i + 1) % 3]))
    for i in range(30):
        out.append(_config(len(out), MAP_KINDS[i % 15], (5 * i + 3) % 16, E_VALUES[(i // 3) % 10], ACD_KINDS[(i + 2) % 3]))
    return tuple(out)


def config_by_kind(kind, nth=0):
    return [c for c in configs() if c.tag.split(":")[1].split("/")[0] == kind][nth]


def lap_uap(cfg):
    return cfg.address & 0xFFFFFF, cfg.address >> 24


@functools.lru_cache(maxsize=None)
def groups_with_f(f, how_many=4):
    """groups t with 16 t mod 79 == f, by search: the first, the last and some between"""
    t = np.nonzero(16 * np.arange(N_GROUPS, dtype=np.int64) % NCHAN == f)[0]
    pick = np.linspace(0, len(t) - 1, how_many).astype(np.int64)
    return t[pick].tolist()


@functools.lru_cache(maxsize=None)
def edge_groups():
    return tuple(sorted(set(groups_with_f(0) + groups_with_f(78) + [0, N_GROUPS - 1])))


def clock_set(i):
    """the clocks btbbx_hop_channels_device gets for configuration i: 2^16 random 32-bit values and the 64 clocks of every edge
    group (f = 0, f = 78, the first and the last group)"""
    rng = np.random.default_rng(6200 + i)
    rand = rng.integers(0, 1 << 32, 1 << 16, dtype=np.uint64).astype(np.uint32)
    whole = (np.array(edge_groups(), np.int64)[:, None] * 64 + np.arange(64)).reshape(-1).astype(np.uint32)
    return np.concatenate([rand, whole])


SLICE_GROUPS = (1, 63, 64, 65, 255, 256, 257, 1000)
SLICE_FIRSTS = ("zero", "odd64", "f78", "end")
GUARD = 0xA5
GUARD_BYTES = 4096


def slices(i):
    """[(kind of first, first, count)] for configuration i: every count, with the four kinds of `first` dealt round so that
    all 32 pairs occur over the configurations"""
    out = []
    for k, g in enumerate(SLICE_GROUPS):
        count = 64 * g
        kind = SLICE_FIRSTS[(k + i + (i // 4)) % 4]
        first = {"zero": 0, "odd64": 64 * (2 * (1000 + 37 * i) + 1), "f78": 64 * groups_with_f(78)[1 + i % 2], "end": SEQ_LEN - count}[kind]
        out.append((kind, first, count))
    return out


# ---- reversal scenarios ------------------------------------------------------------------------------------------------
#
# A scenario: dict(tag, cfg = the configuration's index, c0 = the true clock at the first observation, aliased, obs, cuts, and
# what the model made of it when the table was built: n_open and one (n_before, stop, count) per call).  obs items:
#   o              an observation at offset o on the channel the piconet really hops to there
#   ("ch", o, ch)  an observation at offset o reported on channel ch (a contradiction, or a channel nobody hops on)
#   ("rep", k)     k observations repeating the earlier ones from the first on (they remove nothing)
#   ("rng", s, k)  k observations at random increasing offsets (seed s)
# The first observation opens the list; cuts = observations per winnowing call, the first call starting with observation 0.

def expand(scn):
    """(offsets int32, channels uint8) of a scenario"""
    cfg = configs()[scn["cfg"]]
    off, forced = [], {}
    for item in scn["obs"]:
        if isinstance(item, int):
            off.append(item)
        elif item[0] == "ch":
            forced[len(off)] = item[2]
            off.append(item[1])
        elif item[0] == "rep":
            for k in range(item[1]):
                if k % len(off) in forced:
                    forced[len(off)] = forced[k % len(off)]
                off.append(off[k % len(off)])
        else:
            rng = np.random.default_rng(item[1])
            off.extend((off[-1] + np.cumsum(rng.integers(1, 400, item[2]))).tolist())
    off = np.array(off, np.int64)
    ch = observable(model_hops(cfg.address, cfg.afh_map, scn["c0"] + off), scn["aliased"]).astype(np.uint8)
    for k, v in forced.items():
        ch[k] = v
    return off.astype(np.int32), ch


def replay(scn, variant=None):
    """the model over a scenario: (candidates after open, [(n_before, stop, count, cand0, survivors) per call])"""
    cfg = configs()[scn["cfg"]]
    off, ch = expand(scn)
    assert sum(scn["cuts"]) == len(off)
    cur = model_candidates(cfg.address, cfg.afh_map, scn["c0"] & 63, int(ch[0]), scn["aliased"], variant)
    opened, calls, at, agreed = cur, [], 0, set()
    for n in scn["cuts"]:
        stop, count, cand0, left = model_winnow(cur, off[at:at + n], ch[at:at + n], cfg.address, cfg.afh_map, scn["aliased"], variant,
                                                agreed)
        calls.append((len(cur), stop, count, cand0, left))
        cur, at = left, at + n
    return opened, calls


def one_call(scn):
    """the model over a scenario given as ONE job of the batch reversal: (n_initial, stop, count, cand0, survivors)"""
    opened, calls = replayed(scn["tag"])
    at = 0
    for n, (n_before, stop, count, cand0, left) in zip(scn["cuts"], calls):
        if n_before == 0 or stop < n:                  # the walk over all observations ends inside this call
            return len(opened), at + stop, count, cand0, left
        at += n
    return len(opened), at, count, cand0, left


class _Search:
    """builds one scenario: keeps the model's list while observations are added"""

    def __init__(self, tag, index, c0, aliased, seed):
        self.cfg = configs()[index]
        self.scn = dict(tag=tag, cfg=index, c0=c0, aliased=aliased, obs=[0], cuts=[])
        self.rng = np.random.default_rng(seed)
        ch0 = int(observable(model_hops(self.cfg.address, self.cfg.afh_map, [c0]), aliased)[0])
        self.cur = model_candidates(self.cfg.address, self.cfg.afh_map, c0 & 63, ch0, aliased)
        self.tries = 0

    def _after(self, cur, o):
        ch = int(observable(model_hops(self.cfg.address, self.cfg.afh_map, [self.scn["c0"] + o]), self.scn["aliased"])[0])
        hops = model_hops(self.cfg.address, self.cfg.afh_map, cur.astype(np.int64) + o)
        return cur[observable(hops, self.scn["aliased"]) == ch]

    def new(self, k=1):
        for _ in range(k):
            o = int(self.rng.integers(1, 200000))
            self.cur = self._after(self.cur, o)
            self.scn["obs"].append(o)
        return self

    def to(self, want, outer=400, inner=60, otherwise=None):
        """two more observations after which the list's length satisfies `want` (a number or a predicate): the last one is
        varied, and the one before it when that does not get there.  On a map of two channels an observation keeps one of two
        fixed shares of a list, so a length may be out of reach; `otherwise` is asked for then."""
        pred = want if callable(want) else (lambda n: n == want)
        if otherwise is not None:
            try:
                return self.to(want, outer, inner)
            except LookupError:
                return self.to(otherwise, 400, 60)
        for _ in range(outer):
            o1 = int(self.rng.integers(1, 200000))
            mid = self._after(self.cur, o1)
            for _ in range(inner):
                self.tries += 1
                o2 = int(self.rng.integers(1, 200000))
                left = self._after(mid, o2)
                if pred(len(left)):
                    self.cur = left
                    self.scn["obs"] += [o1, o2]
                    return self
        raise LookupError("%s: no two observations leave the length asked for" % self.scn["tag"])

    def add(self, *items):
        self.scn["obs"] += list(items)
        return self

    def done(self, cuts):
        self.scn["cuts"] = list(cuts)
        opened, calls = replay(self.scn)
        self.scn["n_open"] = len(opened)
        self.scn["calls"] = [c[:3] for c in calls]
        return self.scn


def _scenario_builders():
    """one function per scenario; each returns the _Search it built and the cuts"""
    top = SEQ_LEN - 64
    U1, U2, U32, U78, U79, U2ADJ, U2ENDS, BASIC, BASIC2, BASIC3 = 16, 17, 20, 26, 27, 28, 29, 7, 8, 14
    out = []

    def switch(want):
        # the kernel switch: exactly 16384 candidates (one workgroup) and exactly 16385 (four kernels, n mod 64 = 1) when a call begins
        s = _Search("u2/n%d" % want, U2, 64 * (70000 + want) + 21, 0, 100 + want).new(4).to(want)
        k = len(s.scn["obs"])
        return s.new(1).add(("rep", 255)).new(29), [k, 1, 255, 29]
    out += [lambda: switch(16384), lambda: switch(16385)]

    def prefix(want, otherwise, name):
        # the mask prefix with one word per lane and with two: 65536 candidates (1024 words) and 65537 (1025) where they can be had
        s = _Search("u2/%s" % name, U2, 64 * (900000 + want) + 21, 0, 200 + want).new(2).to(want, outer=12, otherwise=otherwise)
        k = len(s.scn["obs"])
        return s.new(40), [k, 2, 38]
    out += [lambda: prefix(65536, lambda n: 49152 < n <= 65536 and n % 64 == 0, "per1"),
            lambda: prefix(65537, lambda n: 65536 < n <= 81920, "per2")]

    def small(want):
        # n mod 64 = 63 on the large path, then 1023 / 1024 / 1025 candidates on the small one
        s = _Search("u2/n63/n%d" % want, U2, 64 * (1500000 + want) + 21, 0, 300 + want).new(3).to(lambda n: n > 16384 and n % 64 == 63)
        k = len(s.scn["obs"])
        s.new(3).to(want)
        k2 = len(s.scn["obs"])
        return s.new(1).add(("rep", 254)).new(30), [k, k2 - k, 1, 254, 30]
    out += [lambda: small(1023), lambda: small(1024), lambda: small(1025)]
    # every clock a candidate: 2 observations, and 1024 in one call with the true clock in the last group
    out.append(lambda: (_Search("u1/2obs", U1, 64 * 12345 + 17, 0, 401).new(1), [2]))
    out.append(lambda: (_Search("u1/1024obs/top", U1, top + 63, 0, 402).add(("rng", 402, 1023)), [1024]))
    # basic hopping: 1024 fresh observations in the first call (a large list); then calls on the one left and on none
    out.append(lambda: (_Search("basic/1024-large", BASIC, 64 * 777777 + 5, 0, 501).add(("rng", 501, 1023), 2000001, ("ch", 2000002, 79), 2000003),
                        [1024, 1, 1, 1]))
    # lists held back by repeats: 1024 observations without a stop on a large and on a small list, stops at the last and in the middle
    out.append(lambda: (_Search("basic/rep1024/group0", BASIC2, 31, 0, 502).add(("rep", 1023)).to(2).add(("rep", 1023)).new(9), [1024, 2, 1024, 8]))
    out.append(lambda: (_Search("basic/stop-last-of-1023/top", BASIC, top + 1, 0, 503).to(2).add(("rep", 1022)).new(1).add(("rep", 255)),
                        [3, 1023, 255]))
    out.append(lambda: (_Search("aliased/basic/stop-mid-257", BASIC3, 64 * 4242 + 9, 1, 504).new(2).to(2).add(("rep", 124)).new(8).add(("rep", 125))
                        .add(("ch", 5, 128), 7), [5, 257, 1, 1]))
    # aliased on a map, the true clock in the last group: candidate + offset passes 2^27; calls of 1 and 2 observations
    out.append(lambda: (_Search("aliased/u32/top", U32, top + 40, 1, 505).new(40), [1, 2, 38]))
    out.append(lambda: (_Search("aliased/basic/256", BASIC2, 13, 1, 506).add(("rng", 506, 255)), [256]))
    # contradictions at a named observation: channels nobody hops on
    out.append(lambda: (_Search("basic/contradiction-255-at-3", BASIC3, 64 * 99999 + 1, 0, 507).new(2).add(("ch", 777, 255)).new(3), [4, 3]))
    out.append(lambda: (_Search("u78/contradiction-79", U78, 64 * 5 + 62, 0, 508).new(1).add(("ch", 4000, 79)).new(2), [2, 1, 2]))

    def empty():
        s = _Search("basic/open-on-128", BASIC, 1000, 0, 509)
        s.scn["obs"] = [("ch", 0, 128), 50, 60]
        return s, [2, 1]
    out.append(empty)
    # exactly two candidates left at the end of a call, the stop at the first observation of the next
    out.append(lambda: (_Search("u79/two-left", U79, 64 * 1500000 + 33, 0, 510).to(2).add(("rep", 2)).new(8), [3, 2, 8]))
    out.append(lambda: (_Search("u2adj/255", U2ADJ, 64 * 31 + 7, 0, 511).add(("rng", 511, 254)).add(("rep", 257)).new(1), [255, 257, 1]))
    out.append(lambda: (_Search("u2ends/256", U2ENDS, 64 * 2000000 + 2, 0, 512).add(("rng", 512, 255)).add(("rep", 1023)), [256, 1023]))
    return out


def search_scenarios(which=None, log=print):
    """Rebuilds the table of SCENARIOS with the model (minutes of CPU; `which`: indices, to share the work between processes):
    the lengths 16384 / 16385, 65536 / 65537, 1023 / 1024 / 1025 and 2 are found by trying observations.  Returns the list;
    its repr is what stands below."""
    out = []
    for i, build in enumerate(_scenario_builders()):
        if which is None or i in which:
            search, cuts = build()
            s = search.done(cuts)
            log("%-30s tries %-6d n_open %-8d calls %s" % (s["tag"], search.tries, s["n_open"], s["calls"]))
            out.append(s)
    return out


def scenario(tag):
    return [s for s in SCENARIOS if s["tag"] == tag][0]


@functools.lru_cache(maxsize=None)
def replayed(tag):
    """replay() of a frozen scenario, once per process (nobody changes the arrays)"""
    return replay(scenario(tag))


# what search_scenarios() returned; tests/test_hop_lattice_model.py recomputes every figure in it with the model
SCENARIOS = (
    {'tag': 'u2/n16384', 'cfg': 17, 'c0': 5528597, 'aliased': 0, 'cuts': [7, 1, 255, 29], 'n_open': 1048070,
     'calls': [(1048070, 7, 16384), (16384, 1, 9017), (9017, 255, 9017), (9017, 12, 1)],
     'obs': [0, 164419, 1586, 24545, 72470, 9246, 195535, 177586, ('rep', 255), 48973, 138085, 85388, 18926, 38352, 89896, 17437, 12567, 116720,
             19764, 122303, 159837, 10809, 128902, 183733, 126063, 116182, 101305, 94671, 137751, 35092, 42244, 11097, 122826, 6403, 48066, 85296,
             111364, 140953]},
    {'tag': 'u2/n16385', 'cfg': 17, 'c0': 5528661, 'aliased': 0, 'cuts': [7, 1, 255, 29], 'n_open': 1049082,
     'calls': [(1049082, 7, 16385), (16385, 1, 7188), (7188, 255, 7188), (7188, 12, 1)],
     'obs': [0, 123557, 80850, 184654, 185730, 173077, 30574, 182284, ('rep', 255), 196365, 100815, 58308, 136857, 33716, 63509, 95467, 117157,
             56384, 184862, 170899, 198974, 148951, 155519, 191219, 144528, 109705, 161736, 193401, 53876, 26545, 82306, 180919, 99293, 7480, 6150,
             23435, 120926, 126646]},
    # (65536 and 65537 candidates, the two sides of 1024 mask words, are out of reach of this map: an observation keeps one of
    # two fixed shares of a list, and their products pass the two lengths by; 62080 is 970 words, 68083 is 1064)
    {'tag': 'u2/per1', 'cfg': 17, 'c0': 61794325, 'aliased': 0, 'cuts': [5, 2, 38], 'n_open': 1048070,
     'calls': [(1048070, 5, 62080), (62080, 2, 17637), (17637, 13, 1)],
     'obs': [0, 57332, 147358, 186034, 18028, 42814, 120061, 147568, 8876, 99181, 172983, 70025, 42981, 137314, 108502, 104217, 99602, 57040, 67721,
             166126, 177171, 38828, 76669, 158989, 193751, 26667, 66434, 96655, 136801, 149838, 176722, 159198, 91466, 171288, 147743, 39176, 76371,
             15575, 108735, 4260, 154361, 122817, 91222, 152619, 67091]},
    {'tag': 'u2/per2', 'cfg': 17, 'c0': 61794389, 'aliased': 0, 'cuts': [5, 2, 38], 'n_open': 1048070,
     'calls': [(1048070, 5, 68083), (68083, 2, 21284), (21284, 13, 1)],
     'obs': [0, 112114, 14681, 135460, 186797, 47858, 105599, 124864, 186505, 29337, 192157, 42444, 83118, 11839, 41803, 170347, 155726, 109358,
             183857, 12553, 52467, 189058, 125789, 132078, 186220, 150515, 16839, 34295, 102895, 24828, 104806, 97528, 172082, 189706, 39986, 18748,
             193095, 189576, 49113, 165452, 25821, 71779, 115266, 74800, 86661]},
    {'tag': 'u2/n63/n1023', 'cfg': 17, 'c0': 96065493, 'aliased': 0, 'cuts': [6, 5, 1, 254, 30], 'n_open': 1048070,
     'calls': [(1048070, 6, 33599), (33599, 5, 1023), (1023, 1, 442), (442, 254, 442), (442, 9, 1)],
     'obs': [0, 595, 137788, 80131, 180955, 55404, 130468, 137956, 148215, 63736, 99349, 83875, ('rep', 254), 176390, 28023, 59709, 40149, 46043,
             30066, 198441, 106646, 52504, 46053, 132472, 112348, 127049, 69513, 82206, 113968, 169933, 140783, 36820, 143296, 64954, 9211, 38591,
             41919, 95374, 30550, 179701, 113966, 197080, 94196]},
    {'tag': 'u2/n63/n1024', 'cfg': 17, 'c0': 96065557, 'aliased': 0, 'cuts': [6, 5, 1, 254, 30], 'n_open': 1049082,
     'calls': [(1049082, 6, 34559), (34559, 5, 1024), (1024, 1, 621), (621, 254, 621), (621, 12, 1)],
     'obs': [0, 8795, 44606, 117406, 62506, 87529, 136119, 149408, 115072, 156267, 83973, 72310, ('rep', 254), 88766, 63197, 98953, 50930, 40017,
             126004, 174899, 41573, 290, 31322, 167950, 17576, 172792, 86199, 155553, 168276, 172638, 64487, 119698, 45841, 107159, 147821, 72305,
             14944, 135363, 16802, 69742, 86819, 104800, 17409]},
    {'tag': 'u2/n63/n1025', 'cfg': 17, 'c0': 96065621, 'aliased': 0, 'cuts': [6, 5, 1, 254, 30], 'n_open': 1049082,
     'calls': [(1049082, 6, 33215), (33215, 5, 1025), (1025, 1, 612), (612, 254, 612), (612, 8, 1)],
     'obs': [0, 156059, 198989, 111996, 66856, 75257, 116812, 153065, 8446, 63914, 6128, 186887, ('rep', 254), 20695, 71022, 104927, 94092, 7939,
             22149, 6352, 47373, 12158, 184570, 189224, 153916, 61609, 14914, 168744, 11473, 120200, 18430, 163415, 175823, 68107, 131903, 61749,
             171547, 29211, 53516, 25164, 181989, 1044, 6037]},
    {'tag': 'u1/2obs', 'cfg': 16, 'c0': 790097, 'aliased': 0, 'cuts': [2], 'n_open': 2097152, 'calls': [(2097152, 2, 2097152)], 'obs': [0, 85952]},
    {'tag': 'u1/1024obs/top', 'cfg': 16, 'c0': 134217727, 'aliased': 0, 'cuts': [1024], 'n_open': 2097152, 'calls': [(2097152, 1024, 2097152)],
     'obs': [0, ('rng', 402, 1023)]},
    {'tag': 'basic/1024-large', 'cfg': 7, 'c0': 49777733, 'aliased': 0, 'cuts': [1024, 1, 1, 1], 'n_open': 26599,
     'calls': [(26599, 3, 1), (1, 0, 1), (1, 0, 0), (0, 0, 0)], 'obs': [0, ('rng', 501, 1023), 2000001, ('ch', 2000002, 79), 2000003]},
    {'tag': 'basic/rep1024/group0', 'cfg': 8, 'c0': 31, 'aliased': 0, 'cuts': [1024, 2, 1024, 8], 'n_open': 26428,
     'calls': [(26428, 1024, 26428), (26428, 2, 2), (2, 1024, 2), (2, 0, 1)],
     'obs': [0, ('rep', 1023), 113344, 46952, ('rep', 1023), 48836, 88645, 7900, 196875, 34820, 1315, 155594, 9235, 164761]},
    {'tag': 'basic/stop-last-of-1023/top', 'cfg': 7, 'c0': 134217665, 'aliased': 0, 'cuts': [3, 1023, 255], 'n_open': 26375,
     'calls': [(26375, 3, 2), (2, 1022, 1), (1, 0, 1)], 'obs': [0, 52105, 82322, ('rep', 1022), 143091, ('rep', 255)]},
    {'tag': 'aliased/basic/stop-mid-257', 'cfg': 14, 'c0': 271497, 'aliased': 1, 'cuts': [5, 257, 1, 1], 'n_open': 106216,
     'calls': [(106216, 5, 2), (2, 124, 1), (1, 0, 0), (0, 0, 0)],
     'obs': [0, 176383, 2594, 9518, 4792, ('rep', 124), 97348, 118761, 43214, 143197, 150321, 180944, 102124, 191384, ('rep', 125), ('ch', 5, 128), 7]},
    {'tag': 'aliased/u32/top', 'cfg': 20, 'c0': 134217704, 'aliased': 1, 'cuts': [1, 2, 38], 'n_open': 196550,
     'calls': [(196550, 1, 196550), (196550, 2, 194), (194, 1, 1)],
     'obs': [0, 162205, 170084, 61139, 140667, 148439, 3486, 62334, 199844, 40063, 155858, 83189, 102023, 134222, 15659, 43838, 65528, 56762, 161188,
             190627, 135261, 35171, 160527, 61750, 194954, 159947, 114896, 130131, 46504, 68221, 59113, 180806, 169373, 123252, 102165, 9436, 130815,
             125818, 73806, 179966, 162907]},
    {'tag': 'aliased/basic/256', 'cfg': 8, 'c0': 13, 'aliased': 1, 'cuts': [256], 'n_open': 79726, 'calls': [(79726, 5, 1)],
     'obs': [0, ('rng', 506, 255)]},
    {'tag': 'basic/contradiction-255-at-3', 'cfg': 14, 'c0': 6399937, 'aliased': 0, 'cuts': [4, 3], 'n_open': 26700,
     'calls': [(26700, 3, 0), (0, 0, 0)], 'obs': [0, 142617, 53792, ('ch', 777, 255), 7413, 47230, 46058]},
    {'tag': 'u78/contradiction-79', 'cfg': 26, 'c0': 382, 'aliased': 0, 'cuts': [2, 1, 2], 'n_open': 27065,
     'calls': [(27065, 2, 504), (504, 0, 0), (0, 0, 0)], 'obs': [0, 101637, ('ch', 4000, 79), 169171, 48667]},
    {'tag': 'basic/open-on-128', 'cfg': 7, 'c0': 1000, 'aliased': 0, 'cuts': [2, 1], 'n_open': 0, 'calls': [(0, 0, 0), (0, 0, 0)],
     'obs': [('ch', 0, 128), 50, 60]},
    {'tag': 'u79/two-left', 'cfg': 27, 'c0': 96000033, 'aliased': 0, 'cuts': [3, 2, 8], 'n_open': 26599,
     'calls': [(26599, 3, 2), (2, 2, 2), (2, 0, 1)],
     'obs': [0, 24589, 195854, ('rep', 2), 23896, 198315, 101864, 36717, 122312, 181046, 50787, 103828]},
    {'tag': 'u2adj/255', 'cfg': 28, 'c0': 1991, 'aliased': 0, 'cuts': [255, 257, 1], 'n_open': 1048468,
     'calls': [(1048468, 20, 1), (1, 0, 1), (1, 0, 1)], 'obs': [0, ('rng', 511, 254), ('rep', 257), 151402]},
    {'tag': 'u2ends/256', 'cfg': 29, 'c0': 128000002, 'aliased': 0, 'cuts': [256, 1023], 'n_open': 1048476,
     'calls': [(1048476, 22, 1), (1, 0, 1)], 'obs': [0, ('rng', 512, 255), ('rep', 1023)]},
)
