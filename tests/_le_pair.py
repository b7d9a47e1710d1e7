"""Test-side model of LE legacy pairing key recovery (include/btbbx.h btbbx_le_pair_device, rules 1 to 9) -- Python over the message
tuples of tests/_le_data.py, written from the rules and not from the kernels.  AES is tests/_le_crypt.py's (built from its
definition); the search over the tk axis is the same AES in numpy, an S-box look-up by fancy indexing, one key schedule and two
blocks per lane, held against the scalar aes by tests/test_le_pair_model.py.

* key / c1 / s1: the primitives, over arrays as received (least significant octet first)
* Rules: the model's branch points as options; VARIANTS are deliberately wrong models
* pair: the model -> Out(pairs, keys, n_keys)
* exchange: the SMP messages of one pairing, planted under a TK; Plant: hand-made message lists
* pair_world / pair_capture / capture_model: a connection that pairs and then encrypts under its STK, as records and as a capture
"""
import collections
import functools

import numpy as np

import _le_crypt as cm
import _le_data as dm

NONE_M, LEGACY, SECURE, OOB, INVALID = range(5)
F_PREQ, F_PRSP, F_MCONF, F_SCONF, F_MRAND, F_SRAND, F_ARMED, F_CRACKED = 1, 2, 4, 8, 16, 32, 64, 128
K_STK, K_LTK_CENTRAL, K_LTK_PERIPHERAL = 1, 2, 4
NONE = 0xFFFFFFFF
SMP_CID = 6
SEEDED = 1

Pair = collections.namedtuple("Pair", "stk ltk preq prsp mconf sconf mrand srand tk method flags keys key_size key")
Out = collections.namedtuple("Out", "pairs keys n_keys")
Seed = collections.namedtuple("Seed", "init_a adv_a tx_add rx_add flags")
NOTHING = Pair(bytes(16), (bytes(16), bytes(16)), NONE, NONE, NONE, NONE, NONE, NONE, NONE, 0, 0, 0, 0, 0xFF)


class Rules:
    """Rules() is the model; every other value is a wrong one."""

    def __init__(self, **kw):
        self.a_swapped = False              # rule 4: a = iat, rat, pres, preq
        self.types_swapped = False          # rule 4: a = rat, iat, ...
        self.addresses_swapped = False      # rule 4: b = init_a, adv_a
        self.random_as_received = False     # rule 4: block(r)[j] = r[j]
        self.confirm_as_received = False    # rule 4: conf compared without reading the output block back
        self.tk_in_front = False            # rule 4: BE32(tk) in key octets 0..3
        self.s1_swapped = False             # rule 6: c = srand[0..7], mrand[0..7]
        self.stk_whole = False              # rule 6: the STK is not cut to the key size
        self.stk_cut_at_the_end = False     # rule 6: output octets ks .. 15 set to zero
        self.prsp_anywhere = False          # rule 2: PRSP is the first such message, above PREQ or not
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


MODEL = Rules()
VARIANTS = {name: {name: True} for name in ("a_swapped", "types_swapped", "addresses_swapped", "random_as_received", "confirm_as_received",
                                            "tk_in_front", "s1_swapped", "stk_whole", "stk_cut_at_the_end", "prsp_anywhere")}


# ---- the primitives ------------------------------------------------------------------------------------------------------------------
def key(tk, rules=MODEL):
    """Key octets, most significant first: 0..11 zero, 12..15 BE32(tk)."""
    be = int(tk).to_bytes(4, "big")
    return be + bytes(12) if rules.tk_in_front else bytes(12) + be


def _xor(x, y):
    return bytes(p ^ q for p, q in zip(x, y))


def _arrays(preq, pres, iat, rat, init_a, adv_a, rules=MODEL):
    """Rule 4's a and b, least significant octet first."""
    types = bytes([rat, iat]) if rules.types_swapped else bytes([iat, rat])
    a = types + (bytes(pres) + bytes(preq) if rules.a_swapped else bytes(preq) + bytes(pres))
    b = (bytes(init_a) + bytes(adv_a) if rules.addresses_swapped else bytes(adv_a) + bytes(init_a)) + bytes(4)
    assert len(a) == 16 and len(b) == 16
    return a, b


def c1(tk, r, preq, pres, iat, rat, init_a, adv_a, rules=MODEL):
    """Rule 4 -> the Confirm value as it is sent (octets 1..16 of the message).  r, preq, pres, init_a, adv_a: as received."""
    a, b = _arrays(preq, pres, iat, rat, init_a, adv_a, rules)
    k = key(tk, rules)
    first = _xor(r, a) if rules.random_as_received else _xor(r, a)[::-1]       # block[j] = x[15 - j]
    p = cm.aes(k, first)                                                        # an output block, not read back: o ^ block(b)
    o = cm.aes(k, _xor(p, b[::-1]))
    return o if rules.confirm_as_received else o[::-1]                          # x[i] = o[15 - i]


def s1(tk, mrand, srand, ks=16, rules=MODEL):
    """Rule 6 -> the STK, output octet 0 first.  mrand, srand: the Random values as received (16 octets each)."""
    c = bytes(srand[:8]) + bytes(mrand[:8]) if rules.s1_swapped else bytes(mrand[:8]) + bytes(srand[:8])
    stk = cm.aes(key(tk, rules), c[::-1])
    if rules.stk_whole:
        return stk
    return stk[:ks] + bytes(16 - ks) if rules.stk_cut_at_the_end else bytes(16 - ks) + stk[16 - ks:]


# ---- AES over the tk axis ------------------------------------------------------------------------------------------------------------
_SB = np.array(cm.SBOX, np.uint8)
_SHIFT = [r + 4 * ((c + r) % 4) for c in range(4) for r in range(4)]


def _xtime(a):
    return ((a << 1) & 0xFF).astype(np.uint8) ^ np.where(a & 0x80, 0x1B, 0).astype(np.uint8)


def schedules(keys):
    """keys: (n, 16) uint8 -> the round keys, (n, 11, 16)."""
    n = len(keys)
    w = np.zeros((n, 44, 4), np.uint8)
    w[:, :4] = keys.reshape(n, 4, 4)
    rcon = 1
    for i in range(4, 44):
        t = w[:, i - 1].copy()
        if i % 4 == 0:
            t = _SB[np.roll(t, -1, axis=1)]
            t[:, 0] ^= rcon
            rcon = cm._gmul(rcon, 2)
        w[:, i] = w[:, i - 4] ^ t
    return w.reshape(n, 11, 16)


def aes_many(rk, blocks):
    """rk: (n, 11, 16); blocks: (n, 16) or (16,) uint8 -> (n, 16)."""
    n = len(rk)
    s = np.broadcast_to(np.asarray(blocks, np.uint8), (n, 16)) ^ rk[:, 0]
    for rnd in range(1, 11):
        s = _SB[s][:, _SHIFT]
        if rnd < 10:
            a = s.reshape(n, 4, 4)
            a1, a2, a3 = np.roll(a, -1, axis=2), np.roll(a, -2, axis=2), np.roll(a, -3, axis=2)
            s = (_xtime(a) ^ _xtime(a1) ^ a1 ^ a2 ^ a3).reshape(n, 16)
        s = s ^ rk[:, rnd]
    return s


def keys_of(tks, rules=MODEL):
    tks = np.asarray(tks, np.uint32)
    k = np.zeros((len(tks), 16), np.uint8)
    at = 0 if rules.tk_in_front else 12
    for j in range(4):
        k[:, at + j] = (tks >> (8 * (3 - j))) & 0xFF
    return k


def search(checks, a, b, tks, rules=MODEL):
    """Rule 5 over the values tks (ascending): the smallest under which every check (r, conf) holds, or NONE."""
    tks = np.asarray(tks, np.uint32)
    for lo in range(0, len(tks), 1 << 15):
        part = tks[lo:lo + (1 << 15)]
        rk = schedules(keys_of(part, rules))
        ok = np.ones(len(part), bool)
        for r, conf in checks:
            first = _xor(r, a) if rules.random_as_received else _xor(r, a)[::-1]
            p = aes_many(rk, np.frombuffer(first, np.uint8))
            o = aes_many(rk, p ^ np.frombuffer(b[::-1], np.uint8))
            want = conf if rules.confirm_as_received else conf[::-1]
            ok &= (o == np.frombuffer(bytes(want), np.uint8)).all(axis=1)
        if ok.any():
            return int(part[np.flatnonzero(ok)[0]])
    return NONE


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def _smp(m, k, payload, byte_cap):
    """Rule 1 and the guards -> the message's octets, or None."""
    if m.conn >= k or m.byte_offset + m.bytes > byte_cap or m.bytes < 4 + m.l2cap_len:
        return None
    need = dm.COMPLETE | dm.STORED
    if m.flags & need != need or m.cid != SMP_CID or m.l2cap_len < 1:
        return None
    return bytes(payload[m.byte_offset + 4:m.byte_offset + 4 + m.l2cap_len])


def pair(k, seeds, msgs, payload, byte_cap, tk_limit, key_cap, rules=MODEL, claims=None):
    """k: the connections; seeds: one Seed (or anything with its fields) or None per connection; msgs: the W records that are looked
    at; claims: per connection the only tk values that are tried (ascending), where the whole range would take the model too long -- a
    128-bit match has no false positive.  -> Out: one Pair per connection, the key table (key_cap * 16 octets) and the key count."""
    octets = [_smp(m, k, payload, byte_cap) for m in msgs]
    pairs = []
    for g in range(k):
        mine = [M for M, m in enumerate(msgs) if octets[M] is not None and m.conn == g]

        def first(role, code, length, above, mine=mine):
            if above is None:
                return None
            return next((M for M in mine if M > above and msgs[M].role == role and octets[M][0] == code and len(octets[M]) == length), None)

        preq = first(dm.CENTRAL, 1, 7, -1)
        prsp = first(dm.PERIPHERAL, 2, 7, -1 if rules.prsp_anywhere and preq is not None else preq)
        mconf = first(dm.CENTRAL, 3, 17, prsp)
        sconf = first(dm.PERIPHERAL, 3, 17, mconf)
        mrand = first(dm.CENTRAL, 4, 17, sconf if sconf is not None else mconf)
        srand = first(dm.PERIPHERAL, 4, 17, mrand)
        proc = [preq, prsp, mconf, sconf, mrand, srand]
        flags = sum(bit for bit, M in zip((F_PREQ, F_PRSP, F_MCONF, F_SCONF, F_MRAND, F_SRAND), proc) if M is not None)
        method, ks = NONE_M, 0
        if preq is not None and prsp is not None:                   # rule 3
            q, s = octets[preq], octets[prsp]
            ks = min(q[4], s[4])
            if ks < 7 or ks > 16:
                method = INVALID
            elif q[3] & s[3] & 8:
                method = SECURE
            elif q[2] == 1 and s[2] == 1:
                method = OOB
            else:
                method = LEGACY
        checks = []                                                 # rule 4
        if mconf is not None and mrand is not None:
            checks.append((octets[mrand][1:], octets[mconf][1:]))
        if sconf is not None and srand is not None:
            checks.append((octets[srand][1:], octets[sconf][1:]))
        seed = seeds[g]
        tk, stk, keys = NONE, bytes(16), 0
        if method == LEGACY and seed is not None and seed.flags & SEEDED and checks and tk_limit >= 1:
            flags |= F_ARMED
            a, b = _arrays(octets[preq], octets[prsp], seed.tx_add & 1, seed.rx_add & 1, seed.init_a, seed.adv_a, rules)
            tks = range(tk_limit) if claims is None else [t for t in claims[g] if t < tk_limit]
            tk = search(checks, a, b, list(tks), rules) if len(tks) else NONE                         # rule 5
            if tk != NONE:
                flags |= F_CRACKED
                if mrand is not None and srand is not None:         # rule 6
                    stk, keys = s1(tk, octets[mrand][1:], octets[srand][1:], ks, rules), K_STK
        ltk = []
        for role, bit in ((dm.CENTRAL, K_LTK_CENTRAL), (dm.PERIPHERAL, K_LTK_PERIPHERAL)):                # rule 8
            M = first(role, 6, 17, -1)
            ltk.append(octets[M][:0:-1] if M is not None else bytes(16))
            keys |= bit if M is not None else 0
        pairs.append(Pair(stk, tuple(ltk), *[NONE if M is None else M for M in proc], tk, method, flags, keys, ks, 0xFF))
    table, n_keys = bytearray(16 * key_cap), 0                      # rule 7
    for g, p in enumerate(pairs):
        if p.keys & K_STK:
            if n_keys < key_cap:
                table[16 * n_keys:16 * n_keys + 16] = p.stk
                pairs[g] = p._replace(key=n_keys)
            n_keys += 1
    return Out(pairs, bytes(table), n_keys)


def pair_array(pairs, dtype):
    a = np.zeros(len(pairs), dtype)
    for i, p in enumerate(pairs):
        a[i] = (list(p.stk), [list(p.ltk[0]), list(p.ltk[1])]) + tuple(p[2:]) + ((0,) * 7,)
    return a


# ---- planted exchanges ---------------------------------------------------------------------------------------------------------------
def octets(seed, n):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tolist())


PREQ7 = bytes([1, 4, 0, 0x05, 16, 7, 7])                           # KeyboardDisplay, bonding | MITM, key size 16
PRSP7 = bytes([2, 0, 0, 0x05, 16, 7, 7])                           # DisplayOnly: the passkey is shown there and typed here


def exchange(tk, seed, n=0, ks=(16, 16), preq=None, pres=None, tk_peripheral=None):
    """The six SMP messages of one legacy pairing under tk between the addresses of `seed`, as (role, octets) in time order; n picks
    the Random values; ks: the two maximum key sizes; tk_peripheral: the peripheral's Confirm made under another TK.
    -> (messages, mrand, srand)."""
    preq = bytes(preq) if preq is not None else PREQ7[:4] + bytes([ks[0]]) + PREQ7[5:]
    pres = bytes(pres) if pres is not None else PRSP7[:4] + bytes([ks[1]]) + PRSP7[5:]
    mrand, srand = octets(7000 + 2 * n, 16), octets(7001 + 2 * n, 16)
    iat, rat = seed.tx_add & 1, seed.rx_add & 1
    mconf = c1(tk, mrand, preq, pres, iat, rat, seed.init_a, seed.adv_a)
    sconf = c1(tk if tk_peripheral is None else tk_peripheral, srand, preq, pres, iat, rat, seed.init_a, seed.adv_a)
    return ([(dm.CENTRAL, preq), (dm.PERIPHERAL, pres), (dm.CENTRAL, b"\x03" + mconf), (dm.PERIPHERAL, b"\x03" + sconf),
             (dm.CENTRAL, b"\x04" + mrand), (dm.PERIPHERAL, b"\x04" + srand)], mrand, srand)


def seed_of(n, seeded=True, tx_add=None, rx_add=None):
    return Seed(octets(8000 + n, 6), octets(8100 + n, 6), n & 1 if tx_add is None else tx_add, (n >> 1) & 1 if rx_add is None else rx_add,
                SEEDED if seeded else 0)


class Plant:
    """A hand-made message list: add() appends one message of a connection and returns its index."""

    def __init__(self, pad=0):
        self.msgs, self.payload = [], bytearray(b"\x5a" * pad)

    def add(self, conn, role, body, cid=SMP_CID, flags=dm.COMPLETE | dm.STORED, claim=None, bytes_=None, offset=None, fill=0):
        frame = dm.l2cap(cid, body, claim)
        self.payload += b"\x5a" * fill                              # (octets of no message: the next one lies at another residue)
        at = len(self.payload) if offset is None else offset
        if offset is None:
            self.payload += frame
        self.msgs.append(dm.Msg(at, conn, 0, 1, len(frame) if bytes_ is None else bytes_, len(body) if claim is None else claim, cid, role, flags))
        return len(self.msgs) - 1

    def all(self, conn, messages, **kw):
        return [self.add(conn, role, body, **kw) for role, body in messages]


# ---- a planted capture -----------------------------------------------------------------------------------------------------------------
WORLD_TK = 271828
LEGACY_NAME, PLAIN_NAME, SECURE_NAME = "pair: legacy, then encrypts under the STK", "pair: never pairs", "pair: Secure Connections"
WORLD_SEEDS = {LEGACY_NAME: seed_of(1), PLAIN_NAME: seed_of(2), SECURE_NAME: seed_of(5)}
DISTRIBUTED_LTK = b"\x06" + octets(41, 16)                         # the Encryption Information the peripheral sends under the STK


@functools.lru_cache(maxsize=None)
def pair_world():
    """tests/_le_crypt.py's CryptWorld with a connection that pairs (SMP over its data PDUs, passkey WORLD_TK) and then encrypts under
    the STK, one that never pairs and one that pairs with LE Secure Connections.  No PDU is longer than 27 octets on the air.
    -> (Built, the STK)"""
    P, E, REQ, RSP, BEGIN = cm.P, cm.E, cm.REQ, cm.RSP, cm.BEGIN
    w = cm.CryptWorld(seed=33)
    r = np.random.default_rng(9)
    rest = lambda first, last: [(c, [E, E]) for c in range(first, last)]                       # noqa: E731
    messages, mrand, srand = exchange(WORLD_TK, WORLD_SEEDS[LEGACY_NAME], n=40)
    stk = s1(WORLD_TK, mrand, srand, 16)
    smp = [dm.l2cap(SMP_CID, body) for _, body in messages]
    a19, b30, c9 = (dm.l2cap(4, dm._octets(r, n)) for n in (15, 26, 5))
    w.conn(LEGACY_NAME, [(0, [P(2, c9), E]), (1, [P(2, smp[0]), P(2, smp[1])]), (2, [P(2, smp[2]), P(2, smp[3])]),
                         (3, [P(2, smp[4]), P(2, smp[5])]), (4, [REQ, RSP]), (5, [E, BEGIN]), (6, [P(3, b"\x06"), P(3, b"\x06")]),
                         (7, [P(2, a19), P(2, dm.l2cap(SMP_CID, DISTRIBUTED_LTK))]), (8, [P(2, b30[:20]), P(2, c9), P(1, b30[20:]), E]),
                         (9, [P(2, c9), P(2, a19)])] + rest(10, 30), ltk=stk, hop=7, u0=7, at=0)
    w.conn(PLAIN_NAME, [(0, [P(2, a19), E]), (1, [P(2, b30[:23]), P(2, c9), P(1, b30[23:]), E]), (2, [P(3, b"\x12"), E])] + rest(3, 31),
           hop=11, u0=11, at=1300)
    sc = exchange(5, WORLD_SEEDS[SECURE_NAME], n=41, preq=bytes([1, 4, 0, 0x0D, 16, 7, 7]), pres=bytes([2, 0, 0, 0x09, 16, 7, 7]))[0]
    w.conn(SECURE_NAME, [(c, [P(2, dm.l2cap(SMP_CID, sc[2 * c][1])), P(2, dm.l2cap(SMP_CID, sc[2 * c + 1][1]))]) for c in range(3)] +
           rest(3, 32), hop=5, u0=5, at=2600)
    w.noise(30)
    return w.built(), stk


@functools.lru_cache(maxsize=None)
def pair_capture():
    """pair_world's 37 data streams and three advertising streams of noise behind them, with the CONNECT_IND of the two connections
    that pair on the first of them -> Capture."""
    import _le
    import _le_discover as ld
    import _le_follow as lf
    b = pair_world()[0]
    n_words = b.n_words
    adv = np.random.default_rng(44).integers(0, 2, (3, 64 * n_words), dtype=np.uint8)
    at = 200
    for p in b.planted:
        if p.name != PLAIN_NAME:
            s = WORLD_SEEDS[p.name]
            body = lf.connect_ind(p.aa, p.crc_init, (1 << 37) - 1, 7, dm.INTERVAL, tx_add=s.tx_add, rx_add=s.rx_add, init_a=s.init_a, adv_a=s.adv_a)
            sym = _le.tx_bits(_le.ADV_AA, 37, body[4:40], _le.ADV_CRC_INIT)
            adv[0, at:at + len(sym)] = sym
            at += 900
    words = np.vstack([np.asarray(b.words)] + [_le.pack(row)[None, :] for row in adv])
    words.flags.writeable = False
    return ld.Capture(words, n_words, n_words, 64 * n_words - 39, lf.CHAIN_MHZ, b.planted, 27)


@functools.lru_cache(maxsize=None)
def capture_model():
    """Discovery (min_count 2, max_len 27), tracking, the advertising scan, seeds and the data stage's model on pair_capture
    -> (conns, cands, tracks, pkts, seeds, data)."""
    import _le
    import _le_discover as ld
    import _le_follow as lf
    import _le_track as lt
    cap = pair_capture()
    conns, cands = ld.group(ld.capture_candidates(cap, 27), 2)
    tracks, pkts = lt.track(cands, len(conns), cap.mhz, len(cap.mhz), dm.UNIT, dm.IFS, dm.JITTER, lt.REMAP)
    adv = []
    for s in range(len(cap.mhz)):
        offs, errs, _ = _le.match_all(cap.words[s], cap.n_words, cap.search_bits, _le.ADV_AA, 0)
        adv += [_le.decode(cap.words[s], cap.n_words, s, int(o), int(e), int(cap.mhz[s]), _le.ADV_CRC_INIT) for o, e in zip(offs, errs)]
    seeds = lf.seed(adv, conns, tracks, dm.UNIT)
    data = dm.data(conns, cands, pkts, cap.words, cap.n_words, 1 << 20, 1 << 30)
    return conns, cands, tracks, pkts, seeds, data
