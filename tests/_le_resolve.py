"""Test-side model of LE address resolution (include/btbbx.h btbbx_le_resolve_device, rules 1 to 8) -- Python over the advertising
record dicts of tests/_le.py and the message tuples of tests/_le_data.py, written from the rules and not from the kernels.  AES is
tests/_le_crypt.py's (built from its definition); the bulk trials are tests/_le_pair.py's numpy AES, one schedule per table slot over
all the addresses that are tried.

* ah / rpa: the random address hash of Core Vol 3 Part H 2.2.2 and an address made with it
* Rules: the model's branch points as options; VARIANTS are deliberately wrong models
* resolve: the model -> Out(slot_addr, addrs, n_addrs, irks, n_irks, peers)
* rec / Plant: hand-made advertising records; resolve_world / resolve_capture / capture_model: a connection that pairs under a passkey,
  encrypts under the STK and distributes both identities, under advertising streams that carry their RPAs
"""
import collections
import functools

import numpy as np

import _le_crypt as cm
import _le_data as dm
import _le_pair as pm

PUBLIC, NONRESOLVABLE, RESOLVABLE, RESERVED, STATIC = range(5)
ADVERTISER, SCANNER, INITIATOR, TARGET = 1, 2, 4, 8
GIVEN, HARVESTED, HAS_ADDR, NULLKEY = 1, 2, 4, 8
NONE, NO_IRK = 0xFFFFFFFF, 0xFFFF
SEEDED = 1
MAX_IRKS = 4096

Addr = collections.namedtuple("Addr", "first_offset last_offset n_slots first_rec addr random kind irk roles channels")
Irk = collections.namedtuple("Irk", "key id_addr id_random flags conn n_addrs n_slots role")
Peer = collections.namedtuple("Peer", "init_addr adv_addr init_irk adv_irk irk")
Out = collections.namedtuple("Out", "slot_addr addrs n_addrs irks n_irks peers")
Seed = collections.namedtuple("Seed", "request flags")
EMPTY_IRK = Irk(bytes(16), bytes(6), 0, 0, NONE, 0, 0, 0)


class Rules:
    """Rules() is the model; every other value is a wrong one."""

    def __init__(self, **kw):
        self.hash_prand_swapped = False     # rule 5: prand = a[2..0], hash = a[5..3]
        self.block_reversed = False         # rule 5: the block's octets, and the output's, in the other order
        self.key_as_received = False        # rule 4: key[j] = v[1 + j]
        self.no_kind_test = False           # rule 5: every address is tried
        self.no_random_bit = False          # rule 3: the key is the 48 address bits alone
        self.largest_slot = False           # rule 5: the largest matching slot
        self.scan_req_tx_add = False        # rule 2: slot 1 of SCAN_REQ with adv_tx_add
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


MODEL = Rules()
VARIANTS = {name: {name: True} for name in ("hash_prand_swapped", "block_reversed", "key_as_received", "no_kind_test", "no_random_bit",
                                            "largest_slot", "scan_req_tx_add")}


# ---- the primitives ------------------------------------------------------------------------------------------------------------------
def ah(key, prand):
    """key: 16 octets, most significant first; prand: 3 octets, most significant first -> the 3-octet hash, most significant first."""
    return cm.aes(bytes(key), bytes(13) + bytes(prand))[13:]


def rpa(key, n, top=1):
    """An address a[0..5] (as it lies in the PDU) under `key`, its prand picked by n; top: a[5] >> 6, 1 for an RPA."""
    r = np.random.default_rng(5000 + n).integers(0, 256, 3, dtype=np.uint8).tolist()
    prand = bytes([(r[0] & 0x3F) | (top << 6), r[1], r[2]])
    return (prand + ah(key, prand))[::-1]


def kind(t, a):
    return PUBLIC if not t else 1 + (a[5] >> 6)


def matches(key, a, rules=MODEL):
    """Rule 5's MATCH of one address and one key (no kind test)."""
    a = bytes(a)
    prand, want = (a[2::-1], a[:2:-1]) if rules.hash_prand_swapped else (a[:2:-1], a[2::-1])
    block = bytes(13) + prand
    if rules.block_reversed:
        return cm.aes(bytes(key), block[::-1])[2::-1] == want
    return cm.aes(bytes(key), block)[13:] == want


def slots(r, rules=MODEL):
    """Rule 2 -> the record's two slots, each None or (t, a, role)."""
    if not r["crc_ok"] or r["is_data"] or r["channel_idx"] < 37:
        return [None, None]
    b, ty, n = r["bytes"], r["adv_type"], r["length"]
    first, second = bytes(b[6:12]), bytes(b[12:18])
    tx, rx = int(bool(r["adv_tx_add"])), int(bool(r["adv_rx_add"]))
    if ty in (0, 2, 4, 6):
        return [(tx, first, ADVERTISER) if n >= 6 else None, None]
    if ty in (1, 3, 5) and n >= 12:
        role0 = {1: ADVERTISER, 3: SCANNER, 5: INITIATOR}[ty]
        t1 = tx if ty == 3 and rules.scan_req_tx_add else rx
        return [(tx, first, role0), (t1, second, TARGET if ty == 1 else ADVERTISER)]
    return [None, None]


def _key_of(t, a, rules):
    return (0 if rules.no_random_bit else t << 48) | int.from_bytes(a, "little")


def _smp(m, k, payload, byte_cap):
    """The pairing stage's rule 1 and the guards -> the message's octets, or None."""
    if m.conn >= k or m.byte_offset + m.bytes > byte_cap or m.bytes < 4 + m.l2cap_len:
        return None
    need = dm.COMPLETE | dm.STORED
    if m.flags & need != need or m.cid != pm.SMP_CID or m.l2cap_len < 1 or m.role > 1:
        return None
    return bytes(payload[m.byte_offset + 4:m.byte_offset + 4 + m.l2cap_len])


def table(k, msgs, payload, byte_cap, given, irk_cap, rules=MODEL):
    """Rule 4 -> (the irk_cap records without their tallies, the count, {(conn, role): slot})."""
    irks = [Irk(bytes(g), bytes(6), 0, GIVEN | (0 if any(g) else NULLKEY), NONE, 0, 0, 0) for g in given]
    octets = [_smp(m, k, payload, byte_cap) for m in msgs]
    found = {}
    for M, m in enumerate(msgs):
        v = octets[M]
        if v is None:
            continue
        if v[0] == 0x08 and len(v) == 17:
            found.setdefault((m.conn, m.role), [None, None])
            if found[(m.conn, m.role)][0] is None:
                found[(m.conn, m.role)][0] = v
        elif v[0] == 0x09 and len(v) == 8:
            found.setdefault((m.conn, m.role), [None, None])
            if found[(m.conn, m.role)][1] is None:
                found[(m.conn, m.role)][1] = v
    where = {}
    for (g, role) in sorted(found):
        info, ident = found[(g, role)]
        if info is None:
            continue
        key = info[1:] if rules.key_as_received else info[:0:-1]
        flags = HARVESTED | (0 if any(key) else NULLKEY) | (HAS_ADDR if ident is not None else 0)
        where[(g, role)] = len(irks)
        irks.append(Irk(key, ident[2:8] if ident is not None else bytes(6), ident[1] & 1 if ident is not None else 0, flags, g, 0, 0, role))
    count = len(irks)
    where = {at: slot for at, slot in where.items() if slot < irk_cap}
    irks = (irks + [EMPTY_IRK] * irk_cap)[:irk_cap]
    return irks, count, where


def trials(keys, addrs, rules=MODEL):
    """keys: the slots that are tried as (slot, key); addrs: (t, a) per address -> per address the matching slots, ascending."""
    out = [[] for _ in addrs]
    tried = [i for i, (t, a) in enumerate(addrs) if rules.no_kind_test or kind(t, a) == RESOLVABLE]
    if not tried or not keys:
        return out
    if rules.hash_prand_swapped or rules.block_reversed:
        for i in tried:
            out[i] = [slot for slot, key in keys if matches(key, addrs[i][1], rules)]
        return out
    blocks = np.zeros((len(tried), 16), np.uint8)
    want = np.zeros((len(tried), 3), np.uint8)
    for row, i in enumerate(tried):
        a = addrs[i][1]
        blocks[row, 13:] = (a[5], a[4], a[3])
        want[row] = (a[2], a[1], a[0])
    for slot, key in keys:
        rk = np.broadcast_to(pm.schedules(np.frombuffer(bytes(key), np.uint8).reshape(1, 16)), (len(tried), 11, 16))
        hit = (pm.aes_many(rk, blocks)[:, 13:] == want).all(axis=1)
        for row in np.flatnonzero(hit):
            out[tried[row]].append(slot)
    return out


def resolve(adv, k, seeds, msgs, payload, byte_cap, given, irk_cap, addr_cap, rules=MODEL):
    """adv: the A records that are looked at; k: the connections; seeds: one Seed (or anything with request and flags) or None per
    connection; msgs: the W message records that are looked at; given: the caller's keys -> Out.  addrs holds ALL N records: the
    entry stores the first addr_cap of them."""
    assert len(given) <= irk_cap <= MAX_IRKS
    per_slot = [s for r in adv for s in slots(r, rules)]
    keys = sorted({_key_of(s[0], s[1], rules) for s in per_slot if s is not None})
    rank = {key: i for i, key in enumerate(keys)}
    slot_addr = [NONE if s is None else rank[_key_of(s[0], s[1], rules)] for s in per_slot]
    irks, n_irks, where = table(k, msgs, payload, byte_cap, given, irk_cap, rules)
    tried = [(slot, irk.key) for slot, irk in enumerate(irks[:min(n_irks, irk_cap)]) if not irk.flags & NULLKEY]
    ident = [((key >> 48) & 1 if not rules.no_random_bit else 1, key.to_bytes(7, "little")[:6]) for key in keys]
    if rules.no_random_bit:                                 # (the bit is that of the first slot that holds the address)
        first_t = {}
        for s in per_slot:
            if s is not None:
                first_t.setdefault(_key_of(s[0], s[1], rules), s[0])
        ident = [(first_t[key], a) for key, (_, a) in zip(keys, ident)]
    hits = trials(tried, ident, rules)
    addrs, held = [], collections.defaultdict(list)
    for s, r in enumerate(slot_addr):
        held[r].append(s)
    for i, (t, a) in enumerate(ident):
        mine = held[i]
        recs = [adv[s >> 1] for s in mine]
        irk = NO_IRK if not hits[i] else (max(hits[i]) if rules.largest_slot else min(hits[i]))
        addrs.append(Addr(min(r["offset"] for r in recs), max(r["offset"] for r in recs), len(mine), mine[0] >> 1, a, t, kind(t, a), irk,
                          _or(per_slot[s][2] for s in mine), _or(1 << (r["channel_idx"] - 37) for r in recs)))
    tally = collections.defaultdict(lambda: [0, 0])
    for x in addrs:
        tally[x.irk][0] += 1
        tally[x.irk][1] += x.n_slots
    irks = [irk._replace(n_addrs=tally[i][0], n_slots=tally[i][1]) for i, irk in enumerate(irks)]
    peers = []
    for g in range(k):
        s = seeds[g]
        pa = [NONE, NONE]
        if s is not None and s.flags & SEEDED and s.request < len(adv):
            pa = [slot_addr[2 * s.request], slot_addr[2 * s.request + 1]]
        pi = [NO_IRK if x == NONE else addrs[x].irk for x in pa]
        peers.append(Peer(pa[0], pa[1], pi[0], pi[1], (where.get((g, 0), NO_IRK), where.get((g, 1), NO_IRK))))
    return Out(slot_addr, addrs, len(addrs), irks, n_irks, peers)


def _or(values):
    out = 0
    for v in values:
        out |= v
    return out


def addr_array(addrs, dtype):
    a = np.zeros(len(addrs), dtype)
    for i, x in enumerate(addrs):
        a[i] = tuple(x[:4]) + (list(x.addr),) + tuple(x[5:]) + ((0,) * 4,)
    return a


def irk_array(irks, dtype):
    a = np.zeros(len(irks), dtype)
    for i, x in enumerate(irks):
        a[i] = (list(x.key), list(x.id_addr)) + tuple(x[2:]) + ((0,) * 3,)
    return a


def peer_array(peers, dtype):
    a = np.zeros(len(peers), dtype)
    for i, x in enumerate(peers):
        a[i] = tuple(x[:4]) + (list(x.irk),)
    return a


# ---- hand-made advertising records -----------------------------------------------------------------------------------------------------
def rec(offset, adv_type, first, second=None, tx=0, rx=0, ch=37, length=None, crc_ok=1, is_data=0, stream=0):
    """One advertising record as a dict keyed like LE_PKT_DTYPE: what the stage does not read is noise it must not read."""
    body = bytes(first) + (bytes(second) if second is not None else b"")
    length = len(body) if length is None else length
    noise = bytes(np.random.default_rng(offset & 0xFFFF).integers(0, 256, 64, dtype=np.uint8).tolist())
    raw = (noise[:4] + bytes([adv_type | (tx << 6) | (rx << 7), length]) + body + noise)[:64]
    return dict(offset=offset, stream=stream, aa_errors=noise[20] & 3, crc_ok=crc_ok, crc_rx=noise[21], crc_calc=noise[22], pdu_bytes=2 + length,
                truncated=0, channel_idx=ch, channel_k=noise[23] & 63, is_data=is_data, length=length, adv_type=adv_type, adv_tx_add=tx,
                adv_rx_add=rx, access_address_ok=noise[24] & 1, access_address_offenses=noise[25] & 7, access_address=noise[26], bytes=raw)


def octets(seed, n):
    return bytes(np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tolist())


def identity(role, n, random=0):
    """The two SMP messages by which `role` distributes the identity n -> ((role, Identity Information), (role, Identity Address
    Information), the key in AES order, the identity address)."""
    key, addr = octets(9000 + n, 16), octets(9100 + n, 6)
    return (role, b"\x08" + key[::-1]), (role, b"\x09" + bytes([random]) + addr), key, addr


# ---- a planted capture -----------------------------------------------------------------------------------------------------------------
WORLD_TK = 314159
WORLD_NAME = "resolve: pairs, encrypts under the STK, distributes both identities"
CENTRAL_ID, PERIPHERAL_ID, THIRD_IRK, UNKNOWN_IRK = identity(dm.CENTRAL, 1, 0), identity(dm.PERIPHERAL, 2, 1), octets(9003, 16), octets(9004, 16)
IRK_C, IRK_P = CENTRAL_ID[2], PERIPHERAL_ID[2]
INIT_A, ADV_A = rpa(IRK_C, 0), rpa(IRK_P, 0)
WORLD_SEED = pm.Seed(INIT_A, ADV_A, 1, 1, SEEDED)
RPAS_C, RPAS_P = [rpa(IRK_C, n) for n in range(1, 4)], [rpa(IRK_P, n) for n in range(1, 4)]
RPA_THIRD, RPA_UNKNOWN = rpa(THIRD_IRK, 7), rpa(UNKNOWN_IRK, 8)
# look-alikes: the 48 bits of an RPA sent as a public address; a static and a non-resolvable address whose hash holds under a key
PUBLIC_ALIKE, STATIC_ALIKE, NONRESOLVABLE_ALIKE = RPAS_P[0], rpa(IRK_P, 9, top=3), rpa(IRK_C, 10, top=0)
PUBLIC_DEVICE = octets(9005, 6)


def adv_plan():
    """The advertising PDUs of the planted capture as (stream 0..2, adv_type, tx, rx, payload, good CRC), in the order they are
    sent on their stream; one PDU of each of the eight types 0 to 7 at least."""
    data = octets(9006, 9)
    return [
        (0, 0, 1, 0, RPAS_P[0] + data, True), (1, 0, 1, 0, RPAS_P[0] + data, True),           # ADV_IND, the same RPA on two channels
        (2, 0, 1, 0, RPAS_P[1] + data, True), (0, 2, 1, 0, RPAS_P[2] + data[:3], True),       # ADV_NONCONN_IND
        (1, 4, 1, 0, RPAS_P[1] + data, True),                                                 # SCAN_RSP
        (2, 6, 1, 0, RPAS_C[0] + data[:5], True),                                             # ADV_SCAN_IND
        (0, 1, 1, 1, RPAS_C[1] + RPAS_P[0], True), (1, 1, 1, 1, RPAS_C[1] + RPAS_P[0], True), # ADV_DIRECT_IND
        (2, 3, 0, 1, PUBLIC_ALIKE + RPAS_P[1], True),                                         # SCAN_REQ: a public scanner, an RPA
        (0, 3, 1, 1, RPAS_C[2] + RPAS_P[2], True),
        (1, 0, 1, 0, RPA_THIRD + data, True), (2, 0, 1, 0, RPA_UNKNOWN + data, True),
        (0, 0, 1, 0, STATIC_ALIKE + data, True), (1, 0, 1, 0, NONRESOLVABLE_ALIKE + data, True),
        (2, 0, 0, 0, PUBLIC_DEVICE + data, True),
        (0, 7, 1, 0, RPAS_C[0] + data, True),                                                 # ADV_EXT_IND: not read
        (1, 0, 1, 0, rpa(IRK_C, 11) + data, False),                                           # a bad CRC: fills no slot
        (2, 5, 1, 1, RPAS_C[0] + RPAS_P[1] + octets(9007, 22), True),                         # a CONNECT_IND of no connection here
    ]


@functools.lru_cache(maxsize=None)
def resolve_world():
    """tests/_le_crypt.py's CryptWorld with one connection that pairs under the passkey WORLD_TK between two RPAs, encrypts under the
    STK and, behind the encryption start, distributes both identities.  No PDU is longer than 27 octets on the air.
    -> (Built, the STK)"""
    P, E, REQ, RSP, BEGIN = cm.P, cm.E, cm.REQ, cm.RSP, cm.BEGIN
    w = cm.CryptWorld(seed=35)
    messages, mrand, srand = pm.exchange(WORLD_TK, WORLD_SEED, n=50)
    stk = pm.s1(WORLD_TK, mrand, srand, 16)
    smp = [dm.l2cap(pm.SMP_CID, body) for _, body in messages]
    ids = [dm.l2cap(pm.SMP_CID, body) for _, body in (CENTRAL_ID[0], PERIPHERAL_ID[0], CENTRAL_ID[1], PERIPHERAL_ID[1])]
    assert max(len(f) for f in smp + ids) <= 27
    w.conn(WORLD_NAME, [(0, [E, E]), (1, [P(2, smp[0]), P(2, smp[1])]), (2, [P(2, smp[2]), P(2, smp[3])]), (3, [P(2, smp[4]), P(2, smp[5])]),
                        (4, [REQ, RSP]), (5, [E, BEGIN]), (6, [P(3, b"\x06"), P(3, b"\x06")]), (7, [P(2, ids[0]), P(2, ids[1])]),
                        (8, [P(2, ids[2]), P(2, ids[3])])] + [(c, [E, E]) for c in range(9, 30)], ltk=stk, hop=7, u0=7, at=0)
    w.noise(20)
    return w.built(), stk


@functools.lru_cache(maxsize=None)
def resolve_capture():
    """resolve_world's 37 data streams and three advertising streams behind them: noise, the connection's CONNECT_IND between its two
    RPAs on the first, and adv_plan's PDUs -> Capture."""
    import _le
    import _le_discover as ld
    import _le_follow as lf
    b = resolve_world()[0]
    n_words = b.n_words
    adv = np.random.default_rng(45).integers(0, 2, (3, 64 * n_words), dtype=np.uint8)
    p = b.planted[0]
    body = lf.connect_ind(p.aa, p.crc_init, (1 << 37) - 1, 7, dm.INTERVAL, tx_add=1, rx_add=1, init_a=INIT_A, adv_a=ADV_A)
    sym = _le.tx_bits(_le.ADV_AA, 37, body[4:40], _le.ADV_CRC_INIT)
    adv[0, 200:200 + len(sym)] = sym
    at = [3000, 3100, 3200]
    for s, ty, tx, rx, payload, good in adv_plan():
        sym = _le.tx_bits(_le.ADV_AA, 37 + s, _le.make_pdu(ty | (tx << 6) | (rx << 7), payload), _le.ADV_CRC_INIT).copy()
        if not good:
            sym[60] ^= 1
        adv[s, at[s]:at[s] + len(sym)] = sym
        at[s] += 700
    words = np.vstack([np.asarray(b.words)] + [_le.pack(row)[None, :] for row in adv])
    words.flags.writeable = False
    return ld.Capture(words, n_words, n_words, 64 * n_words - 39, lf.CHAIN_MHZ, b.planted, 27)


@functools.lru_cache(maxsize=None)
def adv_records():
    """The advertising scan's model on resolve_capture's three advertising streams alone (streams 0 to 2), in the scan's (stream,
    offset) order -> the record dicts."""
    import _le
    cap = resolve_capture()
    adv = []
    for s in range(37, len(cap.mhz)):
        offs, errs, _ = _le.match_all(cap.words[s], cap.n_words, cap.search_bits, _le.ADV_AA, 0)
        adv += [_le.decode(cap.words[s], cap.n_words, s - 37, int(o), int(e), int(cap.mhz[s]), _le.ADV_CRC_INIT) for o, e in zip(offs, errs)]
    return adv


@functools.lru_cache(maxsize=None)
def capture_model():
    """Discovery (min_count 2, max_len 31), tracking, the advertising scan, seeds, the data stage's and the decryption stage's models
    under the STK on resolve_capture -> (conns, cands, tracks, pkts, adv, seeds, plain)."""
    import _le
    import _le_discover as ld
    import _le_follow as lf
    import _le_track as lt
    cap = resolve_capture()
    conns, cands = ld.group(ld.capture_candidates(cap, 31), 2)
    tracks, pkts = lt.track(cands, len(conns), cap.mhz, len(cap.mhz), dm.UNIT, dm.IFS, dm.JITTER, lt.REMAP)
    adv = []
    for s in range(len(cap.mhz)):
        offs, errs, _ = _le.match_all(cap.words[s], cap.n_words, cap.search_bits, _le.ADV_AA, 0)
        adv += [_le.decode(cap.words[s], cap.n_words, s, int(o), int(e), int(cap.mhz[s]), _le.ADV_CRC_INIT) for o, e in zip(offs, errs)]
    seeds = lf.seed(adv, conns, tracks, dm.UNIT)
    data = dm.data(conns, cands, pkts, cap.words, cap.n_words, 0, 0)
    plain = cm.crypt(conns, cands, pkts, data.dpkts, cap.words, cap.n_words, [resolve_world()[1]], 8, 1 << 16, 1 << 22)
    return conns, cands, tracks, pkts, adv, seeds, plain
