"""Test-side model of LE decryption (include/btbbx.h btbbx_le_crypt_device, rules 1 to 9) -- plain Python over the tuples of
tests/_le_data.py, written from the rules and not from the kernels: AES is built from its definition (the S-box from the field
inverse and the affine map, octet by octet, no round tables), a connection is walked member by member.

* aes / ccm_encrypt / session_key: the primitives (tests/test_le_crypt_model.py holds them against FIPS-197, openssl and the Core
  Specification's sample data)
* Rules: the model's branch points as options; VARIANTS are deliberately wrong models
* crypt: the model -> Out(crypt, cpkts, ppkts, msgs, payload, n_msgs, n_bytes)
* CryptWorld: tests/_le_data.py's World, extended from the outside: the three procedure PDUs, then every non-empty new PDU encrypted
  with its true counter; what was planted is the PLAINTEXT
* Hand: hand-made lists whose packets are written into the streams at chosen bit offsets
"""
import collections
import functools

import numpy as np

import _le
import _le_data as dm

CLEAR, VERIFIED, FAILED, SKIPPED, SHORT = range(5)
F_REQ, F_RSP, F_START, F_ARMED, F_KEYED = 1, 2, 4, 8, 16
NONE = 0xFFFFFFFF

Crypt = collections.namedtuple("Crypt", "session_key iv req rsp start n_encrypted n_verified n_failed n_skipped key max_skew flags")
CPkt = collections.namedtuple("CPkt", "counter ordinal state skew opcode counter_hi")
Out = collections.namedtuple("Out", "crypt cpkts ppkts msgs payload n_msgs n_bytes")
NO_MEMBER = Crypt(bytes(16), bytes(8), 0, 0, 0, 0, 0, 0, 0, 0, 0, 0)


# ---- AES-128 from its definition (FIPS-197) ------------------------------------------------------------------------------------------
def _gmul(a, b):
    r = 0
    while b:
        if b & 1:
            r ^= a
        a = (a << 1) ^ (0x11B if a & 0x80 else 0)
        b >>= 1
    return r


def _sbox():
    box = []
    for x in range(256):
        inv = next((y for y in range(1, 256) if _gmul(x, y) == 1), 0)
        s = 0
        for bit in range(8):                # b'_i = b_i ^ b_(i+4) ^ b_(i+5) ^ b_(i+6) ^ b_(i+7) ^ c_i, c = 0x63
            v = (inv >> bit) ^ (inv >> ((bit + 4) % 8)) ^ (inv >> ((bit + 5) % 8)) ^ (inv >> ((bit + 6) % 8)) ^ (inv >> ((bit + 7) % 8)) ^ (0x63 >> bit)
            s |= (v & 1) << bit
        box.append(s)
    return box


SBOX = _sbox()
_MUL2 = [_gmul(x, 2) for x in range(256)]
_MUL3 = [_gmul(x, 3) for x in range(256)]


@functools.lru_cache(maxsize=4096)
def _schedule(key):
    w = [list(key[4 * i:4 * i + 4]) for i in range(4)]
    rcon = 1
    for i in range(4, 44):
        t = list(w[i - 1])
        if i % 4 == 0:
            t = [SBOX[t[1]] ^ rcon, SBOX[t[2]], SBOX[t[3]], SBOX[t[0]]]
            rcon = _gmul(rcon, 2)
        w.append([a ^ b for a, b in zip(w[i - 4], t)])
    return [sum(w[4 * r:4 * r + 4], []) for r in range(11)]


def aes(key, block):
    """AES-128 of one block; key and block are 16 octets, octet 0 first.  The state is FIPS-197's: s[r + 4c] = in[r + 4c]."""
    rk = _schedule(bytes(key))
    s = [a ^ b for a, b in zip(block, rk[0])]
    for rnd in range(1, 11):
        s = [SBOX[v] for v in s]
        s = [s[(r + 4 * ((c + r) % 4))] for c in range(4) for r in range(4)]             # ShiftRows: row r moves r columns left
        if rnd < 10:
            out = []
            for c in range(4):
                a0, a1, a2, a3 = s[4 * c:4 * c + 4]
                out += [_MUL2[a0] ^ _MUL3[a1] ^ a2 ^ a3, a0 ^ _MUL2[a1] ^ _MUL3[a2] ^ a3, a0 ^ a1 ^ _MUL2[a2] ^ _MUL3[a3],
                        _MUL3[a0] ^ a1 ^ a2 ^ _MUL2[a3]]
            s = out
        s = [a ^ b for a, b in zip(s, rk[rnd])]
    return bytes(s)


# ---- the rules -----------------------------------------------------------------------------------------------------------------------
class Rules:
    """Rules() is the model; every other value is a wrong one."""

    def __init__(self, **kw):
        self.dir_flip = False               # rule 5: the direction bit the other way round
        self.aad_unmasked = False           # rule 5: header0 in B1 as it is, not & 0xE3
        self.count_retx = False             # rule 1: retransmissions COUNT
        self.count_empty = False            # rule 4: empty PDUs behind START take an ordinal
        self.skd_swap = False               # rule 3: skd = SKDs | SKDm
        self.iv_swap = False                # rule 3: iv = IVs | IVm
        self.b0_whole_length = False        # rule 5: BE16(L) in B0, not BE16(L - 4)
        self.block_counter_le = False       # rule 5: LE16(i) in the counter blocks
        self.no_padding = False             # rule 5: the last CBC block filled with the keystream behind the plaintext, not zeros
        self.largest_key = False            # rule 6: the largest k of the largest score
        for k, v in kw.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


MODEL = Rules()
VARIANTS = {name: {name: True} for name in ("dir_flip", "aad_unmasked", "count_retx", "count_empty", "skd_swap", "iv_swap", "b0_whole_length",
                                            "block_counter_le", "no_padding", "largest_key")}


def session_key(ltk, skdm, skds, rules=MODEL):
    """Rule 3.  ltk: most significant octet first; skdm, skds: as received."""
    skd = bytes(skds) + bytes(skdm) if rules.skd_swap else bytes(skdm) + bytes(skds)
    return aes(ltk, skd[::-1])


def _ccm(sk, iv, counter, direction, header0, text, decrypt, rules=MODEL):
    """Rule 5 -> (the other text, the MIC computed over the plaintext).  text: plaintext, or ciphertext without its MIC."""
    m = len(text)
    nonce = bytes([counter & 0xFF, (counter >> 8) & 0xFF, (counter >> 16) & 0xFF, (counter >> 24) & 0xFF,
                   ((counter >> 32) & 0x7F) | (direction ^ int(rules.dir_flip)) << 7]) + bytes(iv)
    a = lambda i: bytes([1]) + nonce + (bytes([i & 0xFF, i >> 8]) if rules.block_counter_le else bytes([i >> 8, i & 0xFF]))   # noqa: E731
    stream = b"".join(aes(sk, a(1 + j)) for j in range((m + 15) // 16))
    other = bytes(t ^ s for t, s in zip(text, stream))
    plain = other if decrypt else bytes(text)
    claimed = m + 4 if rules.b0_whole_length else m
    x = aes(sk, bytes([0x49]) + nonce + bytes([claimed >> 8, claimed & 0xFF]))
    b1 = bytes([0, 1, header0 if rules.aad_unmasked else header0 & 0xE3]) + bytes(13)
    x = aes(sk, bytes(p ^ q for p, q in zip(x, b1)))
    pad = stream[m:] if rules.no_padding else bytes(len(stream) - m)
    padded = plain + pad
    for j in range(0, len(padded), 16):
        x = aes(sk, bytes(p ^ q for p, q in zip(x, padded[j:j + 16])))
    s0 = aes(sk, a(0))
    return other, bytes(p ^ q for p, q in zip(x[:4], s0[:4]))


def ccm_encrypt(sk, iv, counter, direction, header0, plain):
    """-> ciphertext | MIC, by the right rules."""
    cipher, mic = _ccm(sk, iv, counter, direction, header0, plain, False)
    return cipher + mic


def trial(sk, iv, counter, direction, header0, octets, rules=MODEL):
    """Rule 5 on the L >= 5 payload octets of a member -> the plaintext if the trial verifies, else None."""
    plain, mic = _ccm(sk, iv, counter, direction, header0, octets[:-4], True, rules)
    return plain if mic == bytes(octets[-4:]) else None


def _octets(cands, pkts, rows, n_words, i):
    c = cands[i]
    if c.stream >= len(rows):
        return bytes(c.length)
    return bytes(dm.payload_octets(rows[c.stream], n_words, c.offset, c.length, pkts[i].channel))


def crypt(conns, cands, pkts, dpkts, rows, n_words, keys, window, msg_cap, byte_cap, rules=MODEL):
    """dpkts: the data stage's per-candidate records (DPkt or None), keys: 16-octet strings.  -> Out: one Crypt per connection, one
    CPkt and one DPkt (the effective members') or None (no member) per candidate, the first msg_cap Msg records, the stored prefix of
    the octets, and the two counts."""
    cpkts, ppkts = [None] * len(cands), [None] * len(cands)
    records, messages = [], []
    for g, order in enumerate(dm.members_of(conns, cands, pkts)):
        if not order:
            records.append(NO_MEMBER)
            continue
        octets = {i: _octets(cands, pkts, rows, n_words, i) for i in order}
        counting = {i: dpkts[i].role < 2 and (dpkts[i].kind not in (dm.RETRANSMIT, dm.UNKNOWN) or
                                              (rules.count_retx and dpkts[i].kind == dm.RETRANSMIT)) for i in order}
        proc = [None, None, None]                                   # rule 2: positions in `order`
        for pos, i in enumerate(order):
            c, role = cands[i], dpkts[i].role
            if not counting[i] or c.header0 & 3 != 3 or c.length < 1:
                continue
            shape = (role, c.length, octets[i][0])
            if proc[0] is None:
                if shape == (dm.CENTRAL, 23, 3):
                    proc[0] = pos
            elif proc[1] is None:
                if shape == (dm.PERIPHERAL, 13, 4):
                    proc[1] = pos
            elif proc[2] is None and shape == (dm.PERIPHERAL, 1, 5):
                proc[2] = pos
        armed = proc[2] is not None
        state, ordinal, taken, encrypted, skipped = {}, {}, [0, 0], [], 0
        for pos, i in enumerate(order):                             # rule 4
            c, role = cands[i], dpkts[i].role
            st = CLEAR
            if armed and pos > proc[2]:
                if not counting[i]:
                    st = SKIPPED if c.length >= 1 else CLEAR
                elif c.header0 & 3 and c.length >= 1:
                    st = "encrypted" if c.length >= 5 else SHORT
                elif rules.count_empty and c.length == 0:
                    taken[role] += 1
            if st == "encrypted":
                ordinal[i] = taken[role]
                taken[role] += 1
                encrypted.append(i)
            skipped += st == SKIPPED
            state[i] = st
        sk, iv, key = bytes(16), bytes(8), 0xFF
        if armed:                                                   # rules 3 and 6
            req, rsp = octets[order[proc[0]]], octets[order[proc[1]]]
            iv = rsp[9:13] + req[19:23] if rules.iv_swap else req[19:23] + rsp[9:13]
            sks = [session_key(k, req[11:19], rsp[1:9], rules) for k in keys]
            verify = lambda s, i, d: trial(s, iv, ordinal[i] + d, int(dpkts[i].role == dm.CENTRAL), cands[i].header0, octets[i], rules)   # noqa: E731
            scores = [sum(any(verify(s, i, d) is not None for d in range(window)) for i in encrypted[:4]) for s in sks]
            if scores and max(scores) >= 1:
                best = [k for k, s in enumerate(scores) if s == max(scores)]
                key = best[-1] if rules.largest_key else best[0]
        plain, skew = {}, {}
        for i in encrypted:                                         # rule 7
            state[i], skew[i] = FAILED, 0xFF
            if key != 0xFF:
                for d in range(window):
                    got = verify(sks[key], i, d)
                    if got is not None:
                        state[i], skew[i], plain[i] = VERIFIED, d, got
                        break
        n_verified = sum(state[i] == VERIFIED for i in encrypted)
        records.append(Crypt(sks[key] if key != 0xFF else bytes(16), iv if armed else bytes(8),
                             *[order[p] if p is not None else NONE for p in proc], len(encrypted), n_verified, len(encrypted) - n_verified,
                             skipped, key, max([skew[i] for i in encrypted if state[i] == VERIFIED], default=0),
                             (F_REQ if proc[0] is not None else 0) | (F_RSP if proc[1] is not None else 0) |
                             (F_START | F_ARMED if armed else 0) | (F_KEYED if key != 0xFF else 0)))
        open_msg, mine = {}, []                                     # rule 8: the data stage's rule 5 over the effective members
        for i in order:
            c, d, st = cands[i], dpkts[i], state[i]
            counter = ordinal[i] + (skew[i] if st == VERIFIED else 0) if i in ordinal else 0
            opcode = plain[i][0] if st == VERIFIED and c.header0 & 3 == 3 else 0xFF
            cpkts[i] = CPkt(counter & 0xFFFFFFFF, ordinal.get(i, 0), st, skew.get(i, 0), opcode, (counter >> 32) & 0x7F)
            if st == VERIFIED:
                kind, body = {2: dm.START, 1: dm.CONTINUATION, 3: dm.CONTROL}[c.header0 & 3], plain[i]
            elif st == CLEAR:
                kind, body = d.kind, octets[i]
            else:
                kind, body = dm.IGNORED, b""
            if kind == dm.START:
                m = dict(conn=g, start=i, role=d.role, frags=1, octets=bytearray(body))
                open_msg[d.role] = m
                mine.append(m)
                ppkts[i] = (m, 0, d.role, kind, d.bits)
            elif kind == dm.CONTINUATION and d.role in open_msg:
                m = open_msg[d.role]
                ppkts[i] = (m, len(m["octets"]), d.role, kind, d.bits)
                m["frags"] += 1
                m["octets"] += body
            else:
                ppkts[i] = dm.DPkt(NONE, 0, d.role, dm.ORPHAN if kind == dm.CONTINUATION else kind, d.bits)
        messages += mine                                            # (walked in time order: by the rank of the START)
    msgs, payload, offset = [], bytearray(), 0
    for M, m in enumerate(messages):                                # the data stage's rule 6
        m["M"] = M
        body, flags, l2cap_len, cid = m["octets"], dm.RUNT, 0xFFFF, 0xFFFF
        start_len = len(body) if m["frags"] == 1 else None
        first = cands[m["start"]].length - (4 if cpkts[m["start"]].state == VERIFIED else 0)
        assert start_len is None or start_len == first
        if first >= 4:
            l2cap_len, cid = body[0] | body[1] << 8, body[2] | body[3] << 8
            flags = dm.COMPLETE if len(body) == 4 + l2cap_len else (dm.OVERRUN if len(body) > 4 + l2cap_len else 0)
        if M < msg_cap and offset + len(body) <= byte_cap:
            flags |= dm.STORED
            payload[offset:offset + len(body)] = body
        if M < msg_cap:
            msgs.append(dm.Msg(offset, m["conn"], m["start"], m["frags"], len(body), l2cap_len, cid, m["role"], flags))
        offset += len(body)
    ppkts = [dm.DPkt(d[0]["M"], *d[1:]) if d is not None and isinstance(d[0], dict) else d for d in ppkts]
    return Out(records, cpkts, ppkts, msgs, bytes(payload), len(messages), offset)


def built_model(b, keys, window=8, msg_cap=1 << 20, byte_cap=1 << 30, rules=MODEL):
    """The data stage's model, then this stage's, on a Built of tests/_le_data.py -> (the data stage's Out, this stage's Out)."""
    data = dm.built_model(b)
    return data, crypt(b.conns, b.cands, b.pkts, data.dpkts, b.words, b.n_words, keys, window, msg_cap, byte_cap, rules)


# ---- records -------------------------------------------------------------------------------------------------------------------------
def crypt_array(records, dtype):
    a = np.zeros(len(records), dtype)
    for i, r in enumerate(records):
        a[i] = (list(r.session_key), list(r.iv)) + tuple(r[2:]) + (0,)
    return a


def cpkt_array(cpkts, dtype):
    a = np.zeros(len(cpkts), dtype)
    for i, p in enumerate(cpkts):
        if p is None:
            a[i:i + 1].view(np.uint8)[:] = 0xFF
        else:
            a[i] = tuple(p) + ((0, 0, 0, 0),)
    return a


# ---- planted worlds ------------------------------------------------------------------------------------------------------------------
P, E = dm.P, dm.E
REQ, RSP, BEGIN = P(3, b"<LL_ENC_REQ>"), P(3, b"<LL_ENC_RSP>"), P(3, b"<LL_START_ENC_REQ>")


def ltk(n):
    """A long-term key, most significant octet first."""
    return bytes(np.random.default_rng(1000 + n).integers(0, 256, 16, dtype=np.uint8).tolist())


class CryptWorld(dm.World):
    """World whose connections may encrypt: in a connection given an ltk, REQ, RSP and BEGIN among its packets become the three procedure
    PDUs with random SKD and IV halves, and every non-empty new PDU behind BEGIN is sent encrypted with its true counter -- a lost one,
    too, has taken a counter.  What is planted as messages is the plaintext."""

    def conn(self, name, events, ltk=None, **kw):
        skdm, skds, ivm, ivs = (bytes(self.rng.integers(0, 256, n, dtype=np.uint8).tolist()) for n in (8, 8, 4, 4))
        sk = session_key(ltk, skdm, skds) if ltk is not None else None
        on, counters, sent = False, [0, 0], []
        for c, packets in events:
            out = []
            for k, p in enumerate(packets):
                role = k & 1
                if p is REQ:
                    p = P(3, bytes([3]) + bytes(self.rng.integers(0, 256, 10, dtype=np.uint8).tolist()) + skdm + ivm)
                elif p is RSP:
                    p = P(3, bytes([4]) + skds + ivs)
                elif p is BEGIN:
                    p, on = P(3, bytes([5])), sk is not None
                    out.append(p)
                    continue
                if on and not p.retx and p.llid and p.payload:
                    p = p._replace(payload=ccm_encrypt(sk, ivm + ivs, counters[role], int(role == dm.CENTRAL), p.llid, p.payload))
                    counters[role] += 1
                out.append(p)
            sent.append((c, out))
        super().conn(name, sent, **kw)
        # the plaintext messages, as World.conn collects the sent ones
        timed, messages, cur = kw.get("timed", True), [], [None, None]
        for n_ev, (c, packets) in enumerate(events):
            tail = not timed and n_ev > 0
            for k, p in enumerate(packets):
                role = k & 1
                if p.lost:
                    tail = True
                elif not tail and not p.retx and p not in (REQ, RSP, BEGIN):
                    if p.llid == 2 and p.payload:
                        cur[role] = [role, bytearray(p.payload)]
                        messages.append(cur[role])
                    elif p.llid == 1 and p.payload and cur[role] is not None:
                        cur[role][1] += p.payload
        self.planted[-1] = self.planted[-1]._replace(messages=[(r, bytes(b)) for r, b in messages])


WORLD_KEYS = (ltk(0), ltk(1), ltk(2), ltk(1), ltk(3))              # (ltk(1) twice: the smaller index is the connection's key)


@functools.lru_cache(maxsize=None)
def planted_world():
    """Two connections that encrypt under different keys of one table, one that never does and one whose key is not in the table,
    interleaved on the air, plus noise.  PDUs of up to 27 plaintext octets: 31 on the air."""
    w = CryptWorld(seed=21)
    r = np.random.default_rng(6)
    a23, b40, c9, d31 = (dm.l2cap(4, dm._octets(r, n)) for n in (19, 36, 5, 27))
    rest = lambda first, last: [(c, [E, E]) for c in range(first, last)]                       # noqa: E731
    # a message in the clear, the procedure, the two LL_START_ENC_RSP; one-fragment and two-fragment messages of both roles, a
    # message begun in the clear and continued encrypted, a control PDU, a retransmission in each role behind the start
    w.conn("crypt: encrypts", [(0, [P(2, a23), P(2, b40[:27])]), (1, [REQ, RSP]), (2, [E, BEGIN]), (3, [P(3, b"\x06"), P(3, b"\x06")]),
                               (4, [P(2, b40[:27]), P(1, b40[27:]), P(1, b40[27:]), P(2, c9)]), (5, [P(0, retx=True), P(0, retx=True)]),
                               (6, [P(2, a23[:10]), E, P(1, a23[10:]), P(2, d31[:27])]), (7, [P(3, b"\x12"), P(1, d31[27:])]),
                               (8, [P(2, c9), P(2, c9)])] + rest(9, 30), ltk=WORLD_KEYS[1], hop=7, u0=0, at=0)
    w.conn("crypt: never encrypts", [(0, [P(2, a23), E]), (1, [P(2, b40[:27]), P(2, c9), P(1, b40[27:]), E]), (2, [P(3, b"\x12"), E]),
                                     (3, [E, P(2, a23[:10]), E, P(1, a23[10:])])] + rest(4, 31), hop=11, u0=3, at=1300)
    # two packets of the central in a row that the capture lacks, behind the start: its counters run two ahead from there (skew 2:
    # one lost packet alone makes the next look like a retransmission, the data stage's limit); another key
    w.conn("crypt: a lost packet", [(0, [REQ, RSP]), (1, [E, BEGIN]), (2, [P(3, b"\x06"), P(3, b"\x06")]), (3, [P(2, c9), P(2, a23)]),
                                    (4, [E, P(2, c9), P(2, a23, lost=True)]), (5, [P(2, c9, lost=True)]),
                                    (6, [P(2, b40[:27]), P(2, c9), P(1, b40[27:]), E]),
                                    (7, [P(2, c9), P(2, d31[:20]), E, P(1, d31[20:])])] + rest(8, 33), ltk=WORLD_KEYS[2], hop=5, u0=20, at=2600)
    w.conn("crypt: a key that is not in the table", [(0, [REQ, RSP]), (1, [E, BEGIN]), (2, [P(2, c9), P(2, a23)]), (3, [P(2, a23), E])] +
           rest(4, 33), ltk=ltk(9), hop=9, u0=14, at=5300)
    w.noise(40)
    return w.built()


def check_planted(b, out, keyed):
    """The model's messages of the connections named in `keyed` are the planted plaintext, octet for octet -> the messages checked."""
    n = 0
    for g, name in enumerate(b.names):
        if name not in keyed:
            continue
        plant = [p for p in b.planted if p.name == name][0]
        msgs = [m for m in out.msgs if m.conn == g]
        assert [(m.role, out.payload[m.byte_offset:m.byte_offset + m.bytes]) for m in msgs] == plant.messages, name
        n += len(msgs)
    return n


# ---- hand-made lists -----------------------------------------------------------------------------------------------------------------
class Hand:
    """Hand-made connections whose packets are written into small streams: Hand.link() starts one, Link.event() appends an event of
    packets that alternate central, peripheral from its first.  Every packet lies at the bit offset asked for (`at`, or the next free
    one with offset % 64 == `mod`); nothing but the payload bits is read of it, so a packet may lie across the stream's end."""

    def __init__(self, n_words, n_streams=2, seed=5):
        self.rng = np.random.default_rng(seed)
        self.n_words, self.n_streams = n_words, n_streams
        self.bits = self.rng.integers(0, 2, (n_streams, 64 * n_words + 4096), dtype=np.uint8)
        self.free = [0] * n_streams
        self.links = []

    def link(self, ltk=None, stream=0):
        self.links.append(Link(self, ltk, stream))
        return self.links[-1]

    def built(self, **kw):
        words = np.stack([_le.pack(self.bits[s, :64 * self.n_words]) for s in range(self.n_streams)])
        return dm.hand_built([k.members for k in self.links], self.n_words, n_streams=self.n_streams, words=words, **kw)


class Link:
    def __init__(self, hand, ltk, stream):
        rnd = lambda n: bytes(hand.rng.integers(0, 256, n, dtype=np.uint8).tolist())           # noqa: E731
        self.hand, self.ltk, self.stream = hand, ltk, stream
        self.skdm, self.skds, self.ivm, self.ivs = rnd(8), rnd(8), rnd(4), rnd(4)
        self.members, self.events, self.sn, self.last, self.counters, self.on = [], 0, [0, 0], [None, None], [0, 0], False
        self.plain = []                                             # (role, counter, plaintext) of every encrypted PDU listed

    def req(self, **kw):
        return P(3, bytes([3]) + bytes(10) + self.skdm + self.ivm, **kw)

    def rsp(self, **kw):
        return P(3, bytes([4]) + self.skds + self.ivs, **kw)

    def event(self, packets, tail=False, mod=None, at=None, begins=False, clear=False):
        """packets: P records (retx: the role's last packet once more; lost: encrypted and counted by its sender, but not listed and
        with no part in the SN sequence the list shows).  tail: the event carries the counter of the one before it, so its members'
        roles are UNKNOWN; like them it has no part in the SN sequence.  mod: every packet's offset % 64.  at: the offset of the
        event's first packet, which may lie anywhere (the next free offset stays).  begins: encryption is on behind this event.
        clear: nothing of this event is encrypted."""
        h = self.hand
        counter = self.events - 1 if tail else self.events
        cursor = h.free[self.stream] if at is None else at
        for k, p in enumerate(packets):
            role = k & 1
            if p.retx:
                h0, payload = self.last[role]
            else:
                h0, payload = p.llid | self.sn[role] << 3 | self.sn[role ^ 1] << 2 | p.md << 4, bytes(p.payload)
                if self.on and not clear and p.llid and payload:
                    sk = session_key(self.ltk, self.skdm, self.skds)
                    if not p.lost:
                        self.plain.append((role, self.counters[role], payload))
                    payload = ccm_encrypt(sk, self.ivm + self.ivs, self.counters[role], int(role == dm.CENTRAL), h0, payload)
                    self.counters[role] += 1
                if p.lost:
                    continue
                if not tail:
                    self.sn[role] ^= 1
                    self.last[role] = (h0, payload)
            o = cursor
            if mod is not None:
                o += (mod - o) % 64
            sym = _le.tx_bits(0x50000000, self.stream % 37, bytes([h0, len(payload)]) + payload, 0x100)
            room = h.bits.shape[1] - o
            h.bits[self.stream, o:o + min(len(sym), room)] = sym[:room]
            cursor = o + len(sym) + 3
            self.members.append(dm.H(self.events, counter, h0, len(payload), o, self.stream))
        if at is None:
            h.free[self.stream] = cursor
        self.events += 1
        if begins:
            self.on = True

    def start(self, **kw):
        """The procedure: REQ and RSP in one event, an empty PDU and START in the next."""
        self.event([self.req(), self.rsp()], **kw)
        self.event([E, P(3, bytes([5]))], begins=True, **kw)
