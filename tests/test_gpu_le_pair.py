"""LE legacy pairing key recovery (libbtbb_amd/csrc/le_pair.h) on the GPU: btbbx_le_pair_device over hand-made message lists of a few
dozen records (tests/_le_pair.py's Plant), held against the model, every byte of d_pairs, d_keys and d_key_count; the chain data
stage -> pairing stage -> decryption stage -> pairing stage on the device with no host step; the host wrapper and the Python entries
against the models composed.  Output buffers start as 0xA5 and are a record longer than their caps, so a byte a kernel leaves
unwritten, or writes where it should not, shows.

Rule 2 puts SCONF above MCONF and SRAND above MRAND, so the peripheral's check never exists without the central's: "only one check"
is the central's alone here, with SCONF missing."""
import numpy as np
import pytest

import _le_data as dm
import _le_pair as pm
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu

SEED, MSG, PAIR = bt.LE_SEED_DTYPE, bt.LE_MSG_DTYPE, bt.LE_PAIR_DTYPE
C, S = dm.CENTRAL, dm.PERIPHERAL


@pytest.fixture(scope="module", autouse=True)
def _init():
    import torch                                            # (a torch that does not import fails these tests, it does not skip them)
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    bt.init(2)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    pad = (-a.nbytes) % 8
    raw = np.frombuffer(a.tobytes() + bytes(pad), np.int64).copy() if a.nbytes else np.zeros(1, np.int64)
    return torch.from_numpy(raw).cuda()


def _filled(nbytes):
    import torch
    return torch.full(((nbytes + 15) // 16 * 16 + 16,), 0xA5, dtype=torch.uint8, device="cuda")


def seed_array(seeds):
    """LE_SEED_DTYPE records: what the stage reads is the seeds', every other field is noise it must not read."""
    a = np.frombuffer(np.random.default_rng(77).integers(0, 256, max(len(seeds), 1) * SEED.itemsize, dtype=np.uint8).tobytes(), SEED).copy()
    for i, s in enumerate(seeds):
        if s is None:                                               # not SEEDED
            a[i]["flags"] = 0xFE
            continue
        a[i]["init_a"], a[i]["adv_a"] = np.frombuffer(s.init_a, np.uint8), np.frombuffer(s.adv_a, np.uint8)
        a[i]["tx_add"], a[i]["rx_add"] = s.tx_add | 0xA4, s.rx_add | 0x52                    # (bit 0 alone counts)
        a[i]["flags"] = s.flags
    return a


def _device(count, seeds, msgs, payload, tk_limit, key_cap, conn_cap=None, msg_cap=None, byte_cap=None, n_msgs=None):
    """btbbx_le_pair_device -> (pairs, keys, n_keys), the buffers whole: a record longer than their caps."""
    import torch
    lib = bt.lib()
    conn_cap = len(seeds) if conn_cap is None else conn_cap
    msg_cap = len(msgs) if msg_cap is None else msg_cap
    byte_cap = len(payload) if byte_cap is None else byte_cap
    d_seeds, d_msgs, d_bytes = _dev(seed_array(seeds)), _dev(dm.msg_array(msgs, MSG)), _dev(np.frombuffer(bytes(payload), np.uint8))
    d_cnt = torch.from_numpy(np.array([count, len(msgs) if n_msgs is None else n_msgs], np.uint32).view(np.int32)).cuda()
    d_pairs, d_keys, d_n = _filled((conn_cap + 1) * PAIR.itemsize), _filled(16 * (key_cap + 1)), _filled(16)
    scratch = lib.btbbx_le_pair_scratch_bytes(conn_cap)
    d_scr = _filled(scratch)
    p = d_cnt.data_ptr()
    bt.check(lib.btbbx_le_pair_device(p, conn_cap, d_seeds.data_ptr(), d_msgs.data_ptr() if msg_cap else None, p + 4, msg_cap,
                                      d_bytes.data_ptr() if byte_cap else None, byte_cap, tk_limit, d_pairs.data_ptr(),
                                      d_keys.data_ptr() if key_cap else None, key_cap, d_n.data_ptr(), d_scr.data_ptr(), scratch, None),
             "btbbx_le_pair_device")
    torch.cuda.synchronize()
    assert set(d_scr.cpu().numpy()[scratch:].tolist()) == {0xA5}                # nothing behind the scratch
    n = d_n.cpu().numpy()
    assert n[4:].tobytes() == b"\xa5" * (len(n) - 4)
    return d_pairs.cpu().numpy()[:(conn_cap + 1) * PAIR.itemsize].view(PAIR), d_keys.cpu().numpy(), int(n[:4].view(np.uint32)[0])


def _check(count, seeds, plant, tk_limit, key_cap, claims=None, **kw):
    """The device against the model -> the model's Out."""
    conn_cap = kw.get("conn_cap", len(seeds))
    k = min(count, conn_cap)
    byte_cap = kw.get("byte_cap", len(plant.payload))
    w = min(kw.get("n_msgs", len(plant.msgs)), kw.get("msg_cap", len(plant.msgs)))
    want = pm.pair(k, seeds, plant.msgs[:w], bytes(plant.payload), byte_cap, tk_limit, key_cap, claims=claims)
    pairs, keys, n_keys = _device(count, seeds, plant.msgs, plant.payload, tk_limit, key_cap, **kw)
    model = pm.pair_array(want.pairs, PAIR)
    if pairs[:k].tobytes() != model.tobytes():
        bad = [g for g in range(k) if pairs[g].tobytes() != model[g].tobytes()]
        raise AssertionError("connection %d: %s, model %s (%d of %d differ)" % (bad[0], pairs[bad[0]], model[bad[0]], len(bad), k))
    assert pairs[k:].tobytes() == b"\xa5" * (PAIR.itemsize * (len(pairs) - k))  # nothing behind the K records
    assert n_keys == want.n_keys
    assert keys[:16 * key_cap].tobytes() == want.keys and set(keys[16 * key_cap:].tolist()) == {0xA5}
    return want


def _pairings(tks, plant=None, interleave=True, **kw):
    """One connection per tk, each with a whole exchange; the connections' messages interleaved -> (seeds, plant)."""
    plant = pm.Plant() if plant is None else plant
    seeds = [pm.seed_of(g) for g in range(len(tks))]
    lists = [pm.exchange(tk, seeds[g], n=g, **kw)[0] for g, tk in enumerate(tks)]
    if interleave:
        for step in range(6):
            for g, messages in enumerate(lists):
                plant.add(g, *messages[step], fill=(g + step) % 3)
    else:
        for g, messages in enumerate(lists):
            plant.all(g, messages)
    return seeds, plant


# ---- the search --------------------------------------------------------------------------------------------------------------------------
def test_the_tk_lattice_and_every_octet_alignment():
    tks = (0, 1, 63, 64, 65, 255, 256, 4095)
    seeds, plant = _pairings(tks)
    assert {m.byte_offset % 8 for m in plant.msgs} == set(range(8))
    want = _check(len(tks), seeds, plant, 4096, 64)
    assert [p.tk for p in want.pairs] == list(tks) and all(p.flags == 0xFF and p.keys == pm.K_STK for p in want.pairs)
    assert [p.key for p in want.pairs] == list(range(8)) and want.n_keys == 8


@pytest.mark.parametrize("tk_limit", [1, 2, 257, 1000])
def test_the_limit_is_exclusive(tk_limit):
    seeds, plant = _pairings((tk_limit - 1, tk_limit, 0))
    want = _check(3, seeds, plant, tk_limit, 4)
    assert [p.tk for p in want.pairs] == [tk_limit - 1, pm.NONE, 0]
    assert [p.flags for p in want.pairs] == [0xFF, 0x7F, 0xFF] and [p.key for p in want.pairs] == [0, 0xFF, 1]


def test_the_full_range_in_one_launch():
    """A 128-bit match has no false positive, so the model checks the claimed TK alone."""
    seeds, plant = _pairings((999999, 1000000))
    want = _check(2, seeds, plant, 1000000, 64, claims=[[999999], [1000000]])
    assert [p.tk for p in want.pairs] == [999999, pm.NONE] and [p.flags for p in want.pairs] == [0xFF, 0x7F]
    assert want.n_keys == 1 and want.pairs[0].stk == want.keys[:16] and any(want.keys[:16])


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_many_armed_connections(n):
    rng = np.random.default_rng(n)
    tks = rng.integers(0, 96, n).tolist()
    seeds, plant = _pairings(tks, interleave=bool(n & 1))
    want = _check(n, seeds, plant, 96, 64)
    assert [p.tk for p in want.pairs] == tks and want.n_keys == n
    assert [p.key for p in want.pairs] == [g if g < 64 else 0xFF for g in range(n)]
    if n == 65:
        assert want.pairs[64].keys == pm.K_STK and any(want.pairs[64].stk)      # beyond key_cap: the STK stays in its record


@pytest.mark.parametrize("key_cap", [0, 1, 3])
def test_the_key_table(key_cap):
    """Connections 1 and 3 have no STK: the slots go by ascending connection index over those that have one."""
    seeds, plant = _pairings((5, 200, 7, 9, 11), interleave=False)
    plant.msgs[6 + 5] = plant.msgs[6 + 5]._replace(flags=dm.COMPLETE)            # connection 1: SRAND not STORED
    seeds[3] = seeds[3]._replace(flags=0)                                       # connection 3: not SEEDED
    want = _check(5, seeds, plant, 128, key_cap)
    assert [p.keys for p in want.pairs] == [1, 0, 1, 0, 1] and want.n_keys == 3
    assert [p.key for p in want.pairs] == [s if s < key_cap else 0xFF for s in (0, 0xFF, 1, 0xFF, 2)]
    assert want.pairs[1].flags == 0x1F | pm.F_ARMED and want.pairs[3].flags == 0x3F


def test_counts_and_caps():
    seeds, plant = _pairings((3, 4, 5))
    every = len(plant.msgs)
    for kw in (dict(count=0), dict(count=2), dict(count=7), dict(count=3, conn_cap=2), dict(count=3, n_msgs=0), dict(count=3, n_msgs=every - 1),
               dict(count=3, n_msgs=every + 9), dict(count=3, msg_cap=every - 4, n_msgs=every), dict(count=3, msg_cap=0),
               dict(count=3, byte_cap=len(plant.payload) - 1), dict(count=3, byte_cap=0)):
        count = kw.pop("count")
        want = _check(count, seeds, plant, 16, 2, **kw)
        if kw.get("n_msgs") == 0 or kw.get("msg_cap") == 0 or kw.get("byte_cap") == 0:
            assert all(p == pm.NOTHING for p in want.pairs) and len(want.pairs) == 3
    # conn_cap == 0: the count and the zeroed table, nothing else
    pairs, keys, n_keys = _device(3, seeds, plant.msgs, plant.payload, 16, 2, conn_cap=0)
    assert n_keys == 0 and keys[:32].tobytes() == bytes(32) and set(keys[32:].tolist()) == {0xA5} and set(pairs.tobytes()) == {0xA5}


# ---- the procedure -----------------------------------------------------------------------------------------------------------------------
def test_each_message_missing_in_turn():
    seeds = [pm.seed_of(g) for g in range(7)]
    plant = pm.Plant()
    for g in range(7):
        messages = pm.exchange(10 + g, seeds[g], n=g)[0]
        plant.all(g, [m for step, m in enumerate(messages) if step != g])
    want = _check(7, seeds, plant, 32, 8)
    assert [p.flags for p in want.pairs] == [0, pm.F_PREQ, 0x03, 0x37 | pm.F_ARMED | pm.F_CRACKED, 0x0F, 0x1F | pm.F_ARMED | pm.F_CRACKED, 0xFF]
    # only the central's check, SCONF missing: the TK is found, and the STK too, for both Random values are there
    assert (want.pairs[3].tk, want.pairs[3].keys, want.pairs[3].sconf, want.pairs[3].srand != pm.NONE) == (13, pm.K_STK, pm.NONE, True)
    assert (want.pairs[5].tk, want.pairs[5].keys) == (15, 0)                    # SRAND missing: CRACKED, no STK
    assert want.pairs[0].method == want.pairs[1].method == pm.NONE_M and want.pairs[2].method == pm.LEGACY


def test_the_second_check_under_another_tk():
    seeds = [pm.seed_of(g) for g in range(3)]
    plant = pm.Plant()
    plant.all(0, pm.exchange(5, seeds[0], n=0, tk_peripheral=6)[0])
    plant.all(1, pm.exchange(6, seeds[1], n=1, tk_peripheral=5)[0])
    plant.all(2, pm.exchange(6, seeds[2], n=2)[0])
    want = _check(3, seeds, plant, 64, 4)
    assert [p.flags for p in want.pairs] == [0x7F, 0x7F, 0xFF] and want.n_keys == 1 and want.pairs[2].key == 0


DECOYS = ("wrong role", "a length too short", "a length too long", "CID 4", "not COMPLETE", "not STORED", "conn >= K", "beyond byte_cap",
          "an offset that wraps", "bytes < 4 + l2cap_len")


def test_messages_that_do_not_count():
    """In front of each of the six messages of a pairing stands a message of the same code that must not be taken for it."""
    seeds = [pm.seed_of(g) for g in range(len(DECOYS))]
    plant = pm.Plant(pad=3)
    k = len(DECOYS)
    for g, how in enumerate(DECOYS):
        for step, (role, body) in enumerate(pm.exchange(20 + g, seeds[g], n=g)[0]):
            fake = body[:1] + pm.octets(900 + 10 * g + step, len(body) - 1)
            if how == "wrong role":
                plant.add(g, role ^ 1, fake)
            elif how == "a length too short":
                plant.add(g, role, fake[:-1])
            elif how == "a length too long":
                plant.add(g, role, fake + b"\x00")
            elif how == "CID 4":
                plant.add(g, role, fake, cid=4)
            elif how == "not COMPLETE":
                plant.add(g, role, fake, flags=dm.STORED)
            elif how == "not STORED":
                plant.add(g, role, fake, flags=dm.COMPLETE)
            elif how == "conn >= K":
                plant.add(k if step & 1 else 0xFFFFFFFF, role, fake)
            elif how == "beyond byte_cap":                              # its last octet would be the first one beyond
                plant.add(g, role, fake, offset=("end", 4 + len(fake) - 1))
            elif how == "an offset that wraps":
                plant.add(g, role, fake, offset=(1 << 64) - 8)
            else:
                plant.add(g, role, fake, bytes_=4 + len(fake) - 1)
            plant.add(g, role, body, fill=step % 2)
    end = len(plant.payload)
    plant.msgs = [m._replace(byte_offset=end - m.byte_offset[1]) if isinstance(m.byte_offset, tuple) else m for m in plant.msgs]
    want = _check(k, seeds, plant, 64, 16)
    assert [p.tk for p in want.pairs] == [20 + g for g in range(k)] and all(p.flags == 0xFF for p in want.pairs)
    assert all([p.preq, p.prsp, p.mconf, p.sconf, p.mrand, p.srand] == [12 * g + 2 * s + 1 for s in range(6)] for g, p in enumerate(want.pairs))


def test_messages_out_of_order():
    """Each message counts only above the one the table names: a pairing whose messages come in another order is not followed."""
    orders = ([1, 0, 2, 3, 4, 5], [0, 2, 1, 3, 4, 5], [0, 1, 3, 2, 4, 5], [0, 1, 2, 4, 3, 5], [0, 1, 2, 3, 5, 4], [5, 4, 3, 2, 1, 0],
              [0, 1, 4, 5, 2, 3], [0, 1, 2, 3, 4, 5])
    seeds = [pm.seed_of(g) for g in range(len(orders))]
    plant = pm.Plant()
    for g, order in enumerate(orders):
        messages = pm.exchange(g, seeds[g], n=g)[0]
        plant.all(g, [messages[i] for i in order])
    want = _check(len(orders), seeds, plant, 16, 16)
    assert [p.flags for p in want.pairs] == [0x01, 0x03, 0x37 | 0xC0, 0x0F, 0x1F | 0xC0, 0x01, 0x0F, 0xFF]
    # the peripheral's Confirm in front of the central's: the central's check alone, under the right TK, and the STK
    assert want.pairs[2].tk == 2 and want.pairs[2].sconf == pm.NONE and want.pairs[2].keys == pm.K_STK
    assert want.pairs[4].tk == 4 and want.pairs[4].srand == pm.NONE and want.pairs[4].keys == 0


def test_methods_seeds_and_key_sizes():
    sc = dict(preq=bytes([1, 4, 0, 0x0D, 16, 7, 7]), pres=bytes([2, 0, 0, 0x09, 16, 7, 7]))
    oob = dict(preq=bytes([1, 4, 1, 0x05, 16, 7, 7]), pres=bytes([2, 0, 1, 0x05, 16, 7, 7]))
    one_sc = dict(preq=bytes([1, 4, 1, 0x0D, 16, 7, 7]), pres=bytes([2, 0, 0, 0x05, 16, 7, 7]))
    cases = [sc, oob, one_sc, dict(ks=(6, 16)), dict(ks=(16, 6)), dict(ks=(17, 17)), dict(ks=(255, 16)), dict(ks=(7, 16)), dict(ks=(16, 15)),
             dict(ks=(16, 16)), dict(ks=(16, 16))]
    seeds = [pm.seed_of(g, seeded=g != 10) for g in range(len(cases))]
    plant = pm.Plant()
    for g, kw in enumerate(cases):
        plant.all(g, pm.exchange(g, seeds[g], n=g, **kw)[0])
    want = _check(len(cases), seeds, plant, 16, 16)
    assert [p.method for p in want.pairs] == [pm.SECURE, pm.OOB, pm.LEGACY, pm.INVALID, pm.INVALID, pm.INVALID, pm.LEGACY, pm.LEGACY, pm.LEGACY,
                                              pm.LEGACY, pm.LEGACY]
    assert [p.key_size for p in want.pairs] == [16, 16, 16, 6, 6, 17, 16, 7, 15, 16, 16]
    assert [p.flags for p in want.pairs] == [0x3F, 0x3F, 0xFF, 0x3F, 0x3F, 0x3F, 0xFF, 0xFF, 0xFF, 0xFF, 0x3F]
    for g, size in ((7, 7), (8, 15), (9, 16)):
        stk = want.pairs[g].stk
        assert stk[:16 - size] == bytes(16 - size) and len(set(stk[16 - size:])) > 4


def test_distributed_keys_and_a_limit_of_zero():
    ltk = [b"\x06" + pm.octets(600 + j, 16) for j in range(4)]
    seeds = [pm.seed_of(g) for g in range(5)]
    plant = pm.Plant()
    plant.add(1, C, ltk[0], fill=1)
    plant.add(2, S, ltk[1], fill=1)
    plant.add(3, S, ltk[2], fill=1)
    plant.add(3, C, ltk[3], fill=1)
    plant.add(3, C, ltk[0])                                                     # the first of each role counts
    plant.add(3, S, ltk[0])
    plant.add(4, C, ltk[0][:-1])                                                # 16 octets: none
    plant.add(4, S, ltk[0], cid=4)
    plant.all(1, pm.exchange(2, seeds[1], n=1)[0])
    for tk_limit in (0, 8):
        want = _check(5, seeds, plant, tk_limit, 4)
        assert [p.keys & 6 for p in want.pairs] == [0, pm.K_LTK_CENTRAL, pm.K_LTK_PERIPHERAL, 6, 0]
        assert want.pairs[1].ltk == (ltk[0][:0:-1], bytes(16)) and want.pairs[3].ltk == (ltk[3][:0:-1], ltk[2][:0:-1])
        assert want.pairs[1].flags == (0xFF if tk_limit else 0x3F) and want.n_keys == (1 if tk_limit else 0)
        assert want.pairs[0] == pm.NOTHING and want.pairs[4] == pm.NOTHING


# ---- the chain on the device ---------------------------------------------------------------------------------------------------------
def test_capture_in_plaintext_out_with_no_host_step():
    """btbbx_le_data_device -> btbbx_le_pair_device (seeds written here) -> btbbx_le_crypt_device under the pairing stage's table with
    n_keys = key_cap -> btbbx_le_pair_device with tk_limit 0 over the decrypted messages, on one stream with nothing read in between:
    the planted plaintext comes out octet for octet, and the second pass returns the LTK the peripheral distributed."""
    import torch
    import _le_crypt as cm
    import _le_discover as ld
    import _le_track as lt
    CAND, CONN, TRACK, PKT = bt.LE_CAND_DTYPE, bt.LE_CONN_DTYPE, bt.LE_TRACK_DTYPE, bt.LE_TRACK_PKT_DTYPE
    DATA, DPKT, CRYPT, CPKT = bt.LE_DATA_DTYPE, bt.LE_DATA_PKT_DTYPE, bt.LE_CRYPT_DTYPE, bt.LE_CRYPT_PKT_DTYPE
    b, stk = pm.pair_world()
    lib = bt.lib()
    n, k, key_cap, window = len(b.cands), len(b.conns), 4, 8
    seeds = [pm.WORLD_SEEDS.get(name) for name in b.names]
    legacy, secure = b.names.index(pm.LEGACY_NAME), b.names.index(pm.SECURE_NAME)
    # the models composed
    data = dm.built_model(b)
    claims = [[pm.WORLD_TK]] * k
    first = pm.pair(k, seeds, data.msgs, data.payload, data.n_bytes + 11, 1000000, key_cap, claims=claims)
    table = [first.keys[16 * j:16 * j + 16] for j in range(key_cap)]
    plain = cm.crypt(b.conns, b.cands, b.pkts, data.dpkts, b.words, b.n_words, table, window, 1 << 20, 1 << 30)
    second = pm.pair(k, seeds, plain.msgs, plain.payload, plain.n_bytes + 11, 0, 0)
    assert first.pairs[legacy].stk == stk == table[0] and first.n_keys == 1 and first.pairs[secure].method == pm.SECURE
    assert cm.check_planted(b, plain, (pm.LEGACY_NAME, pm.PLAIN_NAME, pm.SECURE_NAME)) >= 15
    assert second.pairs[legacy].ltk == (bytes(16), pm.DISTRIBUTED_LTK[:0:-1]) and not first.pairs[legacy].keys & pm.K_LTK_PERIPHERAL
    # the device
    words = np.asarray(b.words)
    d_words, d_phys = _dev(words.reshape(-1)), _dev(np.asarray(dm.MHZ, np.uint16))
    d_cands, d_conns, d_pkts = _dev(ld.cand_array(b.cands, CAND)), _dev(ld.conn_array(b.conns, CONN)), _dev(lt.pkt_array(b.pkts, PKT))
    d_tracks, d_seeds = _filled(k * TRACK.itemsize), _dev(seed_array(seeds))
    d_cnt = torch.from_numpy(np.array([n, k], np.uint32).view(np.int32)).cuda()
    caps = [(data.n_msgs + 3, data.n_bytes + 11), (plain.n_msgs + 3, plain.n_bytes + 11)]
    d_msgs = [_filled((m + 1) * MSG.itemsize) for m, _ in caps]
    d_bytes = [_filled(c + 64) for _, c in caps]
    d_counts = [_filled(16), _filled(16)]
    d_data, d_dpkts, d_ppkts = _filled((k + 1) * DATA.itemsize), _filled((n + 1) * DPKT.itemsize), _filled((n + 1) * DPKT.itemsize)
    d_crypt, d_cpkts = _filled((k + 1) * CRYPT.itemsize), _filled((n + 1) * CPKT.itemsize)
    d_pairs, d_keys, d_nkeys = [_filled((k + 1) * PAIR.itemsize) for _ in range(2)], _filled(16 * (key_cap + 1)), [_filled(16), _filled(16)]
    sizes = (lib.btbbx_le_data_scratch_bytes(n, k), lib.btbbx_le_pair_scratch_bytes(k), lib.btbbx_le_crypt_scratch_bytes(n, k, key_cap))
    d_scr = [_filled(size) for size in sizes]
    p = d_cnt.data_ptr()
    stream = (d_words.data_ptr(), b.n_words, words.shape[1], words.shape[0], d_phys.data_ptr(), d_cands.data_ptr(), p, n, d_conns.data_ptr(),
              p + 4, k, d_tracks.data_ptr(), d_pkts.data_ptr())
    bt.check(lib.btbbx_le_data_device(*stream, d_data.data_ptr(), d_dpkts.data_ptr(), d_msgs[0].data_ptr(), caps[0][0], d_counts[0].data_ptr() + 8,
                                      d_bytes[0].data_ptr(), caps[0][1], d_counts[0].data_ptr(), d_scr[0].data_ptr(), sizes[0], None), "data")
    bt.check(lib.btbbx_le_pair_device(p + 4, k, d_seeds.data_ptr(), d_msgs[0].data_ptr(), d_counts[0].data_ptr() + 8, caps[0][0],
                                      d_bytes[0].data_ptr(), caps[0][1], 1000000, d_pairs[0].data_ptr(), d_keys.data_ptr(), key_cap,
                                      d_nkeys[0].data_ptr(), d_scr[1].data_ptr(), sizes[1], None), "pair")
    bt.check(lib.btbbx_le_crypt_device(*stream, d_dpkts.data_ptr(), d_keys.data_ptr(), key_cap, window, d_crypt.data_ptr(), d_cpkts.data_ptr(),
                                       d_ppkts.data_ptr(), d_msgs[1].data_ptr(), caps[1][0], d_counts[1].data_ptr() + 8, d_bytes[1].data_ptr(),
                                       caps[1][1], d_counts[1].data_ptr(), d_scr[2].data_ptr(), sizes[2], None), "crypt")
    bt.check(lib.btbbx_le_pair_device(p + 4, k, d_seeds.data_ptr(), d_msgs[1].data_ptr(), d_counts[1].data_ptr() + 8, caps[1][0],
                                      d_bytes[1].data_ptr(), caps[1][1], 0, d_pairs[1].data_ptr(), None, 0, d_nkeys[1].data_ptr(),
                                      d_scr[1].data_ptr(), sizes[1], None), "pair, over the plaintext")
    torch.cuda.synchronize()
    for got, want in zip(d_pairs, (first, second)):
        records = got.cpu().numpy()[:(k + 1) * PAIR.itemsize].view(PAIR)
        assert records[:k].tobytes() == pm.pair_array(want.pairs, PAIR).tobytes() and set(records[k:].tobytes()) == {0xA5}
    keys = d_keys.cpu().numpy()
    assert keys[:16 * key_cap].tobytes() == first.keys and set(keys[16 * key_cap:].tolist()) == {0xA5}
    assert [int(c.cpu().numpy()[:4].view(np.uint32)[0]) for c in d_nkeys] == [1, 0]
    counts = d_counts[1].cpu().numpy()
    assert (int(counts[8:12].view(np.uint32)[0]), int(counts[:8].view(np.uint64)[0])) == (plain.n_msgs, plain.n_bytes)
    msgs = d_msgs[1].cpu().numpy()[:plain.n_msgs * MSG.itemsize].view(MSG)
    assert msgs.tobytes() == dm.msg_array(plain.msgs, MSG).tobytes()
    assert d_bytes[1].cpu().numpy()[:plain.n_bytes].tobytes() == plain.payload                 # the planted plaintext, octet for octet
    crypt = d_crypt.cpu().numpy()[:k * CRYPT.itemsize].view(CRYPT)
    assert crypt.tobytes() == cm.crypt_array(plain.crypt, CRYPT).tobytes() and crypt[legacy]["key"] == 0 and crypt[legacy]["n_failed"] == 0


# ---- the host wrapper and the Python entries ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain():
    """pair_capture and the models composed on it: discovery, tracking, the advertising scan, seeds, data, pairing."""
    cap = pm.pair_capture()
    conns, cands, tracks, pkts, seeds, data = pm.capture_model()
    by = {(p.aa, p.crc_init): p.name for p in cap.planted}
    names = [by.get((c.access_address, c.crc_init)) for c in conns]
    assert sorted(n for n in names if n) == sorted((pm.LEGACY_NAME, pm.PLAIN_NAME, pm.SECURE_NAME))
    assert [s is not None for s in seeds] == [n in (pm.LEGACY_NAME, pm.SECURE_NAME) for n in names]
    return cap, conns, cands, tracks, pkts, seeds, data, names


def _pair_model(chain, msg_cap, byte_cap, tk_limit, key_cap):
    cap, conns, cands, tracks, pkts, seeds, data, names = chain
    cut = dm.data(conns, cands, pkts, cap.words, cap.n_words, msg_cap, byte_cap)
    return pm.pair(len(conns), seeds, cut.msgs, cut.payload, byte_cap, tk_limit, key_cap, claims=[[pm.WORLD_TK]] * len(conns))


def test_the_host_wrapper_on_the_planted_capture(chain):
    import _le_discover as ld
    import _le_follow as lf
    import _le_track as lt
    CAND, CONN, TRACK, PKT = bt.LE_CAND_DTYPE, bt.LE_CONN_DTYPE, bt.LE_TRACK_DTYPE, bt.LE_TRACK_PKT_DTYPE
    cap, conns, cands, tracks, pkts, seeds, data, names = chain
    lib = bt.lib()
    legacy = names.index(pm.LEGACY_NAME)
    words, phys = np.ascontiguousarray(cap.words).reshape(-1), np.ascontiguousarray(cap.mhz, dtype=np.uint16)
    fill = lambda count, dtype: np.full(count * dtype.itemsize, 0xA5, np.uint8).view(dtype)              # noqa: E731
    k, n = len(conns) + 1, len(cands) + 1
    for msg_cap, byte_cap, tk_limit, key_cap in ((1 << 12, 1 << 16, 1000000, 64), (1 << 12, 1 << 16, pm.WORLD_TK, 2), (1 << 12, 1 << 16, 300000, 1),
                                                 (6, 1 << 16, 300000, 0), (0, 0, 300000, 3)):
        want = _pair_model(chain, msg_cap, byte_cap, tk_limit, key_cap)
        o_conns, o_cands, o_tracks, o_pkts = np.zeros(k, CONN), np.zeros(n, CAND), np.zeros(k, TRACK), np.zeros(n, PKT)
        o_seeds, o_pairs, o_keys = fill(k, SEED), fill(k, PAIR), np.full(16 * (key_cap + 1), 0xA5, np.uint8)
        counts, n_keys = np.zeros(1, np.uint64), np.full(2, 0xA5A5A5A5, np.uint32)
        got = lib.btbbx_le_pair_host(bt._ptr(words), cap.n_words, cap.pitch_words, len(cap.mhz), cap.search_bits, bt._ptr(phys), 27, 2,
                                     bt._ptr(o_conns), k, bt._ptr(o_cands), n, counts.ctypes.data, dm.UNIT, dm.IFS, dm.JITTER, lt.REMAP, 0,
                                     bt._ptr(o_tracks), bt._ptr(o_pkts), bt._ptr(o_seeds), msg_cap, byte_cap, tk_limit, bt._ptr(o_pairs),
                                     bt._ptr(o_keys) if key_cap else None, key_cap, n_keys.ctypes.data)
        assert got == len(conns), lib.btbbx_last_error()
        assert counts[0] == len(cands) and n_keys.tolist() == [want.n_keys, 0xA5A5A5A5]
        assert o_conns[:k - 1].tobytes() == ld.conn_array(conns, CONN).tobytes() and o_cands[:n - 1].tobytes() == ld.cand_array(cands, CAND).tobytes()
        assert o_tracks[:k - 1].tobytes() == lt.track_array(tracks, TRACK).tobytes() and o_pkts[:n - 1].tobytes() == lt.pkt_array(pkts, PKT).tobytes()
        assert o_seeds[:k - 1].tobytes() == lf.seed_array(seeds, SEED).tobytes() and set(o_seeds[k - 1:].tobytes()) == {0xA5}
        assert o_pairs[:k - 1].tobytes() == pm.pair_array(want.pairs, PAIR).tobytes() and set(o_pairs[k - 1:].tobytes()) == {0xA5}
        assert o_keys[:16 * key_cap].tobytes() == want.keys and set(o_keys[16 * key_cap:].tolist()) == {0xA5}
        cracked = tk_limit > pm.WORLD_TK and msg_cap > 6
        assert (want.pairs[legacy].tk == pm.WORLD_TK) == cracked and want.n_keys == int(cracked)
    # no connection stored: the table zeroed, the count 0
    o_keys[:], n_keys[:] = 0xA5, 0xA5A5A5A5
    got = lib.btbbx_le_pair_host(bt._ptr(words), cap.n_words, cap.pitch_words, len(cap.mhz), cap.search_bits, bt._ptr(phys), 27, 1000,
                                 bt._ptr(o_conns), k, bt._ptr(o_cands), n, None, dm.UNIT, dm.IFS, dm.JITTER, lt.REMAP, 0, bt._ptr(o_tracks),
                                 bt._ptr(o_pkts), bt._ptr(o_seeds), 64, 4096, 16, bt._ptr(o_pairs), bt._ptr(o_keys), 3, n_keys.ctypes.data)
    assert got == 0 and n_keys.tolist() == [0, 0xA5A5A5A5] and o_keys.tobytes() == bytes(48) + b"\xa5" * 16
    # no candidate at all: the same
    o_keys[:], n_keys[:] = 0xA5, 0xA5A5A5A5
    blank = np.zeros(256, np.uint64)
    got = lib.btbbx_le_pair_host(bt._ptr(blank), 256, 256, 1, 64 * 256 - 400, bt._ptr(phys), 27, 2, bt._ptr(o_conns), k, bt._ptr(o_cands), n,
                                 counts.ctypes.data, dm.UNIT, dm.IFS, dm.JITTER, lt.REMAP, 0, bt._ptr(o_tracks), bt._ptr(o_pkts), bt._ptr(o_seeds),
                                 64, 4096, 16, bt._ptr(o_pairs), bt._ptr(o_keys), 3, n_keys.ctypes.data)
    assert got == 0 and counts[0] == 0 and n_keys.tolist() == [0, 0xA5A5A5A5] and o_keys.tobytes() == bytes(48) + b"\xa5" * 16


def test_le_pair_and_le_crack_from_python(chain):
    import _le_crypt as cm
    import _le_discover as ld
    import _le_follow as lf
    cap, conns, cands, tracks, pkts, seeds, data, names = chain
    legacy = names.index(pm.LEGACY_NAME)
    kw = dict(min_count=2, n_streams=len(cap.mhz), pitch_words=cap.pitch_words, n_words=cap.n_words, unit_bits=dm.UNIT, ifs_bits=dm.IFS,
              jitter_bits=dm.JITTER)
    want = _pair_model(chain, 1 << 16, 1 << 22, 1000000, 64)
    pair, plain = bt.le_crack(cap.words, cap.search_bits, cap.mhz, **kw)
    g_conns, g_cands, g_tracks, g_pkts, g_seeds, pairs, keys, n_keys = pair
    assert g_conns.tobytes() == ld.conn_array(conns, bt.LE_CONN_DTYPE).tobytes() and g_cands.tobytes() == ld.cand_array(cands, bt.LE_CAND_DTYPE).tobytes()
    assert g_seeds.tobytes() == lf.seed_array(seeds, SEED).tobytes() and pairs.tobytes() == pm.pair_array(want.pairs, PAIR).tobytes()
    assert keys.shape == (64, 16) and keys.tobytes() == want.keys and n_keys == want.n_keys == 1
    assert int(pairs[legacy]["tk"]) == pm.WORLD_TK and pairs[legacy]["stk"].tobytes() == pm.pair_world()[1]
    # le_decrypt under the one recovered key: the models composed, and the planted plaintext octet for octet
    model = cm.crypt(conns, cands, pkts, data.dpkts, cap.words, cap.n_words, [want.keys[:16]], 8, 1 << 20, 1 << 30)
    msgs, payload, crypt = plain[6], plain[7], plain[8]
    assert msgs.tobytes() == dm.msg_array(model.msgs, MSG).tobytes() and payload.tobytes() == model.payload
    assert crypt.tobytes() == cm.crypt_array(model.crypt, bt.LE_CRYPT_DTYPE).tobytes() and crypt[legacy]["key"] == 0
    for p in cap.planted:
        mine = msgs[msgs["conn"] == names.index(p.name)]
        assert [(int(m["role"]), payload[int(m["byte_offset"]):int(m["byte_offset"]) + int(m["bytes"])].tobytes()) for m in mine] == p.messages
    # the passkey out of reach: nothing is raised, the pairs alone
    pair, plain = bt.le_crack(cap.words, cap.search_bits, cap.mhz, tk_limit=1000, **kw)
    assert plain is None and pair[7] == 0 and not pair[6].any() and int(pair[5][legacy]["flags"]) == 0x7F
    assert bt.le_pair(cap.words, cap.search_bits, cap.mhz, tk_limit=0, key_cap=0, **kw)[6].shape == (0, 16)
