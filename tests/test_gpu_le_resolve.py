"""LE address resolution (libbtbb_amd/csrc/le_resolve.h) on the GPU: btbbx_le_resolve_device over hand-made advertising records and
message lists, held against the model of tests/_le_resolve.py, every byte of d_slot_addr, d_addrs, d_irks, d_peers and the two
counts; the host wrappers and the Python entries on the planted capture against the models composed.  Output buffers start as 0xA5
and are a record longer than their caps, so a byte a kernel leaves unwritten, or writes where it should not, shows.

What counts as resolved is what the model computes, accidental matches included: with a few thousand addresses and up to 130 keys
there are 2^-5 of them to expect, and the comparison does not care."""
import numpy as np
import pytest

import _le_data as dm
import _le_follow as lf
import _le_pair as pm
import _le_resolve as rm
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu

PKT, SEED, MSG, ADDR, IRK, PEER = bt.LE_PKT_DTYPE, bt.LE_SEED_DTYPE, bt.LE_MSG_DTYPE, bt.LE_ADDR_DTYPE, bt.LE_IRK_DTYPE, bt.LE_PEER_DTYPE
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
    """LE_SEED_DTYPE records: what the stage reads is flags and request, every other field is noise it must not read."""
    a = np.frombuffer(np.random.default_rng(78).integers(0, 256, max(len(seeds), 1) * SEED.itemsize, dtype=np.uint8).tobytes(), SEED).copy()
    for i, s in enumerate(seeds):
        if s is None:                                               # not SEEDED
            a[i]["flags"] = 0xFE
            continue
        a[i]["request"], a[i]["flags"] = s.request, s.flags
    return a


def _device(adv, seeds, msgs, payload, given, irk_cap, addr_cap, adv_count=None, adv_cap=None, conn_count=None, conn_cap=None, msg_cap=None,
            byte_cap=None, n_msgs=None):
    """btbbx_le_resolve_device -> (slot_addr, addrs, n_addrs, irks, n_irks, peers), the buffers whole: a record longer than their caps."""
    import torch
    lib = bt.lib()
    adv_cap = len(adv) if adv_cap is None else adv_cap
    conn_cap = len(seeds) if conn_cap is None else conn_cap
    msg_cap = len(msgs) if msg_cap is None else msg_cap
    byte_cap = len(payload) if byte_cap is None else byte_cap
    d_adv, d_seeds, d_msgs = _dev(lf.adv_array(adv, PKT)), _dev(seed_array(seeds)), _dev(dm.msg_array(msgs, MSG))
    d_bytes, d_given = _dev(np.frombuffer(bytes(payload), np.uint8)), _dev(np.frombuffer(b"".join(given), np.uint8))
    counts = [len(adv) if adv_count is None else adv_count, len(seeds) if conn_count is None else conn_count, len(msgs) if n_msgs is None else n_msgs]
    d_cnt = torch.from_numpy(np.array(counts, np.uint32).view(np.int32)).cuda()
    d_slots, d_addrs, d_irks = _filled(8 * adv_cap + 8), _filled((addr_cap + 1) * ADDR.itemsize), _filled((irk_cap + 1) * IRK.itemsize)
    d_peers, d_n = _filled((conn_cap + 1) * PEER.itemsize), _filled(16)
    scratch = lib.btbbx_le_resolve_scratch_bytes(adv_cap, conn_cap, irk_cap)
    d_scr = _filled(scratch)
    p = d_cnt.data_ptr()
    bt.check(lib.btbbx_le_resolve_device(d_adv.data_ptr(), p, adv_cap, p + 4, conn_cap, d_seeds.data_ptr(), d_msgs.data_ptr() if msg_cap else None,
                                         p + 8, msg_cap, d_bytes.data_ptr() if byte_cap else None, byte_cap,
                                         d_given.data_ptr() if given else None, len(given), d_slots.data_ptr(),
                                         d_addrs.data_ptr() if addr_cap else None, addr_cap, d_n.data_ptr(),
                                         d_irks.data_ptr() if irk_cap else None, irk_cap, d_n.data_ptr() + 4, d_peers.data_ptr(), d_scr.data_ptr(),
                                         scratch, None), "btbbx_le_resolve_device")
    torch.cuda.synchronize()
    assert set(d_scr.cpu().numpy()[scratch:].tolist()) == {0xA5}                # nothing behind the scratch
    n = d_n.cpu().numpy()
    assert n[8:].tobytes() == b"\xa5" * (len(n) - 8)
    return (d_slots.cpu().numpy(), d_addrs.cpu().numpy(), int(n[:4].view(np.uint32)[0]), d_irks.cpu().numpy(), int(n[4:8].view(np.uint32)[0]),
            d_peers.cpu().numpy())


def _check(adv, seeds, plant, given, irk_cap, addr_cap, **kw):
    """The device against the model -> the model's Out."""
    a = min(kw.get("adv_count", len(adv)), kw.get("adv_cap", len(adv)))
    adv_cap = kw.get("adv_cap", len(adv))
    conn_cap = kw.get("conn_cap", len(seeds))
    k = min(kw.get("conn_count", len(seeds)), conn_cap)
    byte_cap = kw.get("byte_cap", len(plant.payload))
    w = min(kw.get("n_msgs", len(plant.msgs)), kw.get("msg_cap", len(plant.msgs)))
    want = rm.resolve(adv[:a], k, seeds, plant.msgs[:w], bytes(plant.payload), byte_cap, given, irk_cap, addr_cap)
    slots, addrs, n_addrs, irks, n_irks, peers = _device(adv, seeds, plant.msgs, plant.payload, given, irk_cap, addr_cap, **kw)
    assert (n_addrs, n_irks) == (want.n_addrs, want.n_irks)
    model = np.array(want.slot_addr + [rm.NONE] * (2 * (adv_cap - a)), np.uint32)
    got = slots[:8 * adv_cap].view(np.uint32)
    assert got.tobytes() == model.tobytes(), np.flatnonzero(got != model)[:8]
    assert set(slots[8 * adv_cap:].tolist()) == {0xA5}
    stored = min(want.n_addrs, addr_cap)
    model = rm.addr_array(want.addrs[:stored], ADDR)
    got = addrs[:stored * ADDR.itemsize].view(ADDR)
    if got.tobytes() != model.tobytes():
        bad = [i for i in range(stored) if got[i].tobytes() != model[i].tobytes()]
        raise AssertionError("address %d: %s, model %s (%d of %d differ)" % (bad[0], got[bad[0]], model[bad[0]], len(bad), stored))
    assert set(addrs[stored * ADDR.itemsize:].tolist()) == {0xA5}               # nothing behind the stored records
    model = rm.irk_array(want.irks, IRK)
    got = irks[:irk_cap * IRK.itemsize].view(IRK)
    if got.tobytes() != model.tobytes():
        bad = [i for i in range(irk_cap) if got[i].tobytes() != model[i].tobytes()]
        raise AssertionError("slot %d: %s, model %s (%d of %d differ)" % (bad[0], got[bad[0]], model[bad[0]], len(bad), irk_cap))
    assert set(irks[irk_cap * IRK.itemsize:].tolist()) == {0xA5}
    assert peers[:k * PEER.itemsize].tobytes() == rm.peer_array(want.peers, PEER).tobytes(), (peers[:k * PEER.itemsize].view(PEER), want.peers)
    assert set(peers[k * PEER.itemsize:].tolist()) == {0xA5}
    return want


# ---- hand-made lists -----------------------------------------------------------------------------------------------------------------
def keys_of(n, seed):
    """A table of n keys: with two or more a NULLKEY in front; with four or more the HOT key at slots 1, 2 and n - 1 (a duplicate at a
    smaller and at a larger slot than the one in the middle) -> (keys, the keys addresses are made under)."""
    keys = [rm.octets(100 * seed + j, 16) for j in range(n)]
    if n >= 2:
        keys[0] = bytes(16)
    if n >= 4:
        keys[1] = keys[2] = keys[n - 1]
    return keys, [keys[j] for j in sorted({n - 1, n // 2, 0}) if n]


def adv_list(n_addr, under, seed):
    """Records that hold n_addr distinct addresses in all: every fourth an RPA under one of `under` (the all-zero key among them),
    the others RPAs of no key, static, non-resolvable and public addresses; two keys that differ in bit 48 alone; PDUs of every type,
    every second address in two slots or more, offsets out of order."""
    rng = np.random.default_rng(seed)
    made = []
    while len(made) < n_addr:
        i = len(made)
        if i == 1 and made[0][0] == 1:
            made.append((0, made[0][1]))                            # the same 48 bits as a public address
        elif i % 4 == 0 and under:
            made.append((1, rm.rpa(under[(i // 4) % len(under)], 10 * seed + i)))
        else:
            a = bytearray(rng.integers(0, 256, 6, dtype=np.uint8).tolist())
            t = int(i % 7 != 3)
            a[5] = (a[5] & 0x3F) | ((1, 1, 3, 0, 1, 2, 1)[i % 7] << 6)
            if (t, bytes(a)) not in made:
                made.append((t, bytes(a)))
    recs = []
    for i, (t, a) in enumerate(made):
        other_t, other = made[(i * 7 + 3) % len(made)]
        ty = (0, 2, 4, 6, 1, 3, 5, 0)[i % 8]
        off = int(rng.integers(0, 1 << 40))
        ch = 37 + i % 3
        if ty in (1, 3, 5):
            recs.append(rm.rec(off, ty, a, other, tx=t, rx=other_t, ch=ch))
        else:
            recs.append(rm.rec(off, ty, a + b"\x01\x02\x03", tx=t, rx=int(rng.integers(0, 2)), ch=ch))
        if i % 2:
            recs.append(rm.rec(int(rng.integers(0, 1 << 40)), 0, a, tx=t, ch=37 + (i + 1) % 3))
    if recs:                                                        # records that fill no slot
        recs.insert(len(recs) // 2, rm.rec(5, 0, made[0][1], tx=made[0][0], crc_ok=0))
        recs.append(rm.rec(6, 0, rm.octets(seed, 6), tx=1, is_data=1))
        recs.append(rm.rec(7, 0, rm.octets(seed + 1, 6), tx=1, ch=36))
        recs.append(rm.rec(8, 7, rm.octets(seed + 2, 6), tx=1))
        recs.append(rm.rec(9, 0, rm.octets(seed + 3, 6), tx=1, length=5))
        recs.append(rm.rec(10, 3, rm.octets(seed + 4, 6), rm.octets(seed + 5, 6), tx=1, rx=1, length=11))
    return recs


LATTICE = ((0, 2), (1, 0), (63, 1), (64, 63), (65, 64), (255, 65), (256, 2), (257, 1), (4095, 2), (4096, 64), (4097, 130))


@pytest.mark.parametrize("n_addr,n_keys", LATTICE)
def test_the_address_and_table_lattice(n_addr, n_keys):
    """4095 to 4097 distinct addresses cross a sort tile; 4097 addresses times 130 slots are more trials than the fixed grid takes in
    one stride."""
    keys, under = keys_of(n_keys, n_addr)
    adv = adv_list(n_addr, under, n_addr)
    want = _check(adv, [], pm.Plant(), keys, n_keys, n_addr + 3)
    assert want.n_addrs == n_addr and want.n_irks == n_keys
    if n_addr >= 63 and n_keys:
        hot = n_keys - 1 if n_keys < 4 else 1
        if n_keys >= 2:
            assert want.irks[0].flags == rm.GIVEN | rm.NULLKEY and want.irks[0].n_addrs == 0
        if n_keys >= 4:
            assert want.irks[2].n_addrs == want.irks[n_keys - 1].n_addrs == 0   # the duplicates: the smallest slot has them all
        if n_keys != 2:
            assert want.irks[hot].n_addrs >= n_addr // 16 and want.irks[hot].n_slots >= want.irks[hot].n_addrs
        resolved = sum(x.irk != rm.NO_IRK for x in want.addrs)
        assert resolved >= (n_addr // 8 if n_keys > 2 else 0) and all(x.kind == rm.RESOLVABLE for x in want.addrs if x.irk != rm.NO_IRK)
    if n_addr >= 2:
        twins = [x for x in want.addrs if x.addr == bytes(adv[0]["bytes"][6:12])]
        assert [x.random for x in twins] == [0, 1]                              # two keys that differ in bit 48 alone


def test_one_address_in_5000_slots():
    """A segment over two sort tiles and twenty workgroups of the tallies."""
    key = rm.octets(77, 16)
    busy, quiet = rm.rpa(key, 1), rm.rpa(key, 2)
    rng = np.random.default_rng(3)
    adv = [rm.rec(int(o), 0, busy, tx=1, ch=37 + j % 3) for j, o in enumerate(rng.integers(1000, 1 << 47, 2500))]
    adv += [rm.rec(int(o), 3, quiet, busy, tx=1, rx=1, ch=38) for o in rng.integers(1000, 1 << 47, 2499)]
    adv += [rm.rec(999, 5, quiet, busy, tx=1, rx=1, ch=39), rm.rec(1 << 47, 1, busy, quiet, tx=1, rx=1, ch=37)]
    order = rng.permutation(len(adv))
    adv = [adv[j] for j in order]
    want = _check(adv, [], pm.Plant(), [key], 1, 4)
    by = {x.addr: x for x in want.addrs}
    assert by[busy].n_slots == 5001 and by[quiet].n_slots == 2501 and want.n_addrs == 2
    assert (by[busy].first_offset, by[busy].last_offset, by[busy].roles, by[busy].channels) == (999, 1 << 47, 1, 7) and by[quiet].roles == 14
    assert want.irks[0].n_addrs == 2 and want.irks[0].n_slots == 7502


def _identities():
    """Four connections: 0 distributes both identities, 1 the peripheral's key without an address, 2 an address without a key and an
    all-zero key, 3 nothing; decoys in front.  Their CONNECT_INDs between RPAs of those keys -> (adv, seeds, plant, the identities)."""
    ids = [rm.identity(C, 11), rm.identity(S, 12, 1), rm.identity(S, 13), rm.identity(C, 14, 1)]
    plant = pm.Plant(pad=3)
    plant.add(0, C, b"\x08" + rm.octets(1, 15))                                 # 16 octets: none
    plant.add(0, C, ids[0][0][1], cid=4)
    plant.add(0, C, ids[0][0][1], flags=dm.COMPLETE)
    plant.add(0, S, ids[1][1][1], fill=1)                                       # the address in front of the key
    plant.add(0, C, ids[0][0][1], fill=2)
    plant.add(0, C, b"\x08" + rm.octets(2, 16))                                 # the first of each counts
    plant.add(0, S, ids[1][0][1])
    plant.add(0, C, ids[0][1][1], fill=1)
    plant.add(0, C, b"\x09\x01" + rm.octets(3, 6))
    plant.add(1, S, ids[2][0][1])
    plant.add(2, C, ids[3][1][1])
    plant.add(2, S, b"\x08" + bytes(16))
    plant.add(9, C, ids[3][0][1])                                               # conn >= K
    plant.add(3, 2, ids[3][0][1])                                               # a role that is none
    keys = [ids[0][2], ids[1][2], ids[2][2]]
    adv = [rm.rec(5000, 0, rm.rpa(keys[2], 1), tx=1), rm.rec(100, 5, rm.rpa(keys[0], 2), rm.rpa(keys[1], 3), tx=1, rx=1, length=34),
           rm.rec(200, 5, rm.rpa(keys[0], 4), rm.rpa(keys[2], 5), tx=1, rx=1, length=34, ch=38),
           rm.rec(300, 5, rm.octets(4, 6), rm.rpa(bytes(16), 6), tx=0, rx=1, length=34, ch=39), rm.rec(400, 0, rm.rpa(keys[1], 3), tx=1)]
    seeds = [rm.Seed(1, 1), rm.Seed(2, 1), rm.Seed(3, 1), None]
    return adv, seeds, plant, keys


def test_the_harvest_and_the_peers():
    adv, seeds, plant, keys = _identities()
    given = [rm.octets(5, 16)]
    want = _check(adv, seeds, plant, given, 8, 16)
    assert want.n_irks == 5 and [x.flags for x in want.irks[:5]] == [1, 6, 6, 2, 2 | 8]
    assert [(x.conn, x.role) for x in want.irks[1:5]] == [(0, 0), (0, 1), (1, 1), (2, 1)] and [x.key for x in want.irks[1:4]] == keys
    assert want.irks[2].id_random == 1 and want.irks[1].id_addr == rm.identity(C, 11)[3]
    assert [p.irk for p in want.peers] == [(1, 2), (rm.NO_IRK, 3), (rm.NO_IRK, 4), (rm.NO_IRK, rm.NO_IRK)]
    assert [(p.init_irk, p.adv_irk) for p in want.peers] == [(1, 2), (1, 3), (rm.NO_IRK, rm.NO_IRK), (rm.NO_IRK, rm.NO_IRK)]
    assert want.peers[3].init_addr == rm.NONE and want.peers[2].init_addr != rm.NONE


def test_counts_and_caps():
    adv, seeds, plant, keys = _identities()
    given = [keys[2], rm.octets(5, 16)]
    every = len(plant.msgs)
    full = rm.resolve(adv, 4, seeds, plant.msgs, bytes(plant.payload), len(plant.payload), given, 8, 16)
    for kw in (dict(irk_cap=3), dict(irk_cap=2), dict(irk_cap=5), dict(addr_cap=0), dict(addr_cap=full.n_addrs - 1), dict(adv_cap=3),
               dict(adv_count=2), dict(adv_count=9), dict(adv_count=0), dict(conn_cap=0), dict(conn_cap=1), dict(conn_count=2),
               dict(conn_count=9), dict(msg_cap=0), dict(msg_cap=every - 5), dict(n_msgs=every - 3), dict(n_msgs=every + 4), dict(n_msgs=0),
               dict(byte_cap=len(plant.payload) - 1), dict(byte_cap=0)):
        irk_cap, addr_cap = kw.pop("irk_cap", 8), kw.pop("addr_cap", 16)
        want = _check(adv, seeds, plant, given, irk_cap, addr_cap, **kw)
        if irk_cap < 8:                                                         # the count says what there was; beyond the cap: not tried
            assert want.n_irks == 6 and [p.irk for p in want.peers][0] == tuple(s if s < irk_cap else rm.NO_IRK for s in (2, 3))
        if kw.get("msg_cap") == 0 or kw.get("n_msgs") == 0 or kw.get("byte_cap") == 0 or kw.get("conn_cap") == 0:
            assert want.n_irks == 2
        if kw.get("adv_cap") == 3 or kw.get("adv_count") == 2:                  # a seed whose request is >= A
            assert want.peers[2].init_addr == rm.NONE and want.peers[2].adv_addr == rm.NONE


def test_argument_errors_write_nothing():
    import torch
    lib = bt.lib()
    buf = _filled(1 << 16)
    p = buf.data_ptr()
    scratch = lib.btbbx_le_resolve_scratch_bytes(4, 2, 8)

    def run(irk_cap=8, n_given=1, scr_bytes=scratch, adv=p, addrs=p + 1024, scr=p + 4096):
        return lib.btbbx_le_resolve_device(adv, p, 4, p, 2, p, p, p, 4, p, 64, p, n_given, p, addrs, 4, p, p + 2048, irk_cap, p, p + 3072, scr,
                                           scr_bytes, None)

    assert scratch + 4096 < 1 << 16
    for kw in (dict(irk_cap=4097), dict(n_given=9), dict(scr_bytes=scratch - 1), dict(adv=None), dict(adv=p + 4), dict(addrs=p + 1028),
               dict(scr=p + 4104), dict(scr=None)):
        assert run(**kw) == -3, kw
        assert b"btbbx_le_resolve_device" in lib.btbbx_last_error()
    torch.cuda.synchronize()
    assert set(buf.cpu().numpy().tolist()) == {0xA5}


# ---- the host wrappers and the Python entries ----------------------------------------------------------------------------------------------
def _planted_checks(addrs, slot_of):
    """The planted addresses in a resolved list: every planted RPA on its key, the look-alikes and the unknown RPA on none."""
    by = {(int(x["random"]), x["addr"].tobytes()): int(x["irk"]) for x in addrs}
    for a in rm.RPAS_C + [rm.INIT_A]:
        assert by[(1, a)] == slot_of["central"], a
    for a in rm.RPAS_P + [rm.ADV_A]:
        assert by[(1, a)] == slot_of["peripheral"], a
    assert by[(1, rm.RPA_THIRD)] == slot_of["third"]
    for t, a in ((1, rm.RPA_UNKNOWN), (0, rm.PUBLIC_ALIKE), (1, rm.STATIC_ALIKE), (1, rm.NONRESOLVABLE_ALIKE), (0, rm.PUBLIC_DEVICE)):
        assert by[(t, a)] == rm.NO_IRK, (t, a)
    assert (1, rm.rpa(rm.IRK_C, 11)) not in by                                  # the PDU with a bad CRC filled no slot


def test_le_resolve_on_the_advertising_streams():
    cap = rm.resolve_capture()
    adv = rm.adv_records()
    given = [rm.THIRD_IRK, rm.IRK_C, rm.IRK_P]
    want = rm.resolve(adv, 0, [], [], b"", 0, given, 3, 1 << 20)
    words = np.ascontiguousarray(cap.words[37:])
    got_adv, slot_addr, addrs, table = bt.le_resolve(words, cap.search_bits, cap.mhz[37:], given, n_streams=3, pitch_words=cap.pitch_words,
                                                     n_words=cap.n_words)
    assert got_adv.tobytes() == lf.adv_array(adv, PKT).tobytes() and len(adv) == 19
    assert slot_addr.reshape(-1).tolist() == want.slot_addr
    assert addrs.tobytes() == rm.addr_array(want.addrs, ADDR).tobytes() and table.tobytes() == rm.irk_array(want.irks, IRK).tobytes()
    _planted_checks(addrs, dict(third=0, central=1, peripheral=2))
    # the caps: the prefixes, the counts say so
    lib = bt.lib()
    o_adv, o_slots, o_addrs = np.full(5 * PKT.itemsize, 0xA5, np.uint8), np.full(8 * 5, 0xA5, np.uint8), np.full(4 * ADDR.itemsize, 0xA5, np.uint8)
    o_irks, n = np.full(3 * IRK.itemsize, 0xA5, np.uint8), np.full(2, 0xA5A5A5A5, np.uint32)
    phys, flat = np.ascontiguousarray(cap.mhz[37:], dtype=np.uint16), words.reshape(-1)
    keys = np.frombuffer(b"".join(given), np.uint8)
    got = lib.btbbx_le_resolve_adv_host(bt._ptr(flat), cap.n_words, cap.pitch_words, 3, cap.search_bits, bt._ptr(phys), 0, bt._ptr(keys), 2,
                                        bt._ptr(o_adv), 4, bt._ptr(o_slots), bt._ptr(o_addrs), 3, n.ctypes.data, bt._ptr(o_irks), 2,
                                        n.ctypes.data + 4)
    assert got == 19, lib.btbbx_last_error()
    cut = rm.resolve(adv[:4], 0, [], [], b"", 0, given[:2], 2, 3)
    assert n.tolist() == [cut.n_addrs, 2] and cut.n_addrs > 3
    assert o_adv[:4 * PKT.itemsize].tobytes() == lf.adv_array(adv[:4], PKT).tobytes() and set(o_adv[4 * PKT.itemsize:].tolist()) == {0xA5}
    assert o_slots[:32].view(np.uint32).tolist() == cut.slot_addr and set(o_slots[32:].tolist()) == {0xA5}
    assert o_addrs[:3 * ADDR.itemsize].tobytes() == rm.addr_array(cut.addrs[:3], ADDR).tobytes() and set(o_addrs[3 * ADDR.itemsize:].tolist()) == {0xA5}
    assert o_irks[:2 * IRK.itemsize].tobytes() == rm.irk_array(cut.irks, IRK).tobytes() and set(o_irks[2 * IRK.itemsize:].tolist()) == {0xA5}


def test_le_identify_and_le_crack_identify():
    import _le_discover as ld
    cap = rm.resolve_capture()
    conns, cands, tracks, pkts, adv, seeds, plain = rm.capture_model()
    stk = rm.resolve_world()[1]
    assert len(conns) == 1 and seeds[0] is not None
    kw = dict(max_len=31, min_count=2, n_streams=len(cap.mhz), pitch_words=cap.pitch_words, n_words=cap.n_words, unit_bits=dm.UNIT,
              ifs_bits=dm.IFS, jitter_bits=dm.JITTER)
    given = [rm.THIRD_IRK]
    want = rm.resolve(adv, 1, seeds, plain.msgs, plain.payload, 1 << 22, given, 8, 64)
    got = bt.le_identify(cap.words, cap.search_bits, cap.mhz, [stk], irks=given, irk_cap=8, addr_cap=64, **kw)
    g_conns, g_cands, g_tracks, g_pkts, g_seeds, peers, table, addrs, n_irks, n_addrs = got
    assert g_conns.tobytes() == ld.conn_array(conns, bt.LE_CONN_DTYPE).tobytes() and g_seeds.tobytes() == lf.seed_array(seeds, SEED).tobytes()
    assert (n_irks, n_addrs) == (want.n_irks, want.n_addrs) == (3, len(want.addrs))
    assert table.tobytes() == rm.irk_array(want.irks, IRK).tobytes() and addrs.tobytes() == rm.addr_array(want.addrs, ADDR).tobytes()
    assert peers.tobytes() == rm.peer_array(want.peers, PEER).tobytes()
    # the two harvested keys, their identity addresses, both peers' slots
    assert table[1]["key"].tobytes() == rm.IRK_C and table[2]["key"].tobytes() == rm.IRK_P
    assert table[1]["id_addr"].tobytes() == rm.CENTRAL_ID[3] and table[2]["id_addr"].tobytes() == rm.PERIPHERAL_ID[3]
    assert (int(table[1]["id_random"]), int(table[2]["id_random"])) == (0, 1) and [int(f) for f in table["flags"][:3]] == [1, 6, 6]
    assert peers[0]["irk"].tolist() == [1, 2] and (int(peers[0]["init_irk"]), int(peers[0]["adv_irk"])) == (1, 2)
    assert addrs[int(peers[0]["init_addr"])]["addr"].tobytes() == rm.INIT_A and addrs[int(peers[0]["adv_addr"])]["addr"].tobytes() == rm.ADV_A
    _planted_checks(addrs, dict(third=0, central=1, peripheral=2))
    # no key given: the passkey is searched, the identities come out the same; out of reach: None
    pair, ident = bt.le_crack_identify(cap.words, cap.search_bits, cap.mhz, irks=given, irk_cap=8, addr_cap=64, **kw)
    assert pair[7] == 1 and pair[6][0].tobytes() == stk and int(pair[5][0]["tk"]) == rm.WORLD_TK
    assert all(x.tobytes() == y.tobytes() for x, y in zip(ident[:8], got[:8])) and ident[8:] == got[8:]
    pair, ident = bt.le_crack_identify(cap.words, cap.search_bits, cap.mhz, tk_limit=1000, **kw)
    assert ident is None and pair[7] == 0


def test_le_identify_when_the_advertising_block_had_to_grow():
    """tests/_le_follow.py's crowded capture: more advertising hits than the chain's first block holds, so the stage runs over the
    second, larger block with a slot map and a scratch of its own.  Nothing pairs there: the table is the caller's key alone."""
    import _le_discover as ld
    cap = lf.crowded_adv_capture()
    conns, cands, tracks, pkts, adv, seeds = lf.capture_model(cap)[:6]
    assert len(adv) > 4096 + cap.search_bits // 16384 * len(cap.mhz) and sum(s is not None for s in seeds) == 1
    given = [rm.octets(1, 16)]
    want = rm.resolve(adv, len(conns), seeds, [], b"", 0, given, 4, 64)
    got = bt.le_identify(cap.words, cap.search_bits, cap.mhz, [bytes(range(16))], irks=given, irk_cap=4, addr_cap=64, max_len=27, min_count=2,
                         n_streams=len(cap.mhz), pitch_words=cap.pitch_words, n_words=cap.n_words)
    g_conns, g_cands, g_tracks, g_pkts, g_seeds, peers, table, addrs, n_irks, n_addrs = got
    assert g_conns.tobytes() == ld.conn_array(conns, bt.LE_CONN_DTYPE).tobytes() and g_seeds.tobytes() == lf.seed_array(seeds, SEED).tobytes()
    assert (n_irks, n_addrs) == (want.n_irks, want.n_addrs) == (1, len(want.addrs)) and n_addrs >= 2
    assert table.tobytes() == rm.irk_array(want.irks, IRK).tobytes() and addrs.tobytes() == rm.addr_array(want.addrs, ADDR).tobytes()
    assert peers.tobytes() == rm.peer_array(want.peers, PEER).tobytes()
    seeded = [g for g, s in enumerate(seeds) if s is not None][0]
    assert int(peers[seeded]["init_addr"]) != rm.NONE and int(peers[seeded]["adv_addr"]) != rm.NONE
    assert addrs[int(peers[seeded]["adv_addr"])]["kind"] == rm.RESERVED and addrs[int(peers[seeded]["init_addr"])]["kind"] == rm.PUBLIC
