"""The model of LE address resolution (tests/_le_resolve.py) without a GPU: the random address hash against the Core Specification's
own sample and the local openssl, the bulk trials against the scalar ones, the planted world's identities, and every deliberately
wrong model told from the right one on that world.  What counts as resolved is what the model computes, never "the planted ones"."""
import shutil
import subprocess

import pytest

import _le_crypt as cm
import _le_resolve as rm

# the Core Specification's sample of the random address hash function ah (Vol 3 Part H 2.2.2)
SPEC_IRK, SPEC_PRAND, SPEC_HASH = "ec0234a357c8ad05341010a60a397d9b", "708194", "0dfbaa"
SPEC_ADDR = bytes.fromhex("aafb0d948170")                           # a[0..5]: the hash, then prand, least significant octet first
GIVEN = [rm.THIRD_IRK, rm.THIRD_IRK]                                # (twice: the smallest matching slot is told from the largest)


def test_the_specification_sample():
    key = bytes.fromhex(SPEC_IRK)
    block = cm.aes(key, bytes(13) + bytes.fromhex(SPEC_PRAND))
    assert block.hex() == "159d5fb72ebe2311a48c1bdcc40dfbaa" and rm.ah(key, bytes.fromhex(SPEC_PRAND)).hex() == SPEC_HASH
    assert rm.kind(1, SPEC_ADDR) == rm.RESOLVABLE and rm.kind(0, SPEC_ADDR) == rm.PUBLIC
    assert rm.matches(key, SPEC_ADDR) and not rm.matches(key[::-1], SPEC_ADDR)
    for name in ("hash_prand_swapped", "block_reversed"):
        assert not rm.matches(key, SPEC_ADDR, rm.Rules(**{name: True})), name
        assert not rm.matches(key[::-1], SPEC_ADDR, rm.Rules(**{name: True})), name
    # through the model: t = 1 resolves under the key as given and under no byte-reversed form of it; t = 0 is not tried
    adv = [rm.rec(100, 0, SPEC_ADDR, tx=1), rm.rec(200, 0, SPEC_ADDR, tx=0, ch=38)]
    out = rm.resolve(adv, 0, [], [], b"", 0, [key[::-1], key], 2, 4)
    assert [(x.random, x.kind, x.irk) for x in out.addrs] == [(0, rm.PUBLIC, rm.NO_IRK), (1, rm.RESOLVABLE, 1)]
    assert [(x.n_addrs, x.n_slots) for x in out.irks] == [(0, 0), (1, 1)] and out.slot_addr == [1, rm.NONE, 0, rm.NONE]


def test_the_same_through_openssl():
    exe = shutil.which("openssl")
    if exe is None:
        pytest.skip("no openssl binary on this machine")
    got = subprocess.run([exe, "enc", "-aes-128-ecb", "-nopad", "-K", SPEC_IRK], input=bytes(13) + bytes.fromhex(SPEC_PRAND), capture_output=True,
                         check=True).stdout
    assert got[13:].hex() == SPEC_HASH
    for n, key in enumerate((rm.IRK_C, rm.IRK_P, rm.THIRD_IRK)):
        a = rm.rpa(key, 40 + n)
        got = subprocess.run([exe, "enc", "-aes-128-ecb", "-nopad", "-K", key.hex()], input=bytes(13) + a[:2:-1], capture_output=True,
                             check=True).stdout
        assert got[13:] == a[2::-1] and a[5] >> 6 == 1


def test_the_bulk_trials_are_the_scalar_ones():
    keys = [(j, rm.octets(400 + j, 16)) for j in range(5)]
    addrs = [(1, rm.rpa(keys[j % 5][1], j)) for j in range(20)] + [(1, rm.rpa(rm.octets(9, 16), j)) for j in range(20)]
    addrs += [(0, addrs[0][1]), (1, rm.rpa(keys[0][1], 50, top=3)), (1, rm.rpa(keys[0][1], 51, top=0)), (1, rm.rpa(keys[0][1], 52, top=2))]
    got = rm.trials(keys, addrs)
    want = [[slot for slot, key in keys if rm.kind(t, a) == rm.RESOLVABLE and rm.matches(key, a)] for t, a in addrs]
    assert got == want and [g for g in got[:20]] == [[j % 5] for j in range(20)] and not any(got[20:])
    everything = rm.trials(keys, addrs, rm.Rules(no_kind_test=True))
    assert everything[40:43] == [[0], [0], [0]]                     # the look-alikes hold under the key: only the kind keeps them out


@pytest.fixture(scope="module")
def world():
    conns, cands, tracks, pkts, adv, seeds, plain = rm.capture_model()
    assert len(conns) == 1 and seeds[0] is not None and seeds[0].request == 0
    return adv, seeds, plain


def _run(world, rules=rm.MODEL):
    adv, seeds, plain = world
    return rm.resolve(adv, 1, seeds, plain.msgs, plain.payload, 1 << 22, GIVEN, 8, 64, rules)


def test_the_planted_identities(world):
    adv, seeds, plain = world
    assert sorted({r["adv_type"] for r in adv}) == list(range(8)) and sum(not r["crc_ok"] for r in adv) == 1
    out = _run(world)
    assert out.n_irks == 4 and [x.flags for x in out.irks[:4]] == [1, 1, 6, 6]
    assert (out.irks[2].key, out.irks[2].id_addr, out.irks[2].id_random, out.irks[2].conn, out.irks[2].role) == (rm.IRK_C, rm.CENTRAL_ID[3], 0, 0, 0)
    assert (out.irks[3].key, out.irks[3].id_addr, out.irks[3].id_random, out.irks[3].conn, out.irks[3].role) == (rm.IRK_P, rm.PERIPHERAL_ID[3], 1, 0, 1)
    by = {(x.random, x.addr): x for x in out.addrs}
    assert all(by[(1, a)].irk == 2 for a in rm.RPAS_C + [rm.INIT_A]) and all(by[(1, a)].irk == 3 for a in rm.RPAS_P + [rm.ADV_A])
    assert by[(1, rm.RPA_THIRD)].irk == 0 and out.irks[1].n_addrs == 0
    for t, a, k in ((1, rm.RPA_UNKNOWN, rm.RESOLVABLE), (0, rm.PUBLIC_ALIKE, rm.PUBLIC), (1, rm.STATIC_ALIKE, rm.STATIC),
                    (1, rm.NONRESOLVABLE_ALIKE, rm.NONRESOLVABLE), (0, rm.PUBLIC_DEVICE, rm.PUBLIC)):
        assert (by[(t, a)].irk, by[(t, a)].kind) == (rm.NO_IRK, k)
    assert (1, rm.rpa(rm.IRK_C, 11)) not in by                       # the PDU with a bad CRC
    # an RPA repeated on two channels; the roles an address was seen in; the connection's two ends
    assert (by[(1, rm.RPAS_P[0])].channels, by[(1, rm.RPAS_P[0])].n_slots) == (3, 4) and by[(1, rm.RPAS_P[0])].roles == rm.ADVERTISER | rm.TARGET
    assert by[(1, rm.RPAS_C[2])].roles == rm.SCANNER and by[(1, rm.INIT_A)].roles == rm.INITIATOR and by[(0, rm.PUBLIC_ALIKE)].roles == rm.SCANNER
    peer = out.peers[0]
    assert (out.addrs[peer.init_addr].addr, out.addrs[peer.adv_addr].addr) == (rm.INIT_A, rm.ADV_A)
    assert (peer.init_irk, peer.adv_irk, peer.irk) == (2, 3, (2, 3))
    assert [x.n_addrs for x in out.irks[:4]] == [1, 0, 4, 4] and sum(x.n_slots for x in out.addrs) == sum(s != rm.NONE for s in out.slot_addr)


def test_every_wrong_model_is_told_from_the_right_one(world):
    right = _run(world)
    told = {}
    for name, kw in rm.VARIANTS.items():
        got = _run(world, rm.Rules(**kw))
        told[name] = (got.addrs, got.irks, got.peers, got.slot_addr) != (right.addrs, right.irks, right.peers, right.slot_addr)
        assert told[name], name
        resolved = sum(x.irk != rm.NO_IRK for x in got.addrs)
        if name in ("hash_prand_swapped", "block_reversed"):
            assert resolved == 0
        elif name == "key_as_received":                             # the caller's key still works, the harvested ones do not
            assert resolved == 1 and got.irks[2].key == rm.IRK_C[::-1]
        elif name == "no_kind_test":
            assert resolved == sum(x.irk != rm.NO_IRK for x in right.addrs) + 3
        elif name == "no_random_bit":
            assert got.n_addrs == right.n_addrs - 1
        elif name == "largest_slot":
            assert [x.n_addrs for x in got.irks[:2]] == [0, 1]
        else:
            assert got.n_addrs == right.n_addrs + 1                 # the SCAN_REQ's advertiser under the scanner's bit
    assert len(told) == 7
