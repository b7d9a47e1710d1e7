"""The model of LE decryption (tests/_le_crypt.py) without a GPU: its AES against FIPS-197 and the local openssl, rules 3 and 5
against the Core Specification's encryption sample data (tests/golden/le_crypt_core_spec_samples.json), the planted worlds recovered
octet for octet, and every deliberately wrong model told from the right one."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import _le_crypt as cm
import _le_data as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = bytes.fromhex


def test_aes_fips_197_c1():
    assert cm.SBOX[:4] == [0x63, 0x7C, 0x77, 0x7B] and cm.SBOX[0x53] == 0xED and sorted(cm.SBOX) == list(range(256))
    assert cm.aes(bytes(range(16)), H("00112233445566778899aabbccddeeff")) == H("69c4e0d86a7b0430d8cdb78070b4c55a")


def test_aes_against_openssl():
    exe = shutil.which("openssl")
    if exe is None:
        pytest.skip("no openssl binary on this machine")
    rng = np.random.default_rng(12)
    for _ in range(4):
        key, blocks = rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), rng.integers(0, 256, 16 * 8, dtype=np.uint8).tobytes()
        got = subprocess.run([exe, "enc", "-aes-128-ecb", "-nopad", "-K", key.hex()], input=blocks, capture_output=True, check=True).stdout
        assert got == b"".join(cm.aes(key, blocks[j:j + 16]) for j in range(0, len(blocks), 16))


@pytest.fixture(scope="module")
def samples():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "le_crypt_core_spec_samples.json")))


def test_the_session_key_of_the_specification(samples):
    sk = cm.session_key(H(samples["ltk"]), H(samples["skdm_as_received"]), H(samples["skds_as_received"]))
    assert sk == H(samples["session_key"])
    assert cm.session_key(H(samples["ltk"]), H(samples["skdm_as_received"]), H(samples["skds_as_received"]), cm.Rules(skd_swap=True)) != sk


def test_the_packets_of_the_specification(samples):
    sk, iv = H(samples["session_key"]), H(samples["ivm"]) + H(samples["ivs"])
    assert len(samples["packets"]) == 3
    for p in samples["packets"]:
        plain, octets = H(p["plaintext"]), H(p["ciphertext"]) + H(p["mic"])
        args = (p["counter"], int(p["central"]), int(p["header0"], 16))
        assert cm.ccm_encrypt(sk, iv, *args, plain) == octets
        assert cm.trial(sk, iv, *args, octets) == plain
        assert cm.trial(sk, iv, p["counter"] + 1, *args[1:], octets) is None
        wrong = [v for v in ("dir_flip", "aad_unmasked", "b0_whole_length", "block_counter_le", "no_padding")
                 if cm.trial(sk, iv, *args, octets, cm.Rules(**{v: True})) is None]
        # (a one-octet plaintext has one keystream block, whose number reads the same in either byte order only when it is 0 -- block
        # 1 does not; the unmasked AAD differs because every sample header has SN, NESN or MD set)
        assert wrong == ["dir_flip", "aad_unmasked", "b0_whole_length", "block_counter_le", "no_padding"], (p, wrong)
    assert cm.trial(sk, H(samples["ivs"]) + H(samples["ivm"]), 0, 1, 0x0F, H("9FCDA7F448")) is None


KEYS = list(cm.WORLD_KEYS)


@pytest.fixture(scope="module")
def world():
    b = cm.planted_world()
    return b, cm.built_model(b, KEYS)


def test_the_planted_plaintext_is_recovered(world):
    b, (data, out) = world
    by = {name: g for g, name in enumerate(b.names)}
    rec = {name: out.crypt[g] for name, g in by.items() if name}
    a, never, lost, nokey = (rec["crypt: " + n] for n in ("encrypts", "never encrypts", "a lost packet", "a key that is not in the table"))
    assert a.flags == 31 and a.key == 1 and a.n_failed == 0 and a.n_verified == a.n_encrypted >= 12 and a.n_skipped == 2 and a.max_skew == 0
    assert never.flags == 0 and never.key == 0xFF and never.n_encrypted == 0
    assert lost.flags == 31 and lost.key == 2 and lost.n_failed == 0 and lost.max_skew == 2 and lost.n_skipped == 0
    assert nokey.flags == 15 and nokey.key == 0xFF and nokey.n_failed == nokey.n_encrypted == 3 and nokey.n_verified == 0
    names = ("crypt: encrypts", "crypt: never encrypts", "crypt: a lost packet")
    assert cm.check_planted(b, out, names) == sum(len(p.messages) for p in b.planted if p.name in names) == 19
    # the data stage on the same list hands out ciphertext: its messages differ behind the start
    assert out.payload != data.payload and data.n_bytes > out.n_bytes
    opcodes = [out.cpkts[i].opcode for i, c in enumerate(b.cands) if c.channel == by["crypt: encrypts"] and out.cpkts[i].opcode != 0xFF]
    assert sorted(opcodes) == [0x06, 0x06, 0x12]
    g = by["crypt: a key that is not in the table"]             # rule 8: FAILED members are no fragments
    assert all(out.ppkts[i].kind == dm.IGNORED for i, c in enumerate(b.cands) if c.channel == g and out.cpkts[i].state == cm.FAILED)


def test_without_an_armed_connection_the_messages_are_the_data_stages():
    b = dm.planted_world()
    data, out = cm.built_model(b, KEYS)
    assert (out.msgs, out.payload, out.n_msgs, out.n_bytes, out.ppkts) == (data.msgs, data.payload, data.n_msgs, data.n_bytes, data.dpkts)
    assert all(r.flags == 0 and r.key == 0xFF for r in out.crypt) and {p.state for p in out.cpkts if p is not None} == {cm.CLEAR}
    for msg_cap, byte_cap in ((7, 1 << 30), (1 << 20, 300), (0, 0)):
        cut = cm.crypt(b.conns, b.cands, b.pkts, data.dpkts, b.words, b.n_words, KEYS, 8, msg_cap, byte_cap)
        want = dm.planted_model(msg_cap, byte_cap)
        assert (cut.msgs, cut.payload, cut.n_msgs, cut.n_bytes) == (want.msgs, want.payload, want.n_msgs, want.n_bytes)


def _unarmed(name):
    """(the data model, the decryption model) of a world of tests/_le_data_lattice.py; `sequence_under_caps`: under the caps of the data
    stage's own test."""
    import _le_data_lattice as dl
    from test_le_data_lattice_model import sequence_caps
    b = dl.product_list() if name == "product" else dl.sequence_world()
    caps = sequence_caps(dl.sequence_model()) if name == "sequence_under_caps" else (1 << 20, 1 << 30)
    data = dm.built_model(b, *caps) if name == "product" else dl.sequence_model(None, *caps)
    return data, cm.crypt(b.conns, b.cands, b.pkts, data.dpkts, b.words, b.n_words, KEYS, 8, *caps)


@pytest.mark.parametrize("name", ["sequence", "sequence_under_caps", "product"])
def test_no_connection_of_the_data_lattices_is_armed(name):
    """What tests/test_gpu_le_crypt.py's identity over these worlds rests on: their CONTROL members have two octets, no procedure PDU
    has, so no record carries a flag and the messages are the data stage's."""
    data, out = _unarmed(name)
    assert all(r.flags == 0 and r.key == 0xFF for r in out.crypt) and {p.state for p in out.cpkts if p is not None} == {cm.CLEAR}
    assert (out.n_msgs, out.n_bytes) == (data.n_msgs, data.n_bytes) and out.n_msgs > 2048
    assert (out.msgs, out.payload, out.ppkts) == (data.msgs, data.payload, data.dpkts)


@pytest.mark.parametrize("variant", sorted(cm.VARIANTS))
def test_every_wrong_model_is_told_from_the_right_one(world, variant):
    b, (data, out) = world
    rules = cm.Rules(**cm.VARIANTS[variant])
    wrong = cm.crypt(b.conns, b.cands, b.pkts, data.dpkts, b.words, b.n_words, KEYS, 8, 1 << 20, 1 << 30, rules)
    assert (wrong.crypt, wrong.cpkts) != (out.crypt, out.cpkts), variant
    if variant != "largest_key":                                    # (the same key at another index decrypts as well)
        assert wrong.payload != out.payload


def test_hand_made_lists_carry_what_was_planted():
    h = cm.Hand(256)
    k = h.link(cm.ltk(0))
    k.event([cm.P(2, dm.l2cap(4, b"clear")), cm.E])
    k.start()
    for n, m in enumerate((1, 15, 16, 17, 31, 32, 33, 247, 251)):
        k.event([cm.P(2, bytes(range(m))), cm.P(2, bytes(range(1, m + 1)))], mod=(0, 1, 31, 63)[n % 4])
    b = h.built()
    data, out = cm.built_model(b, [cm.ltk(1), cm.ltk(0)], window=2)
    assert out.crypt[0].flags == 31 and out.crypt[0].key == 1 and out.crypt[0].n_verified == 18 and out.crypt[0].n_failed == 0
    got = sorted((m.role, out.payload[m.byte_offset:m.byte_offset + m.bytes]) for m in out.msgs[1:])
    assert got == sorted((role, plain) for role, counter, plain in k.plain) and out.msgs[0].cid == 4
    assert sorted((p.counter, p.ordinal) for p in out.cpkts if p is not None and p.state == cm.VERIFIED) == sorted([(n, n) for n in range(9)] * 2)
