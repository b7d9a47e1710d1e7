"""The model of LE legacy pairing key recovery (tests/_le_pair.py) without a GPU: c1 and s1 against the Core Specification's own
examples and the local openssl (tests/golden/le_pair_core_spec_samples.json), the vectorised AES of the search against the scalar
one, a planted exchange recovered -- TK, STK, key sizes 7 and 16 --, and every deliberately wrong model told from the right one."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import _le_crypt as cm
import _le_data as dm
import _le_pair as pm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "le_pair_core_spec_samples.json")


@pytest.fixture(scope="module")
def spec():
    return json.load(open(GOLDEN))


def test_the_as_received_arrays_are_the_printed_values_reversed(spec):
    msb, rx = spec["msb_first"], spec["as_received"]
    rev = lambda s: list(bytes.fromhex(s)[::-1])                                 # noqa: E731
    assert rx["random"] == rev(msb["random"]) and rx["init_a"] == rev(msb["init_a"]) and rx["adv_a"] == rev(msb["adv_a"])
    p1 = bytes([rx["iat"], rx["rat"]] + rx["preq"] + rx["pres"])
    p2 = bytes(rx["adv_a"] + rx["init_a"] + [0, 0, 0, 0])
    assert p1[::-1].hex().upper() == msb["p1"] and p2[::-1].hex().upper() == msb["p2"]
    assert (p1, p2) == pm._arrays(rx["preq"], rx["pres"], rx["iat"], rx["rat"], rx["init_a"], rx["adv_a"])
    assert bytes(rx["mrand_0_7"] + rx["srand_0_7"])[::-1].hex().upper() == msb["r_prime"]
    for name in ("tk_0", "tk_123456"):
        assert spec[name]["confirm_as_received"] == rev(spec[name]["confirm"])
    assert pm.key(0).hex() == spec["tk_0"]["key"] and pm.key(123456).hex().upper() == spec["tk_123456"]["key"]


@pytest.mark.parametrize("name, tk", [("tk_0", 0), ("tk_123456", 123456)])
def test_c1_and_s1_against_the_specification(spec, name, tk):
    rx, want = spec["as_received"], spec[name]
    got = pm.c1(tk, bytes(rx["random"]), rx["preq"], rx["pres"], rx["iat"], rx["rat"], rx["init_a"], rx["adv_a"])
    assert list(got) == want["confirm_as_received"]
    mrand, srand = bytes(rx["mrand_0_7"]) + bytes(8), bytes(rx["srand_0_7"]) + bytes(8)
    assert pm.s1(tk, mrand, srand).hex() == want["stk"]
    # octets 8..15 of the Random values have no part in the STK
    assert pm.s1(tk, mrand[:8] + b"\xff" * 8, srand[:8] + b"\x55" * 8).hex() == want["stk"]


@pytest.mark.parametrize("name", ["tk_0", "tk_123456"])
def test_the_same_through_openssl(spec, name):
    exe = shutil.which("openssl")
    if exe is None:
        pytest.skip("no openssl binary on this machine")
    msb, want = spec["msb_first"], spec[name]
    ecb = lambda block: subprocess.run([exe, "enc", "-aes-128-ecb", "-nopad", "-K", want["key"]], input=block, capture_output=True,   # noqa: E731
                                       check=True).stdout
    xor = lambda x, y: bytes(p ^ q for p, q in zip(x, y))                        # noqa: E731
    r, p1, p2 = (bytes.fromhex(msb[k]) for k in ("random", "p1", "p2"))
    assert ecb(xor(ecb(xor(r, p1)), p2)).hex() == want["confirm"]
    assert ecb(bytes.fromhex(msb["r_prime"])).hex() == want["stk"]


def test_the_vectorised_aes_is_the_scalar_one():
    rng = np.random.default_rng(31)
    tks = [0, 1, 255, 256, 65535, 65536, 123456, 999999] + rng.integers(0, 1000000, 24).tolist()
    for rules in (pm.MODEL, pm.Rules(tk_in_front=True)):
        keys = pm.keys_of(tks, rules)
        assert [bytes(k) for k in keys] == [pm.key(t, rules) for t in tks]
        rk = pm.schedules(keys)
        one = rng.integers(0, 256, 16, dtype=np.uint8)
        many = rng.integers(0, 256, (len(tks), 16), dtype=np.uint8)
        assert [bytes(o) for o in pm.aes_many(rk, one)] == [cm.aes(bytes(k), bytes(one)) for k in keys]
        assert [bytes(o) for o in pm.aes_many(rk, many)] == [cm.aes(bytes(k), bytes(b)) for k, b in zip(keys, many)]
    full = rng.integers(0, 256, (16, 16), dtype=np.uint8)                       # and with keys that are not mostly zero
    assert [bytes(o) for o in pm.aes_many(pm.schedules(full), one)] == [cm.aes(bytes(k), bytes(one)) for k in full]


# ---- a planted exchange ---------------------------------------------------------------------------------------------------------------
def _planted(tk, ks=(16, 16), rules=pm.MODEL, shuffle=None, tk_limit=4096, **kw):
    """One connection that pairs under tk, its messages between another connection's -> (Out, mrand, srand, plant)."""
    seed = pm.seed_of(1)
    messages, mrand, srand = pm.exchange(tk, seed, n=1, ks=ks, **kw)
    if shuffle:
        messages = [messages[i] for i in shuffle]
    p = pm.Plant()
    p.add(1, dm.CENTRAL, b"\x0bnot SMP", cid=4)
    for role, body in messages:
        p.add(0, role, body)
        p.add(1, role, body if len(body) == 7 else body[:1] + pm.octets(50 + role, 16))   # the other's: random Confirm and Random values
    out = pm.pair(2, [seed, pm.seed_of(4)], p.msgs, bytes(p.payload), len(p.payload), tk_limit, 4, rules)
    return out, mrand, srand, p


@pytest.mark.parametrize("tk, ks", [(0, (16, 16)), (1234, (16, 16)), (4095, (7, 16)), (77, (16, 7)), (3, (12, 9))])
def test_a_planted_exchange_is_recovered(tk, ks):
    out, mrand, srand, p = _planted(tk, ks)
    got, other = out.pairs
    assert (got.tk, got.method, got.key_size, got.key) == (tk, pm.LEGACY, min(ks), 0)
    assert got.flags == 0xFF and got.keys == pm.K_STK
    assert [got.preq, got.prsp, got.mconf, got.sconf, got.mrand, got.srand] == [1, 3, 5, 7, 9, 11]
    whole = cm.aes(pm.key(tk), (mrand[:8] + srand[:8])[::-1])
    assert got.stk == bytes(16 - min(ks)) + whole[16 - min(ks):] and any(got.stk)
    assert out.n_keys == 1 and out.keys == got.stk + bytes(48)
    # the other connection: the same shapes, no key
    assert other.flags == 0x3F | pm.F_ARMED and other.tk == pm.NONE and other.key == 0xFF and other.stk == bytes(16)


def test_the_limit_is_exclusive():
    assert _planted(100, tk_limit=101)[0].pairs[0].tk == 100
    assert _planted(100, tk_limit=100)[0].pairs[0].tk == pm.NONE
    none = _planted(0, tk_limit=0)[0].pairs[0]
    assert (none.flags, none.method, none.tk) == (0x3F, pm.LEGACY, pm.NONE)


def test_both_checks_must_hold_under_one_tk():
    out = _planted(5, tk_peripheral=6)[0]
    assert out.pairs[0].flags == 0x3F | pm.F_ARMED and out.n_keys == 0 and out.keys == bytes(64)


def test_methods():
    sc = dict(preq=bytes([1, 4, 0, 0x0D, 16, 7, 7]), pres=bytes([2, 0, 0, 0x09, 16, 7, 7]))
    oob = dict(preq=bytes([1, 4, 1, 0x05, 16, 7, 7]), pres=bytes([2, 0, 1, 0x05, 16, 7, 7]))
    half = dict(preq=bytes([1, 4, 1, 0x0D, 16, 7, 7]), pres=bytes([2, 0, 0, 0x05, 16, 7, 7]))    # one side only: LEGACY
    assert _planted(9, **sc)[0].pairs[0][8:12] == (pm.NONE, pm.SECURE, 0x3F, 0)
    assert _planted(9, **oob)[0].pairs[0][8:12] == (pm.NONE, pm.OOB, 0x3F, 0)
    assert _planted(9, **half)[0].pairs[0][8:11] == (9, pm.LEGACY, 0xFF)
    assert _planted(9, ks=(6, 16))[0].pairs[0][8:13] == (pm.NONE, pm.INVALID, 0x3F, 0, 6)
    assert _planted(9, ks=(17, 17))[0].pairs[0][8:13] == (pm.NONE, pm.INVALID, 0x3F, 0, 17)


# ---- wrong models ----------------------------------------------------------------------------------------------------------------------
def test_every_wrong_model_is_told_from_the_right_one():
    """Each variant fails to recover what the right rules planted, or recovers another key."""
    right, mrand, srand, _ = _planted(1234, ks=(16, 10))
    assert right.pairs[0].tk == 1234
    told = {}
    for name, kw in pm.VARIANTS.items():
        rules = pm.Rules(**kw)
        if name == "prsp_anywhere":                                 # the Pairing Response in front of the Pairing Request
            order = [1, 0, 2, 3, 4, 5]
            want, got = _planted(1234, shuffle=order)[0], _planted(1234, shuffle=order, rules=rules)[0]
            assert want.pairs[0].flags == pm.F_PREQ and want.pairs[0].method == pm.NONE_M
        else:
            want, got = right, _planted(1234, ks=(16, 10), rules=rules)[0]
        told[name] = got.pairs[0] != want.pairs[0]
        assert told[name], name
        if name in ("s1_swapped", "stk_whole", "stk_cut_at_the_end"):            # the TK is found, the STK is another
            assert got.pairs[0].tk == 1234 and got.pairs[0].stk != want.pairs[0].stk
        elif name != "prsp_anywhere":
            assert got.pairs[0].tk == pm.NONE
    assert len(told) == 10
    # the types matter only where they differ, the variant is told because seed_of(1) has iat != rat
    assert pm.seed_of(1).tx_add != pm.seed_of(1).rx_add
