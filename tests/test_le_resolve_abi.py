"""The C ABI of LE address resolution without a GPU: the numpy dtypes against the structs of include/btbbx.h (sizes and offsets, read
from a C90 program compiled against the header), the constants, the rule words in the header, the exported names, the scratch size,
and -- on a machine without a device -- that the entries refuse bad arguments first, writing nothing, and then fail with an error
instead of computing anything on the host."""
import os
import re
import subprocess

import numpy as np
import pytest

import _le_resolve as rm
import libbtbb_amd as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"btbbx_le_addr": (bt.LE_ADDR_DTYPE, 40), "btbbx_le_irk": (bt.LE_IRK_DTYPE, 40), "btbbx_le_peer": (bt.LE_PEER_DTYPE, 16)}
CONSTANTS = {"BTBBX_LE_RESOLVE_MAX_IRKS": bt.LE_RESOLVE_MAX_IRKS, "BTBBX_LE_ADDR_PUBLIC": bt.LE_ADDR_PUBLIC,
             "BTBBX_LE_ADDR_NONRESOLVABLE": bt.LE_ADDR_NONRESOLVABLE, "BTBBX_LE_ADDR_RESOLVABLE": bt.LE_ADDR_RESOLVABLE,
             "BTBBX_LE_ADDR_RESERVED": bt.LE_ADDR_RESERVED, "BTBBX_LE_ADDR_STATIC": bt.LE_ADDR_STATIC,
             "BTBBX_LE_ADDR_ADVERTISER": bt.LE_ADDR_ADVERTISER, "BTBBX_LE_ADDR_SCANNER": bt.LE_ADDR_SCANNER,
             "BTBBX_LE_ADDR_INITIATOR": bt.LE_ADDR_INITIATOR, "BTBBX_LE_ADDR_TARGET": bt.LE_ADDR_TARGET, "BTBBX_LE_IRK_GIVEN": bt.LE_IRK_GIVEN,
             "BTBBX_LE_IRK_HARVESTED": bt.LE_IRK_HARVESTED, "BTBBX_LE_IRK_HAS_ADDR": bt.LE_IRK_HAS_ADDR, "BTBBX_LE_IRK_NULLKEY": bt.LE_IRK_NULLKEY}
NAMES = {"btbbx_le_resolve_scratch_bytes", "btbbx_le_resolve_device", "btbbx_le_resolve_adv_host", "btbbx_le_resolve_host"}
OFFSETS = {"btbbx_le_addr": dict(first_offset=0, last_offset=8, n_slots=16, first_rec=20, addr=24, random=30, kind=31, irk=32, roles=34, channels=35,
                                 reserved=36),
           "btbbx_le_irk": dict(key=0, id_addr=16, id_random=22, flags=23, conn=24, n_addrs=28, n_slots=32, role=36, reserved=37),
           "btbbx_le_peer": dict(init_addr=0, adv_addr=4, init_irk=8, adv_irk=10, irk=12)}


def test_dtypes_and_constants_match_the_header_which_compiles_as_c90(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <btbbx.h>", "int main(void) {"]
    for name, (dtype, _) in STRUCTS.items():
        lines.append('printf("%s %%lu\\n", (unsigned long)sizeof(%s));' % (name, name))
        for field in dtype.names:
            lines.append('printf("%s.%s %%lu\\n", (unsigned long)offsetof(%s, %s));' % (name, field, name, field))
    for c in CONSTANTS:
        lines.append('printf("%s %%lu\\n", (unsigned long)%s);' % (c, c))
    lines += ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c90", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for name, (dtype, size) in STRUCTS.items():
        assert int(got[name]) == dtype.itemsize == size
        for field in dtype.names:
            assert int(got["%s.%s" % (name, field)]) == dtype.fields[field][1] == OFFSETS[name][field], (name, field)
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1), flags=re.S)
        fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split(None, 1)[1].split(",")]
        assert [re.sub(r"(\[\d+\])+", "", f) for f in fields] == list(dtype.names), fields
    for c, value in CONSTANTS.items():
        assert int(got[c]) == value, c
    # the model's tuples carry the records' fields in the records' order, and its constants are the header's
    assert list(rm.Addr._fields) == list(bt.LE_ADDR_DTYPE.names)[:-1] and list(rm.Irk._fields) == list(bt.LE_IRK_DTYPE.names)[:-1]
    assert list(rm.Peer._fields) == list(bt.LE_PEER_DTYPE.names)
    assert (rm.PUBLIC, rm.NONRESOLVABLE, rm.RESOLVABLE, rm.RESERVED, rm.STATIC) == tuple(range(5))
    assert (rm.ADVERTISER, rm.SCANNER, rm.INITIATOR, rm.TARGET) == (1, 2, 4, 8) == (rm.GIVEN, rm.HARVESTED, rm.HAS_ADDR, rm.NULLKEY)
    assert (rm.MAX_IRKS, rm.NONE, rm.NO_IRK) == (bt.LE_RESOLVE_MAX_IRKS, bt.LE_NO_ADDR, bt.LE_NO_IRK) == (4096, 0xFFFFFFFF, 0xFFFF)


def test_the_rules_and_the_limits_stand_in_the_header():
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    section = text[text.index("LE address resolution: IRKs from SMP"):text.index("btbbx_le_resolve_host(")]
    for n, word in enumerate(("KIND", "SLOTS", "DISTINCT LIST", "IRK TABLE", "RESOLVE", "ADDRESS RECORDS", "IRK RECORDS", "PEERS"), 1):
        assert re.search(r"\b%d\. %s" % (n, word), section), word
    for word in ("LIMITS", "2^-24", "256 of 2^20", "ah of Core Vol 3 Part H 2.2.2", "key[j] = v[16 - j]", "0x08", "0x09", "NULLKEY 8", "WRITES",
                 "The count of launches, 32", "extended advertising", "smallest matching slot", "whatever addr_cap is", "44 words"):
        assert word in section, word
    assert text.index("btbbx_le_pair_host(") < text.index("LE address resolution: IRKs from SMP") < text.index("hop selection and CLK1-27 reversal")


def test_signatures_are_declared():
    for name in NAMES:
        assert name in bt.SIGNATURES and getattr(bt.lib(), name) is not None
    epoch, host = bt.SIGNATURES["btbbx_le_epoch_host"][1], bt.SIGNATURES["btbbx_le_resolve_host"][1]
    assert host[:21] == epoch[:21] and len(host) == 35 and bt.SIGNATURES["btbbx_le_resolve_host"][0] == bt.SIGNATURES["btbbx_le_epoch_host"][0]
    assert len(bt.SIGNATURES["btbbx_le_resolve_device"][1]) == 24 and len(bt.SIGNATURES["btbbx_le_resolve_scratch_bytes"][1]) == 3
    assert len(bt.SIGNATURES["btbbx_le_resolve_adv_host"][1]) == 18
    assert callable(bt.le_resolve) and callable(bt.le_identify) and callable(bt.le_crack_identify)
    assert "irks" in bt.le_resolve.__doc__ and "irks" in bt.le_identify.__doc__ and "None" in bt.le_crack_identify.__doc__


def test_the_four_names_are_exported_and_nothing_else_of_the_family():
    out = subprocess.run(["nm", "-D", "--defined-only", bt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {n for n in names if "le_resolve" in n} == NAMES
    header = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n


def test_scratch_size_is_monotone_and_aligned():
    lib = bt.lib()
    last = 0
    for adv in (0, 1, 2, 511, 512, 513, 4096, 65537, 1 << 20, (1 << 31) - 1):
        got = lib.btbbx_le_resolve_scratch_bytes(adv, 4, 8)
        assert got % 256 == 0 and got >= 120 * max(adv, 1) and got >= last
        last = got
    assert lib.btbbx_le_resolve_scratch_bytes(0, 0, 0) == lib.btbbx_le_resolve_scratch_bytes(0, 1, 1)
    small, large = lib.btbbx_le_resolve_scratch_bytes(64, 4, 1), lib.btbbx_le_resolve_scratch_bytes(64, 4, 4096)
    assert large - small >= 4095 * 44 * 4                           # 44 words of schedule per table slot
    assert lib.btbbx_le_resolve_scratch_bytes(64, 1 << 20, 8) > lib.btbbx_le_resolve_scratch_bytes(64, 4, 8)


def test_bad_arguments_are_refused_before_anything_else():
    lib = bt.lib()
    buf = np.zeros(1 << 16, np.uint64)
    p = buf.ctypes.data
    big = 1 << 18

    def run(adv=p, acnt=p, adv_cap=4, ccnt=p, conn_cap=2, seeds=p, msgs=p, mcnt=p, msg_cap=8, octets=p, byte_cap=64, given=p, n_given=1, slots=p,
            addrs=p, addr_cap=4, ncnt=p, irks=p, irk_cap=8, icnt=p, peers=p, scr=p, scr_bytes=big):
        return lib.btbbx_le_resolve_device(adv, acnt, adv_cap, ccnt, conn_cap, seeds, msgs, mcnt, msg_cap, octets, byte_cap, given, n_given, slots,
                                           addrs, addr_cap, ncnt, irks, irk_cap, icnt, peers, scr, scr_bytes, None)

    for kw in (dict(adv=None), dict(acnt=None), dict(ccnt=None), dict(seeds=None), dict(msgs=None), dict(mcnt=None), dict(octets=None),
               dict(given=None), dict(slots=None), dict(addrs=None), dict(ncnt=None), dict(irks=None), dict(icnt=None), dict(peers=None),
               dict(scr=None), dict(irk_cap=4097), dict(irk_cap=(1 << 32) - 1), dict(n_given=9), dict(irk_cap=0), dict(adv_cap=1 << 31),
               dict(adv=p + 4), dict(seeds=p + 4), dict(msgs=p + 4), dict(addrs=p + 4), dict(irks=p + 4), dict(peers=p + 4), dict(slots=p + 2),
               dict(acnt=p + 2), dict(ccnt=p + 2), dict(mcnt=p + 2), dict(ncnt=p + 2), dict(icnt=p + 2), dict(scr=p + 8),
               dict(scr_bytes=lib.btbbx_le_resolve_scratch_bytes(4, 2, 8) - 1)):
        assert run(**kw) == -3, kw
        assert b"btbbx_le_resolve_device" in lib.btbbx_last_error()

    def adv_host(adv_errors=0, given=p, n_given=1, adv=p, slots=p, addrs=p, irks=p, irk_cap=4):
        return lib.btbbx_le_resolve_adv_host(p, 64, 64, 1, 1000, p, adv_errors, given, n_given, adv, 4, slots, addrs, 4, None, irks, irk_cap, None)

    for kw in (dict(adv_errors=5), dict(given=None), dict(n_given=5), dict(adv=None), dict(slots=None), dict(addrs=None), dict(irks=None),
               dict(irk_cap=4097)):
        assert adv_host(**kw) == -3, kw
        assert b"btbbx_le_resolve_adv_host" in lib.btbbx_last_error()

    # the chain's wrapper: its own conditions, the follow wrapper's, then the null pointers
    def host(max_len=27, unit=1250, adv_errors=0, seeds=p, keys=p, n_keys=1, window=8, given=p, n_given=1, peers=p, irks=p, irk_cap=4, addrs=p):
        return lib.btbbx_le_resolve_host(p, 64, 64, 1, 1000, p, max_len, 2, p, 4, p, 8, None, unit, 200, 50, 1, adv_errors, p, p, seeds, keys, n_keys,
                                         window, 16, 256, given, n_given, peers, irks, irk_cap, None, addrs, 4, None)

    for kw in (dict(max_len=256), dict(unit=1), dict(adv_errors=5), dict(seeds=None), dict(keys=None), dict(n_keys=0), dict(given=None),
               dict(n_given=5), dict(peers=None), dict(irks=None), dict(irk_cap=4097), dict(addrs=None)):
        assert host(**kw) == -3, kw
        assert b"btbbx_le_resolve_host" in lib.btbbx_last_error()
    assert not buf.any()


def test_fails_loudly_without_gpu():
    """No CPU fallback: without a device the entries report an error, after the argument checks."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = bt.lib()
    buf = np.zeros(1 << 16, np.uint64)
    p = buf.ctypes.data
    for cap in (4, 0):                                              # (with the caps 0 everything but the two counts and the scratch may be null)
        q = p if cap else None
        rc = lib.btbbx_le_resolve_device(q, q, cap, q, cap, q, q, q, cap, q, 16 * cap, q, cap and 1, q, q, cap, p, q, cap, p, q, p, 1 << 18, None)
        assert rc < 0                                               # (and not one of this entry's own refusals:)
        assert b"HIP" in lib.btbbx_last_error() and b"btbbx_le_resolve_device" not in lib.btbbx_last_error()
    assert not buf.any()
    with pytest.raises(bt.BtbbError):
        bt.le_resolve(np.zeros(64, np.uint64), 1000, 2402, [bytes(16)])
    with pytest.raises(bt.BtbbError):
        bt.le_identify(np.zeros(64, np.uint64), 1000, 2404, [bytes(16)])
    with pytest.raises(bt.BtbbError):
        bt.le_crack_identify(np.zeros(64, np.uint64), 1000, 2404)
