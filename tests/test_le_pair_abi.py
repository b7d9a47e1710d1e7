"""The C ABI of LE legacy pairing key recovery without a GPU: the numpy dtype against the struct of include/btbbx.h (size and offsets,
read from a C90 program compiled against the header), the constants, the rule words in the header, the exported names, the scratch
size, and -- on a machine without a device -- that the entries refuse bad arguments first and then fail with an error instead of
computing anything on the host."""
import os
import re
import subprocess

import numpy as np
import pytest

import _le_pair as pm
import libbtbb_amd as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONSTANTS = {"BTBBX_LE_PAIR_NONE": bt.LE_PAIR_NONE, "BTBBX_LE_PAIR_LEGACY": bt.LE_PAIR_LEGACY, "BTBBX_LE_PAIR_SECURE": bt.LE_PAIR_SECURE,
             "BTBBX_LE_PAIR_OOB": bt.LE_PAIR_OOB, "BTBBX_LE_PAIR_INVALID": bt.LE_PAIR_INVALID, "BTBBX_LE_PAIR_PREQ": bt.LE_PAIR_PREQ,
             "BTBBX_LE_PAIR_PRSP": bt.LE_PAIR_PRSP, "BTBBX_LE_PAIR_MCONF": bt.LE_PAIR_MCONF, "BTBBX_LE_PAIR_SCONF": bt.LE_PAIR_SCONF,
             "BTBBX_LE_PAIR_MRAND": bt.LE_PAIR_MRAND, "BTBBX_LE_PAIR_SRAND": bt.LE_PAIR_SRAND, "BTBBX_LE_PAIR_ARMED": bt.LE_PAIR_ARMED,
             "BTBBX_LE_PAIR_CRACKED": bt.LE_PAIR_CRACKED, "BTBBX_LE_PAIR_KEY_STK": bt.LE_PAIR_KEY_STK,
             "BTBBX_LE_PAIR_KEY_LTK_CENTRAL": bt.LE_PAIR_KEY_LTK_CENTRAL, "BTBBX_LE_PAIR_KEY_LTK_PERIPHERAL": bt.LE_PAIR_KEY_LTK_PERIPHERAL}
NAMES = {"btbbx_le_pair_scratch_bytes", "btbbx_le_pair_device", "btbbx_le_pair_host"}


def test_dtype_and_constants_match_the_header(tmp_path):
    name, dtype = "btbbx_le_pair", bt.LE_PAIR_DTYPE
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <btbbx.h>", "int main(void) {"]
    lines.append('printf("%s %%lu\\n", (unsigned long)sizeof(%s));' % (name, name))
    for field in dtype.names:
        lines.append('printf("%s.%s %%lu\\n", (unsigned long)offsetof(%s, %s));' % (name, field, name, field))
    lines.append('printf("ltk.row %%lu\\n", (unsigned long)sizeof(((%s *)0)->ltk[0]));' % name)
    for c in CONSTANTS:
        lines.append('printf("%s %%lu\\n", (unsigned long)%s);' % (c, c))
    lines += ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c90", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got[name]) == dtype.itemsize == 88
    for field in dtype.names:
        assert int(got["%s.%s" % (name, field)]) == dtype.fields[field][1], field
    assert int(got["ltk.row"]) == 16 and dtype.fields["ltk"][0].shape == (2, 16) and dtype.fields["reserved"][0].shape == (7,)
    for c, value in CONSTANTS.items():
        assert int(got[c]) == value, c
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1), flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split(None, 1)[1].split(",")]
    assert [re.sub(r"(\[\d+\])+", "", f) for f in fields] == list(dtype.names), fields
    # the model's tuple carries the record's fields in the record's order, and its constants are the header's
    assert list(pm.Pair._fields) == list(dtype.names)[:-1]
    assert (pm.NONE_M, pm.LEGACY, pm.SECURE, pm.OOB, pm.INVALID) == tuple(range(5))
    assert (pm.F_PREQ, pm.F_PRSP, pm.F_MCONF, pm.F_SCONF, pm.F_MRAND, pm.F_SRAND, pm.F_ARMED, pm.F_CRACKED) == tuple(1 << j for j in range(8))
    assert (pm.K_STK, pm.K_LTK_CENTRAL, pm.K_LTK_PERIPHERAL) == (1, 2, 4)
    assert (bt.LE_PAIR_MAX_TK, bt.LE_PAIR_MAX_KEYS) == (1000000, 64)


def test_the_rules_and_the_limits_stand_in_the_header():
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    section = text[text.index("LE legacy pairing key recovery"):text.index("btbbx_le_pair_host(")]
    for n, word in enumerate(("SMP MESSAGE", "PROCEDURE", "METHOD", "CHECKS", "SEARCH", "STK", "KEY TABLE", "DISTRIBUTED KEYS", "RECORDS"), 1):
        assert re.search(r"\b%d\. %s" % (n, word), section), word
    for word in ("LIMITS", "only the first pairing", "never ARMED", "named, not broken", "EDIV / Rand, IRK and CSRK", "do not count",
                 "block[j] = x[15 - j]", "BE32(tk)", "0x0006", "n_keys = key_cap", "WRITES", "The count of launches, 12"):
        assert word in section, word
    assert text.index("btbbx_le_crypt_host(") < text.index("LE legacy pairing key recovery") < text.index("hop selection and CLK1-27 reversal")


def test_signatures_are_declared():
    for name in NAMES:
        assert name in bt.SIGNATURES and getattr(bt.lib(), name) is not None
    epoch, host = bt.SIGNATURES["btbbx_le_epoch_host"][1], bt.SIGNATURES["btbbx_le_pair_host"][1]
    assert host[:21] == epoch[:21] and len(host) == 28 and bt.SIGNATURES["btbbx_le_pair_host"][0] == bt.SIGNATURES["btbbx_le_epoch_host"][0]
    assert len(bt.SIGNATURES["btbbx_le_pair_device"][1]) == 16 and len(bt.SIGNATURES["btbbx_le_pair_scratch_bytes"][1]) == 1
    assert callable(bt.le_pair) and callable(bt.le_crack) and "tk_limit" in bt.le_pair.__doc__ and "None" in bt.le_crack.__doc__


def test_the_three_names_are_exported_and_nothing_else_of_the_family():
    out = subprocess.run(["nm", "-D", "--defined-only", bt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {n for n in names if "le_pair" in n} == NAMES
    assert not any("le_crypt" in n for n in NAMES)
    header = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n


def test_scratch_size_is_monotone():
    lib = bt.lib()
    last = 0
    for conns in (0, 1, 2, 64, 65, 1000, 4096, 65537, 1 << 20, (1 << 32) - 1):
        got = lib.btbbx_le_pair_scratch_bytes(conns)
        assert got % 256 == 0 and got >= 1024 + 148 * max(conns, 1) and got >= last
        last = got
    assert lib.btbbx_le_pair_scratch_bytes(0) == lib.btbbx_le_pair_scratch_bytes(1)


def test_bad_arguments_are_refused_before_anything_else():
    lib = bt.lib()
    buf = np.zeros(1 << 16, np.uint64)
    p = buf.ctypes.data
    big = 1 << 18

    def run(ccnt=p, conn_cap=4, seeds=p, msgs=p, mcnt=p, msg_cap=8, octets=p, byte_cap=64, tk_limit=1000, pairs=p, keys=p, key_cap=4, kcnt=p,
            scr=p, scr_bytes=big):
        return lib.btbbx_le_pair_device(ccnt, conn_cap, seeds, msgs, mcnt, msg_cap, octets, byte_cap, tk_limit, pairs, keys, key_cap, kcnt, scr,
                                        scr_bytes, None)

    for kw in (dict(ccnt=None), dict(seeds=None), dict(msgs=None), dict(mcnt=None), dict(octets=None), dict(pairs=None), dict(keys=None),
               dict(kcnt=None), dict(scr=None), dict(tk_limit=1000001), dict(tk_limit=(1 << 32) - 1), dict(key_cap=65), dict(seeds=p + 4),
               dict(msgs=p + 4), dict(pairs=p + 4), dict(ccnt=p + 2), dict(mcnt=p + 2), dict(kcnt=p + 2), dict(scr=p + 8),
               dict(scr_bytes=lib.btbbx_le_pair_scratch_bytes(4) - 1), dict(conn_cap=0, scr=None), dict(conn_cap=0, pairs=None)):
        assert run(**kw) == -3, kw
        assert b"btbbx_le_pair_device" in lib.btbbx_last_error()

    # the host wrapper: its own conditions, the follow wrapper's, then the null pointers
    def host(max_len=27, unit=1250, adv_errors=0, seeds=p, tk_limit=1000, pairs=p, keys=p, key_cap=4):
        return lib.btbbx_le_pair_host(p, 64, 64, 1, 1000, p, max_len, 2, p, 4, p, 8, None, unit, 200, 50, 1, adv_errors, p, p, seeds, 16, 256,
                                      tk_limit, pairs, keys, key_cap, None)

    for kw in (dict(max_len=256), dict(unit=1), dict(adv_errors=5), dict(seeds=None), dict(tk_limit=1000001), dict(key_cap=65), dict(pairs=None),
               dict(keys=None)):
        assert host(**kw) == -3, kw
        assert b"btbbx_le_pair_host" in lib.btbbx_last_error()
    assert not buf.any()


def test_fails_loudly_without_gpu():
    """No CPU fallback: without a device the entries report an error, after the argument checks."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = bt.lib()
    buf = np.zeros(1 << 16, np.uint64)
    p = buf.ctypes.data
    for msg_cap, byte_cap, key_cap in ((8, 64, 4), (0, 0, 0)):      # (the three that may be null with their caps 0)
        rc = lib.btbbx_le_pair_device(p, 4, p, p if msg_cap else None, p, msg_cap, p if byte_cap else None, byte_cap, 1000, p,
                                      p if key_cap else None, key_cap, p, p, 1 << 18, None)
        assert rc < 0                                               # (and not one of this entry's own refusals:)
        assert b"HIP" in lib.btbbx_last_error() and b"btbbx_le_pair_device" not in lib.btbbx_last_error()
    assert not buf.any()
    with pytest.raises(bt.BtbbError):
        bt.le_pair(np.zeros(64, np.uint64), 1000, 2404)
    with pytest.raises(bt.BtbbError):
        bt.le_crack(np.zeros(64, np.uint64), 1000, 2404)
