"""The C ABI of LE decryption without a GPU: the numpy dtypes against the structs of include/btbbx.h (sizes and offsets, read from a C90
program compiled against the header), the constants, the exported names, the scratch size, and -- on a machine without a device --
that the entries refuse bad arguments first and then fail with an error instead of computing anything on the host."""
import os
import re
import subprocess

import numpy as np
import pytest

import _le_crypt as cm
import libbtbb_amd as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"btbbx_le_crypt": bt.LE_CRYPT_DTYPE, "btbbx_le_crypt_pkt": bt.LE_CRYPT_PKT_DTYPE}
CONSTANTS = {"BTBBX_LE_CRYPT_CLEAR": bt.LE_CRYPT_CLEAR, "BTBBX_LE_CRYPT_VERIFIED": bt.LE_CRYPT_VERIFIED, "BTBBX_LE_CRYPT_FAILED": bt.LE_CRYPT_FAILED,
             "BTBBX_LE_CRYPT_SKIPPED": bt.LE_CRYPT_SKIPPED, "BTBBX_LE_CRYPT_SHORT": bt.LE_CRYPT_SHORT, "BTBBX_LE_CRYPT_REQ": bt.LE_CRYPT_REQ,
             "BTBBX_LE_CRYPT_RSP": bt.LE_CRYPT_RSP, "BTBBX_LE_CRYPT_START": bt.LE_CRYPT_START, "BTBBX_LE_CRYPT_ARMED": bt.LE_CRYPT_ARMED,
             "BTBBX_LE_CRYPT_KEYED": bt.LE_CRYPT_KEYED}
NAMES = {"btbbx_le_crypt_scratch_bytes", "btbbx_le_crypt_device", "btbbx_le_crypt_host"}


def test_dtypes_and_constants_match_the_header(tmp_path):
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <btbbx.h>", "int main(void) {"]
    for name, dtype in STRUCTS.items():
        lines.append('printf("%s %%lu\\n", (unsigned long)sizeof(%s));' % (name, name))
        for field in dtype.names:
            lines.append('printf("%s.%s %%lu\\n", (unsigned long)offsetof(%s, %s));' % (name, field, name, field))
    for name in CONSTANTS:
        lines.append('printf("%s %%lu\\n", (unsigned long)%s);' % (name, name))
    lines += ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c90", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    for name, dtype in STRUCTS.items():
        assert int(got[name]) == dtype.itemsize, name
        for field in dtype.names:
            assert int(got["%s.%s" % (name, field)]) == dtype.fields[field][1], (name, field)
    assert (bt.LE_CRYPT_DTYPE.itemsize, bt.LE_CRYPT_PKT_DTYPE.itemsize) == (56, 16)
    for name, value in CONSTANTS.items():
        assert int(got[name]) == value, name
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for name, dtype in STRUCTS.items():
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1), flags=re.S)
        fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split(None, 1)[1].split(",")]
        assert [re.sub(r"\[\d+\]", "", f) for f in fields] == list(dtype.names), (name, fields)
    # the model's tuples carry the records' fields in the records' order, and its constants are the header's
    assert list(cm.Crypt._fields) == list(bt.LE_CRYPT_DTYPE.names)[:-1] and list(cm.CPkt._fields) == list(bt.LE_CRYPT_PKT_DTYPE.names)[:-1]
    assert (cm.CLEAR, cm.VERIFIED, cm.FAILED, cm.SKIPPED, cm.SHORT) == tuple(range(5))
    assert (cm.F_REQ, cm.F_RSP, cm.F_START, cm.F_ARMED, cm.F_KEYED) == (1, 2, 4, 8, 16)
    # the rules and the limits stand in the header
    section = text[text.index("LE decryption"):text.index("btbbx_le_crypt_host(")]
    for word in ("COUNTING members", "PROCEDURE PDUs", "SESSION KEY", "ENCRYPTED members", "TRIAL", "KEY.", "SKEW", "MESSAGES", "RECORDS",
                 "LIMITS", "LL_PAUSE_ENC", "not fed back", "max_len >= 31"):
        assert word in section, word


def test_signatures_are_declared():
    for name in NAMES:
        assert name in bt.SIGNATURES and getattr(bt.lib(), name) is not None
    data, crypt = bt.SIGNATURES["btbbx_le_data_device"][1], bt.SIGNATURES["btbbx_le_crypt_device"][1]
    assert crypt[:13] == data[:13] and len(crypt) == 29 and crypt[-9:] == data[-9:]
    d_host, c_host = bt.SIGNATURES["btbbx_le_data_host"][1], bt.SIGNATURES["btbbx_le_crypt_host"][1]
    assert c_host[:21] == d_host[:21] and c_host[-6:] == d_host[-6:] and len(c_host) == 33
    assert bt.SIGNATURES["btbbx_le_crypt_scratch_bytes"][1] == bt.SIGNATURES["btbbx_le_span_scratch_bytes"][1] and callable(bt.le_decrypt)
    assert "max_len >= 31" in bt.le_decrypt.__doc__


def test_the_three_names_are_exported_and_nothing_else_of_the_family():
    out = subprocess.run(["nm", "-D", "--defined-only", bt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {n for n in names if "le_crypt" in n} == NAMES
    header = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n


def test_scratch_size_is_monotone():
    lib = bt.lib()
    for cands in (0, 1, 64, 1000, 4097, 1 << 20, (1 << 32) - 1):
        for conns in (0, 1, 64, 1000, 65537):
            for keys in (1, 16, 64):
                got = lib.btbbx_le_crypt_scratch_bytes(cands, conns, keys)
                assert got % 256 == 0 and got >= 68 * max(cands, 1) + 180 * keys * max(conns, 1)
                assert got >= lib.btbbx_le_data_scratch_bytes(cands, conns)
                assert lib.btbbx_le_crypt_scratch_bytes(cands + 1 if cands < (1 << 32) - 1 else cands, conns, keys) >= got
                assert lib.btbbx_le_crypt_scratch_bytes(cands, conns + 1, keys) >= got
                assert lib.btbbx_le_crypt_scratch_bytes(cands, conns, keys + 1) >= got


def test_bad_arguments_are_refused_before_anything_else():
    lib = bt.lib()
    buf = np.zeros(1 << 16, np.uint64)
    p = buf.ctypes.data
    big = 1 << 18

    def run(words=p, phys=p, cands=p, cnt=p, conns=p, ccnt=p, tracks=p, pkts=p, in_dpkts=p, keys=p, n_keys=2, window=4, crypt=p, cpkts=p,
            ppkts=p, msgs=p, msg_cap=4, mcnt=p, octets=p, byte_cap=64, bcnt=p, scr=p, scr_bytes=big, n_streams=2, n_words=8, pitch=8):
        return lib.btbbx_le_crypt_device(words, n_words, pitch, n_streams, phys, cands, cnt, 8, conns, ccnt, 4, tracks, pkts, in_dpkts, keys,
                                         n_keys, window, crypt, cpkts, ppkts, msgs, msg_cap, mcnt, octets, byte_cap, bcnt, scr, scr_bytes, None)

    for kw in (dict(words=None), dict(phys=None), dict(cands=None), dict(cnt=None), dict(conns=None), dict(ccnt=None), dict(tracks=None),
               dict(pkts=None), dict(in_dpkts=None), dict(keys=None), dict(crypt=None), dict(cpkts=None), dict(ppkts=None), dict(msgs=None),
               dict(mcnt=None), dict(octets=None), dict(bcnt=None), dict(scr=None), dict(n_keys=0), dict(n_keys=65), dict(window=0),
               dict(window=33), dict(n_streams=0), dict(n_words=0), dict(n_words=(1 << 42) + 1, pitch=1 << 43), dict(pitch=7),
               dict(words=p + 4), dict(phys=p + 1), dict(cands=p + 4), dict(conns=p + 4), dict(tracks=p + 4), dict(pkts=p + 4),
               dict(in_dpkts=p + 2), dict(crypt=p + 4), dict(cpkts=p + 8), dict(ppkts=p + 2), dict(msgs=p + 4), dict(octets=p + 4),
               dict(bcnt=p + 4), dict(mcnt=p + 2), dict(cnt=p + 2), dict(ccnt=p + 2), dict(scr=p + 8),
               dict(scr_bytes=lib.btbbx_le_crypt_scratch_bytes(8, 4, 2) - 1)):
        assert run(**kw) == -3, kw
        assert b"btbbx_le_crypt_device" in lib.btbbx_last_error()

    # the host wrapper: its own conditions, the data wrapper's, then the null pointers
    def host(max_len=31, unit=1250, data=p, keys=p, n_keys=2, window=8, crypt=p, msgs=p, msg_cap=4, octets=p, byte_cap=64):
        return lib.btbbx_le_crypt_host(p, 64, 64, 1, 1000, p, max_len, 2, p, 4, p, 8, None, unit, 200, 50, 1, p, p, data, p, keys, n_keys, window,
                                       crypt, p, p, msgs, msg_cap, None, octets, byte_cap, None)

    for kw in (dict(max_len=256), dict(unit=1), dict(data=None), dict(keys=None), dict(n_keys=0), dict(n_keys=65), dict(window=0),
               dict(window=33), dict(crypt=None), dict(msgs=None), dict(octets=None)):
        assert host(**kw) == -3, kw
        assert b"btbbx_le_crypt_host" in lib.btbbx_last_error()
    assert not buf.any()


def test_fails_loudly_without_gpu():
    """No CPU fallback: without a device the entries report an error, after the argument checks."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = bt.lib()
    buf = np.zeros(1 << 16, np.uint64)
    p = buf.ctypes.data
    assert lib.btbbx_le_crypt_device(p, 8, 8, 2, p, p, p, 8, p, p, 4, p, p, p, p, 2, 4, p, p, p, p, 4, p, p, 64, p, p, 1 << 18, None) < 0
    assert b"HIP" in lib.btbbx_last_error() and b"btbbx_le_crypt_device" not in lib.btbbx_last_error()
    assert not buf.any()
    with pytest.raises(bt.BtbbError):
        bt.le_decrypt(np.zeros(64, np.uint64), 1000, 2404, [bytes(16)])
