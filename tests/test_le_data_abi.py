"""The C ABI of LE data extraction without a GPU: the numpy dtypes against the structs of include/btbbx.h (sizes and offsets, read from
a C90 program compiled against the header), the constants, the exported names, the scratch size, and -- on a machine without a
device -- that the entries refuse bad arguments first and then fail with an error instead of computing anything on the host."""
import os
import re
import subprocess

import numpy as np
import pytest

import _le_data as dm
import libbtbb_amd as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"btbbx_le_data": bt.LE_DATA_DTYPE, "btbbx_le_data_pkt": bt.LE_DATA_PKT_DTYPE, "btbbx_le_msg": bt.LE_MSG_DTYPE}
CONSTANTS = {"BTBBX_LE_DATA_START": bt.LE_DATA_START, "BTBBX_LE_DATA_CONTINUATION": bt.LE_DATA_CONTINUATION,
             "BTBBX_LE_DATA_ORPHAN": bt.LE_DATA_ORPHAN, "BTBBX_LE_DATA_EMPTY": bt.LE_DATA_EMPTY, "BTBBX_LE_DATA_CONTROL": bt.LE_DATA_CONTROL,
             "BTBBX_LE_DATA_IGNORED": bt.LE_DATA_IGNORED, "BTBBX_LE_DATA_RETRANSMIT": bt.LE_DATA_RETRANSMIT,
             "BTBBX_LE_DATA_UNKNOWN": bt.LE_DATA_UNKNOWN, "BTBBX_LE_ROLE_CENTRAL": bt.LE_ROLE_CENTRAL,
             "BTBBX_LE_ROLE_PERIPHERAL": bt.LE_ROLE_PERIPHERAL, "BTBBX_LE_ROLE_UNKNOWN": bt.LE_ROLE_UNKNOWN,
             "BTBBX_LE_MSG_COMPLETE": bt.LE_MSG_COMPLETE, "BTBBX_LE_MSG_OVERRUN": bt.LE_MSG_OVERRUN, "BTBBX_LE_MSG_RUNT": bt.LE_MSG_RUNT,
             "BTBBX_LE_MSG_STORED": bt.LE_MSG_STORED}
NAMES = {"btbbx_le_data_scratch_bytes", "btbbx_le_data_device", "btbbx_le_data_host"}


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
    assert (bt.LE_DATA_DTYPE.itemsize, bt.LE_DATA_PKT_DTYPE.itemsize, bt.LE_MSG_DTYPE.itemsize) == (48, 12, 32)
    for name, value in CONSTANTS.items():
        assert int(got[name]) == value, name
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for name, dtype in STRUCTS.items():
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1), flags=re.S)
        fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split(None, 1)[1].split(",")]
        assert [re.sub(r"\[\d+\]", "", f) for f in fields] == list(dtype.names), (name, fields)
    # the model's tuples carry the records' fields in the records' order, and its constants are the header's
    assert list(dm.Data._fields) == list(bt.LE_DATA_DTYPE.names) and list(dm.DPkt._fields) == list(bt.LE_DATA_PKT_DTYPE.names)[:-1]
    assert list(dm.Msg._fields) == list(bt.LE_MSG_DTYPE.names)[:-1]
    assert (dm.START, dm.CONTINUATION, dm.ORPHAN, dm.EMPTY, dm.CONTROL, dm.IGNORED, dm.RETRANSMIT, dm.UNKNOWN) == tuple(range(8))
    assert (dm.COMPLETE, dm.OVERRUN, dm.RUNT, dm.STORED) == (1, 2, 4, 8)
    # the rules and the limits stand in the header
    section = text[text.index("LE data extraction"):text.index("btbbx_le_data_host(")]
    for word in ("HEADER", "HEAD events", "ROLE", "NEW / RETRANSMIT", "MESSAGES", "ORDER and BYTES", "RECORDS", "LIMITS", "not TIMED",
                 "split over fragments"):
        assert word in section, word


def test_signatures_are_declared():
    for name in NAMES:
        assert name in bt.SIGNATURES and getattr(bt.lib(), name) is not None
    epoch, data = bt.SIGNATURES["btbbx_le_epoch_device"][1], bt.SIGNATURES["btbbx_le_data_device"][1]
    assert data[:13] == epoch[:13] and len(data) == 24 and data[-3:] == epoch[-3:]
    t_host, d_host = bt.SIGNATURES["btbbx_le_track_host"][1], bt.SIGNATURES["btbbx_le_data_host"][1]
    assert d_host[:19] == t_host and len(d_host) == 27
    assert bt.SIGNATURES["btbbx_le_data_scratch_bytes"][1] == bt.SIGNATURES["btbbx_le_track_scratch_bytes"][1] and callable(bt.le_data)


def test_the_three_names_are_exported_and_nothing_else_of_the_family():
    out = subprocess.run(["nm", "-D", "--defined-only", bt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {n for n in names if "le_data" in n} == NAMES
    assert not any("follow" in n for n in NAMES)
    header = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n


def test_scratch_size_is_monotone():
    lib = bt.lib()
    for cands in (0, 1, 64, 1000, 4097, 1 << 20, (1 << 32) - 1):
        for conns in (0, 1, 64, 1000, 65537, 1 << 22):
            got = lib.btbbx_le_data_scratch_bytes(cands, conns)
            assert got % 256 == 0 and got >= 44 * max(cands, 1) + 96 * max(conns, 1)
            assert lib.btbbx_le_data_scratch_bytes(cands + 1 if cands < (1 << 32) - 1 else cands, conns) >= got
            assert lib.btbbx_le_data_scratch_bytes(cands, conns + 1) >= got


def test_bad_arguments_are_refused_before_anything_else():
    lib = bt.lib()
    buf = np.zeros(1 << 16, np.uint64)
    p = buf.ctypes.data
    big = 1 << 18

    def run(words=p, phys=p, cands=p, cnt=p, conns=p, ccnt=p, tracks=p, pkts=p, data=p, dpkts=p, msgs=p, msg_cap=4, mcnt=p, octets=p,
            byte_cap=64, bcnt=p, scr=p, scr_bytes=big, n_streams=2, n_words=8, pitch=8):
        return lib.btbbx_le_data_device(words, n_words, pitch, n_streams, phys, cands, cnt, 8, conns, ccnt, 4, tracks, pkts, data, dpkts, msgs,
                                        msg_cap, mcnt, octets, byte_cap, bcnt, scr, scr_bytes, None)

    for kw in (dict(words=None), dict(phys=None), dict(cands=None), dict(cnt=None), dict(conns=None), dict(ccnt=None), dict(tracks=None),
               dict(pkts=None), dict(data=None), dict(dpkts=None), dict(msgs=None), dict(mcnt=None), dict(octets=None), dict(bcnt=None),
               dict(scr=None), dict(n_streams=0), dict(n_words=0), dict(n_words=(1 << 42) + 1, pitch=1 << 43), dict(pitch=7),
               dict(words=p + 4), dict(phys=p + 1), dict(cands=p + 4), dict(conns=p + 4), dict(tracks=p + 4), dict(pkts=p + 4),
               dict(data=p + 4), dict(dpkts=p + 2), dict(msgs=p + 4), dict(octets=p + 4), dict(bcnt=p + 4), dict(mcnt=p + 2),
               dict(cnt=p + 2), dict(ccnt=p + 2), dict(scr=p + 8), dict(scr_bytes=lib.btbbx_le_data_scratch_bytes(8, 4) - 1)):
        assert run(**kw) == -3, kw
        assert b"btbbx_le_data_device" in lib.btbbx_last_error()
    # the host wrapper: the tracking wrapper's conditions, then its own null pointers
    def host(max_len=27, unit=1250, data=p, msgs=p, msg_cap=4, octets=p, byte_cap=64):
        return lib.btbbx_le_data_host(p, 64, 64, 1, 1000, p, max_len, 2, p, 4, p, 8, None, unit, 200, 50, 1, p, p, data, p, msgs, msg_cap, None,
                                      octets, byte_cap, None)

    for kw in (dict(max_len=256), dict(unit=1), dict(data=None), dict(msgs=None), dict(octets=None)):
        assert host(**kw) == -3, kw
        assert b"btbbx_le_data_host" in lib.btbbx_last_error()
    assert not buf.any()


def test_fails_loudly_without_gpu():
    """No CPU fallback: without a device the entries report an error, after the argument checks."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = bt.lib()
    buf = np.zeros(1 << 16, np.uint64)
    p = buf.ctypes.data
    assert lib.btbbx_le_data_device(p, 8, 8, 2, p, p, p, 8, p, p, 4, p, p, p, p, p, 4, p, p, 64, p, p, 1 << 18, None) < 0
    assert b"HIP" in lib.btbbx_last_error() and b"btbbx_le_data_device" not in lib.btbbx_last_error()
    assert not buf.any()
    with pytest.raises(bt.BtbbError):
        bt.le_data(np.zeros(64, np.uint64), 1000, 2404)
