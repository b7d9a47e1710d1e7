"""The C ABI of LE following from CONNECT_IND without a GPU: the numpy dtypes against the structs of include/btbbx.h (sizes and
offsets, read from a C program compiled against the header), the constants, the scratch size, and -- on a machine without a
device -- that the entries refuse bad arguments first and then fail with an error instead of computing anything on the host."""
import os
import re
import subprocess

import numpy as np
import pytest

import _le_follow as lf
import libbtbb_amd as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"btbbx_le_seed": bt.LE_SEED_DTYPE, "btbbx_le_follow": bt.LE_FOLLOW_DTYPE, "btbbx_le_follow_pkt": bt.LE_FOLLOW_PKT_DTYPE}
CONSTANTS = {"BTBBX_LE_SEED_SEEDED": bt.LE_SEED_SEEDED, "BTBBX_LE_FOLLOW_SEEDED": bt.LE_FOLLOW_SEEDED,
             "BTBBX_LE_FOLLOW_COUNTED": bt.LE_FOLLOW_COUNTED, "BTBBX_LE_FOLLOW_STOPPED": bt.LE_FOLLOW_STOPPED,
             "BTBBX_LE_FOLLOW_TERMINATED": bt.LE_FOLLOW_TERMINATED, "BTBBX_LE_FOLLOW_ENCRYPTED": bt.LE_FOLLOW_ENCRYPTED,
             "BTBBX_LE_STATE_COUNTED": bt.LE_STATE_COUNTED, "BTBBX_LE_STATE_BEFORE": bt.LE_STATE_BEFORE,
             "BTBBX_LE_STATE_BEYOND": bt.LE_STATE_BEYOND, "BTBBX_LE_PDU_DATA": bt.LE_PDU_DATA, "BTBBX_LE_PDU_CONTROL": bt.LE_PDU_CONTROL,
             "BTBBX_LE_PDU_MAP_UPDATE": bt.LE_PDU_MAP_UPDATE, "BTBBX_LE_PDU_PARAM_UPDATE": bt.LE_PDU_PARAM_UPDATE,
             "BTBBX_LE_PDU_TERMINATE": bt.LE_PDU_TERMINATE, "BTBBX_LE_PDU_ENC_START": bt.LE_PDU_ENC_START,
             "BTBBX_LE_PDU_OPAQUE": bt.LE_PDU_OPAQUE}


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
    assert (bt.LE_SEED_DTYPE.itemsize, bt.LE_FOLLOW_DTYPE.itemsize, bt.LE_FOLLOW_PKT_DTYPE.itemsize) == (56, 48, 12)
    for name, value in CONSTANTS.items():
        assert int(got[name]) == value, name
    # every field of the header's structs has a dtype field of the same name (and, for an array, of its length)
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for name, dtype in STRUCTS.items():
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1), flags=re.S)
        fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split(None, 1)[1].split(",")]
        assert [re.sub(r"\[\d+\]", "", f) for f in fields] == list(dtype.names), (name, fields)
        for f in fields:
            m = re.match(r"(\w+)\[(\d+)\]", f)
            if m:
                assert dtype.fields[m.group(1)][0].shape == (int(m.group(2)),), f
    # the model's tuples carry the records' fields in the records' order
    assert list(lf.Seed._fields) == list(bt.LE_SEED_DTYPE.names)[:-1] and list(lf.Follow._fields) == list(bt.LE_FOLLOW_DTYPE.names)[:-1]
    assert list(lf.FPkt._fields) == list(bt.LE_FOLLOW_PKT_DTYPE.names)[:-1]
    assert (lf.SEEDED, lf.COUNTED, lf.STOPPED, lf.TERMINATED, lf.ENCRYPTED) == (1, 2, 4, 8, 16)
    assert (lf.DATA, lf.CONTROL, lf.MAP_UPDATE, lf.PARAM_UPDATE, lf.TERMINATE, lf.ENC_START, lf.OPAQUE) == tuple(range(7))


def test_signatures_are_declared():
    for name in ("btbbx_le_seed_device", "btbbx_le_epoch_scratch_bytes", "btbbx_le_epoch_device", "btbbx_le_epoch_host"):
        assert name in bt.SIGNATURES and getattr(bt.lib(), name) is not None
    assert len(bt.SIGNATURES["btbbx_le_seed_device"][1]) == 10 and len(bt.SIGNATURES["btbbx_le_epoch_device"][1]) == 21
    host = bt.SIGNATURES["btbbx_le_epoch_host"][1]
    assert host[:17] == bt.SIGNATURES["btbbx_le_track_host"][1][:17] and len(host) == 23
    assert callable(bt.le_follow)


def test_the_four_names_are_exported_and_nothing_else_of_the_family():
    out = subprocess.run(["nm", "-D", "--defined-only", bt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    family = {n for n in names if "le_follow" in n or "le_seed" in n or "le_epoch" in n}
    assert not any("follow" in n for n in family)          # (tests/test_follow_abi.py keeps that word for the BR/EDR stage's two names)
    assert family == {"btbbx_le_seed_device", "btbbx_le_epoch_scratch_bytes", "btbbx_le_epoch_device", "btbbx_le_epoch_host"}
    header = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for n in family:
        assert re.search(r"\b%s\s*\(" % n, header), n


def test_scratch_size_is_monotone():
    lib = bt.lib()
    for cands in (0, 1, 63, 64, 1000, 4097, 1 << 20, (1 << 32) - 1):
        for conns in (0, 1, 3, 64, 1000, 65537, 1 << 22):
            got = lib.btbbx_le_epoch_scratch_bytes(cands, conns)
            assert got % 256 == 0 and got >= 92 * max(cands, 1) + 64 * max(conns, 1)
            assert got <= 140 * max(cands, 1) + 64 * max(conns, 1) + 64 * 256                  # "about 130 per candidate and 64 per connection"
            assert lib.btbbx_le_epoch_scratch_bytes(cands + 1 if cands < (1 << 32) - 1 else cands, conns) >= got
            assert lib.btbbx_le_epoch_scratch_bytes(cands, conns + 1) >= got
    sizes = [lib.btbbx_le_epoch_scratch_bytes(n, 100) for n in range(0, 5000, 37)]
    assert sizes == sorted(sizes) and len(set(sizes)) > 100


def test_adv_errors_outside_0_4_is_refused_before_anything_else():
    lib = bt.lib()
    buf = np.zeros(4096, np.uint64)
    p = buf.ctypes.data
    for bad in (-1, 5):
        assert lib.btbbx_le_epoch_host(p, 64, 64, 1, 1000, p, 27, 2, p, 4, p, 8, None, 1250, 200, 50, 1, bad, p, p, p, p, p) == -3
        assert b"btbbx_le_epoch_host: max_errors must be 0..4" in lib.btbbx_last_error()
    assert not buf.any()


def test_fails_loudly_without_gpu():
    """No CPU fallback: without a device the entries report an error, after the argument checks."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = bt.lib()
    buf = np.zeros(1 << 16, np.uint64)
    p = buf.ctypes.data
    big = 1 << 18
    follow = lambda words=p, unit=1250: lib.btbbx_le_epoch_device(words, 8, 8, 2, p, p, p, 8, p, p, 4, p, p, p, unit, 50, p, p, p, big, None)  # noqa: E731
    assert follow(words=None) == -3                                                  # the argument check comes first
    assert b"btbbx_le_epoch_device: null pointer" in lib.btbbx_last_error()
    assert follow(unit=1) == -3 and b"btbbx_le_epoch_device" in lib.btbbx_last_error()
    assert follow() < 0
    assert b"HIP" in lib.btbbx_last_error() and b"btbbx_le_epoch_device" not in lib.btbbx_last_error()
    assert lib.btbbx_le_seed_device(p, p, 2, p, p, 4, p, 1250, None, None) == -3
    assert b"btbbx_le_seed_device: null pointer" in lib.btbbx_last_error()
    assert lib.btbbx_le_seed_device(p, p, 2, p, p, 4, p, 1250, p, None) < 0
    assert b"HIP" in lib.btbbx_last_error() and b"btbbx_le_seed_device" not in lib.btbbx_last_error()
    assert not buf.any()
    with pytest.raises(bt.BtbbError):
        bt.le_follow(np.zeros(64, np.uint64), 1000, 2404)
