"""The C ABI of LE following through connection parameter updates without a GPU: the numpy dtypes against the structs of
include/btbbx.h (sizes and offsets, read from a C90 program compiled against the header), the constants, the exported names, the
scratch size, and -- on a machine without a device -- that the entries refuse bad arguments first and then fail with an error
instead of computing anything on the host."""
import os
import re
import subprocess

import numpy as np
import pytest

import _le_span as ls
import libbtbb_amd as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"btbbx_le_span": bt.LE_SPAN_DTYPE, "btbbx_le_span_pkt": bt.LE_SPAN_PKT_DTYPE, "btbbx_le_span_rec": bt.LE_SPAN_REC_DTYPE}
CONSTANTS = {"BTBBX_LE_SPAN_CAPPED": bt.LE_SPAN_CAPPED, "BTBBX_LE_SPAN_REFUSED": bt.LE_SPAN_REFUSED, "BTBBX_LE_STATE_GAP": bt.LE_STATE_GAP}
NAMES = {"btbbx_le_span_scratch_bytes", "btbbx_le_span_device", "btbbx_le_span_host"}


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
    assert (bt.LE_SPAN_DTYPE.itemsize, bt.LE_SPAN_PKT_DTYPE.itemsize, bt.LE_SPAN_REC_DTYPE.itemsize) == (56, 16, 40)
    for name, value in CONSTANTS.items():
        assert int(got[name]) == value, name
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
    assert list(ls.Span._fields) == list(bt.LE_SPAN_DTYPE.names) and list(ls.SPkt._fields) == list(bt.LE_SPAN_PKT_DTYPE.names)[:-1]
    assert list(ls.Rec._fields) == list(bt.LE_SPAN_REC_DTYPE.names)[:-1]
    assert (ls.CAPPED, ls.REFUSED, ls.ST_GAP) == (32, 64, 3)
    # the three places that still said where following ends point to this stage now
    assert "the next step" not in text and text.count("btbbx_le_span_device") >= 3


def test_signatures_are_declared():
    for name in NAMES:
        assert name in bt.SIGNATURES and getattr(bt.lib(), name) is not None
    epoch, span = bt.SIGNATURES["btbbx_le_epoch_device"][1], bt.SIGNATURES["btbbx_le_span_device"][1]
    assert span[:16] == epoch[:16] and len(span) == 23 and span[-3:] == epoch[-3:]
    e_host, s_host = bt.SIGNATURES["btbbx_le_epoch_host"][1], bt.SIGNATURES["btbbx_le_span_host"][1]
    assert s_host[:21] == e_host[:21] and len(s_host) == 25
    assert len(bt.SIGNATURES["btbbx_le_span_scratch_bytes"][1]) == 3 and callable(bt.le_span)


def test_the_three_names_are_exported_and_nothing_else_of_the_family():
    out = subprocess.run(["nm", "-D", "--defined-only", bt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {n for n in names if "le_span" in n} == NAMES
    header = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n


def test_scratch_size_is_monotone_in_all_three_arguments():
    lib = bt.lib()
    for cands in (0, 1, 64, 1000, 4097, 1 << 20, (1 << 32) - 1):
        for conns in (0, 1, 64, 1000, 65537, 1 << 22):
            for ups in (0, 1, 4, 15, 16):
                got = lib.btbbx_le_span_scratch_bytes(cands, conns, ups)
                assert got % 256 == 0 and got >= lib.btbbx_le_epoch_scratch_bytes(cands, conns) + 16 * max(cands, 1) + (96 + 4 * (ups + 1)) * max(conns, 1)
                assert lib.btbbx_le_span_scratch_bytes(cands + 1 if cands < (1 << 32) - 1 else cands, conns, ups) >= got
                assert lib.btbbx_le_span_scratch_bytes(cands, conns + 1, ups) >= got
                assert ups == 16 or lib.btbbx_le_span_scratch_bytes(cands, conns, ups + 1) >= got
    sizes = [lib.btbbx_le_span_scratch_bytes(100, 1000, u) for u in range(17)]
    assert sizes == sorted(sizes) and len(set(sizes)) > 8


def test_max_updates_17_and_bad_arguments_are_refused_before_anything_else():
    lib = bt.lib()
    buf = np.zeros(1 << 16, np.uint64)
    p = buf.ctypes.data
    big = 1 << 18

    def span(words=p, unit=1250, ups=2, spans=p, spkts=p, recs=p, scr_bytes=big, n_streams=2, jitter=50, n_words=8):
        return lib.btbbx_le_span_device(words, n_words, 8, n_streams, p, p, p, 8, p, p, 4, p, p, p, unit, jitter, ups, spans, spkts, recs, p,
                                        scr_bytes, None)

    assert span(ups=17, words=None) == -3 and b"btbbx_le_span_device: max_updates must be 0..16" in lib.btbbx_last_error()
    for kw in (dict(words=None), dict(spans=None), dict(spkts=None), dict(recs=None), dict(unit=1), dict(jitter=625), dict(n_streams=0),
               dict(n_words=0), dict(spans=p + 4), dict(spkts=p + 4), dict(recs=p + 4), dict(words=p + 4),
               dict(scr_bytes=lib.btbbx_le_span_scratch_bytes(8, 4, 2) - 1)):
        assert span(**kw) == -3, kw
        assert b"btbbx_le_span_device" in lib.btbbx_last_error()
    for bad in (-1, 5):
        assert lib.btbbx_le_span_host(p, 64, 64, 1, 1000, p, 27, 2, p, 4, p, 8, None, 1250, 200, 50, 1, bad, p, p, p, 4, p, p, p) == -3
        assert b"btbbx_le_span_host: max_errors must be 0..4" in lib.btbbx_last_error()
    assert lib.btbbx_le_span_host(p, 64, 64, 1, 1000, p, 27, 2, p, 4, p, 8, None, 1250, 200, 50, 1, 0, p, p, p, 17, p, p, p) == -3
    assert b"btbbx_le_span_host: max_updates must be 0..16" in lib.btbbx_last_error()
    assert lib.btbbx_le_span_host(p, 64, 64, 1, 1000, p, 27, 2, p, 4, p, 8, None, 1250, 200, 50, 1, 0, p, p, p, 4, None, p, p) == -3
    assert b"btbbx_le_span_host: null pointer" in lib.btbbx_last_error()
    assert not buf.any()


def test_fails_loudly_without_gpu():
    """No CPU fallback: without a device the entries report an error, after the argument checks."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = bt.lib()
    buf = np.zeros(1 << 16, np.uint64)
    p = buf.ctypes.data
    assert lib.btbbx_le_span_device(p, 8, 8, 2, p, p, p, 8, p, p, 4, p, p, p, 1250, 50, 4, p, p, p, p, 1 << 18, None) < 0
    assert b"HIP" in lib.btbbx_last_error() and b"btbbx_le_span_device" not in lib.btbbx_last_error()
    assert not buf.any()
    with pytest.raises(bt.BtbbError):
        bt.le_span(np.zeros(64, np.uint64), 1000, 2404)
