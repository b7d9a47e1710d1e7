"""The C ABI of the LE Coded PHY scan without a GPU, as tests/test_le_resolve_abi.py: the numpy dtype against the struct of
include/btbbx.h (size and offsets, read from a C90 program compiled against the header), the constants, the rule words in the
header, the exported names, and -- on a machine without a device -- that the entries refuse bad arguments first, writing nothing,
and then fail with an error instead of computing anything on the host.  The decoder keeps its decisions in LDS and takes no
scratch (btbbx_le_coded_scratch_bytes is 0 for every cap), so there is no scratch that could be too short to refuse."""
import os
import re
import subprocess

import numpy as np
import pytest

import _le_coded as m
import libbtbb_amd as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONSTANTS = {"BTBBX_LE_CODED_PATTERN": bt.LE_CODED_PATTERN, "BTBBX_LE_CODED_MAX_ERRORS": bt.LE_CODED_MAX_ERRORS,
             "BTBBX_LE_CODED_LAG": bt.LE_CODED_LAG}
NAMES = {"btbbx_le_coded_scan_device", "btbbx_le_coded_scratch_bytes", "btbbx_le_coded_decode_hits_device", "btbbx_le_coded_scan_host"}
OFFSETS = dict(symbols=0, metric2=4, metric1=8, ci=10, s=11, header_moved=12, reserved=13)


def test_dtype_and_constants_match_the_header_which_compiles_as_c90(tmp_path):
    name, dtype = "btbbx_le_coded_info", bt.LE_CODED_INFO_DTYPE
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <btbbx.h>", "int main(void) {",
             'printf("%s %%lu\\n", (unsigned long)sizeof(%s));' % (name, name)]
    for field in dtype.names:
        lines.append('printf("%s.%s %%lu\\n", (unsigned long)offsetof(%s, %s));' % (name, field, name, field))
    for c in CONSTANTS:
        lines.append('printf("%s %%lu\\n", (unsigned long)%s);' % (c, c))
    lines += ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c90", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got[name]) == dtype.itemsize == 16
    for field in dtype.names:
        assert int(got["%s.%s" % (name, field)]) == dtype.fields[field][1] == OFFSETS[field], field
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1), flags=re.S)
    fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split(None, 1)[1].split(",")]
    assert [re.sub(r"(\[\d+\])+", "", f) for f in fields] == list(dtype.names), fields
    for c, value in CONSTANTS.items():
        assert int(got[c]) == value, c
    assert (m.PATTERN, m.MAX_ERRORS, m.LAG) == (bt.LE_CODED_PATTERN, bt.LE_CODED_MAX_ERRORS, bt.LE_CODED_LAG) == (336, 63, 24)
    assert list(m.INFO_FIELDS) == list(dtype.names)[:-1]


def test_the_rules_and_the_limits_stand_in_the_header():
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    section = text[text.index("LE Coded PHY scan: coded access address search"):text.index("btbbx_le_coded_scan_host(")]
    for n, word in enumerate(("MATCH", "TRELLIS", "BLOCK 1", "S", "LENGTH", "BODY", "RECORD", "WRITES"), 1):
        assert re.search(r"\b%d\. %s\b" % (n, word), section), word
    for word in ("LIMITS", "AIR FORMAT", "0 0 1 1 1 1 0 0", "a0 = b ^ b1 ^ b2 ^ b3", "a1 = b ^ b2 ^ b3", "0 0 1 1", "1 1 0 0", "376 + S * N", "17040",
                 "x = 0 on equal sums", "smallest state index on ties", "L is not revised", "o + symbols > 64 * n_words", "nothing is suppressed",
                 "104", "84 over 200", "unknown AA", "AuxPtr", "2M PHY", "soft decisions", "beyond 64", "returns 0 for every cap"):
        assert word in section, word
    assert text.index("btbbx_le_resolve_host(") < text.index("LE Coded PHY scan: coded access address search") < \
        text.index("hop selection and CLK1-27 reversal")


def test_signatures_are_declared():
    for name in NAMES:
        assert name in bt.SIGNATURES and getattr(bt.lib(), name) is not None
    assert bt.SIGNATURES["btbbx_le_coded_scan_device"] == bt.SIGNATURES["btbbx_le_scan_device"]
    one_m, coded = bt.SIGNATURES["btbbx_le_decode_hits_device"][1], bt.SIGNATURES["btbbx_le_coded_decode_hits_device"][1]
    assert coded[:9] == one_m[:9] and len(coded) == 13
    one_m, coded = bt.SIGNATURES["btbbx_le_scan_host"][1], bt.SIGNATURES["btbbx_le_coded_scan_host"][1]
    assert coded[:10] == one_m[:10] and len(coded) == 12 and bt.SIGNATURES["btbbx_le_coded_scan_host"][0] == bt.SIGNATURES["btbbx_le_scan_host"][0]
    assert callable(bt.le_coded_scan) and "LE_CODED_INFO_DTYPE" in bt.le_coded_scan.__doc__


def test_the_four_names_are_exported_and_nothing_else_of_the_family():
    out = subprocess.run(["nm", "-D", "--defined-only", bt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {n for n in names if "le_coded" in n} == NAMES
    header = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n
    assert {n for n in names if n.startswith("lell_")}              # (the lell_* entries are still there, and still abort)


def test_no_scratch_is_needed():
    lib = bt.lib()
    for cap in (0, 1, 8, 65, 1 << 20, (1 << 32) - 1):
        assert lib.btbbx_le_coded_scratch_bytes(cap) == 0


def test_bad_arguments_are_refused_before_anything_else():
    lib = bt.lib()
    buf = np.zeros(1 << 12, np.uint64)
    p = buf.ctypes.data

    def scan(words=p, n_words=64, pitch=64, n_streams=1, search_bits=64 * 64 - 335, max_errors=16, hits=p, hit_cap=4, count=p):
        return lib.btbbx_le_coded_scan_device(words, n_words, pitch, n_streams, search_bits, bt.LE_ADV_AA, max_errors, hits, hit_cap, count, None)

    for kw in (dict(max_errors=64), dict(max_errors=-1), dict(search_bits=64 * 64 - 334), dict(n_words=5, search_bits=1), dict(n_streams=0),
               dict(n_streams=2, pitch=63), dict(words=None), dict(count=None), dict(hits=None), dict(words=p + 4), dict(hits=p + 8),
               dict(count=p + 2)):
        assert scan(**kw) == -3, kw
        assert b"btbbx_le_coded_scan_device" in lib.btbbx_last_error()

    def decode(words=p, hits=p, count=p, cap=4, phys=p, out=p, info=p, n_words=64):
        return lib.btbbx_le_coded_decode_hits_device(words, n_words, 64, hits, count, cap, phys, 0x555555, out, info, None, 0, None)

    for kw in (dict(words=None), dict(hits=None), dict(count=None), dict(phys=None), dict(out=None), dict(info=None), dict(words=p + 4),
               dict(hits=p + 4), dict(count=p + 2), dict(phys=p + 1), dict(out=p + 4), dict(info=p + 2), dict(n_words=(1 << 40) + 1)):
        assert decode(**kw) == -3, kw
        assert b"btbbx_le_coded_decode_hits_device" in lib.btbbx_last_error()

    def host(words=p, search_bits=64 * 64 - 335, phys=p, max_errors=16, pkts=p, info=p, cap=4):
        return lib.btbbx_le_coded_scan_host(words, 64, 64, 1, search_bits, phys, bt.LE_ADV_AA, 0x555555, max_errors, pkts, info, cap)

    for kw in (dict(max_errors=64), dict(search_bits=64 * 64 - 334), dict(words=None), dict(phys=None), dict(pkts=None), dict(info=None)):
        assert host(**kw) == -3, kw
        assert b"btbbx_le_coded_scan_host" in lib.btbbx_last_error()
    assert not buf.any()


def test_fails_loudly_without_gpu():
    """No CPU fallback: without a device the entries report an error, after the argument checks."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = bt.lib()
    buf = np.zeros(1 << 12, np.uint64)
    p = buf.ctypes.data
    for rc in (lib.btbbx_le_coded_scan_device(p, 64, 64, 1, 1000, bt.LE_ADV_AA, 16, p, 4, p, None),
               lib.btbbx_le_coded_decode_hits_device(p, 64, 64, p, p, 4, p, 0x555555, p, p, None, 0, None),
               lib.btbbx_le_coded_decode_hits_device(None, 64, 64, None, None, 0, None, 0x555555, None, None, None, 0, None),
               lib.btbbx_le_coded_scan_host(p, 64, 64, 1, 1000, p, bt.LE_ADV_AA, 0x555555, 16, p, p, 4)):
        assert rc < 0
        assert b"HIP" in lib.btbbx_last_error() and b"btbbx_le_coded" not in lib.btbbx_last_error()
    assert not buf.any()
    with pytest.raises(bt.BtbbError):
        bt.le_coded_scan(np.zeros(64, np.uint64), 1000, 2402)
