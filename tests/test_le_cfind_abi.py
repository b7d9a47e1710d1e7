"""The C ABI of the promiscuous LE Coded connection discovery without a GPU, as tests/test_le_coded_abi.py: the numpy dtype against
the struct of include/btbbx.h (read from a C90 program compiled against the header), the rule words in the header, the exported
names, the scratch size, and -- on a machine without a device -- that the entries refuse bad arguments first, writing nothing, and
then fail with an error instead of computing anything on the host.  The entries are named le_cfind: tests/test_le_coded_abi.py pins
the exported names that contain le_coded to the coded scan's four."""
import os
import re
import subprocess

import numpy as np
import pytest

import libbtbb_amd as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"btbbx_le_cfind_scratch_bytes", "btbbx_le_cfind_scan_device", "btbbx_le_cfind_host"}
OFFSETS = dict(symbols=0, metric2=4, metric1=8, errors=10, ci=11, s=12, reserved=13)


def test_dtype_matches_the_header_which_compiles_as_c90(tmp_path):
    name, dtype = "btbbx_le_coded_cand_info", bt.LE_CODED_CAND_INFO_DTYPE
    lines = ["#include <stdio.h>", "#include <stddef.h>", "#include <btbbx.h>", "int main(void) {",
             'printf("%s %%lu\\n", (unsigned long)sizeof(%s));' % (name, name)]
    for field in dtype.names:
        lines.append('printf("%s.%s %%lu\\n", (unsigned long)offsetof(%s, %s));' % (name, field, name, field))
    lines += ["return 0; }"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c90", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got[name]) == dtype.itemsize == 16
    for field in dtype.names:
        assert int(got["%s.%s" % (name, field)]) == dtype.fields[field][1] == OFFSETS[field], field


def test_the_rules_and_the_limits_stand_in_the_header():
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    section = text[text.index("promiscuous LE Coded connection discovery: access address and CRCInit"):text.index("btbbx_le_cfind_host(")]
    words = ("CHANNEL", "RANGE", "BLOCK 1", "MATCH", "ADDRESS", "S", "HEADER", "FIT", "BODY", "CRCINIT", "RECORD", "WRITES")
    for n, word in enumerate(words, 1):
        assert re.search(r"\b%d\. %s\b" % (n, word), section), word
    flat = re.sub(r"[\s*]+", " ", section)                 # (the comment's line breaks and stars taken out)
    for word in ("LIMITS", "DECODED address", "lie 8 symbols apart", "header_moved must be 0", "o + 376 + S (8 (L + 5) + 3) <= 64 n_words",
                 "search_bits + 335 <= 64 n_words", "btbbx_le_discover_group_device", "parallel to THIS list only", "in no order",
                 "tracking coded candidates", "AUX_CONNECT_REQ", "soft decisions", "2M PHY", "lell_", "16 pre_cap"):
        assert word in flat, word
    coded = text[text.index("LE Coded PHY scan: coded access address search"):text.index("btbbx_le_coded_scan_host(")]
    assert "unknown AA" in coded and "promiscuous LE Coded connection discovery" in re.sub(r"[\s*]+", " ", coded)
    assert text.index("btbbx_le_coded_scan_host(") < text.index("promiscuous LE Coded connection discovery: access") < \
        text.index("hop selection and CLK1-27 reversal")


def test_signatures_are_declared():
    for name in NAMES:
        assert name in bt.SIGNATURES and getattr(bt.lib(), name) is not None
    scan, one_m = bt.SIGNATURES["btbbx_le_cfind_scan_device"][1], bt.SIGNATURES["btbbx_le_discover_scan_device"][1]
    assert scan[:7] == one_m[:7] and len(scan) == 16
    host, one_m = bt.SIGNATURES["btbbx_le_cfind_host"], bt.SIGNATURES["btbbx_le_discover_host"]
    assert host[0] == one_m[0] and host[1][:7] == one_m[1][:7] and host[1][8:] == one_m[1][7:] and len(host[1]) == 14
    assert callable(bt.le_coded_discover) and "LE_CAND_DTYPE" in bt.le_coded_discover.__doc__


def test_the_three_names_are_exported_and_nothing_else_of_the_family():
    out = subprocess.run(["nm", "-D", "--defined-only", bt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {n for n in names if "cfind" in n} == NAMES
    header = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n


def test_scratch_size_is_monotone_in_pre_cap():
    lib = bt.lib()
    sizes = [lib.btbbx_le_cfind_scratch_bytes(cap) for cap in (0, 1, 2, 63, 64, 65, 4096, 1 << 20, (1 << 32) - 16, (1 << 32) - 1)]
    assert sizes == sorted(sizes) and sizes[0] == 0 and sizes[1] == 16 and sizes[-1] == 16 * ((1 << 32) - 1)


def test_bad_arguments_are_refused_before_anything_else():
    lib = bt.lib()
    buf = np.zeros(1 << 12, np.uint64)
    p = buf.ctypes.data

    def scan(words=p, n_words=64, pitch=64, n_streams=1, search_bits=64 * 64 - 335, phys=p, max_len=27, max_errors=16, cands=p, info=p,
             cand_cap=4, count=p, pre_count=p, scratch=p, scratch_bytes=64):
        return lib.btbbx_le_cfind_scan_device(words, n_words, pitch, n_streams, search_bits, phys, max_len, max_errors, cands, info, cand_cap,
                                              count, pre_count, scratch, scratch_bytes, None)

    for kw in (dict(max_errors=64), dict(max_errors=-1), dict(max_len=256), dict(search_bits=64 * 64 - 334), dict(n_words=5, search_bits=1),
               dict(n_streams=0), dict(n_streams=2, pitch=63), dict(words=None), dict(phys=None), dict(count=None), dict(pre_count=None),
               dict(cands=None), dict(scratch=None), dict(scratch_bytes=15), dict(scratch_bytes=0), dict(words=p + 4), dict(cands=p + 4),
               dict(info=p + 8), dict(count=p + 2), dict(pre_count=p + 2), dict(phys=p + 1), dict(scratch=p + 8)):
        assert scan(**kw) == -3, kw
        assert b"btbbx_le_cfind_scan_device" in lib.btbbx_last_error()

    def host(words=p, search_bits=64 * 64 - 335, phys=p, max_len=27, max_errors=16, conns=p, conn_cap=4, cands=p, cand_cap=4):
        return lib.btbbx_le_cfind_host(words, 64, 64, 1, search_bits, phys, max_len, max_errors, 2, conns, conn_cap, cands, cand_cap, None)

    for kw in (dict(max_errors=64), dict(max_len=256), dict(search_bits=64 * 64 - 334), dict(words=None), dict(phys=None), dict(conns=None),
               dict(cands=None)):
        assert host(**kw) == -3, kw
        assert b"btbbx_le_cfind_host" in lib.btbbx_last_error()
    assert not buf.any()


def test_fails_loudly_without_gpu():
    """No CPU fallback: without a device the entries report an error, after the argument checks."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = bt.lib()
    buf = np.zeros(1 << 12, np.uint64)
    p = buf.ctypes.data
    for rc in (lib.btbbx_le_cfind_scan_device(p, 64, 64, 1, 1000, p, 27, 16, p, None, 4, p, p, p, 64, None),
               lib.btbbx_le_cfind_host(p, 64, 64, 1, 1000, p, 27, 16, 2, p, 4, p, 4, None)):
        assert rc < 0
        assert b"HIP" in lib.btbbx_last_error() and b"btbbx_le_cfind" not in lib.btbbx_last_error()
    assert not buf.any()
    with pytest.raises(bt.BtbbError):
        bt.le_coded_discover(np.zeros(64, np.uint64), 1000, 2440)
