"""The C ABI of the LE channel selection #2 stage without a GPU: the numpy dtypes against the structs of include/btbbx.h (sizes
and offsets, read from a C program compiled against the header), the flag constants, the scratch size, and -- on a machine
without a device -- that the entries fail with an error instead of computing anything on the host."""
import os
import re
import subprocess

import numpy as np
import pytest

import libbtbb_amd as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"btbbx_le_csa2": bt.LE_CSA2_DTYPE, "btbbx_le_csa2_pkt": bt.LE_CSA2_PKT_DTYPE}
CONSTANTS = {"BTBBX_LE_CSA2_REMAP": bt.LE_CSA2_REMAP, "BTBBX_LE_CSA2_EVALUATED": bt.LE_CSA2_EVALUATED,
             "BTBBX_LE_CSA2_UNIQUE": bt.LE_CSA2_UNIQUE, "BTBBX_LE_CSA2_PREFERRED": bt.LE_CSA2_PREFERRED}


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
    assert (bt.LE_CSA2_DTYPE.itemsize, bt.LE_CSA2_PKT_DTYPE.itemsize) == (24, 8)
    for name, value in CONSTANTS.items():
        assert int(got[name]) == value, name
    # every field of the header's structs has a dtype field of the same name
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for name, dtype in STRUCTS.items():
        body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1), flags=re.S)
        fields = [f.strip() for decl in body.split(";") if decl.strip() for f in decl.split(None, 1)[1].split(",")]
        assert fields == list(dtype.names), (name, fields)


def test_signatures_are_declared():
    for name in ("btbbx_le_csa2_scratch_bytes", "btbbx_le_csa2_device", "btbbx_le_csa2_host"):
        assert name in bt.SIGNATURES and getattr(bt.lib(), name) is not None
    assert len(bt.SIGNATURES["btbbx_le_csa2_device"][1]) == 14
    assert bt.SIGNATURES["btbbx_le_csa2_host"][1][:19] == bt.SIGNATURES["btbbx_le_track_host"][1] and len(bt.SIGNATURES["btbbx_le_csa2_host"][1]) == 21


def test_scratch_size_is_monotone_and_as_the_header_states():
    lib = bt.lib()
    up = lambda x: (x + 255) // 256 * 256                                  # noqa: E731
    for cands in (0, 1, 63, 64, 1000, 4097, 1 << 20, (1 << 32) - 1):
        for conns in (0, 1, 3, 64, 1000, 65537, 1 << 22):
            got = lib.btbbx_le_csa2_scratch_bytes(cands, conns)
            c, k = max(cands, 1), max(conns, 1)
            assert got == 256 + up(4 * (k + 1)) + up(4 * c) + up(1024 * k), (cands, conns)
            assert lib.btbbx_le_csa2_scratch_bytes(cands + 1 if cands < (1 << 32) - 1 else cands, conns) >= got
            assert lib.btbbx_le_csa2_scratch_bytes(cands, conns + 1) >= got
    sizes = [lib.btbbx_le_csa2_scratch_bytes(n, 100) for n in range(0, 5000, 37)]
    assert sizes == sorted(sizes)
    sizes = [lib.btbbx_le_csa2_scratch_bytes(100, k) for k in range(0, 5000, 37)]
    assert sizes == sorted(sizes) and len(set(sizes)) > 100


def test_fails_loudly_without_gpu():
    """No CPU fallback: without a device the entries report an error, after the argument checks."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = bt.lib()
    buf = np.zeros(4096, np.uint64)
    p = buf.ctypes.data
    assert lib.btbbx_le_csa2_device(None, p, 8, p, p, 4, p, p, 1, p, p, p, 1 << 15, None) == -3     # the argument check comes first
    assert b"btbbx_le_csa2_device: null pointer" in lib.btbbx_last_error()
    assert lib.btbbx_le_csa2_device(p, p, 8, p, p, 4, p, p, 1, p, p, p, 1 << 15, None) < 0
    assert b"HIP" in lib.btbbx_last_error() and b"btbbx_le_csa2_device" not in lib.btbbx_last_error()
    assert not buf.any()
    with pytest.raises(bt.BtbbError):
        bt.le_csa2(np.zeros(64, np.uint64), 1000, 2404)
