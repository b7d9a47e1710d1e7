"""The C ABI of keyed LE following without a GPU: the new flag and the exported names against include/btbbx.h, the signatures beside
the unkeyed entries', the scratch sizes, and -- on a machine without a device -- that the entries refuse bad arguments first and
then fail with an error instead of computing anything on the host."""
import os
import re
import subprocess

import numpy as np
import pytest

import _le_crypt as cm
import _le_keyed as lk
import libbtbb_amd as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"btbbx_le_keyed_epoch_scratch_bytes", "btbbx_le_keyed_epoch_device", "btbbx_le_keyed_span_scratch_bytes",
         "btbbx_le_keyed_span_device", "btbbx_le_keyed_span_host"}


def test_the_flag_and_the_records_match_the_header(tmp_path):
    lines = ["#include <stdio.h>", "#include <btbbx.h>", "int main(void) {",
             'printf("%lu %lu %lu %lu %lu\\n", (unsigned long)BTBBX_LE_FOLLOW_DECRYPTED, (unsigned long)sizeof(btbbx_le_follow), '
             '(unsigned long)sizeof(btbbx_le_span), (unsigned long)sizeof(btbbx_le_crypt), (unsigned long)sizeof(btbbx_le_crypt_pkt));',
             "return 0; }"]
    src, exe = tmp_path / "flag.c", tmp_path / "flag"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c90", "-pedantic", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [bt.LE_FOLLOW_DECRYPTED, bt.LE_FOLLOW_DTYPE.itemsize, bt.LE_SPAN_DTYPE.itemsize, bt.LE_CRYPT_DTYPE.itemsize,
                   bt.LE_CRYPT_PKT_DTYPE.itemsize]
    # the free bit of both flag bytes, beside every other flag
    others = (bt.LE_FOLLOW_SEEDED, bt.LE_FOLLOW_COUNTED, bt.LE_FOLLOW_STOPPED, bt.LE_FOLLOW_TERMINATED, bt.LE_FOLLOW_ENCRYPTED, bt.LE_SPAN_CAPPED,
              bt.LE_SPAN_REFUSED)
    assert bt.LE_FOLLOW_DECRYPTED == lk.DECRYPTED == 128 and sum(others) + 128 == 255
    # the model reads the records the stages write
    assert list(cm.Crypt._fields) == list(bt.LE_CRYPT_DTYPE.names)[:-1] and list(cm.CPkt._fields) == list(bt.LE_CRYPT_PKT_DTYPE.names)[:-1]
    # the three LIMITS that said the gap point to the keyed entries now
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    assert text.count("btbbx_le_keyed_epoch_device") >= 3 and text.count("btbbx_le_keyed_span_device") >= 3


def test_signatures_are_declared():
    for name in NAMES:
        assert name in bt.SIGNATURES and getattr(bt.lib(), name) is not None
    for plain, keyed in (("btbbx_le_epoch_device", "btbbx_le_keyed_epoch_device"), ("btbbx_le_span_device", "btbbx_le_keyed_span_device")):
        a, b = bt.SIGNATURES[plain], bt.SIGNATURES[keyed]
        assert a[0] == b[0] and b[1][:14] == a[1][:14] and b[1][17:] == a[1][14:] and len(b[1]) == len(a[1]) + 3   # three arrays behind d_seeds
    s_host, k_host = bt.SIGNATURES["btbbx_le_span_host"][1], bt.SIGNATURES["btbbx_le_keyed_span_host"][1]
    assert k_host[:21] == s_host[:21] and k_host[26:] == s_host[21:] and len(k_host) == len(s_host) + 5
    assert bt.SIGNATURES["btbbx_le_keyed_epoch_scratch_bytes"] == bt.SIGNATURES["btbbx_le_epoch_scratch_bytes"]
    assert bt.SIGNATURES["btbbx_le_keyed_span_scratch_bytes"] == bt.SIGNATURES["btbbx_le_span_scratch_bytes"]
    assert callable(bt.le_span_keyed) and callable(bt.le_crack_span)


def test_the_names_are_exported_and_nothing_else_of_the_family():
    out = subprocess.run(["nm", "-D", "--defined-only", bt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {n for n in names if "keyed" in n} == NAMES
    header = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n


def test_scratch_is_the_unkeyed_stage_16_bytes_and_2_bits_per_candidate():
    lib = bt.lib()
    for cands in (0, 1, 64, 4097, 1 << 20, (1 << 32) - 1):
        for conns in (0, 1, 1000, 65537):
            want = 16 * max(cands, 1) + 2 * 8 * ((max(cands, 1) + 63) // 64)
            got = lib.btbbx_le_keyed_epoch_scratch_bytes(cands, conns) - lib.btbbx_le_epoch_scratch_bytes(cands, conns)
            assert want <= got < want + 1024 and got % 256 == 0
            for ups in (0, 4, 16, 17):
                got = lib.btbbx_le_keyed_span_scratch_bytes(cands, conns, ups) - lib.btbbx_le_span_scratch_bytes(cands, conns, ups)
                assert want <= got < want + 1024 and got % 256 == 0


def test_bad_arguments_are_refused_before_anything_else():
    lib = bt.lib()
    buf = np.zeros(1 << 16, np.uint64)
    p = buf.ctypes.data
    big = 1 << 18

    def span(words=p, dpkts=p, crypt=p, cpkts=p, ups=2, spans=p, scr_bytes=big, unit=1250):
        return lib.btbbx_le_keyed_span_device(words, 8, 8, 2, p, p, p, 8, p, p, 4, p, p, p, dpkts, crypt, cpkts, unit, 50, ups, spans, p, p, p,
                                              scr_bytes, None)

    def epoch(words=p, dpkts=p, crypt=p, cpkts=p, follows=p, scr_bytes=big, unit=1250):
        return lib.btbbx_le_keyed_epoch_device(words, 8, 8, 2, p, p, p, 8, p, p, 4, p, p, p, dpkts, crypt, cpkts, unit, 50, follows, p, p,
                                               scr_bytes, None)

    assert span(ups=17, words=None) == -3 and b"btbbx_le_keyed_span_device: max_updates must be 0..16" in lib.btbbx_last_error()
    for kw in (dict(dpkts=None), dict(crypt=None), dict(cpkts=None), dict(dpkts=p + 2), dict(crypt=p + 4), dict(cpkts=p + 8), dict(words=None),
               dict(unit=1), dict(words=p + 4)):
        assert span(**kw) == -3, kw
        assert b"btbbx_le_keyed_span_device" in lib.btbbx_last_error()
        assert epoch(**kw) == -3, kw
        assert b"btbbx_le_keyed_epoch_device" in lib.btbbx_last_error()
    assert span(spans=None) == -3 and epoch(follows=None) == -3
    assert span(scr_bytes=lib.btbbx_le_keyed_span_scratch_bytes(8, 4, 2) - 1) == -3
    assert epoch(scr_bytes=lib.btbbx_le_keyed_epoch_scratch_bytes(8, 4) - 1) == -3
    # (these alignments are enough: the call gets as far as the scratch's size, and no further -- nothing is launched on host memory)
    assert span(dpkts=p + 4, cpkts=p + 16, crypt=p + 8, scr_bytes=0) == -3
    assert b"misaligned" not in lib.btbbx_last_error() and b"or scratch of" in lib.btbbx_last_error()

    def host(n_keys=1, window=8, ups=4, keys=p, crypt=p, spans=p, adv=0):
        return lib.btbbx_le_keyed_span_host(p, 64, 64, 1, 1000, p, 27, 2, p, 4, p, 8, None, 1250, 200, 50, 1, adv, p, p, p, keys, n_keys, window,
                                            crypt, p, ups, spans, p, p)

    for kw, what in ((dict(ups=17), b"max_updates must be 0..16"), (dict(n_keys=0), b"n_keys must be 1..64"), (dict(n_keys=65), b"n_keys"),
                     (dict(window=0), b"window 1..32"), (dict(window=33), b"window"), (dict(keys=None), b"null pointer"),
                     (dict(crypt=None), b"null pointer"), (dict(spans=None), b"null pointer"), (dict(adv=5), b"max_errors must be 0..4")):
        assert host(**kw) == -3, kw
        assert b"btbbx_le_keyed_span_host" in lib.btbbx_last_error() and what in lib.btbbx_last_error(), (kw, lib.btbbx_last_error())
    assert not buf.any()


def test_fails_loudly_without_gpu():
    """No CPU fallback: without a device the entries report an error, after the argument checks."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = bt.lib()
    buf = np.zeros(1 << 16, np.uint64)
    p = buf.ctypes.data
    assert lib.btbbx_le_keyed_span_device(p, 8, 8, 2, p, p, p, 8, p, p, 4, p, p, p, p, p, p, 1250, 50, 4, p, p, p, p, 1 << 18, None) < 0
    assert b"HIP" in lib.btbbx_last_error() and b"btbbx_le_keyed_span_device" not in lib.btbbx_last_error()
    assert lib.btbbx_le_keyed_epoch_device(p, 8, 8, 2, p, p, p, 8, p, p, 4, p, p, p, p, p, p, 1250, 50, p, p, p, 1 << 18, None) < 0
    assert not buf.any()
    with pytest.raises(bt.BtbbError):
        bt.le_span_keyed(np.zeros(64, np.uint64), 1000, 2404, [bytes(16)])
