"""The C ABI of the LE Coded connection tracking without a GPU, as tests/test_le_cfind_abi.py: the rule words and the limits in
the header, the exported names, the declared signatures, and -- on a machine without a device -- that the entries refuse bad
arguments first, writing nothing, and then fail with an error instead of computing anything on the host.  The entries are named
le_ctrack: the other families' ABI tests pin the exported names that contain le_track, le_coded and cfind to their own."""
import os
import re
import subprocess

import numpy as np
import pytest

import libbtbb_amd as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"btbbx_le_ctrack_symbols_device", "btbbx_le_ctrack_device", "btbbx_le_ctrack_host"}
FOREIGN = ("le_coded", "le_cfind", "le_span", "le_data", "le_crypt", "le_pair", "le_resolve", "le_follow", "le_seed", "le_epoch", "le_track")


def test_the_rules_and_the_limits_stand_in_the_header():
    text = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    title = "LE Coded connection tracking: coded durations, events, hop check"
    assert text.index("btbbx_le_cfind_host(") < text.index(title) < text.index("hop selection and CLK1-27 reversal")
    section = text[text.index(title):text.index("hop selection and CLK1-27 reversal")]
    for n, word in enumerate(("STREAM", "CI", "S", "WRITES"), 1):
        assert re.search(r"\b%d\. %s\b" % (n, word), section), word
    flat = re.sub(r"[\s*]+", " ", section)                 # (the comment's line breaks and stars taken out)
    for word in ("decoder's rules 2 and 3", "symbols_i = 0", "37 steps of 8 symbols from o + 80", "x = 0 on equal sums", "ci = bits 32..33",
                 "not whitened", "symbols_i = 376 + S (8 (L + 5) + 3)", "symbols_i = 376", "btbbx_le_coded_cand_info", "below 2^48",
                 "end_m = offset_m + d_symbols[m]", "rules 1, 2 and 4 to 7", "d_symbols[i] = 80 + 8 cands[i].length", "btbbx_le_track_scratch_bytes",
                 "n_words > 2^40", "n_streams outside 1..65535", "pitch_words < n_words", "cand_cap == 0 succeeds", "LIMITS", "seed, follow, span, data,",
                 "LL_PHY_UPDATE_IND", "AUX_CONNECT_REQ", "soft decisions", "2M PHY", "lell_", "when sel is NULL", "0xff fill"):
        assert word in flat, word
    # the pointer from the discovery's LIMITS, which still name the gap in their own words
    cfind = re.sub(r"[\s*]+", " ", text[text.index("promiscuous LE Coded connection discovery: access address and CRCInit"):text.index("btbbx_le_cfind_host(")])
    assert "tracking coded candidates" in cfind and "LE Coded connection tracking" in cfind and "btbbx_le_ctrack_device" in cfind


def test_signatures_are_declared():
    for name in NAMES:
        assert name in bt.SIGNATURES and getattr(bt.lib(), name) is not None
    track, ctrack = bt.SIGNATURES["btbbx_le_track_device"], bt.SIGNATURES["btbbx_le_ctrack_device"]
    assert ctrack[0] == track[0] and ctrack[1][:8] == track[1][:8] and ctrack[1][9:] == track[1][8:] and len(ctrack[1]) == 18
    host, csa2, cfind = (bt.SIGNATURES[n] for n in ("btbbx_le_ctrack_host", "btbbx_le_csa2_host", "btbbx_le_cfind_host"))
    assert host[0] == cfind[0] and host[1][:14] == cfind[1] and host[1][14:22] == csa2[1][13:] and len(host[1]) == 23
    assert len(bt.SIGNATURES["btbbx_le_ctrack_symbols_device"][1]) == 9
    assert callable(bt.le_coded_track) and "symbols" in bt.le_coded_track.__doc__


def test_the_three_names_are_exported_and_nothing_else_of_the_family():
    out = subprocess.run(["nm", "-D", "--defined-only", bt.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert {n for n in names if "le_ctrack" in n} == NAMES
    assert not any(s in n for n in NAMES for s in FOREIGN)
    assert not any("le_track_run" in n for n in names)       # the way into le.hip's launcher is no export
    header = open(os.path.join(ROOT, "include", "btbbx.h")).read()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, header), n


def test_bad_arguments_are_refused_before_anything_else():
    lib = bt.lib()
    buf = np.zeros(1 << 12, np.uint64)
    p = buf.ctypes.data

    def sym(words=p, n_words=64, pitch=64, n_streams=1, cands=p, count=p, cand_cap=4, out=p):
        return lib.btbbx_le_ctrack_symbols_device(words, n_words, pitch, n_streams, cands, count, cand_cap, out, None)

    for kw in (dict(words=None), dict(cands=None), dict(count=None), dict(out=None), dict(words=p + 4), dict(cands=p + 4), dict(out=p + 2),
               dict(count=p + 2), dict(n_streams=0), dict(n_streams=65536), dict(n_streams=2, pitch=63), dict(n_words=(1 << 40) + 1, pitch=1 << 41),
               dict(cand_cap=0, n_streams=0), dict(cand_cap=0, out=p + 1)):
        assert sym(**kw) == -3, kw
        assert b"btbbx_le_ctrack_symbols_device" in lib.btbbx_last_error()

    scratch = lib.btbbx_le_track_scratch_bytes(4, 4)

    def track(cands=p, count=p, cand_cap=4, conns=p, conn_count=p, conn_cap=4, phys=p, n_streams=1, symbols=p, unit=1250, ifs=200, jitter=50,
              tracks=p, pkts=p, scr=p, scratch_bytes=scratch):
        return lib.btbbx_le_ctrack_device(cands, count, cand_cap, conns, conn_count, conn_cap, phys, n_streams, symbols, unit, ifs, jitter, 1,
                                          tracks, pkts, scr, scratch_bytes, None)

    assert scratch <= buf.nbytes
    for kw in (dict(symbols=None), dict(symbols=p + 2), dict(cands=None), dict(count=None), dict(conns=None), dict(conn_count=None), dict(phys=None),
               dict(tracks=None), dict(pkts=None), dict(scr=None), dict(scratch_bytes=scratch - 1), dict(cands=p + 4), dict(tracks=p + 4),
               dict(pkts=p + 4), dict(scr=p + 4), dict(count=p + 2), dict(phys=p + 1), dict(n_streams=0), dict(unit=1), dict(jitter=625),
               dict(cand_cap=0, symbols=None)):
        assert track(**kw) == -3, kw
        assert b"btbbx_le_ctrack_device" in lib.btbbx_last_error()

    def host(words=p, search_bits=64 * 64 - 335, phys=p, max_len=27, max_errors=16, conns=p, conn_cap=4, cands=p, cand_cap=4, unit=1250, jitter=50,
             tracks=p):
        return lib.btbbx_le_ctrack_host(words, 64, 64, 1, search_bits, phys, max_len, max_errors, 2, conns, conn_cap, cands, cand_cap, None, unit,
                                        200, jitter, 1, tracks, None, None, None, None)

    for kw in (dict(max_errors=64), dict(max_errors=-1), dict(max_len=256), dict(search_bits=64 * 64 - 334), dict(words=None), dict(phys=None),
               dict(conns=None), dict(cands=None), dict(tracks=None), dict(unit=1), dict(jitter=625)):
        assert host(**kw) == -3, kw
        assert b"btbbx_le_ctrack_host" in lib.btbbx_last_error()
    assert not buf.any()


def test_fails_loudly_without_gpu():
    """No CPU fallback: without a device the entries report an error, after the argument checks."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    lib = bt.lib()
    buf = np.zeros(1 << 12, np.uint64)
    p = buf.ctypes.data
    for rc in (lib.btbbx_le_ctrack_symbols_device(p, 64, 64, 1, p, p, 4, p, None),
               lib.btbbx_le_ctrack_device(p, p, 4, p, p, 4, p, 1, p, 1250, 200, 50, 1, p, p, p, lib.btbbx_le_track_scratch_bytes(4, 4), None),
               lib.btbbx_le_ctrack_host(p, 64, 64, 1, 1000, p, 27, 16, 2, p, 4, p, 4, None, 1250, 200, 50, 1, p, None, None, None, None)):
        assert rc < 0
        assert b"HIP" in lib.btbbx_last_error() and b"btbbx_le_ctrack" not in lib.btbbx_last_error()
    assert not buf.any()
    with pytest.raises(bt.BtbbError):
        bt.le_coded_track(np.zeros(64, np.uint64), 1000, 2440)
