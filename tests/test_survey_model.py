"""The piconet survey's semantics, on the CPU: the expected records of tests/_survey.py over the oracle port equal the same
loop over the compiled reference, that loop equals the reference's real survey mode, and the fixture captures reach every
branch of btbb_uap_from_header (counted from the reference alone).  Plus what of the new ABI answers without a GPU."""
import ctypes as C

import numpy as np
import pytest

import _libs
import _survey as sv
import libbtbb_amd as bt

needs_ref = pytest.mark.skipif(_libs.ref() is None, reason="compiled reference not available")


@pytest.fixture(scope="module")
def reference_records():
    eng = sv.ReferenceEngine()
    out = {}
    for name, make in sv.FIXTURES.items():
        cap, kw = make()
        hits = cap.hits()
        stats = {}
        recs, cand = sv.expected(eng, cap, hits, stats=stats, **kw)
        out[name] = (cap, kw, hits, recs, cand, stats)
    return out


@needs_ref
def test_oracle_loop_equals_reference_loop(reference_records):
    eng = sv.OracleEngine()
    for name, (cap, kw, hits, recs, cand, _) in reference_records.items():
        got, got_cand = sv.expected(eng, cap, hits, **kw)
        sv.assert_records_equal(got, got_cand, recs, cand, name)
        perm = np.random.default_rng(3).permutation(len(hits))             # the order of the list does not matter
        got, got_cand = sv.expected(eng, cap, hits[perm], **kw)
        back = got.copy()
        back["settled_hit"] = [perm[i] if i != 0xFFFFFFFF else i for i in got["settled_hit"]]
        sv.assert_records_equal(back, got_cand, recs, cand, name + " permuted")


@needs_ref
def test_reference_loop_is_the_survey_mode(reference_records):
    """btbb_init_survey + btbb_process_packet(pkt, NULL) in global time order + btbb_next_survey_result leave the piconets the
    three-line loop leaves (piconets come out in order of first appearance)."""
    cap, kw, hits, recs, cand, _ = reference_records["multi"]
    eng = sv.ReferenceEngine()
    lib = eng.lib
    lib.btbb_init_survey.restype = C.c_int
    lib.btbb_next_survey_result.restype = C.c_void_p
    lib.refint_survey_off.restype = None
    lib.btbb_piconet_get_lap = getattr(lib, "btbb_piconet_get_lap")
    lib.btbb_piconet_get_lap.restype, lib.btbb_piconet_get_lap.argtypes = C.c_uint32, [C.c_void_p]
    seen = {}
    with sv._Stdout():
        try:
            lib.btbb_init_survey()
            for k in np.lexsort((hits["stream"], hits["offset"])):
                h = hits[k]
                ch = int(cap.channels[int(h["stream"])])
                clkn = (kw["clkn0"] + (int(h["offset"]) + kw["clk_phase"]) // cap.clk_div) & 0xFFFFFFFF
                p = eng.packet(int(h["lap"]), int(h["ac_errors"]), sv.packet_symbols(cap, h), ch, clkn)
                lib.btbb_process_packet(p, None)
                eng.free_packet(p)
            order = []
            while True:
                pn = lib.btbb_next_survey_result()
                if not pn:
                    break
                pn = C.c_void_p(pn)
                lap = int(lib.btbb_piconet_get_lap(pn))
                order.append(lap)
                seen[lap] = eng.state(pn)
        finally:
            lib.refint_survey_off()
    assert sorted(seen) == recs["lap"].tolist()
    first = recs[np.lexsort((recs["first_stream"], recs["first_offset"]))]["lap"].tolist()
    assert order == first, "first_offset / first_stream restore the order of btbb_next_survey_result"
    for r, c in zip(recs, cand):
        s = seen[int(r["lap"])]
        assert (s["flags"], s["uap"], s["clk_offset"], s["used_channels"], s["packets_observed"], s["total"], s["first_pkt_time"]) == \
            (r["flags"], r["uap"], r["clk_offset"], r["used_channels"], r["packets_observed"], r["total_packets_observed"],
             r["first_pkt_time"]), hex(int(r["lap"]))
        assert s["afh_map"] == r["afh_map"].tobytes() and (s["cand"] == c).all()


@needs_ref
def test_fixtures_reach_every_branch(reference_records):
    recs = np.concatenate([v[3] for v in reference_records.values()])
    cand = np.concatenate([v[4] for v in reference_records.values()])
    stats = [v[5] for v in reference_records.values()]
    left = (cand >= 0).sum(axis=1)
    assert (recs["settled_by"] == 2).sum() >= 8
    assert (recs["settled_by"] == 1).sum() >= 4
    assert (recs["n_resets"] > 0).sum() >= 4
    assert sum(s.get("oops", 0) for s in stats) >= 1, "no group filled the pattern memory"
    assert ((recs["settled_by"] == 0) & (recs["n_walked"] > 0) & (recs["packets_observed"] > 0) & (left >= 2)).sum() >= 4
    assert sum(s.get("no_header", 0) for s in stats) >= 50
    twins = 0
    for v in reference_records.values():
        h = v[2]
        keys, counts = np.unique(np.stack([h["lap"].astype(np.uint64), h["offset"]], axis=1), axis=0, return_counts=True)
        twins += int((counts > 1).sum())
    assert twins >= 2
    # a CRC settle whose winner is not candidate 0, on a piconet that was reset before: candidates above the winner are stale
    winner = (recs["clk_offset"].astype(np.int64) + recs["first_pkt_time"]) & 63
    assert ((recs["settled_by"] == 2) & (recs["n_resets"] > 0) & (winner != 0)).sum() >= 1
    # the records are consistent with themselves
    assert (recs["used_channels"] == [bin(int.from_bytes(m.tobytes(), "little")).count("1") for m in recs["afh_map"]]).all()


def test_scratch_size_answers_without_a_device():
    lib = bt.lib()
    sizes = [lib.btbbx_survey_scratch_bytes(c) for c in (0, 1, 2, 100, 4096, 4097, 1 << 20, 1 << 24)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    assert sizes[-2] >= (1 << 20) * (400 + 256)           # the gathered packets and their trial tables


def test_argument_errors_come_before_device_work():
    lib = bt.lib()
    entry = sv.entry_state(0)
    words = np.zeros(64, np.uint64)
    rec = np.zeros(4, bt.SURVEY_DTYPE)
    bad_channels = np.array([3, 79], np.uint8)

    def host(n_streams=1, channels=None, clk_div=625, clk_phase=0):
        return lib.btbbx_survey_host(bt._ptr(words), 32 if n_streams > 1 else 64, 32, n_streams, 100, 2,
                                     None if channels is None else bt._ptr(channels), 0, clk_div, clk_phase, bt._ptr(rec), 4, None)
    assert host(n_streams=2, channels=bad_channels) == -3
    assert host(clk_div=0) == -3
    assert host(clk_div=625, clk_phase=625) == -3

    def device(n_streams=1, channels=None, clk_div=625, clk_phase=0, scratch=1 << 20, scratch_bytes=None, hits=1 << 20):
        need = lib.btbbx_survey_scratch_bytes(16)
        return lib.btbbx_survey_hits_device(1 << 21, 64, 64, n_streams, hits, None, 16, None if channels is None else bt._ptr(channels),
                                            bt._ptr(entry), clk_div, clk_phase, 3125, 1 << 22, 16, 1 << 23, None, scratch,
                                            need if scratch_bytes is None else scratch_bytes, None)
    assert device(n_streams=2, channels=bad_channels) == -3
    assert device(n_streams=80) == -3                     # more streams than BR/EDR channels and no table
    assert device(clk_div=0) == -3
    assert device(clk_phase=700) == -3
    assert device(scratch_bytes=1000) == -3
    assert device(scratch=(1 << 20) + 8) == -3            # misaligned scratch
    assert device(hits=(1 << 20) + 4) == -3               # misaligned hit list
    assert b"" != lib.btbbx_last_error()


def test_survey_without_a_device_raises():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the failure path cannot be shown")
    with pytest.raises(bt.BtbbError):
        bt.survey(np.zeros(64, np.uint64), 100)
