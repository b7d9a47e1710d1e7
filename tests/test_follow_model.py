"""The yardstick of the follow tests, checked without a GPU: the numpy model of btbbx_follow_hits_device (tests/_follow.py) on the
three hopping piconets of tests/_acquire.py, built with the oracle port's hop pattern, against the oracle port alone -- survey
records from its survey loop, jobs from the builder's model, results from its btbb_init_hop_reversal + btbb_winnow, the decode
from its decoders.  Every planted packet must get its planted clock, sit on its hop and decode its header."""
import numpy as np
import pytest

import _acquire as aq
import _follow as fw
import _survey as sv
import libbtbb_amd as bt


@pytest.fixture(scope="module")
def followed():
    planted, cap, kw, hits, hops = fw.hopping("three")
    engine = sv.OracleEngine()
    recs, _ = sv.expected(engine, cap, hits, kw["clkn0"])
    built = aq.model(engine, cap, hits, recs, kw["clkn0"])
    results = fw.oracle_results(recs, built)
    hop = hops.for_jobs(fw.job_piconets(planted, recs, built["job_rec"]))
    pin, fol, stage_job = fw.model(hits, recs, built["job_rec"], results, built["jobs"], cap.channels, cap.n_streams,
                                   sv.entry_state(kw["clkn0"]), cap.clk_div, 0, hop)
    decoded = fw.oracle_decode(cap, hits, pin)
    yield planted, cap, kw, hits, recs, built, results, pin, fol, fw.sums(len(recs), stage_job, fol, decoded), decoded
    hops.close()


def test_every_piconet_is_acquired(followed):
    planted, cap, kw, hits, recs, built, results, pin, fol, sums, decoded = followed
    assert sorted(recs["lap"][built["job_rec"]].tolist()) == sorted(p.lap for p in planted) and len(built["jobs"]) == 3
    assert (results["status"] == 0).all() and (results["count"] == 1).all()
    laps = recs["lap"].tolist()
    for p in planted:
        assert sums["stage"][laps.index(p.lap)] == 2


def test_planted_clocks_on_hop_and_headers(followed):
    planted, cap, kw, hits, recs, built, results, pin, fol, sums, decoded = followed
    laps = recs["lap"].tolist()
    packets = fw.planted_packets(planted, cap, hits, kw)
    assert len(packets) == 90
    for i, k, slot, lt_addr in packets:
        p = planted[k]
        g = laps.index(p.lap)
        assert (fol["piconet"][i], fol["stage"][i]) == (g, 2)
        assert fol["clkn"][i] == pin["clkn"][i] == (p.c0 + slot) % bt.SEQUENCE_LENGTH, (hex(p.lap), slot)
        assert fol["on_hop"][i] == 1 and fol["hop_channel"][i] == fol["channel"][i] == hits["stream"][i]
        assert pin["uap"][i] == p.uap and pin["flags"][i] == 1 | fw.UAP_VALID | fw.CLK6_VALID | fw.CLK27_VALID
        present, hv, rv, st = decoded[i]
        assert hv != 0 and st["packet_lt_addr"] == lt_addr
        assert sums["lt_addr_mask"][g] >> lt_addr & 1
    for p in planted:
        s = sums[laps.index(p.lap)]
        assert (s["n_hits"], s["n_on_hop"], s["n_off_hop"], s["n_header"]) == (30, 30, 0, 30), (hex(p.lap), s)
        assert s["n_payload"] >= 20                          # POLL, DM1, DH1 and FHS, a quarter each
    # one clock wraps 2^27 inside the capture
    assert any(p.c0 + p.slots[-1] >= bt.SEQUENCE_LENGTH for p in planted)


def test_every_hit_is_counted_once(followed):
    """the capture's noise holds no access code: every hit is a planted packet, and the summaries add up to the list"""
    planted, cap, kw, hits, recs, built, results, pin, fol, sums, decoded = followed
    assert np.isin(hits["lap"], [p.lap for p in planted]).all() and len(hits) == 90
    assert (sums["n_hits"] == recs["n_packets"]).all() and sums["n_hits"].sum() == len(hits)
    assert (fol["piconet"] != fw.NONE).all() and (sums["job"] == np.arange(3)).all()
