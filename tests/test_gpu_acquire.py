"""Clock acquisition from a capture on the GPU: btbbx_survey_clock_jobs_device against the host model of tests/_acquire.py
(byte for byte), the chain survey -> builder -> batch reversal against planted clocks and against the oracle port's
btbb_init_hop_reversal + btbb_winnow, and btbbx_acquire_host against the composition it replaces.  Integer logic throughout:
everything must be equal."""
import functools
import threading

import numpy as np
import pytest

import _acquire as aq
import _hop
import _libs
import _survey as sv
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
BOTH = aq.JOBS_AFH | aq.JOBS_ALIASED


@pytest.fixture(scope="module")
def engine():
    bt.init(2)
    yield sv.OracleEngine()
    _libs.oracle().orc_hop_cache_clear()


@functools.lru_cache(maxsize=None)
def _fixture(name):
    """capture, its arguments, its hit list and the survey records of the oracle loop: computed once, never changed"""
    cap, kw = sv.FIXTURES[name]()
    hits = cap.hits()
    recs, _ = sv.expected(sv.OracleEngine(), cap, hits, kw["clkn0"], kw.get("clk_phase", 0), kw.get("max_length", bt.MAX_SYMBOLS))
    return cap, kw, hits, recs


def _build(cap, kw, hits, **opts):
    return bt.run_survey_clock_jobs(cap.words(), hits, sv.entry_state(kw["clkn0"]), channels=cap.channels, clk_div=cap.clk_div,
                                    clk_phase=kw.get("clk_phase", 0), max_length=kw.get("max_length", bt.MAX_SYMBOLS),
                                    n_words=cap.n_words, sentinel=SENTINEL, **opts)


def _model(engine, cap, kw, hits, recs, **opts):
    return aq.model(engine, cap, hits, recs, kw["clkn0"], kw.get("clk_phase", 0), kw.get("max_length", bt.MAX_SYMBOLS), **opts)


@pytest.mark.parametrize("flags", [0, BOTH])
@pytest.mark.parametrize("name", ["single", "multi"])
def test_builder_equals_the_model(engine, name, flags):
    cap, kw, hits, recs = _fixture(name)
    want = _model(engine, cap, kw, hits, recs, flags=flags)
    out = _build(cap, kw, hits, flags=flags)
    sv.assert_records_equal(out["recs"], None, recs, None, name)
    aq.assert_builder_equals(out, want, SENTINEL, (name, flags))
    settled = recs[want["job_rec"]]
    # a piconet that settled after resets: its run does not begin at the first packet walked
    assert (settled["n_walked"] > settled["packets_observed"]).any()
    # ID packets (nothing walked) and piconets left open (walked, not settled) exist and yield no job
    idle = np.setdiff1d(np.arange(len(recs)), want["job_rec"])
    assert (recs["settled_by"][idle] == 0).all() and (recs["settled_by"][want["job_rec"]] != 0).all()
    assert (recs["n_walked"][idle] == 0).sum() >= 20 and (recs["n_walked"][idle] > 0).sum() >= 3
    assert want["n_jobs"] == len(want["jobs"]) >= 8
    if flags & aq.JOBS_AFH:
        assert (want["jobs"]["cfg"]["afh"] == 1).all() and (want["jobs"]["cfg"]["used_channels"] == settled["used_channels"]).all()
        assert (want["jobs"]["aliased"] == 1).all()


def test_a_piconet_that_never_settles_gives_no_job(engine):
    cap, kw, hits, recs = _fixture("oops")
    assert (recs["settled_by"] == 0).all() and recs["n_resets"].max() >= 1
    out = _build(cap, kw, hits)
    want = _model(engine, cap, kw, hits, recs)
    assert want["n_jobs"] == 0 and want["n_obs"] == 0
    aq.assert_builder_equals(out, want, SENTINEL, "oops")


def test_caps(engine):
    cap, kw, hits, recs = _fixture("multi")
    n_jobs = int((recs["settled_by"] != 0).sum())
    for job_cap in (1, n_jobs - 1):
        out = _build(cap, kw, hits, job_cap=job_cap)
        want = _model(engine, cap, kw, hits, recs, job_cap=job_cap)
        assert want["n_jobs"] == n_jobs and len(want["jobs"]) == job_cap
        aq.assert_builder_equals(out, want, SENTINEL, "job_cap %d" % job_cap)
    for max_obs in (1, 2, 1024):
        out = _build(cap, kw, hits, max_obs=max_obs)
        want = _model(engine, cap, kw, hits, recs, max_obs=max_obs)
        assert want["jobs"]["n_obs"].max() == min(max_obs, _model(engine, cap, kw, hits, recs)["jobs"]["n_obs"].max())
        aq.assert_builder_equals(out, want, SENTINEL, "max_obs %d" % max_obs)
    few = len(recs) // 2
    assert 0 < int((recs["settled_by"][:few] != 0).sum()) < n_jobs
    out = _build(cap, kw, hits, rec_cap=few)
    assert out["n_recs"] == len(recs) and len(out["recs"]) == few
    aq.assert_builder_equals(out, _model(engine, cap, kw, hits, recs[:few]), SENTINEL, "rec_cap below the piconets")
    out = _build(cap, kw, hits, rec_cap=len(recs), rec_count=False)
    aq.assert_builder_equals(out, _model(engine, cap, kw, hits, recs), SENTINEL, "NULL d_rec_count")


# ---- planted clocks ---------------------------------------------------------------------------------------------

def _gpu_hop(p, clocks):
    return bt.hop_channels(bt.hop_cfg(p.lap, p.uap, p.afh_map), clocks)


@functools.lru_cache(maxsize=None)
def _hopping():
    bt.init(2)
    planted = aq.three_piconets()
    cap, kw = aq.hopping_capture(43, planted, _gpu_hop, clkn0=0x0ABCDEF1)
    return planted, cap, kw, cap.hits()


def _first_slot(p, rec, kw):
    """slot of the packet whose stored clock is the record's first_pkt_time"""
    k = (int(rec["first_pkt_time"]) - kw["clkn0"]) & 0xFFFFFFFF
    assert k in p.slots
    return k


def test_planted_clocks_and_reference_reversal(engine):
    planted, cap, kw, hits = _hopping()
    recs, _ = sv.expected(engine, cap, hits, kw["clkn0"])
    out = _build(cap, kw, hits, reversal=True)
    sv.assert_records_equal(out["recs"], None, recs, None, "hopping")
    want = _model(engine, cap, kw, hits, recs)
    aq.assert_builder_equals(out, want, SENTINEL, "hopping")
    nj = out["n_jobs"]
    laps = recs["lap"][out["job_rec"][:nj]].tolist()
    assert sorted(laps) == sorted(p.lap for p in planted)
    assert (out["results"][nj:].view(np.uint8) == SENTINEL).all()
    orc = _libs.oracle()
    for j in range(nj):
        p = [x for x in planted if x.lap == laps[j]][0]
        rec, job, res = recs[out["job_rec"][j]], out["jobs"][j], out["results"][j]
        assert rec["uap"] == p.uap and rec["clk_offset"] == (p.c0 - kw["clkn0"]) & 63
        truth = (p.c0 + _first_slot(p, rec, kw)) % _hop.SEQ_LEN
        assert (res["status"], res["count"], res["cand0"]) == (0, 1, truth), (hex(p.lap), res, truth)
        # the reference's own steps on the oracle port, over the same observations
        pn, _ = _hop.orc_pattern(orc, p.lap, p.uap, None)
        c = pn.contents
        c.first_pkt_time, c.clk_offset = int(rec["first_pkt_time"]), int(rec["clk_offset"])
        lo, n = int(job["obs_first"]), int(job["n_obs"])
        assert 1 <= n <= 1000
        for i in range(n):
            c.pattern_indices[i], c.pattern_channels[i] = int(out["offsets"][lo + i]), int(out["channels"][lo + i])
        c.packets_observed = n
        n_initial = orc.orc_init_hop_reversal(0, pn)
        left = orc.orc_winnow(pn)
        assert left == 1, "the oracle itself must end at one candidate for a planted piconet"
        assert (res["n_initial"], res["count"], res["cand0"]) == (n_initial, c.num_candidates, c.clock_candidates[0])
        assert res["stop"] == c.winnowed
        orc.orc_piconet_free(pn)
        orc.orc_hop_cache_clear()
    # one of the clocks wraps: candidate + offset passes 2^27 inside the run
    assert any(p.c0 + p.slots[-1] >= _hop.SEQ_LEN for p in planted)


def test_afh_piconet(engine):
    planted = aq.afh_piconet()
    p = planted[0]
    cap, kw = aq.hopping_capture(44, planted, _gpu_hop, clkn0=0x00123457)
    hits = cap.hits()
    out = _build(cap, kw, hits, flags=aq.JOBS_AFH, reversal=True)
    g = int(np.nonzero(out["recs"]["lap"] == p.lap)[0][0])
    rec = out["recs"][g]
    assert rec["afh_map"].tolist() == p.afh_map.tolist() and rec["used_channels"] == 20 and rec["settled_by"] != 0
    j = out["job_rec"][:out["n_jobs"]].tolist().index(g)
    assert out["jobs"][j]["cfg"].tobytes() == bytes(bt.hop_cfg(p.lap, p.uap, p.afh_map))
    res = out["results"][j]
    truth = (p.c0 + _first_slot(p, rec, kw)) % _hop.SEQ_LEN
    assert (res["status"], res["count"], res["cand0"]) == (0, 1, truth), (res, truth)


def test_acquire_equals_the_composition_and_runs_from_four_threads(engine):
    planted, cap, kw, hits = _hopping()
    words = cap.words()
    recs = bt.survey(words, cap.search_bits, n_streams=cap.n_streams, clkn0=kw["clkn0"])
    want = _model(engine, cap, kw, hits, recs)              # (the wrapper's list is the ordered scan's: cap.hits() order)
    want_res, want_cand = bt.hop_reversal_batch_raw(want["jobs"], want["offsets"], want["channels"], cand_cap=4)

    def run():
        return bt.acquire(words, cap.search_bits, n_streams=cap.n_streams, clkn0=kw["clkn0"], cand_cap=4)
    got_recs, job_rec, results, cand = run()
    sv.assert_records_equal(got_recs, None, recs, None, "acquire")
    assert job_rec.tolist() == want["job_rec"].tolist() and len(job_rec) == 3
    assert results.tobytes() == want_res.tobytes()
    assert [c.tolist() for c in cand] == [want_cand[j, :int(want_res["n_stored"][j])].tolist() for j in range(len(want_res))]
    assert (results["count"] == 1).all()
    outs, errors = [None] * 4, []

    def work(i):
        try:
            for _ in range(2):
                outs[i] = run()
        except Exception as e:                                          # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for o in outs:
        assert o[0].tobytes() == got_recs.tobytes() and o[1].tolist() == job_rec.tolist() and o[2].tobytes() == results.tobytes()
        assert [c.tolist() for c in o[3]] == [c.tolist() for c in cand]
