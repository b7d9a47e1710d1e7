"""The FOLLOWING stage on the GPU: btbbx_follow_hits_device behind survey -> builder -> batch reversal against the host model of
tests/_follow.py (d_in, d_follow and d_sums byte for byte, d_out against the oracle port's decode with the model's clock, UAP
and flags), on planted clocks, on doctored tables, on counts and caps, and btbbx_follow_host against the composition it
replaces.  Integer logic throughout: everything must be equal, and every hit is compared."""
import ctypes as C
import threading

import numpy as np
import pytest

import _acquire as aq
import _follow as fw
import _libs
import _survey as sv
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
M27 = bt.SEQUENCE_LENGTH - 1


@pytest.fixture(scope="module", autouse=True)
def ready():
    bt.init(2)
    yield
    _libs.oracle().orc_hop_cache_clear()


def _args(cap, kw):
    return dict(channels=cap.channels, clk_div=cap.clk_div, clk_phase=kw.get("clk_phase", 0), max_length=kw.get("max_length", bt.MAX_SYMBOLS),
                n_words=cap.n_words)


def _run(cap, kw, hits, **opts):
    """every output over a sentinel fill; the d_out records of the hits the call decodes start as zeros, as a fresh packet of the
    oracle does (the decoders take a record's content for the packet's earlier state)"""
    n, count = len(opts.get("follow_hits", hits)), opts.get("follow_count", "same")
    count = opts.get("count") if isinstance(count, str) else count
    return bt.run_follow_hits(cap.words(), hits, sv.entry_state(kw["clkn0"]), sentinel=SENTINEL, zero_out=n if count is None else min(n, count),
                              **_args(cap, kw), **opts)


def _check(cap, kw, out, hop, hits, recs=None, job_rec=None, results=None, jobs=None, channels="same", ctx=""):
    """the model over the tables the follow saw (default: what the chain left) against `out`: every output, every hit"""
    recs = out["recs"] if recs is None else recs
    job_rec, results, jobs = (out[k] if v is None else v for k, v in (("job_rec", job_rec), ("results", results), ("jobs", jobs)))
    table = cap.channels if isinstance(channels, str) else channels
    max_length = kw.get("max_length", bt.MAX_SYMBOLS)
    pin, fol, stage_job = fw.model(hits, recs, job_rec, results, jobs, table, cap.n_streams, sv.entry_state(kw["clkn0"]), cap.clk_div,
                                   kw.get("clk_phase", 0), hop)
    decoded = fw.oracle_decode(cap, hits, pin, max_length)
    sums = fw.sums(len(recs), stage_job, fol, decoded)
    fw.assert_follow_equals(out, pin, fol, sums, SENTINEL, ctx=ctx)
    fw.assert_out_equals(out["pkt_out"][:len(hits)], out["lengths"][:len(hits)], decoded, cap, hits, max_length, ctx)
    return pin, fol, sums, decoded


def _same_outputs(a, b, n_recs, ctx):
    for name in ("pkt_in", "follow", "pkt_out", "lengths"):
        assert a[name].tobytes() == b[name].tobytes(), (ctx, name)
    assert a["sums"][:n_recs].tobytes() == b["sums"][:n_recs].tobytes(), (ctx, "sums")


# ---- 1. three hopping piconets ------------------------------------------------------------------------------------

def _three():
    planted, cap, kw, hits, hops = fw.hopping("three")
    return planted, cap, kw, hits, hops


def _hop_of(planted, hops, out):
    return hops.for_jobs(fw.job_piconets(planted, out["recs"], out["job_rec"]))


def test_three_hopping_piconets():
    planted, cap, kw, hits, hops = _three()
    out = _run(cap, kw, hits)
    want_recs, _ = sv.expected(sv.OracleEngine(), cap, hits, kw["clkn0"])
    sv.assert_records_equal(out["recs"], None, want_recs, None, "hopping")
    pin, fol, sums, decoded = _check(cap, kw, out, _hop_of(planted, hops, out), hits, ctx="three")
    got, laps = out["follow"], out["recs"]["lap"].tolist()
    packets = fw.planted_packets(planted, cap, hits, kw)
    assert len(packets) == 90
    for i, k, slot, lt_addr in packets:
        p = planted[k]
        g = laps.index(p.lap)
        assert (got["piconet"][i], got["stage"][i], got["on_hop"][i]) == (g, 2, 1), (hex(p.lap), slot)
        assert got["clkn"][i] == (p.c0 + slot) % bt.SEQUENCE_LENGTH, (hex(p.lap), slot)
        assert out["pkt_out"]["header_rv"][i] != 0 and out["pkt_out"]["lt_addr"][i] == lt_addr
        assert out["sums"]["lt_addr_mask"][g] >> lt_addr & 1
    for p in planted:
        s = out["sums"][laps.index(p.lap)]
        assert (s["stage"], s["n_hits"], s["n_on_hop"], s["n_off_hop"], s["n_header"]) == (2, 30, 30, 0, 30), (hex(p.lap), s)
    assert any(p.c0 + p.slots[-1] >= bt.SEQUENCE_LENGTH for p in planted)       # one clock wraps 2^27 inside the capture


# ---- 2. AFH -------------------------------------------------------------------------------------------------------------

def test_afh_piconet():
    planted, cap, kw, hits, _ = fw.hopping("afh")
    p = planted[0]
    out = _run(cap, kw, hits, flags=aq.JOBS_AFH)
    g = out["recs"]["lap"].tolist().index(p.lap)
    assert out["recs"]["afh_map"][g].tolist() == p.afh_map.tolist()
    hops = fw.OracleHops([(r["lap"], r["uap"], r["afh_map"]) for r in out["recs"][out["job_rec"]]])
    pin, fol, sums, decoded = _check(cap, kw, out, hops.for_jobs(list(range(len(out["job_rec"])))), hits, ctx="afh")
    s = out["sums"][g]
    assert (s["stage"], s["n_hits"], s["n_on_hop"], s["n_off_hop"], s["n_header"]) == (2, 60, 60, 0, 60), s
    for i, k, slot, lt_addr in fw.planted_packets(planted, cap, hits, kw):
        assert out["follow"]["clkn"][i] == (p.c0 + slot) % bt.SEQUENCE_LENGTH and out["follow"]["on_hop"][i] == 1
    # the same capture acquired without the map: whatever the reversal makes of it, the follow equals the model
    out = _run(cap, kw, hits)
    hops = fw.OracleHops([(r["lap"], r["uap"], None) for r in out["recs"][out["job_rec"]]])
    _check(cap, kw, out, hops.for_jobs(list(range(len(out["job_rec"])))), hits, ctx="afh capture, basic hopping assumed")


# ---- 3. stages 0 and 1 -------------------------------------------------------------------------------------------------

def _phase_decode(cap, kw, hits):
    """btbbx_decode_hits_piconet_phase_device over the list, records zeroed on entry"""
    lib, words, n = bt.lib(), cap.words(), len(hits)
    entry = sv.entry_state(kw["clkn0"])
    d_w = bt.DeviceBuffer(words.nbytes + 16).upload(words)
    d_h = bt.DeviceBuffer(hits.nbytes).upload(np.ascontiguousarray(hits))
    d_out = bt.DeviceBuffer(n * bt.PKTOUT_DTYPE.itemsize)
    try:
        bt.check(lib.btbbx_memset(d_out.ptr, 0, d_out.nbytes), "memset")
        bt.check(lib.btbbx_decode_hits_piconet_phase_device(d_w.ptr, cap.n_words, words.shape[1], d_h.ptr, None, n,
                                                            entry.ctypes.data_as(C.c_void_p), cap.clk_div, kw.get("clk_phase", 0),
                                                            kw.get("max_length", bt.MAX_SYMBOLS), d_out.ptr, None, None), "piconet_phase")
        bt.check(lib.btbbx_sync(None), "sync")
        return d_out.download(bt.PKTOUT_DTYPE, n)
    finally:
        for b in (d_w, d_h, d_out):
            b.free()


def test_stages_0_and_1_with_a_phase_and_a_channel_table():
    cap, kw = sv.capture_multi()
    assert kw["clk_phase"] == 624 and cap.channels is not None and cap.n_streams == 8
    hits = cap.hits()
    out = _run(cap, kw, hits)
    pin, fol, sums, decoded = _check(cap, kw, out, fw.gpu_hops(out["jobs"]), hits, ctx="multi")
    stage = out["follow"]["stage"]
    assert (stage == 0).sum() >= 40 and (stage == 1).sum() >= 1 and (stage >= 1).sum() >= 20   # ID packets and open LAPs; settled ones
    settled = out["recs"]["settled_by"][np.minimum(out["follow"]["piconet"], len(out["recs"]) - 1)] != 0
    assert ((stage == 0) == ~settled).all()
    assert (out["pkt_out"]["header_rv"][stage >= 1] != 0).sum() >= 20 and (out["follow"]["clkn"][stage == 1] < 64).all()
    # a stage-0 hit comes out as the one-piconet decoder leaves it
    plain = _phase_decode(cap, kw, hits)
    zero = np.nonzero(stage == 0)[0]
    assert all(out["pkt_out"][i].tobytes() == plain[i].tobytes() for i in zero)
    assert (out["follow"]["clkn"][zero] == fw.stored_clocks(hits[zero], sv.entry_state(kw["clkn0"]), cap.clk_div, kw["clk_phase"])).all()


def test_one_piconet_that_fills_whole_waves():
    """capture_oops: clk_div = 4, 1030 hits of ONE piconet that never settles (stage 0, resets) -- every wave of the tally but the
    last belongs to one record.  Then the same list with a doctored record, job and result: stage 1 (every header decodes) and
    stage 2 (every hit checked against the hop), counted by whole waves."""
    cap, kw = sv.capture_oops()
    hits = cap.hits()
    out = _run(cap, kw, hits)
    assert len(out["recs"]) == 1 and out["recs"]["settled_by"][0] == 0 and out["recs"]["n_resets"][0] >= 1 and len(hits) >= 1030
    _check(cap, kw, out, None, hits, ctx="oops")
    assert (out["follow"]["stage"] == 0).all() and out["sums"]["n_hits"][0] == len(hits)
    recs = out["recs"].copy()
    recs["settled_by"], recs["uap"], recs["clk_offset"] = 1, 0x9D, 21
    got = _run(cap, kw, hits, recs=recs)
    _check(cap, kw, got, None, hits, recs=recs, ctx="oops, settled by hand")
    assert got["sums"]["stage"][0] == 1 and got["sums"]["n_header"][0] >= 1030 and got["sums"]["lt_addr_mask"][0] & 4
    jobs = np.zeros(1, dtype=bt.CLOCK_JOB_DTYPE)
    jobs["cfg"] = np.frombuffer(bytes(bt.hop_cfg(int(recs["lap"][0]), 0x9D)), dtype=bt.HOP_CFG_DTYPE)[0]
    results = np.zeros(1, dtype=bt.CLOCK_RESULT_DTYPE)
    results["count"], results["cand0"] = 1, ((1 << 27) - 704) + ((int(recs["first_pkt_time"][0]) + 21) & 63)
    job_rec = np.zeros(1, dtype=np.uint32)
    got = _run(cap, kw, hits, recs=recs, jobs=jobs, job_rec=job_rec, results=results, n_jobs=1)
    pin, fol, sums, _ = _check(cap, kw, got, fw.gpu_hops(jobs), hits, recs=recs, jobs=jobs, job_rec=job_rec, results=results,
                               ctx="oops, a clock by hand")
    s = got["sums"][0]
    assert s["stage"] == 2 and s["n_on_hop"] + s["n_off_hop"] == len(hits) and s["n_off_hop"] > 900 and s["n_header"] >= 1030
    assert fol["clkn"].min() < 1000 and fol["clkn"].max() > (1 << 27) - 1000        # the clock passes 2^27 inside the list


# ---- 4. doctored tables ---------------------------------------------------------------------------------------------------

def test_doctored_tables():
    planted, cap, kw, hits, hops = _three()
    base = _run(cap, kw, hits)
    recs, jobs, job_rec, results = base["recs"], base["jobs"], base["job_rec"], base["results"]
    hop = _hop_of(planted, hops, base)
    nj = len(job_rec)
    assert nj == 3 and (results["count"] == 1).all()
    two = base["follow"]["stage"] == 2
    d = 12345

    def shifted(first=0, cand=0):
        r, q = recs.copy(), results.copy()
        r["first_pkt_time"][job_rec] += np.uint32(first)
        q["cand0"] += np.uint32(cand)
        return r, q

    # first_pkt_time and cand0 both moved: nothing changes
    r, q = shifted(d, d)
    out = _run(cap, kw, hits, recs=r, results=q)
    _same_outputs(out, base, len(recs), "both shifted")
    # first_pkt_time alone: every clock of a followed piconet moves back, and the hop check notices
    r, q = shifted(first=d)
    out = _run(cap, kw, hits, recs=r)
    _check(cap, kw, out, hop, hits, recs=r, ctx="first_pkt_time shifted")
    assert (out["follow"]["clkn"][two] == (base["follow"]["clkn"][two] - np.uint32(d)) & np.uint32(M27)).all()
    assert (out["follow"]["clkn"][~two] == base["follow"]["clkn"][~two]).all()
    assert out["sums"]["n_off_hop"].sum() >= 80 and out["sums"]["n_on_hop"].sum() + out["sums"]["n_off_hop"].sum() == 90
    # a reversal that did not end at one clock, or rejected its job: CLK1-6 is all there is
    q = results.copy()
    q["count"][0], q["status"][1] = 2, 1
    out = _run(cap, kw, hits, results=q)
    _check(cap, kw, out, hop, hits, results=q, ctx="count 2 / status 1")
    assert out["sums"]["stage"][job_rec].tolist() == [1, 1, 2] and out["sums"]["job"][job_rec].tolist() == [0, 1, 2]
    assert (out["follow"]["clkn"][out["follow"]["stage"] == 1] < 64).all()
    # fewer jobs stored than there are: the records behind the cut have no job
    out = _run(cap, kw, hits, job_cap=2)
    _check(cap, kw, out, hop, hits, job_rec=job_rec[:2], results=results[:2], jobs=jobs[:2], ctx="job_cap 2")
    assert out["sums"]["stage"][job_rec].tolist() == [2, 2, 1] and out["sums"]["job"][job_rec[2]] == fw.NONE
    # no jobs at all, null pointers
    out = _run(cap, kw, hits, job_cap=0)
    _check(cap, kw, out, hop, hits, job_rec=job_rec[:0], results=results[:0], jobs=jobs[:0], ctx="job_cap 0")
    assert out["sums"]["stage"][job_rec].tolist() == [1, 1, 1] and (out["follow"]["job"] == fw.NONE).all()
    # fewer records stored than there are: the LAPs cut off are nobody's
    cut = int(job_rec[2])
    assert 0 < cut < len(recs)
    out = _run(cap, kw, hits, rec_cap=cut)
    _check(cap, kw, out, hop, hits, recs=recs[:cut], ctx="rec_cap below the records")
    gone = hits["lap"] >= recs["lap"][cut]
    assert gone.sum() >= 30 and (out["follow"]["piconet"][gone] == fw.NONE).all() and (out["follow"]["stage"][gone] == 0).all()
    assert (out["follow"]["piconet"][~gone] != fw.NONE).all()
    # aliased jobs compare in aliased form
    j2 = jobs.copy()
    j2["aliased"] = 1
    out = _run(cap, kw, hits, jobs=j2)
    _check(cap, kw, out, hop, hits, jobs=j2, ctx="aliased")
    ch = base["follow"]["hop_channel"][two].astype(np.int64)
    assert (out["follow"]["hop_channel"][two] == (ch + 24) % 25 + 26).all()
    # the follow's own channel table with two streams swapped: exactly the hits on those two leave the hop
    streams = np.unique(hits["stream"][two])
    a, b = int(streams[0]), int(streams[-1])
    table = np.arange(cap.n_streams, dtype=np.uint8)
    table[a], table[b] = b, a
    out = _run(cap, kw, hits, follow_channels=table)
    _check(cap, kw, out, hop, hits, channels=table, ctx="two streams swapped")
    moved = np.isin(hits["stream"], (a, b))
    assert (out["follow"]["on_hop"][two & moved] == 0).all() and (out["follow"]["on_hop"][two & ~moved] == 1).all() and (two & moved).sum() >= 2


# ---- 5. counts and bounds -------------------------------------------------------------------------------------------------

def test_counts_and_bounds():
    planted, cap, kw, hits, hops = _three()
    base = _run(cap, kw, hits)
    recs, jobs, job_rec, results = base["recs"], base["jobs"], base["job_rec"], base["results"]
    hop = _hop_of(planted, hops, base)
    n = len(hits)
    assert n > 64
    # the list's length in HBM below the capacity, for the whole chain
    short = n - 11
    out = _run(cap, kw, hits, count=short)
    _check(cap, kw, out, _hop_of(planted, hops, out), hits[:short], ctx="count below cap")
    # ... and for the follow alone: the records of the later hits keep their stage and job and count nothing
    for count in (50, 0):
        out = _run(cap, kw, hits, follow_count=count)
        _check(cap, kw, out, hop, hits[:count], recs=recs, ctx="follow_count %d" % count)
        assert out["sums"]["n_hits"][:len(recs)].sum() == count
        for name in ("stage", "job"):
            assert (out["sums"][name][:len(recs)] == base["sums"][name][:len(recs)]).all()
    # a sub-list that leaves one piconet out, its length no multiple of 64, without a count; records and jobs without counts
    # either: the record without a hit keeps its stage and job and counts nothing
    sub = np.ascontiguousarray(hits[hits["lap"] != recs["lap"][1]])
    assert len(sub) == 60
    out = _run(cap, kw, hits, follow_hits=sub, follow_count=None, rec_count=None, rec_cap=len(recs), n_jobs=None, job_cap=len(job_rec))
    _check(cap, kw, out, hop, sub, recs=recs, ctx="sub-list, null counts")
    s = out["sums"][1]
    assert (s["stage"], s["job"]) == (2, 1) and [int(s[k]) for k in bt.FOLLOW_SUM_DTYPE.names[2:]] == [0] * 6
    # no d_lengths
    out = _run(cap, kw, hits, lengths=False)
    assert (out["lengths"].view(np.uint8) == SENTINEL).all()
    for name in ("pkt_in", "follow", "pkt_out", "sums"):
        assert out[name].tobytes() == base[name].tobytes(), name


# ---- 6. the host wrapper --------------------------------------------------------------------------------------------------

def test_follow_host_equals_the_composition_and_runs_from_four_threads():
    planted, cap, kw, hits, hops = _three()
    words = cap.words()
    recs, job_rec, results = bt.acquire(words, cap.search_bits, n_streams=cap.n_streams, clkn0=kw["clkn0"])
    jobs = np.zeros(len(job_rec), dtype=bt.CLOCK_JOB_DTYPE)                     # (the model takes `aliased` from them, nothing else)
    hop = hops.for_jobs(fw.job_piconets(planted, recs, job_rec))
    pin, fol, stage_job = fw.model(hits, recs, job_rec, results, jobs, cap.channels, cap.n_streams, sv.entry_state(kw["clkn0"]), cap.clk_div,
                                   0, hop)
    decoded = fw.oracle_decode(cap, hits, pin)
    sums = fw.sums(len(recs), stage_job, fol, decoded)

    def run(**opts):
        return bt.follow(words, cap.search_bits, n_streams=cap.n_streams, clkn0=kw["clkn0"], **opts)
    got = run()
    sv.assert_records_equal(got["recs"], None, recs, None, "follow")
    assert got["job_rec"].tolist() == job_rec.tolist() and got["results"].tobytes() == results.tobytes()
    assert got["n_hits"] == len(hits) and got["hits"].tobytes() == hits.tobytes()              # (the ordered scan's list: cap.hits() order)
    assert got["follow"].tobytes() == fol.tobytes() and got["sums"].tobytes() == sums.tobytes()
    fw.assert_out_equals(got["pkts"], None, decoded, cap, hits, ctx="follow_host")
    assert (got["sums"]["stage"][job_rec] == 2).all() and (got["sums"]["n_on_hop"][job_rec] == 30).all()
    # room for fewer hits than there are: the smallest (stream, offset), the count and the sums still cover all
    few = run(hit_cap=40)
    assert few["n_hits"] == len(hits) and few["hits"].tobytes() == hits[:40].tobytes() and few["follow"].tobytes() == fol[:40].tobytes()
    assert few["pkts"].tobytes() == got["pkts"][:40].tobytes() and few["sums"].tobytes() == sums.tobytes()
    nothing = run(packets=False)
    assert nothing["pkts"] is None and nothing["follow"].tobytes() == fol.tobytes() and nothing["sums"].tobytes() == sums.tobytes()
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
        for name in ("recs", "job_rec", "results", "hits", "follow", "pkts", "sums"):
            assert o[name].tobytes() == got[name].tobytes(), name
