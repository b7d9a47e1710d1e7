"""Helpers of the follow tests (no test in here): the host model of btbbx_follow_hits_device (include/btbbx.h) in numpy.

model() gives d_in and d_follow from (hits, recs, job_rec, results, jobs, channels, timing), oracle_decode() the expected d_out
from the oracle port's header_present / decode_header / decode_payload with the model's clock, UAP and flags, and sums() the
per-record summaries from both.  The hop channel of a stage-2 hit comes from a function the caller hands in: OracleHops (the
oracle port's whole pattern, affordable for a handful of piconets) or gpu_hops (btbbx_hop_channels_device, a kernel with tests
of its own against that pattern).  Nothing in here calls the code under test.
"""
import functools

import numpy as np

import _acquire as aq
import _hop
import _libs
import _pkt
import _survey as sv
import libbtbb_amd as bt

NONE = 0xFFFFFFFF
UAP_VALID, CLK6_VALID, CLK27_VALID = 1 << bt.BTBB_UAP_VALID, 1 << bt.BTBB_CLK6_VALID, 1 << bt.BTBB_CLK27_VALID
M27 = bt.SEQUENCE_LENGTH - 1


def stages(recs, job_rec, results):
    """(stage, job) of every record, from the stored jobs (job_rec ascending) and their results"""
    stage = (recs["settled_by"] != 0).astype(np.uint32)
    job = np.full(len(recs), NONE, dtype=np.uint32)
    for j, g in enumerate(np.asarray(job_rec, dtype=np.int64)):
        if g < len(recs):
            job[g] = j
            if results["status"][j] == 0 and results["count"][j] == 1:
                stage[g] = 2
    return stage, job


def stored_clocks(hits, entry, clk_div, clk_phase):
    """c of every hit: the stored clock of btbbx_survey_hits_device, uint32_t arithmetic"""
    ticks = (hits["offset"].astype(np.uint64) + np.uint64(clk_phase)) // np.uint64(clk_div)
    return ((int(entry["clkn"][0]) + ticks) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def model(hits, recs, job_rec, results, jobs, channels, n_streams, entry, clk_div, clk_phase, hop):
    """-> (d_in, d_follow, (stage, job) per record) for the N = len(hits) hits, the R = len(recs) records and the J = len(job_rec)
    jobs the call sees (the caller cuts them to the counts and caps).  hop(j, clocks) -> the channels job j hops to (not
    aliased).  entry: one PKTIN_DTYPE record."""
    entry = np.asarray(entry, dtype=bt.PKTIN_DTYPE).reshape(1)
    n = len(hits)
    stage_r, job_r = stages(recs, job_rec, results)
    pin, fol = np.zeros(n, dtype=bt.PKTIN_DTYPE), np.zeros(n, dtype=bt.FOLLOW_PKT_DTYPE)
    c = stored_clocks(hits, entry, clk_div, clk_phase)
    pos = np.searchsorted(recs["lap"], hits["lap"])
    known = np.zeros(n, dtype=bool)
    if len(recs):
        known = (pos < len(recs)) & (recs["lap"][np.minimum(pos, len(recs) - 1)] == hits["lap"])
    g = np.where(known, pos, 0)
    stage = np.where(known, stage_r[g] if len(recs) else 0, 0).astype(np.uint32)
    for name in ("flags", "uap", "type", "llid", "flow"):
        pin[name] = entry[name][0]
    pin["clkn"] = c
    fol["piconet"] = np.where(known, pos, NONE)
    fol["job"] = np.where(known, job_r[g] if len(recs) else NONE, NONE)
    fol["stage"] = stage
    stream = hits["stream"].astype(np.int64)
    table = np.arange(256, dtype=np.uint8) if channels is None else np.asarray(channels, dtype=np.uint8)
    fol["channel"] = np.where(stream < n_streams, table[np.minimum(stream, len(table) - 1)], 0xFF)
    fol["hop_channel"] = 0xFF
    one, two = stage == 1, stage == 2
    if len(recs):
        pin["uap"][one | two] = recs["uap"][g][one | two]
        pin["flags"][one] |= UAP_VALID | CLK6_VALID
        pin["flags"][two] |= UAP_VALID | CLK6_VALID | CLK27_VALID
        pin["clkn"][one] = (recs["clk_offset"][g][one].astype(np.uint32) + c[one]) & 0x3F
    for j in np.unique(fol["job"][two]):
        mine = two & (fol["job"] == j)
        first = recs["first_pkt_time"][g][mine].astype(np.uint32)
        clk = (np.uint32(results["cand0"][j]) + c[mine] - first) & np.uint32(M27)
        pin["clkn"][mine] = clk
        ch = np.asarray(hop(int(j), clk), dtype=np.int64)
        if jobs["aliased"][j]:
            ch = (ch + 24) % 25 + 26
        fol["hop_channel"][mine] = ch
    fol["clkn"] = pin["clkn"]
    fol["on_hop"] = two & (fol["hop_channel"] == fol["channel"])
    return pin, fol, (stage_r, job_r)


def oracle_decode(cap, hits, pin, max_length=bt.MAX_SYMBOLS):
    """What the reference's decoders leave for every hit entered with pin[i]: [(header_present, header_rv, payload_rv, state)],
    as test_gpu_packets._oracle_decode does it, with the clock, the UAP, the flags and the entry state of the model."""
    orc = _libs.oracle()
    orc.orc_init(2)
    out = []
    for h, p_in in zip(hits, pin):
        sym = sv.packet_symbols(cap, h, max_length)
        p = orc.orc_packet_new()
        orc.orc_packet_init_found(p, int(h["lap"]), int(h["ac_errors"]))
        orc.orc_packet_set_data(p, _libs.ptr(sym), len(sym), 0, 0)
        c = p.contents
        c.clkn, c.flags, c.UAP = int(p_in["clkn"]), int(p_in["flags"]), int(p_in["uap"])
        c.packet_type, c.payload_llid, c.payload_flow = int(p_in["type"]), int(p_in["llid"]), int(p_in["flow"])
        present = orc.orc_header_present(p)
        hv = orc.orc_decode_header(p)
        rv = orc.orc_decode_payload(p) if hv else 0
        out.append((present, hv, rv, _pkt.orc_state(p)))
        orc.orc_packet_free(p)
    return out


def _bits(b):
    return int(sum(int(x) << k for k, x in enumerate(b)))


def assert_out_equals(out, lengths, decoded, cap, hits, max_length=bt.MAX_SYMBOLS, ctx=""):
    """every field the decoders assign, as test_gpu_packets.test_batch_decode compares them; every hit"""
    assert len(out) == len(decoded) == len(hits)
    for i, (o, (present, hv, rv, st)) in enumerate(zip(out, decoded)):
        at = (ctx, i)
        assert int(o["header_present"]) == present and int(o["header_rv"]) == hv and int(o["payload_rv"]) == rv, at
        assert int(o["flags"]) == st["flags"] and int(o["header_packed"]) == _bits(st["packet_header"]), at
        if lengths is not None:
            assert int(lengths[i]) == len(sv.packet_symbols(cap, hits[i], max_length)), at
        if hv:
            assert (int(o["type"]), int(o["lt_addr"]), int(o["hdr_flags"]), int(o["hec"])) == \
                   (st["packet_type"], st["packet_lt_addr"], st["packet_flags"], st["packet_hec"]), at
            assert (int(o["payload_length"]), int(o["payload_header_length"])) == (st["payload_length"], st["payload_header_length"]), at
            assert (int(o["llid"]), int(o["flow"])) == (st["payload_llid"], st["payload_flow"]), at
            assert int(o["payload_header"]) == _bits(st["payload_header"]), at
            bits = bt.synth.unpack_bits(np.ascontiguousarray(o["payload"]), 2744)
            assert (bits == st["payload"]).all(), (at, np.nonzero(bits != st["payload"])[0][:8])


def sums(n_recs, stage_job, fol, decoded):
    """d_sums of the first n_recs records from the model's d_follow and the oracle's decode"""
    stage_r, job_r = stage_job
    s = np.zeros(n_recs, dtype=bt.FOLLOW_SUM_DTYPE)
    s["stage"], s["job"] = stage_r[:n_recs], job_r[:n_recs]
    for f, (_, hv, rv, st) in zip(fol, decoded):
        g = int(f["piconet"])
        if g == NONE:
            continue
        s["n_hits"][g] += 1
        if hv:
            s["n_header"][g] += 1
            s["lt_addr_mask"][g] |= 1 << st["packet_lt_addr"]
        if rv > 0:
            s["n_payload"][g] += 1
        if f["stage"] == 2:
            s["n_on_hop" if f["on_hop"] else "n_off_hop"][g] += 1
    return s


def assert_follow_equals(out, pin, fol, want_sums, sentinel, n_recs=None, ctx=""):
    """`out`: bt.run_follow_hits over buffers filled with `sentinel` bytes; d_in, d_follow and d_sums byte for byte, and nothing
    behind N hits and R records"""
    n, r = len(pin), len(want_sums) if n_recs is None else n_recs
    for name, want in (("pkt_in", pin), ("follow", fol)):
        got = out[name][:n]
        bad = [i for i in range(n) if got[i].tobytes() != want[i].tobytes()]
        assert not bad, (ctx, name, len(bad), [(i, got[i], want[i]) for i in bad[:4]])
    got = out["sums"][:r]
    bad = [g for g in range(r) if got[g].tobytes() != want_sums[g].tobytes()]
    assert not bad, (ctx, "sums", len(bad), [(g, got[g], want_sums[g]) for g in bad[:4]])
    for name, k in (("pkt_in", n), ("follow", n), ("pkt_out", n), ("lengths", n), ("sums", r)):
        assert (out[name][k:].view(np.uint8) == sentinel).all(), (ctx, name, "written past", k)


# ---- hop channels --------------------------------------------------------------------------------------------------

class OracleHops:
    """hop(j, clocks) from the oracle port's whole pattern (orc_get_hop_pattern: 2^27 channels per piconet, in the port's own
    cache until somebody clears it -- nothing of it is kept here) of the piconets (lap, uap, afh_map or None)."""

    def __init__(self, piconets):
        self.orc = _libs.oracle()
        self.piconets = [(int(lap), int(uap), None if m is None else np.ascontiguousarray(m, dtype=np.uint8)) for lap, uap, m in piconets]

    def for_jobs(self, job_piconet):
        """hop over jobs: job_piconet[j] = index into the piconets"""
        return lambda j, clocks: self.channels(job_piconet[j], clocks)

    def channels(self, k, clocks):
        lap, uap, m = self.piconets[k]
        # (the port's cache is keyed by the address alone, quirk H1: a pattern under AFH is generated afresh and not left behind)
        if m is not None:
            self.orc.orc_hop_cache_clear()
        pn, seq = _hop.orc_pattern(self.orc, lap, uap, m)
        out = seq[np.asarray(clocks, dtype=np.int64) & M27].copy()
        self.orc.orc_piconet_free(pn)
        if m is not None:
            self.orc.orc_hop_cache_clear()
        return out

    def close(self):
        self.orc.orc_hop_cache_clear()


def gpu_hops(jobs):
    """hop(j, clocks) from btbbx_hop_channels_device over the job's own cfg"""
    def hop(j, clocks):
        return bt.hop_channels(bt.HopCfg.from_buffer_copy(jobs[j]["cfg"].tobytes()), np.asarray(clocks, dtype=np.uint32))
    return hop


# ---- the hopping fixtures, built with the oracle's pattern ------------------------------------------------------------

def planted_hops(planted):
    return OracleHops([(p.lap, p.uap, p.afh_map) for p in planted])


@functools.lru_cache(maxsize=None)
def hopping(which="three"):
    """(planted, capture, its arguments, hit list, OracleHops over the planted piconets): _acquire.three_piconets (one clock
    wrapping 2^27) or _acquire.afh_piconet on a _acquire.hopping_capture; built once per process, never changed."""
    planted = aq.three_piconets() if which == "three" else aq.afh_piconet()
    hops = planted_hops(planted)
    index = {id(p): k for k, p in enumerate(planted)}
    seed, clkn0 = (43, 0x0ABCDEF1) if which == "three" else (44, 0x00123457)
    cap, kw = aq.hopping_capture(seed, planted, lambda p, clocks: hops.channels(index[id(p)], clocks), clkn0=clkn0)
    return planted, cap, kw, cap.hits(), hops


def job_piconets(planted, recs, job_rec):
    """which planted piconet every job belongs to (by LAP)"""
    laps = [p.lap for p in planted]
    return [laps.index(int(recs["lap"][g])) for g in job_rec]


def oracle_results(recs, built):
    """The CLOCK_RESULT_DTYPE records of the jobs of `built` (aq.model) from the oracle port's btbb_init_hop_reversal +
    btbb_winnow over the same observations, as test_gpu_acquire.test_planted_clocks_and_reference_reversal runs them.  Jobs
    without AFH only."""
    orc = _libs.oracle()
    res = np.zeros(len(built["jobs"]), dtype=bt.CLOCK_RESULT_DTYPE)
    for j, job in enumerate(built["jobs"]):
        rec = recs[built["job_rec"][j]]
        assert not job["cfg"]["afh"] and not job["aliased"]
        pn, _ = _hop.orc_pattern(orc, int(rec["lap"]), int(rec["uap"]), None)
        c = pn.contents
        c.first_pkt_time, c.clk_offset = int(rec["first_pkt_time"]), int(rec["clk_offset"])
        lo, n = int(job["obs_first"]), int(job["n_obs"])
        assert 1 <= n <= 1000
        for i in range(n):
            c.pattern_indices[i], c.pattern_channels[i] = int(built["offsets"][lo + i]), int(built["channels"][lo + i])
        c.packets_observed = n
        res["n_initial"][j] = orc.orc_init_hop_reversal(0, pn)
        orc.orc_winnow(pn)
        res["count"][j], res["stop"][j] = c.num_candidates, c.winnowed
        res["cand0"][j] = c.clock_candidates[0] if c.num_candidates else 0
        orc.orc_piconet_free(pn)
    return res


def planted_packets(planted, cap, hits, kw):
    """[(hit index, piconet k, slot, LT_ADDR)] of every planted packet: the hit at slot * clk_div on the stream the capture put
    it on, and the LT_ADDR the oracle port decodes from it with the PLANTED clock and UAP (the header must check out)."""
    orc = _libs.oracle()
    where = {(int(h["lap"]), int(h["offset"])): i for i, h in enumerate(hits)}
    out = []
    for k, p in enumerate(planted):
        for slot in p.slots:
            i = where[(p.lap, slot * cap.clk_div)]
            sym = sv.packet_symbols(cap, hits[i])
            pk = orc.orc_packet_new()
            orc.orc_packet_init_found(pk, p.lap, 0)
            orc.orc_packet_set_data(pk, _libs.ptr(sym), len(sym), 0, 0)
            pk.contents.clkn, pk.contents.UAP = (p.c0 + slot) & M27, p.uap
            pk.contents.flags |= UAP_VALID | CLK6_VALID
            assert orc.orc_decode_header(pk) == 1, (hex(p.lap), slot)
            out.append((i, k, slot, int(pk.contents.packet_lt_addr)))
            orc.orc_packet_free(pk)
    return out
