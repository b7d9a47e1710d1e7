"""The crowd capture (tests/_crowd.py) on the CPU: every input the lattice is built for is there (tags over the oracle's
records), the placements are exactly what an access-code search finds, the builder's model has the jobs on both sides of its
1024-record round, and the model split into a shared header pass and a per-variation part still gives what the one-piece model
gave.  Measured: 8 to 12 s for the module (the capture 3 s, the survey loop over the oracle 5 s, the search 0.7 s)."""
import numpy as np

import _acquire as aq
import _crowd as cr
import _survey as sv
import libbtbb_amd as bt


def test_every_tag_is_present():
    c = cr.crowd()
    recs, cands, walked = cr.oracle_records()
    assert len(recs) == cr.N_RECORDS == len(c.kinds) and recs["lap"].tolist() == [cr.lap_of(g) for g in range(cr.N_RECORDS)]
    assert 8000 <= len(c.hits) <= 10000
    assert len(c.hits) > 2 * cr.SORT_TILE and len(c.hits) > 4 * cr.GRP_TILE
    missing = cr.TAGS - cr.tags(recs, c.hits, walked)
    assert not missing, sorted(missing)
    # the kinds do what they are named for
    kinds, settled = np.array(c.kinds), recs["settled_by"] != 0
    assert settled[kinds == "crc"].all() and (recs["settled_by"][kinds == "crc"] == 2).sum() >= 1400
    assert not settled[(kinds == "id") | (kinds == "open")].any()
    assert (recs["n_walked"][kinds == "id"] == 0).all() and (recs["n_walked"][kinds == "open"] == 1).all()
    assert settled[[cr.G_HUGE, cr.G_LONG]].all() and cr.G_HUGE // cr.SLOT_ROUND != cr.G_LONG // cr.SLOT_ROUND
    run = cr.runs(recs, walked)
    assert (run[cr.G_HUGE], run[cr.G_LONG]) == (1101, 151)
    assert 20 <= (kinds == "elim").sum() <= 40 and (recs["settled_by"][kinds == "elim"] == 1).any()
    assert (recs["n_resets"][kinds == "reset"] > 0).sum() >= 100 and settled[kinds == "reset"].sum() >= 50
    assert settled[kinds == "twin"].any() and not settled[kinds == "twin"].all()
    # the huge piconet owns a whole group tile boundary and whole waves of the sorted list
    lo, hi = walked.starts[cr.G_HUGE], walked.starts[cr.G_HUGE + 1]
    assert lo < cr.GRP_TILE < hi and hi - lo == 1101


def test_the_placements_are_what_a_search_finds():
    c = cr.crowd()
    found = c.cap.hits()
    assert len(found) == len(c.hits)
    assert set(map(tuple, found.tolist())) == set(map(tuple, c.hits.tolist()))
    assert len(set(zip(c.hits["stream"].tolist(), c.hits["offset"].tolist()))) == len(c.hits)      # distinct (stream, slot) places
    assert (c.hits["offset"] % 625 == 0).all() and (c.hits["ac_errors"] == 0).all()


def test_the_model_has_jobs_on_both_sides_of_the_round():
    recs, _, _ = cr.oracle_records()
    m = cr.model()
    assert m["n_jobs"] == len(m["jobs"]) >= 1400
    assert (m["job_rec"] < cr.SLOT_ROUND).sum() > 500 and (m["job_rec"] >= cr.SLOT_ROUND).sum() > 500
    assert m["job_rec"].tolist() == np.nonzero(recs["settled_by"])[0].tolist()
    j0 = int((m["job_rec"] < cr.SLOT_ROUND).sum())
    assert m["job_rec"][j0 - 1] == 1023 and m["job_rec"][j0] == 1024          # the last job of round 0, the first of round 1
    jh, jl = (m["job_rec"].tolist().index(g) for g in (cr.G_HUGE, cr.G_LONG))
    assert (m["jobs"]["n_obs"][jh], m["jobs"]["n_obs"][jl]) == (1024, 151)
    assert m["n_obs"] == int(np.minimum(cr.runs(recs, cr.oracle_records()[2]), 1024).sum())
    # a prefix: the same jobs, cut
    few = cr.model(rec_cap=1025)
    assert few["n_jobs"] == j0 + 1 and few["jobs"].tobytes() == m["jobs"][:j0 + 1].tobytes()


def _one_piece_model(engine, cap, hits, recs, clkn0, clk_phase=0, max_length=bt.MAX_SYMBOLS, flags=0, max_obs=1024, job_cap=None):
    """aq.model as it was before the header pass was split off, kept to compare with"""
    hits = np.asarray(hits)
    order = np.lexsort((hits["stream"], hits["offset"], hits["lap"]))
    laps = hits["lap"][order]
    starts = np.concatenate([[0], np.nonzero(np.diff(laps.astype(np.int64)))[0] + 1, [len(order)]]) if len(order) else np.zeros(1, int)
    cfgs, clk6, obs, job_rec, oh = [], [], [], [], []
    n_jobs = 0
    for g, r in enumerate(recs):
        group = order[starts[g]:starts[g + 1]]
        lap = int(r["lap"])
        assert int(hits["lap"][group[0]]) == lap and len(group) == r["n_packets"]
        if not r["settled_by"]:
            continue
        n_jobs += 1
        if job_cap is not None and n_jobs > job_cap:
            continue
        walked, clocks = [], {}
        for k in group:
            h = hits[k]
            st = int(h["stream"])
            ch = st if cap.channels is None else int(cap.channels[st])
            clkn = (clkn0 + (int(h["offset"]) + clk_phase) // cap.clk_div) & 0xFFFFFFFF
            p = engine.packet(lap, int(h["ac_errors"]), sv.packet_symbols(cap, h, max_length), ch, clkn)
            if engine.header_present(p):
                walked.append(int(k))
                clocks[int(k)] = (clkn, ch)
            engine.free_packet(p)
        first = int(r["n_walked"]) - int(r["packets_observed"])
        assert 0 <= first < int(r["n_walked"]) <= len(walked)
        assert walked[int(r["n_walked"]) - 1] == r["settled_hit"]
        run = walked[first:][:max_obs]
        t0 = clocks[run[0]][0]
        assert t0 == r["first_pkt_time"]
        off = np.array([(clocks[k][0] - t0) & 0xFFFFFFFF for k in run], dtype=np.uint32).view(np.int32)
        obs.append((off, np.array([clocks[k][1] for k in run], dtype=np.uint8)))
        oh.append(np.array(run, dtype=np.uint32))
        cfgs.append(bt.hop_cfg(lap, int(r["uap"]), r["afh_map"] if flags & aq.JOBS_AFH else None))
        clk6.append((int(r["clk_offset"]) + t0) & 63)
        job_rec.append(g)
    jobs, offsets, channels = bt.clock_jobs(cfgs, clk6 if clk6 else 0, obs, aliased=bool(flags & aq.JOBS_ALIASED))
    return dict(n_jobs=n_jobs, jobs=jobs, job_rec=np.array(job_rec, dtype=np.uint32), offsets=offsets, channels=channels,
                obs_hits=np.concatenate(oh) if oh else np.zeros(0, np.uint32), n_obs=len(offsets))


def test_the_split_model_equals_the_one_piece_model():
    cap, kw = sv.capture_multi()
    hits = cap.hits()
    engine = sv.OracleEngine()
    recs, _ = sv.expected(engine, cap, hits, kw["clkn0"], kw["clk_phase"])
    shared = aq.Walked(engine, cap, hits, kw["clkn0"], kw["clk_phase"])
    n_jobs = int((recs["settled_by"] != 0).sum())
    assert n_jobs >= 8
    variations = [dict(), dict(flags=aq.JOBS_AFH | aq.JOBS_ALIASED), dict(job_cap=1), dict(job_cap=n_jobs - 1), dict(max_obs=1),
                  dict(max_obs=2), dict(n=len(recs) // 2)]
    for opts in variations:
        opts = dict(opts)
        some = recs[:opts.pop("n", len(recs))]
        want = _one_piece_model(engine, cap, hits, some, kw["clkn0"], kw["clk_phase"], **opts)
        for walked in (None, shared):                                   # the existing signature, and the shared header pass
            got = aq.model(engine, cap, hits, some, kw["clkn0"], kw["clk_phase"], walked=walked, **opts)
            assert got.keys() == want.keys() and got["n_jobs"] == want["n_jobs"] and got["n_obs"] == want["n_obs"], opts
            for name in ("jobs", "job_rec", "offsets", "channels", "obs_hits"):
                assert got[name].dtype == want[name].dtype and got[name].tobytes() == want[name].tobytes(), (opts, name)
