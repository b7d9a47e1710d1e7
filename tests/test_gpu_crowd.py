"""The crowd capture (tests/_crowd.py: 2301 piconets, 8858 packets) through the device: the survey's list stages over more than
one sort tile and four group tiles, the job builder over three rounds of its 1024-record loop with every cap on both sides of
a round, and the chain into the batch reversal at its coarsest tiling.  The oracle side (the survey loop over the oracle port,
the header pass, the numpy model of the builder) is computed once per process and shared.  Integer logic throughout:
everything must be equal."""
import functools

import numpy as np
import pytest

import _acquire as aq
import _crowd as cr
import _libs
import _survey as sv
import libbtbb_amd as bt

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
BOTH = aq.JOBS_AFH | aq.JOBS_ALIASED
N = cr.N_RECORDS
CHAIN_EVERY = 1                                         # the chain test compares every job with the single-piconet path


@pytest.fixture(scope="module", autouse=True)
def ready():
    bt.init(2)
    yield
    _libs.oracle().orc_hop_cache_clear()


@functools.lru_cache(maxsize=None)
def _words():
    return cr.crowd().cap.words()


def _survey(hits, **opts):
    cap = cr.crowd().cap
    return bt.run_survey_hits(_words(), hits, sv.entry_state(cr.CLKN0), clk_div=cap.clk_div, n_words=cap.n_words, **opts)


def _build(**opts):
    c = cr.crowd()
    return bt.run_survey_clock_jobs(_words(), c.hits, sv.entry_state(cr.CLKN0), clk_div=c.cap.clk_div, n_words=c.cap.n_words,
                                    sentinel=SENTINEL, **opts)


def _jobs():
    """(J = all jobs, J0 = those among records 0..1023, the job of the huge piconet, the job of the long one)"""
    rec = cr.model()["job_rec"]
    return len(rec), int((rec < cr.SLOT_ROUND).sum()), rec.tolist().index(cr.G_HUGE), rec.tolist().index(cr.G_LONG)


# ---- 3a. the survey -----------------------------------------------------------------------------------------------

def test_survey_of_the_crowd_in_list_order_shuffled_and_counted():
    hits = cr.crowd().hits
    want, want_cand, _ = cr.oracle_records()
    n, recs, cand = _survey(hits)
    assert n == N
    sv.assert_records_equal(recs, cand, want, want_cand, "list order")
    # shuffled: settled_hit indexes the list that was handed in, nothing else knows the order
    perm = np.random.default_rng(_libs.seed(7701)).permutation(len(hits))
    where = np.zeros(len(hits), dtype=np.uint32)
    where[perm] = np.arange(len(hits), dtype=np.uint32)
    moved = want.copy()
    has = want["settled_hit"] != 0xFFFFFFFF
    moved["settled_hit"][has] = where[want["settled_hit"][has]]
    assert has.sum() > 1400 and (moved["settled_hit"] != want["settled_hit"]).sum() > 1400
    n, recs, cand = _survey(hits[perm])
    assert n == N
    sv.assert_records_equal(recs, cand, moved, want_cand, "shuffled")
    # the count as a device word below a capacity that asks for more tiles than the list fills
    n, recs, cand = _survey(hits, count=len(hits), cap=len(hits) + 3000)
    assert n == N and len(recs) == N
    sv.assert_records_equal(recs, cand, want, want_cand, "counted")


# ---- 3b. the builder: record rounds -------------------------------------------------------------------------------

_REC_CASES = [(r, r != 1025, 0) for r in cr.REC_CAPS] + [(N, False, 0), (1025, False, BOTH), (N, False, BOTH)]


@pytest.mark.parametrize("rec_cap,rec_count,flags", _REC_CASES)
def test_builder_record_rounds(rec_cap, rec_count, flags):
    want_recs, _, _ = cr.oracle_records()
    want = cr.model(rec_cap=rec_cap, flags=flags)
    out = _build(rec_cap=rec_cap, rec_count=rec_count, flags=flags)
    assert out["n_recs"] == N and len(out["recs"]) == rec_cap
    sv.assert_records_equal(out["recs"], None, want_recs[:rec_cap], None, "rec_cap %d" % rec_cap)
    assert want["n_jobs"] == len(want["jobs"]) == int((want_recs["settled_by"][:rec_cap] != 0).sum())
    aq.assert_builder_equals(out, want, SENTINEL, ("rec_cap", rec_cap, rec_count, flags))
    if flags & aq.JOBS_AFH:
        assert (want["jobs"]["cfg"]["afh"] == 1).all() and (want["jobs"]["aliased"] == 1).all()
        assert (want["jobs"]["cfg"]["used_channels"] == want_recs["used_channels"][want["job_rec"]]).all()


def test_builder_record_rounds_cover_both_ends_of_a_prefix():
    settled = cr.oracle_records()[0]["settled_by"] != 0
    ends = [bool(settled[r - 1]) for r in cr.REC_CAPS]
    assert True in ends and False in ends                               # a prefix that ends on a job, one that ends without
    assert settled[N - 1] and settled[1023] and settled[1024] and settled[2047] and settled[2048]


# ---- 3c. the builder: job cap -------------------------------------------------------------------------------------

def _job_caps():
    J, J0, _, _ = _jobs()
    return [1, J0 - 1, J0, J0 + 1, J - 1, J, J + 1]


@pytest.mark.parametrize("which", range(7))
def test_builder_job_cap(which):
    J, J0, _, _ = _jobs()
    job_cap = _job_caps()[which]
    whole = cr.model()
    want = cr.model(rec_cap=N, job_cap=job_cap)
    out = _build(rec_cap=N, job_cap=job_cap)
    assert out["n_jobs"] == want["n_jobs"] == J and len(want["jobs"]) == min(job_cap, J)
    assert out["n_obs"] == want["n_obs"] == int(whole["jobs"]["n_obs"][:job_cap].sum())
    if job_cap == J0:
        # the first job that is not stored is the first job of round 1: its slot and the observations in front of it are the
        # carries of round 0 alone
        assert whole["job_rec"][J0 - 1] == cr.SLOT_ROUND - 1 and whole["job_rec"][J0] == cr.SLOT_ROUND
        assert want["n_obs"] == whole["jobs"]["obs_first"][J0] > 0
    aq.assert_builder_equals(out, want, SENTINEL, ("job_cap", job_cap))       # (nothing behind the stored jobs and observations)


# ---- 3d. the builder: max_obs -------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_obs", [1, 63, 64, 65, 128, 1024])
def test_builder_max_obs(max_obs):
    J, J0, huge, long_ = _jobs()
    want = cr.model(rec_cap=N, max_obs=max_obs)
    out = _build(rec_cap=N, max_obs=max_obs)
    aq.assert_builder_equals(out, want, SENTINEL, ("max_obs", max_obs))
    assert want["jobs"]["n_obs"].max() == max_obs
    if max_obs == 1024:
        assert out["jobs"]["n_obs"][huge] == want["jobs"]["n_obs"][huge] == 1024
        assert out["jobs"]["n_obs"][long_] == 151
    if max_obs == 65:
        assert out["jobs"]["n_obs"][long_] == want["jobs"]["n_obs"][long_] == 65 < 151


# ---- 3e. the chain ------------------------------------------------------------------------------------------------

def test_chain_into_the_batch_reversal_at_full_size():
    """job_cap = the record count: the batch reversal takes 16 tiles per job, its coarsest tiling."""
    J, J0, huge, long_ = _jobs()
    want = cr.model(rec_cap=N)
    out = _build(rec_cap=N, reversal=True)
    aq.assert_builder_equals(out, want, SENTINEL, "chain")
    res = out["results"]
    assert len(res) == N and (res[J:].view(np.uint8) == SENTINEL).all()
    assert (res["status"][:J] == 0).all() and (res["n_stored"][:J] == 0).all()
    named = {0, J0 - 1, J0, J - 1, huge, long_}
    compared = sorted(set(range(0, J, CHAIN_EVERY)) | named)
    assert len(compared) >= 200
    for j in compared:
        job = want["jobs"][j]
        lo, n = int(job["obs_first"]), int(job["n_obs"])
        off, ch = want["offsets"][lo:lo + n], want["channels"][lo:lo + n]
        rev = bt.HopReversal(bt.HopCfg.from_buffer_copy(job["cfg"].tobytes()), int(job["clk6"]), int(ch[0]), False)
        n_initial = rev.count
        stop, count, cand0 = rev.winnow(off, ch)
        rev.close()
        r = res[j]
        assert (int(r["n_initial"]), int(r["stop"]), int(r["count"]), int(r["cand0"])) == (n_initial, stop, count, cand0 if count else 0), \
            (j, int(want["job_rec"][j]), r)
    assert want["jobs"]["n_obs"][huge] == 1024 and want["jobs"]["n_obs"][long_] == 151
