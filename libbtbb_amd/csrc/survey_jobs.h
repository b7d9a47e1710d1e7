// survey_jobs.h -- the job builder: from the records and the scratch of a survey to the job table and the observation
// arrays of the batch CLK1-27 reversal (hop_batch.h), on the device.  Included by survey.hip, whose scratch layout stays there.
//
// A settled record's observations are the header-bearing packets of its LAP from the first packet of the settling run on:
// with W = widx[wpos[gstart[g]] .. wpos[gstart[g + 1]]) the walk stopped at W[n_walked - 1] with packets_observed packets in the
// piconet's pattern memory (a reset consumes its packet without recording it), so the run begins at W[n_walked -
// packets_observed] -- what btbb_init_hop_reversal + btbb_winnow see when the piconet settles (bluetooth_piconet.c:528-531) --
// and every later packet is what try_hop appends (:510-515).
//
//   acquire_slots_kernel   one workgroup walks the records 1024 at a time: settled or not, observations kept, and the
//                          running sums of both (block_exclusive_scan, the carry in registers) -- every job's slot and the
//                          first index of its observations go straight into the job table, the two totals to the caller
//   acquire_fill_kernel    one wave per job: the hop configuration (the loop of btbbx_hop_cfg_init as two ballots and prefix
//                          popcounts), the job record, and a stride over the job's observations
//
// The survey's scratch is only read, and nothing but the caller's outputs is written: the builder has no memory of its own,
// which is why the counting and the scan are one workgroup's loop and not a tile pass per record with tile sums in between
// (records / 1024 rounds of three dependent loads; a capture of 2^16 piconets makes 64 of them).
// The records come as words (16 per record) and the kernels are not named after the survey: its resource test counts the
// survey's kernels by that part of their names.
#pragma once

#define AQ_SLOT_THREADS 1024
#define AQ_SLOT_WAVES   (AQ_SLOT_THREADS / 64)
#define AQ_JOB_WORDS    26                 // sizeof(btbbx_clock_job) / 4
#define AQ_REC_WORDS    16                 // sizeof(btbbx_survey_rec) / 4

static_assert(sizeof(btbbx_clock_job) == 4 * AQ_JOB_WORDS && offsetof(btbbx_clock_job, clk6) == 88 &&
	      offsetof(btbbx_hop_cfg, bank) == 8, "btbbx_clock_job layout");
static_assert(sizeof(btbbx_survey_rec) == 4 * AQ_REC_WORDS && offsetof(btbbx_survey_rec, n_walked) == 28 &&
	      offsetof(btbbx_survey_rec, packets_observed) == 44 && offsetof(btbbx_survey_rec, first_pkt_time) == 52 &&
	      offsetof(btbbx_survey_rec, settled_by) == 11, "btbbx_survey_rec as words");

// records the builder looks at: those the survey stored, those the caller has, those the scratch knows
__device__ __forceinline__ uint32_t aq_records(const uint32_t *d_rec_count, uint32_t rec_cap, const uint32_t *params)
{
	uint32_t n = rec_cap;
	if (d_rec_count)
		n = min(n, *d_rec_count);
	return min(n, params[1]);
}

// The run of record g: *run_first = index into widx of its first observation; returns how many observations are kept
// (0: not settled -- or a record that does not belong to this scratch, which gets no job instead of a read outside widx).
__device__ __forceinline__ uint32_t aq_run(const uint32_t *rec, uint32_t g, uint32_t cap, const uint32_t *gstart, const uint32_t *wpos,
					   uint32_t max_obs, uint32_t *run_first)
{
	const uint32_t settled_by = rec[2] >> 24, n_walked = rec[7], observed = rec[11];
	if (!settled_by)
		return 0;
	const uint32_t wfirst = min(wpos[min(gstart[g], cap)], cap), wend = min(wpos[min(gstart[g + 1], cap)], cap);
	if (wend < wfirst || n_walked > wend - wfirst || observed > n_walked || observed == 0)
		return 0;
	*run_first = wfirst + n_walked - observed;
	return min(wend - *run_first, max_obs);
}

__global__ __launch_bounds__(AQ_SLOT_THREADS) void acquire_slots_kernel(const uint32_t *recs, const uint32_t *d_rec_count, uint32_t rec_cap,
									  uint32_t cap, const uint32_t *params, const uint32_t *gstart,
									  const uint32_t *wpos, uint32_t max_obs, btbbx_clock_job *jobs,
									  uint32_t job_cap, uint32_t *d_n_jobs, uint32_t *job_rec, uint32_t *d_n_obs)
{
	__shared__ uint32_t lds[AQ_SLOT_WAVES];
	__shared__ uint32_t cut;                         // observations in front of the first job that is not stored
	const uint32_t tid = threadIdx.x, n_recs = aq_records(d_rec_count, rec_cap, params);
	uint32_t jobs_before = 0, obs_before = 0;
	for (uint32_t base = 0; base < n_recs; base += AQ_SLOT_THREADS) {
		const uint32_t g = base + tid;
		uint32_t first, kept = 0;
		if (g < n_recs)
			kept = aq_run(recs + (size_t)g * AQ_REC_WORDS, g, cap, gstart, wpos, max_obs, &first);
		uint32_t n_jobs, n_obs;
		const uint32_t slot = jobs_before + block_exclusive_scan<AQ_SLOT_WAVES>(kept ? 1u : 0u, lds, n_jobs);
		const uint32_t obs_first = obs_before + block_exclusive_scan<AQ_SLOT_WAVES>(kept, lds, n_obs);
		if (kept && slot < job_cap) {
			jobs[slot].clk6 = g;                     // (for the fill pass, which puts CLK1-6 there)
			jobs[slot].obs_first = obs_first;
			jobs[slot].n_obs = kept;
			if (job_rec)
				job_rec[slot] = g;
		}
		if (kept && slot == job_cap)
			cut = obs_first;
		jobs_before += n_jobs;
		obs_before += n_obs;
	}
	__syncthreads();
	if (tid == 0) {
		*d_n_jobs = jobs_before;
		if (d_n_obs)
			*d_n_obs = jobs_before > job_cap ? cut : obs_before;
	}
}

__global__ __launch_bounds__(SV_THREADS) void acquire_fill_kernel(const uint32_t *recs, uint32_t cap, const uint32_t *params,
								   const uint32_t *gstart, const uint32_t *wpos, const uint32_t *widx,
								   const btbbx_pkt_in *pin, const btbbx_hit *hits, const uint32_t *vals0,
								   const uint32_t *vals1, SurveyChannels table, int identity, uint32_t flags,
								   uint32_t max_obs, btbbx_clock_job *jobs, uint32_t job_cap, const uint32_t *d_n_jobs,
								   int32_t *index_offsets, uint8_t *channels, uint32_t *obs_hits, uint32_t obs_cap)
{
	__shared__ uint32_t words[SV_WAVES][AQ_JOB_WORDS];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t j = blockIdx.x * SV_WAVES + wave;
	const bool mine = j < min(*d_n_jobs, job_cap);           // (no early return: the barriers below are the workgroup's)
	uint32_t g = 0, obs_first = 0, n_obs = 0, run_first = 0, first_pkt_time = 0;
	if (lane < AQ_JOB_WORDS)
		words[wave][lane] = 0;
	__syncthreads();
	if (mine) {
		g = jobs[j].clk6;
		obs_first = jobs[j].obs_first;
		const uint32_t *rec = recs + (size_t)g * AQ_REC_WORDS;
		n_obs = aq_run(rec, g, cap, gstart, wpos, max_obs, &run_first);      // (= jobs[j].n_obs)
		first_pkt_time = rec[13];
		const uint32_t lap = rec[0], uap = rec[2] & 0xff, clk_offset = (rec[2] >> 8) & 0xff;
		// bank entry i of a full table is channel (2 i) % 79; with a map, the entries whose channel is in use, in that order
		const bool afh = flags & BTBBX_JOBS_AFH;
		const uint32_t c0 = (2 * lane) % 79, c1 = (2 * (lane + 64)) % 79;
		const bool in0 = !afh || ((rec[3 + (c0 >> 5)] >> (c0 & 31)) & 1);
		const bool in1 = lane + 64 < 79 && (!afh || ((rec[3 + (c1 >> 5)] >> (c1 & 31)) & 1));
		const uint64_t m0 = __ballot(in0), m1 = __ballot(in1), below = (1ULL << lane) - 1;
		uint8_t *bank = (uint8_t *)&words[wave][2];
		if (in0)
			bank[__popcll(m0 & below)] = (uint8_t)c0;
		if (in1)
			bank[__popcll(m0) + __popcll(m1 & below)] = (uint8_t)c1;
		if (lane == 0) {
			// used_channels as btbbx_hop_cfg_init counts it: every bit of the ten map bytes
			const uint32_t used = afh ? __popc(rec[3]) + __popc(rec[4]) + __popc(rec[5] & 0xffff) : 79;
			words[wave][0] = ((uap << 24) | lap) & 0xfffffff;
			words[wave][1] = (afh ? 1u : 0u) | (used & 0xff) << 8;
			words[wave][22] = (clk_offset + first_pkt_time) & 0x3f;
			words[wave][23] = flags & BTBBX_JOBS_ALIASED ? 1u : 0u;
			words[wave][24] = obs_first;
			words[wave][25] = n_obs;
		}
	}
	__syncthreads();
	if (!mine)
		return;
	if (lane < AQ_JOB_WORDS)
		((uint32_t *)&jobs[j])[lane] = words[wave][lane];
	const uint32_t *vals = params[2] ? vals1 : vals0;
	for (uint32_t i = lane; i < n_obs; i += 64) {
		const uint32_t at = obs_first + i, idx = widx[run_first + i];
		if (at >= obs_cap || idx >= cap)                      // (cannot happen with the scratch of this list)
			continue;
		const uint32_t stream = hits[idx].stream;
		index_offsets[at] = (int32_t)(pin[idx].clkn - first_pkt_time);
		channels[at] = identity ? (uint8_t)stream : table.ch[stream & (SV_CHAN_STREAMS - 1)];
		if (obs_hits)
			obs_hits[at] = vals[idx];
	}
}
