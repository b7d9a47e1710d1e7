// follow.h -- the FOLLOWING stage for every piconet of a capture at once (btbbx_follow_hits_device, include/btbbx.h): what
// btbb_process_packet does for a packet of an acquired piconet (bluetooth_piconet.c:872-881) -- the piconet's UAP, the
// piconet-aligned clock, CLK6_VALID | CLK27_VALID, decode -- for a whole hit list behind the acquisition chain, plus the
// check of the packet's channel against the hop selection at that clock.  Included by survey.hip.
//
//   follow_stage_kernel   one thread per record: its job (a binary search of the ascending d_job_rec), its stage from the job's
//                         result and settled_by, and the record's summary with zeroed counters
//   follow_clock_kernel   one thread per hit: the record of its LAP (a binary search of the lap field, 64-byte stride), stage and
//                         job from the summary the pass above wrote, the clock, d_in and d_follow; a stage-2 hit also reads its
//                         job's hop configuration and selects the channel with the reversal's own code (hop_core.h)
//   follow_tally_kernel   behind the decoder, one thread per hit: the counters and the LT_ADDR mask of its record, by integer
//                         atomics (every field is order-independent); a wave whose hits all belong to one record sends one
//                         atomic per counter that changed
//
// No LDS, no scratch, nothing of its own in HBM: d_in is the only intermediate and is the caller's.  The kernels are not named
// after the survey, the builder or the hop families: their resource tests count kernels by those parts of their names.
#pragma once
#include "hop_core.h"

#define FW_THREADS    256
#define FW_NONE       0xffffffffu
#define FW_CLK27_MASK (BTBBX_SEQUENCE_LENGTH - 1)
#define FWF_CLK27_VALID (1u << 5)          // BTBB_CLK27_VALID (include/btbb.h)

static_assert(sizeof(btbbx_follow_pkt) == 16 && offsetof(btbbx_follow_pkt, job) == 12, "btbbx_follow_pkt layout (libbtbb_amd.FOLLOW_PKT_DTYPE)");
static_assert(sizeof(btbbx_follow_sum) == 32 && offsetof(btbbx_follow_sum, lt_addr_mask) == 28, "btbbx_follow_sum layout (libbtbb_amd.FOLLOW_SUM_DTYPE)");
static_assert(offsetof(btbbx_clock_job, aliased) == 92 && offsetof(btbbx_hop_cfg, used_channels) == 5, "btbbx_clock_job as words");

// min(*d_count, cap); a null pointer means the cap
__device__ __forceinline__ uint32_t fw_count(const uint32_t *d_count, uint32_t cap)
{
	return d_count ? min(*d_count, cap) : cap;
}

__global__ __launch_bounds__(FW_THREADS) void follow_stage_kernel(const uint32_t *recs, const uint32_t *d_rec_count, uint32_t rec_cap,
								   const uint32_t *job_rec, const btbbx_clock_result *results,
								   const uint32_t *d_n_jobs, uint32_t job_cap, btbbx_follow_sum *sums)
{
	const uint32_t n_recs = fw_count(d_rec_count, rec_cap), n_jobs = job_cap ? fw_count(d_n_jobs, job_cap) : 0;
	const uint32_t g = blockIdx.x * FW_THREADS + threadIdx.x;
	if (g >= n_recs)
		return;
	uint32_t lo = 0, hi = n_jobs;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (job_rec[mid] < g)
			lo = mid + 1;
		else
			hi = mid;
	}
	btbbx_follow_sum s;
	s.job = lo < n_jobs && job_rec[lo] == g ? lo : FW_NONE;
	s.stage = recs[(size_t)g * AQ_REC_WORDS + 2] >> 24 ? 1 : 0;                 // settled_by
	if (s.job != FW_NONE && results[s.job].status == 0 && results[s.job].count == 1)
		s.stage = 2;
	s.n_hits = s.n_header = s.n_payload = s.n_on_hop = s.n_off_hop = s.lt_addr_mask = 0;
	sums[g] = s;
}

// the channel job `jw` (a btbbx_clock_job as words) hops to at CLK1-27 = clkn, as the reversal's agreement walk selects and
// compares it (hop_agree); 0xff for a configuration the batch reversal rejects (AFH over 0 or more than 79 channels)
__device__ __forceinline__ uint32_t fw_hop_channel(const uint32_t *jw, uint32_t clkn)
{
	const uint32_t afh = jw[1] & 0xff, used = (jw[1] >> 8) & 0xff;
	if (afh && (used == 0 || used > HOP_NCHAN))
		return 0xff;
	HopArgs h;
	hop_address_fields(jw[0], afh, used, &h);
	const uint8_t *bank = (const uint8_t *)(jw + 2);
	return (uint32_t)hop_observable(bank[hop_tab_index(h, clkn) % h.mod], (int)jw[23]);
}

__global__ __launch_bounds__(FW_THREADS) void follow_clock_kernel(const btbbx_hit *hits, const uint32_t *d_count, uint32_t cap,
								   const uint32_t *recs, const uint32_t *d_rec_count, uint32_t rec_cap,
								   const btbbx_clock_job *jobs, const btbbx_clock_result *results,
								   const btbbx_follow_sum *sums, SurveyChannels table, int identity,
								   uint32_t n_streams, btbbx_pkt_in entry, uint32_t clk_div, uint32_t clk_phase,
								   btbbx_pkt_in *d_in, btbbx_follow_pkt *d_follow)
{
	const uint32_t n = fw_count(d_count, cap), n_recs = fw_count(d_rec_count, rec_cap);
	const uint32_t i = blockIdx.x * FW_THREADS + threadIdx.x;
	if (i >= n)
		return;
	const btbbx_hit h = hits[i];
	const uint32_t c = entry.clkn + (uint32_t)((h.offset + clk_phase) / clk_div);
	uint32_t lo = 0, hi = n_recs;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (recs[(size_t)mid * AQ_REC_WORDS] < h.lap)
			lo = mid + 1;
		else
			hi = mid;
	}
	const bool known = lo < n_recs && recs[(size_t)lo * AQ_REC_WORDS] == h.lap;
	btbbx_pkt_in p = entry;
	p.length = 0;
	p.clkn = c;
	btbbx_follow_pkt f;
	f.piconet = known ? lo : FW_NONE;
	f.stage = 0;
	f.channel = h.stream < n_streams ? (identity ? (uint8_t)h.stream : table.ch[h.stream & (SV_CHAN_STREAMS - 1)]) : 0xff;
	f.hop_channel = 0xff;
	f.on_hop = 0;
	f.job = FW_NONE;
	if (known) {
		const uint32_t *rec = recs + (size_t)lo * AQ_REC_WORDS;
		f.stage = (uint8_t)sums[lo].stage;
		f.job = sums[lo].job;
		if (f.stage == 2) {
			p.clkn = (results[f.job].cand0 + c - rec[13]) & FW_CLK27_MASK;
			p.flags |= SVF_UAP_VALID | SVF_CLK6_VALID | FWF_CLK27_VALID;
			p.uap = (uint8_t)rec[2];
			f.hop_channel = (uint8_t)fw_hop_channel((const uint32_t *)&jobs[f.job], p.clkn);
			f.on_hop = f.hop_channel == f.channel;
		} else if (f.stage == 1) {
			p.clkn = (((rec[2] >> 8) & 0xff) + c) & 0x3f;
			p.flags |= SVF_UAP_VALID | SVF_CLK6_VALID;
			p.uap = (uint8_t)rec[2];
		}
	}
	f.clkn = p.clkn;
	d_in[i] = p;
	d_follow[i] = f;
}

__global__ __launch_bounds__(FW_THREADS) void follow_tally_kernel(const btbbx_follow_pkt *d_follow, const btbbx_pkt_out *d_out,
								   const uint32_t *d_count, uint32_t cap, btbbx_follow_sum *sums)
{
	const uint32_t n = fw_count(d_count, cap);
	const uint32_t i = blockIdx.x * FW_THREADS + threadIdx.x;
	uint32_t g = FW_NONE, lt = 0;
	bool header = false, payload = false, on = false, off = false;
	if (i < n) {
		const btbbx_follow_pkt f = d_follow[i];
		g = f.piconet;
		if (g != FW_NONE) {
			header = d_out[i].header_rv != 0;
			payload = d_out[i].payload_rv > 0;
			lt = header ? 1u << (d_out[i].lt_addr & 31) : 0;
			on = f.stage == 2 && f.on_hop;
			off = f.stage == 2 && !f.on_hop;
		}
	}
	const bool mine = g != FW_NONE;
	const uint32_t g0 = __shfl(g, 0, 64);
	if (g0 != FW_NONE && __ballot(g == g0) == ~0ULL) {
		// the whole wave is one record's: the counters are popcounts of ballots, the mask an OR over the lanes
		const uint32_t n_header = __popcll(__ballot(header)), n_payload = __popcll(__ballot(payload));
		const uint32_t n_on = __popcll(__ballot(on)), n_off = __popcll(__ballot(off));
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1)
			lt |= __shfl_xor(lt, d, 64);
		if ((threadIdx.x & 63) == 0) {
			btbbx_follow_sum *s = &sums[g0];
			atomicAdd(&s->n_hits, 64u);
			if (n_header)
				atomicAdd(&s->n_header, n_header);
			if (n_payload)
				atomicAdd(&s->n_payload, n_payload);
			if (n_on)
				atomicAdd(&s->n_on_hop, n_on);
			if (n_off)
				atomicAdd(&s->n_off_hop, n_off);
			if (lt)
				atomicOr(&s->lt_addr_mask, lt);
		}
	} else if (mine) {
		btbbx_follow_sum *s = &sums[g];
		atomicAdd(&s->n_hits, 1u);
		if (header) {
			atomicAdd(&s->n_header, 1u);
			atomicOr(&s->lt_addr_mask, lt);
		}
		if (payload)
			atomicAdd(&s->n_payload, 1u);
		if (on)
			atomicAdd(&s->n_on_hop, 1u);
		if (off)
			atomicAdd(&s->n_off_hop, 1u);
	}
}
