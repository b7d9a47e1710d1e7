// hop_batch.h -- the batch CLK1-27 reversal: many piconets in one chain of three kernels (btbbx_hop_reversal_batch_device).
// Job j leaves what open + winnow + candidates of the single path leave, but nothing about a job is known on the host: the
// jobs, their count and their observations are device data.  So no candidate list is kept.  The agreement count of a clock
// (observations matched before the first mismatch) is a pure function of the clock; pass 1 evaluates it for all 2^21 clocks
// congruent to clk6 and keeps only a histogram over it, with the smallest clock of every bin; pass 2 reads the verdict off
// the histogram with the hop_verdict that hop_verdict_kernel uses; pass 3 evaluates again for the jobs that are asked for
// more than one candidate.  Scratch per job: the two rows of HOP_BINS words and the verdict's threshold.
#pragma once
#include "hop_core.h"

#define HOP_BINS 1028             // HOP_MAX_OBS + 1 bins, rounded up to 16 bytes
static_assert(sizeof(btbbx_clock_job) == 104 && offsetof(btbbx_clock_job, clk6) == 88, "btbbx_clock_job layout");
static_assert(sizeof(btbbx_clock_result) == 24, "btbbx_clock_result layout");

__device__ __forceinline__ uint32_t batch_job_count(const uint32_t *n_jobs, uint32_t job_cap)
{
	return n_jobs ? min(*n_jobs, job_cap) : job_cap;
}

// the rules of include/btbbx.h; a job that fails one is never worked on
__device__ __forceinline__ bool batch_job_ok(const btbbx_clock_job &j, uint32_t n_obs_total)
{
	if (j.clk6 > 63 || j.n_obs == 0 || j.n_obs > HOP_MAX_OBS)
		return false;
	if (j.obs_first > n_obs_total || j.n_obs > n_obs_total - j.obs_first)      // obs_first + n_obs without wrapping
		return false;
	return !j.cfg.afh || (j.cfg.used_channels >= 1 && j.cfg.used_channels <= HOP_NCHAN);
}

// observations [0, n) of a job into LDS, channels as the reference's signed chars
__device__ __forceinline__ void batch_stage_obs(HopObs *obs, const int32_t *offsets, const uint8_t *channels, uint32_t first,
						uint32_t n)
{
	for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
		obs[i].offset = offsets[first + i];
		obs[i].channel = (int)(int8_t)channels[first + i];
	}
}

// Pass 1.  Workgroup = (job, tile of the 2^21 groups); a lane takes the clocks clk6 + 64 g of its tile, 256 groups apart.
// rows[job][0][k] += candidates whose first mismatch is observation k (k = n_obs: none); rows[job][1][k] = the complement of
// the smallest such clock (a maximum, so that one memset to zero prepares both rows; a clock is below 2^27, its complement
// is never 0).
__global__ __launch_bounds__(256) void hop_batch_agree_kernel(const btbbx_clock_job *jobs, const uint32_t *n_jobs, uint32_t job_cap,
							       uint32_t tiles_log2, const int32_t *offsets, const uint8_t *channels,
							       uint32_t n_obs_total, uint32_t *rows)
{
	__shared__ uint8_t tab[HOP_TAB];
	__shared__ HopObs obs[HOP_MAX_OBS];
	__shared__ uint32_t lhist[HOP_MAX_OBS + 1], lfirst[HOP_MAX_OBS + 1];
	const uint32_t job = blockIdx.x >> tiles_log2, tile = blockIdx.x & ((1u << tiles_log2) - 1);
	if (job >= batch_job_count(n_jobs, job_cap))
		return;
	const btbbx_clock_job &j = jobs[job];
	if (!batch_job_ok(j, n_obs_total))
		return;
	const uint32_t n_obs = j.n_obs, clk6 = j.clk6;
	const int aliased = j.aliased != 0;
	HopArgs h;
	hop_address_fields(j.cfg.address, j.cfg.afh, j.cfg.used_channels, &h);
	batch_stage_obs(obs, offsets, channels, j.obs_first, n_obs);
	for (uint32_t k = threadIdx.x; k <= n_obs; k += 256) {
		lhist[k] = 0;
		lfirst[k] = 0;
	}
	hop_build_tab<256>(tab, j.cfg.bank, h.mod);
	const int ch0 = obs[0].channel;                         // open(): the candidates are the clocks that hop on ch[0]
	const uint32_t per = HOP_GROUPS >> tiles_log2;          // a multiple of 256
	for (uint32_t g = tile * per + threadIdx.x; g < (tile + 1) * per; g += 256) {
		const uint32_t c = clk6 + 64u * g;
		if (hop_observable(tab[hop_tab_index(h, c)], aliased) != ch0)
			continue;
		const uint32_t k = hop_agree(h, tab, obs, n_obs, aliased, c);
		atomicAdd(&lhist[k], 1u);
		atomicMax(&lfirst[k], ~c);
	}
	__syncthreads();
	uint32_t *hist = rows + (size_t)job * 2 * HOP_BINS;
	for (uint32_t k = threadIdx.x; k <= n_obs; k += 256)
		if (lhist[k]) {
			atomicAdd(&hist[k], lhist[k]);
			atomicMax(&hist[HOP_BINS + k], lfirst[k]);
		}
}

// Pass 2.  One workgroup per job: stop / count / keep_above as hop_verdict_kernel takes them from the histogram, n_initial = its
// total, cand0 = the smallest clock over the bins above keep_above.  Writes the whole result record -- for a rejected job too --
// and the only candidate of a job that ends with one.
__global__ __launch_bounds__(1024) void hop_batch_verdict_kernel(const btbbx_clock_job *jobs, const uint32_t *n_jobs, uint32_t job_cap,
								  uint32_t n_obs_total, const uint32_t *rows, uint32_t *keep_above,
								  btbbx_clock_result *results, uint32_t *candidates, uint32_t cand_cap)
{
	__shared__ uint32_t cum[1024];
	__shared__ uint32_t first, best;
	const uint32_t job = blockIdx.x, k = threadIdx.x;
	if (job >= batch_job_count(n_jobs, job_cap))
		return;
	const btbbx_clock_job &j = jobs[job];
	btbbx_clock_result r = {1, 0, 0, 0, 0, 0};
	if (!batch_job_ok(j, n_obs_total)) {
		if (k == 0)
			results[job] = r;
		return;
	}
	const uint32_t n_obs = j.n_obs;
	const uint32_t *hist = rows + (size_t)job * 2 * HOP_BINS, *lowest = hist + HOP_BINS;
	if (k == 0) {
		first = n_obs;
		best = 0;
	}
	cum[k] = k < n_obs ? hist[k] : 0;
	__syncthreads();
	hop_block_scan(cum);
	const uint32_t n = cum[1023] + hist[n_obs];             // every candidate of open()
	uint32_t stop, last;
	hop_verdict(cum, n, n_obs, &first, stop, last);
	if (k > last && k < n_obs && lowest[k])
		atomicMax(&best, lowest[k]);
	if (k == 0 && lowest[n_obs])                            // bin n_obs has no lane of its own when n_obs = 1024
		atomicMax(&best, lowest[n_obs]);
	__syncthreads();
	if (k == 0) {
		const bool store = candidates && cand_cap;
		r.status = 0;
		r.n_initial = n;
		r.stop = stop;
		r.count = hop_left_after(cum, n, last);
		r.cand0 = r.count ? ~best : 0;
		r.n_stored = store ? min(r.count, cand_cap) : 0;
		results[job] = r;
		keep_above[job] = last;
		if (store && r.count == 1)
			candidates[(size_t)job * cand_cap] = r.cand0;
	}
}

// Pass 3, when candidates are asked for.  One workgroup per job that ended with more than one: the survivors are the clocks
// that agree with observations 0 .. keep_above; they are found again, 1024 groups at a time in ascending order, and
// written through wave ballots and a prefix over the per-wave counts until min(count, cand_cap) are out.
__global__ __launch_bounds__(1024) void hop_batch_emit_kernel(const btbbx_clock_job *jobs, const uint32_t *n_jobs, uint32_t job_cap,
							       const int32_t *offsets, const uint8_t *channels,
							       const uint32_t *keep_above, const btbbx_clock_result *results,
							       uint32_t *candidates, uint32_t cand_cap)
{
	__shared__ uint8_t tab[HOP_TAB];
	__shared__ HopObs obs[HOP_MAX_OBS];
	__shared__ uint32_t wave_cnt[16];
	__shared__ uint32_t base;
	const uint32_t job = blockIdx.x, tid = threadIdx.x;
	if (job >= batch_job_count(n_jobs, job_cap))
		return;
	if (results[job].status || results[job].count <= 1)     // rejected, or pass 2 wrote what there was
		return;
	const btbbx_clock_job &j = jobs[job];
	const uint32_t limit = min(results[job].count, cand_cap), need = keep_above[job] + 1, clk6 = j.clk6;
	const int aliased = j.aliased != 0;
	HopArgs h;
	hop_address_fields(j.cfg.address, j.cfg.afh, j.cfg.used_channels, &h);
	batch_stage_obs(obs, offsets, channels, j.obs_first, need);
	if (tid == 0)
		base = 0;
	hop_build_tab<1024>(tab, j.cfg.bank, h.mod);
	const int ch0 = obs[0].channel;
	uint32_t *dst = candidates + (size_t)job * cand_cap;
	for (uint32_t g0 = 0; g0 < HOP_GROUPS; g0 += 1024) {
		const uint32_t c = clk6 + 64u * (g0 + tid);
		const bool live = hop_observable(tab[hop_tab_index(h, c)], aliased) == ch0 &&
				  hop_agree(h, tab, obs, need, aliased, c) == need;
		const uint32_t at = hop_emit_step(live, wave_cnt, &base);
		if (live && at < limit)
			dst[at] = c;
		if (base >= limit)                              // the same for every lane: the rest is past cand_cap
			break;
	}
}
