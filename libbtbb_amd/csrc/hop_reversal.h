// hop_reversal.h -- the single-piconet CLK1-27 reversal: the candidate list of btbbx_hop_reversal_open and the winnowing
// calls on it.  Candidate lists stay in HBM in ascending order (as the reference keeps them) through ballot masks + a
// prefix over mask words + an ordered scatter.
#pragma once
#include "hop_core.h"

// init_candidates: item j is the clock known6 + 64 j; one ballot word per wave
__global__ __launch_bounds__(256) void hop_candidate_mask_kernel(HopArgs h, uint32_t known6, int channel, int aliased,
								  uint64_t *masks)
{
	__shared__ uint8_t tab[HOP_TAB];
	hop_build_tab<256>(tab, h.bank, h.mod);
	const uint32_t j = blockIdx.x * 256 + threadIdx.x;         // grid covers exactly HOP_GROUPS
	const int ch = hop_observable(tab[hop_tab_index(h, known6 + 64u * j)], aliased);
	const uint64_t m = __ballot(ch == channel);
	if ((threadIdx.x & 63) == 0)
		masks[j >> 6] = m;
}

// exclusive prefix of popcounts over the mask words; one workgroup
__global__ __launch_bounds__(1024) void hop_mask_prefix_kernel(const uint64_t *masks, uint32_t nwords, uint32_t *prefix,
								uint32_t *total)
{
	__shared__ uint32_t part[1024];
	const uint32_t per = (nwords + 1023) / 1024;
	const uint32_t lo = threadIdx.x * per, hi = min(lo + per, nwords);
	uint32_t sum = 0;
	for (uint32_t w = lo; w < hi; w++)
		sum += __popcll(masks[w]);
	part[threadIdx.x] = sum;
	__syncthreads();
	hop_block_scan(part);
	uint32_t run = part[threadIdx.x] - sum;
	for (uint32_t w = lo; w < hi; w++) {
		prefix[w] = run;
		run += __popcll(masks[w]);
	}
	if (threadIdx.x == 1023)
		*total = part[1023];
}

// ordered scatter: src == nullptr -> the value of item i is base + 64 i
__global__ __launch_bounds__(256) void hop_scatter_kernel(const uint64_t *masks, const uint32_t *prefix, uint32_t nwords,
							   const uint32_t *src, uint32_t base, uint32_t *dst)
{
	const uint32_t w = blockIdx.x * 256 + threadIdx.x;
	if (w >= nwords)
		return;
	uint64_t m = masks[w];
	uint32_t o = prefix[w];
	while (m) {
		const uint32_t i = w * 64 + (uint32_t)__builtin_ctzll(m);
		m &= m - 1;
		dst[o++] = src ? src[i] : base + 64u * i;
	}
}

// per candidate: how many of the observations it agrees with before the first mismatch
__global__ __launch_bounds__(256) void hop_winnow_kernel(HopArgs h, const uint32_t *cand, uint32_t n, const HopObs *obs,
							  uint32_t n_obs, int aliased, uint16_t *agree, uint32_t *hist)
{
	__shared__ uint8_t tab[HOP_TAB];
	__shared__ uint32_t lhist[HOP_MAX_OBS + 1];
	for (uint32_t i = threadIdx.x; i <= n_obs; i += 256)
		lhist[i] = 0;
	hop_build_tab<256>(tab, h.bank, h.mod);
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i < n) {
		const uint32_t k = hop_agree(h, tab, obs, n_obs, aliased, cand[i]);
		agree[i] = (uint16_t)k;
		atomicAdd(&lhist[k], 1u);
	}
	__syncthreads();
	for (uint32_t k = threadIdx.x; k <= n_obs; k += 256)
		if (lhist[k])
			atomicAdd(&hist[k], lhist[k]);
}

struct WinnowVerdict {
	uint32_t stop;        // observations applied before the one that left <= 1 candidate (n_obs if none)
	uint32_t count;       // candidates left after that one (or after all)
	uint32_t keep_above;  // survivors are the candidates with agree > keep_above
	uint32_t cand0;       // first survivor (filled by the scatter pass)
};

// hist[k] = candidates whose first mismatch is observation k (k = n_obs: none)
__global__ __launch_bounds__(1024) void hop_verdict_kernel(const uint32_t *hist, uint32_t n, uint32_t n_obs, WinnowVerdict *v)
{
	__shared__ uint32_t cum[1024];
	__shared__ uint32_t first;
	const uint32_t k = threadIdx.x;
	if (k == 0)
		first = n_obs;
	cum[k] = k < n_obs ? hist[k] : 0;
	__syncthreads();
	hop_block_scan(cum);
	uint32_t stop, last;
	hop_verdict(cum, n, n_obs, &first, stop, last);
	if (k == 0) {
		v->stop = stop;
		v->keep_above = last;
		v->count = hop_left_after(cum, n, last);
		v->cand0 = 0;
	}
}

__global__ __launch_bounds__(256) void hop_agree_mask_kernel(const uint16_t *agree, uint32_t n, const WinnowVerdict *v,
							      uint64_t *masks)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;         // grid covers ceil(n / 64) whole words
	const uint64_t m = __ballot(i < n && agree[i] > v->keep_above);
	if ((threadIdx.x & 63) == 0)
		masks[i >> 6] = m;
}

// One workgroup does a whole winnowing call for short lists (the common case after the first
// observed hop): agreement counts, verdict and ordered compaction in a single launch.
#define HOP_SMALL_N 16384
__global__ __launch_bounds__(1024) void hop_winnow_small_kernel(HopArgs h, const uint32_t *cand, uint32_t n,
								 const HopObs *obs, uint32_t n_obs, int aliased,
								 uint32_t *dst, WinnowVerdict *v)
{
	__shared__ uint8_t tab[HOP_TAB];
	__shared__ uint16_t agree[HOP_SMALL_N];
	__shared__ uint32_t cum[1024];
	__shared__ uint32_t wave_cnt[16];
	__shared__ uint32_t first, base;
	const uint32_t tid = threadIdx.x;
	cum[tid] = 0;
	if (tid == 0) {
		first = n_obs;
		base = 0;
	}
	hop_build_tab<1024>(tab, h.bank, h.mod);
	for (uint32_t i = tid; i < n; i += 1024) {
		const uint32_t k = hop_agree(h, tab, obs, n_obs, aliased, cand[i]);
		agree[i] = (uint16_t)k;
		if (k < n_obs)
			atomicAdd(&cum[k], 1u);                 // first mismatch at observation k
	}
	__syncthreads();
	hop_block_scan(cum);
	uint32_t stop, keep;
	hop_verdict(cum, n, n_obs, &first, stop, keep);
	for (uint32_t i0 = 0; i0 < n; i0 += 1024) {                 // ordered compaction, 1024 at a time
		const uint32_t i = i0 + tid;
		const bool live = i < n && agree[i] > keep;
		const uint32_t at = hop_emit_step(live, wave_cnt, &base);
		if (live)
			dst[at] = cand[i];
	}
	if (tid == 0) {
		v->stop = stop;
		v->keep_above = keep;
		v->count = hop_left_after(cum, n, keep);
		v->cand0 = 0;
	}
}

// cand0 of the verdict, read after the compaction on the same stream
__global__ void hop_first_kernel(const uint32_t *cand, WinnowVerdict *v)
{
	if (v->count)
		v->cand0 = cand[0];
}

