// hop_core.h -- what the hop kernel families share: the selection inputs of an address, the index into the bank table, and
// the workgroup pieces of the CLK1-27 reversal (table build, agreement walk, block scan, verdict, ordered emit), which the
// single-piconet path (hop_reversal.h) and the batch path (hop_batch.h) promise the same results from.
#pragma once
#include "common.h"

#define HOP_NCHAN   79
#define HOP_TAB     272          // perm (<32) + e (<128) + f (<79) + 32 = at most 268
#define HOP_GROUPS  (1u << 21)   // values of CLK7-27 = groups of 64 hops
#define HOP_MAX_OBS 1024

struct HopArgs {
	uint32_t a1, b, c1, d1, e;
	uint32_t mod;                // 79, or used_channels under AFH
	uint32_t afh;
	uint8_t bank[80];
};

struct HopObs {                   // one observed hop: clock distance to the first packet, channel
	int32_t offset;
	int32_t channel;              // as the reference's `char channel`: > 127 never matches
};

// butterfly stage s exchanges wires (hop_u(s), hop_v(s)); spec vol 2 part B 2.6.2.3
__device__ __host__ constexpr int hop_u(int s) { constexpr int u[14] = {0, 2, 1, 3, 0, 1, 0, 3, 1, 0, 2, 1, 0, 1}; return u[s]; }
__device__ __host__ constexpr int hop_v(int s) { constexpr int v[14] = {1, 3, 2, 4, 4, 3, 2, 4, 4, 3, 4, 3, 3, 2}; return v[s]; }

// the selection inputs of an address (address_precalc, bluetooth_piconet.c:197-217); the bank is not touched.
// Host (hop_args) and device (the batch reversal derives them per job) share it.
__device__ __host__ inline void hop_address_fields(uint32_t address, uint32_t afh, uint32_t used_channels, HopArgs *h)
{
	address &= 0xfffffff;
	h->a1 = (address >> 23) & 0x1f;
	h->b = (address >> 19) & 0x0f;
	h->d1 = (address >> 10) & 0x1ff;
	h->c1 = 0;
	h->e = 0;
	for (int i = 0; i < 5; i++)
		h->c1 |= ((address >> (2 * i)) & 1) << i;
	for (int i = 0; i < 7; i++)
		h->e |= ((address >> (2 * i + 1)) & 1) << i;
	h->afh = afh ? 1 : 0;
	h->mod = afh ? used_channels : HOP_NCHAN;
}

// tab[i] = bank[i % mod] for the HOP_TAB entries of the table in LDS, by a workgroup of LANES = its launch bound (the
// compiler does not drop the guard of a 256-lane kernel by itself); barrier included
template <int LANES> __device__ __forceinline__ void hop_build_tab(uint8_t *tab, const uint8_t *bank, uint32_t mod)
{
	static_assert(LANES >= 256, "the first 256 lanes fill the table");
	if (LANES == 256 || threadIdx.x < 256) {
		tab[threadIdx.x] = bank[threadIdx.x % mod];
		if (threadIdx.x < HOP_TAB - 256)
			tab[256 + threadIdx.x] = bank[(256 + threadIdx.x) % mod];
	}
	__syncthreads();
}

// index into tab for CLK1-27 value idx: perm5 output + e + f (+32 for odd clocks)
__device__ __forceinline__ uint32_t hop_tab_index(const HopArgs &h, uint32_t idx)
{
	const uint32_t y1 = idx & 1, x = (idx >> 1) & 31, t = idx >> 6;
	const uint32_t a = h.a1 ^ ((t >> 14) & 31);
	const uint32_t c = h.c1 ^ ((t >> 9) & 31) ^ (y1 ? 31u : 0u);
	const uint32_t ctl = (c << 9) | (h.d1 ^ (t & 511));
	uint32_t z = ((x + a) & 31) ^ h.b;
#pragma unroll
	for (int s = 13; s >= 0; s--) {
		const uint32_t sw = ((z >> hop_u(s)) ^ (z >> hop_v(s))) & (ctl >> s) & 1;
		z ^= (sw << hop_u(s)) | (sw << hop_v(s));
	}
	uint32_t f = (16u * t) % HOP_NCHAN;
	if (h.afh)
		f %= h.mod;                           // gen_hops' f_dash (:355), not single_hop's
	return z + h.e + f + 32u * y1;
}

__device__ __forceinline__ int hop_observable(uint32_t ch, int aliased)
{
	return aliased ? (int)((ch + 24) % 25) + 26 : (int)ch;
}

// observations clock c agrees with before its first mismatch, at most `upto`; obs in global memory or in LDS
__device__ __forceinline__ uint32_t hop_agree(const HopArgs &h, const uint8_t *tab, const HopObs *obs, uint32_t upto, int aliased,
					      uint32_t c)
{
	uint32_t k = 0;
	for (; k < upto; k++) {
		const HopObs o = obs[k];
		const uint32_t idx = (c + (uint32_t)o.offset) & (BTBBX_SEQUENCE_LENGTH - 1);
		if (hop_observable(tab[hop_tab_index(h, idx)], aliased) != o.channel)
			break;
	}
	return k;
}

// inclusive scan of a[0 .. 1024) in LDS by 1024 lanes (Hillis-Steele); a[] is behind a barrier on entry and on return
__device__ __forceinline__ void hop_block_scan(uint32_t *a)
{
	for (uint32_t step = 1; step < 1024; step <<= 1) {
		const uint32_t v = threadIdx.x >= step ? a[threadIdx.x - step] : 0;
		__syncthreads();
		a[threadIdx.x] += v;
		__syncthreads();
	}
}

// cum[] = the scanned histogram of the first mismatches of n candidates: this many are left after observation k
__device__ __forceinline__ uint32_t hop_left_after(const uint32_t *cum, uint32_t n, uint32_t k)
{
	return n - cum[k];
}

// The verdict of a winnowing call, by 1024 lanes, for every lane: first = the observation that left <= 1 candidate (n_obs if
// none did), last = the last observation applied -- the survivors agree with more than `last` observations and
// hop_left_after(cum, n, last) of them are left.  *slot (in LDS) holds n_obs behind a barrier on entry.
__device__ __forceinline__ void hop_verdict(const uint32_t *cum, uint32_t n, uint32_t n_obs, uint32_t *slot, uint32_t &first,
					    uint32_t &last)
{
	if (threadIdx.x < n_obs && hop_left_after(cum, n, threadIdx.x) <= 1)
		atomicMin(slot, threadIdx.x);
	__syncthreads();
	first = *slot;
	last = first < n_obs ? first : n_obs - 1;
}

// One step of an ordered emit by 1024 lanes: the lanes with `live` set get the positions *base, *base + 1, ... in lane order
// (wave ballots, the 16 per-wave counts in LDS, a prefix over the waves before this one) and *base (in LDS) advances by
// their number.  Returns this lane's position (of use where live); barriers included, *base is current on return.
__device__ __forceinline__ uint32_t hop_emit_step(bool live, uint32_t *wave_cnt, uint32_t *base)
{
	const uint32_t tid = threadIdx.x;
	const uint64_t m = __ballot(live);
	if ((tid & 63) == 0)
		wave_cnt[tid >> 6] = (uint32_t)__popcll(m);
	__syncthreads();
	uint32_t at = *base;
	for (uint32_t w = 0; w < (tid >> 6); w++)
		at += wave_cnt[w];
	at += __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));   // live lanes below
	__syncthreads();
	if (tid == 0) {
		uint32_t all = 0;
		for (int w = 0; w < 16; w++)
			all += wave_cnt[w];
		*base += all;
	}
	__syncthreads();
	return at;
}
