// survey.hip -- batch piconet survey: UAP and CLK1-6 for every LAP of a hit list, on the device.
//
// What the reference's survey mode does one packet at a time (bluetooth_piconet.c:851-858 around
// btbb_uap_from_header, :648-750) is done here for a whole ordered or unordered hit list:
//
//   1. survey_key_kernel .. survey_scatter_kernel   stable LSD radix sort of (LAP << 40 | offset, hit index), eight bits
//      per pass, with the stream number as the least significant digit: the packets of a LAP end up in (offset, stream) order
//   2. survey_mark_kernel / survey_tiles_kernel / survey_group_kernel   boundary flags and their compaction: one group per
//      LAP with first index and count; the same pass lays out the sorted hit records and one btbbx_pkt_in per packet and ORs
//      every packet's channel into its group's map (in parallel over the list, not by the group's wave)
//   3. gather_kernel + trials kernels + header_flags_kernel (packet.hip)   the 64 {uap, type, rv} of every packet of the
//      list (the kernels read the list's length on the device); survey_wmark / wtiles / wlist_kernel compact the indices of
//      the header-bearing packets, so a walk never visits a packet it would skip
//   4. survey_walk_kernel   one wave per piconet, lane c = candidate c: the elimination of classify_candidates
//      (piconet.cpp) as ballots, candidates in a register for the life of the group
//
//   5. acquire_slots_kernel / acquire_fill_kernel (survey_jobs.h)   a separate entry, btbbx_survey_clock_jobs_device: from the records
//      and this scratch (read only) to the job table and observation arrays of the batch CLK1-27 reversal
//   6. follow_stage / follow_clock / follow_tally_kernel (follow.h)   a separate entry, btbbx_follow_hits_device: behind the
//      reversal, every hit decoded with its piconet's UAP and clock and checked against the piconet's hop selection
//
// Nothing here synchronises or reads back: the list's length stays in device memory.
#include "common.h"
#include "packet_launch.h"
#include "wave_scan.h"
#include "radix_sort.h"
#include <algorithm>
#include <string.h>

#define SV_THREADS     256
#define SV_WAVES       (SV_THREADS / 64)
#define SV_SORT_TILE   RADIX_SORT_TILE     // keys a workgroup ranks per pass (16 rounds of 256)
#define SV_GRP_TILE    2048u               // records a workgroup flags and lays out (8 rounds of 256)
#define SV_BATCH       16                  // trial rows a walking wave keeps in flight
#define SV_MAX_PATTERN 1000                // MAX_PATTERN_LENGTH, bluetooth_piconet.h
#define SV_PAD_OFFSET  (1ULL << 62)        // a hit beyond every stream: gathers as an empty packet
#define SV_CHAN_STREAMS 256u

// piconet flags (include/btbb.h)
#define SVF_UAP_VALID  (1u << 2)
#define SVF_LAP_VALID  (1u << 3)
#define SVF_CLK6_VALID (1u << 4)
#define SVF_GOT_FIRST  (1u << 10)

static_assert(sizeof(btbbx_survey_rec) == 64, "btbbx_survey_rec is 64 bytes");
static_assert(offsetof(btbbx_survey_rec, afh_map) == 12 && offsetof(btbbx_survey_rec, first_stream) == 22 &&
	      offsetof(btbbx_survey_rec, first_offset) == 56, "btbbx_survey_rec layout (libbtbb_amd.SURVEY_DTYPE)");

struct SurveyChannels {
	uint8_t ch[SV_CHAN_STREAMS];           // channel of every stream
};

struct SurveyLayout {
	size_t params, keys[2], vals[2], hist, tot, tiles, wtiles, gstart, wpos, widx, chan, hits, pin, packets, lengths, trials, present, total;
	uint32_t sort_blocks, grp_tiles;
};

static size_t sv_up(size_t x) { return (x + 255) & ~(size_t)255; }

static SurveyLayout survey_layout(uint32_t cap)
{
	SurveyLayout L;
	const size_t c = cap ? cap : 1;
	L.sort_blocks = radix_sort_blocks(c);
	L.grp_tiles = (uint32_t)((c + SV_GRP_TILE - 1) / SV_GRP_TILE);
	size_t at = 0;
	auto take = [&](size_t bytes) { const size_t here = at; at += sv_up(bytes); return here; };
	L.params = take(256);
	L.keys[0] = take(c * 8);
	L.keys[1] = take(c * 8);
	L.vals[0] = take(c * 4);
	L.vals[1] = take(c * 4);
	L.hist = take((size_t)L.sort_blocks * 256 * 4);
	L.tot = take(256 * 4);
	L.tiles = take(((size_t)L.grp_tiles + 1) * 4);
	L.wtiles = take(((size_t)L.grp_tiles + 1) * 4);
	L.gstart = take((c + 1) * 4);
	L.wpos = take((c + 1) * 4);
	L.widx = take(c * 4);
	L.chan = take(c * 16);
	L.hits = take(c * sizeof(btbbx_hit));
	L.pin = take(c * sizeof(btbbx_pkt_in));
	L.packets = take(c * BTBBX_PKT_WORDS * 8);
	L.lengths = take(c * 4);
	L.trials = take(c * 64 * sizeof(btbbx_trial));
	L.present = take(c);
	L.total = at;
	return L;
}

// ---- workgroup helpers ------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t sv_lap_of(uint64_t key) { return (uint32_t)(key >> 40); }

// ---- 1. ordering ------------------------------------------------------------------------------------

// params[0] = records to process, keys and hit indices of the unsorted list
__global__ __launch_bounds__(SV_THREADS) void survey_key_kernel(const btbbx_hit *hits, const uint32_t *d_count, uint32_t cap,
								  uint32_t *params, uint64_t *keys, uint32_t *vals)
{
	uint32_t n = cap;
	if (d_count) {
		const uint32_t have = *d_count;
		n = have < cap ? have : cap;
	}
	const uint32_t i = blockIdx.x * SV_THREADS + threadIdx.x;
	if (i == 0)
		params[0] = n;
	if (i >= n)
		return;
	const btbbx_hit h = hits[i];
	keys[i] = ((uint64_t)(h.lap & 0xffffffu) << 40) | (h.offset & 0xffffffffffULL);
	vals[i] = i;
}

// digit of record i in this pass: eight bits of the key, or of the hit's stream number
__device__ __forceinline__ uint32_t sv_digit(const uint64_t *keys, const uint32_t *vals, const btbbx_hit *hits, uint32_t i,
					     int by_stream, uint32_t shift)
{
	if (by_stream)
		return ((uint32_t)hits[vals[i]].stream >> shift) & 0xff;
	return (uint32_t)(keys[i] >> shift) & 0xff;
}

// hist[d * n_blocks + b] = records of tile b with digit d
__global__ __launch_bounds__(SV_THREADS) void survey_hist_kernel(const uint64_t *keys, const uint32_t *vals, const btbbx_hit *hits,
								   const uint32_t *params, uint32_t n_blocks, int by_stream, uint32_t shift,
								   uint32_t *hist)
{
	__shared__ uint32_t h[256];
	const uint32_t tid = threadIdx.x, n = params[0];
	h[tid] = 0;
	__syncthreads();
	const uint32_t base = blockIdx.x * SV_SORT_TILE;
	for (uint32_t k = 0; k < SV_SORT_TILE / SV_THREADS; k++) {
		const uint32_t i = base + k * SV_THREADS + tid;
		if (i < n)
			atomicAdd(&h[sv_digit(keys, vals, hits, i, by_stream, shift)], 1u);
	}
	__syncthreads();
	hist[(size_t)tid * n_blocks + blockIdx.x] = h[tid];
}

// one workgroup per digit: its row of tile counts becomes exclusive prefix sums, tot[d] the row's sum
__global__ __launch_bounds__(SV_THREADS) void survey_rows_kernel(uint32_t *hist, uint32_t n_blocks, uint32_t *tot)
{
	__shared__ uint32_t lds[SV_WAVES];
	uint32_t *row = hist + (size_t)blockIdx.x * n_blocks;
	uint32_t carry = 0;
	for (uint32_t base = 0; base < n_blocks; base += SV_THREADS) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t v = i < n_blocks ? row[i] : 0;
		uint32_t sum;
		const uint32_t ex = block_exclusive_scan<SV_WAVES>(v, lds, sum);
		if (i < n_blocks)
			row[i] = carry + ex;
		carry += sum;
	}
	if (threadIdx.x == 0)
		tot[blockIdx.x] = carry;
}

// stable scatter of one tile: 256 records per round, ranked by ballots within a wave and by counters between waves
__global__ __launch_bounds__(SV_THREADS) void survey_scatter_kernel(const uint64_t *keys, const uint32_t *vals, const btbbx_hit *hits,
								      const uint32_t *params, uint32_t cap, uint32_t n_blocks, int by_stream,
								      uint32_t shift, const uint32_t *hist, const uint32_t *tot,
								      uint64_t *keys_out, uint32_t *vals_out)
{
	__shared__ uint32_t lds[SV_WAVES];
	__shared__ uint32_t run[256];
	__shared__ uint32_t wcnt[SV_WAVES][256];
	const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = params[0];
	uint32_t all;
	const uint32_t digit_base = block_exclusive_scan<SV_WAVES>(tot[tid], lds, all);
	run[tid] = digit_base + hist[(size_t)tid * n_blocks + blockIdx.x];
#pragma unroll
	for (uint32_t w = 0; w < SV_WAVES; w++)
		wcnt[w][tid] = 0;
	__syncthreads();
	const uint32_t base = blockIdx.x * SV_SORT_TILE;
	for (uint32_t k = 0; k < SV_SORT_TILE / SV_THREADS; k++) {
		if (base + k * SV_THREADS >= n)
			break;                                          // (uniform over the workgroup)
		const uint32_t i = base + k * SV_THREADS + tid;
		const bool valid = i < n;
		uint64_t key = 0;
		uint32_t val = 0, d = 0;
		if (valid) {
			key = keys[i];
			val = vals[i];
			d = by_stream ? ((uint32_t)hits[val].stream >> shift) & 0xff : (uint32_t)(key >> shift) & 0xff;
		}
		uint64_t peers = __ballot(valid);
#pragma unroll
		for (int b = 0; b < 8; b++) {
			const bool bit = (d >> b) & 1;
			const uint64_t m = __ballot(valid && bit);
			peers &= bit ? m : ~m;
		}
		const uint32_t rank = __popcll(peers & ((1ULL << lane) - 1));
		if (valid && rank == 0)
			wcnt[wave][d] = __popcll(peers);
		__syncthreads();
		if (valid) {
			uint32_t pos = run[d] + rank;
			for (uint32_t w = 0; w < wave; w++)
				pos += wcnt[w][d];
			if (pos < cap) {
				keys_out[pos] = key;
				vals_out[pos] = val;
			}
		}
		__syncthreads();
		uint32_t s = 0;
#pragma unroll
		for (uint32_t w = 0; w < SV_WAVES; w++) {
			s += wcnt[w][tid];
			wcnt[w][tid] = 0;
		}
		run[tid] += s;
		__syncthreads();
	}
}

// the passes as launches (radix_sort.h): what every list sorted on the device goes through
int radix_sort_passes(const RadixBufs &b, const btbbx_hit *hits, const RadixPass *passes, int n_passes, int cur, hipStream_t q)
{
	const uint32_t blocks = radix_sort_blocks(b.cap);
	for (int p = 0; p < n_passes; p++) {
		hipLaunchKernelGGL(survey_hist_kernel, dim3(blocks), dim3(SV_THREADS), 0, q, b.keys[cur], b.vals[cur], hits, b.params, blocks,
				   passes[p].by_stream, passes[p].shift, b.hist);
		hipLaunchKernelGGL(survey_rows_kernel, dim3(256), dim3(SV_THREADS), 0, q, b.hist, blocks, b.tot);
		hipLaunchKernelGGL(survey_scatter_kernel, dim3(blocks), dim3(SV_THREADS), 0, q, b.keys[cur], b.vals[cur], hits, b.params, b.cap,
				   blocks, passes[p].by_stream, passes[p].shift, b.hist, b.tot, b.keys[cur ^ 1], b.vals[cur ^ 1]);
		cur ^= 1;
	}
	return cur;
}

// ---- 2. group table, sorted records, channel maps ------------------------------------------------------

__device__ __forceinline__ bool sv_first_of_lap(const uint64_t *keys, uint32_t i, uint32_t n)
{
	return i < n && (i == 0 || sv_lap_of(keys[i]) != sv_lap_of(keys[i - 1]));
}

__global__ __launch_bounds__(SV_THREADS) void survey_mark_kernel(const uint64_t *keys, const uint32_t *params, uint32_t *tiles)
{
	__shared__ uint32_t count;
	const uint32_t tid = threadIdx.x, n = params[0];
	if (tid == 0)
		count = 0;
	__syncthreads();
	uint32_t mine = 0;
	for (uint32_t k = 0; k < SV_GRP_TILE / SV_THREADS; k++)
		mine += sv_first_of_lap(keys, blockIdx.x * SV_GRP_TILE + k * SV_THREADS + tid, n) ? 1u : 0u;
	if (mine)
		atomicAdd(&count, mine);
	__syncthreads();
	if (tid == 0)
		tiles[blockIdx.x] = count;
}

// one workgroup: tile counts -> exclusive prefix sums; the number of groups goes to params[1], *rec_count and,
// as the end of the last group, gstart[groups] = n; params[2] = which of the two vals[] the sort ended in (survey_jobs.h)
__global__ __launch_bounds__(SV_THREADS) void survey_tiles_kernel(uint32_t *tiles, uint32_t n_tiles, uint32_t *params, uint32_t *gstart,
								    uint32_t *rec_count, uint32_t vals_side)
{
	__shared__ uint32_t lds[SV_WAVES];
	uint32_t carry = 0;
	for (uint32_t base = 0; base < n_tiles; base += SV_THREADS) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t v = i < n_tiles ? tiles[i] : 0;
		uint32_t sum;
		const uint32_t ex = block_exclusive_scan<SV_WAVES>(v, lds, sum);
		if (i < n_tiles)
			tiles[i] = carry + ex;
		carry += sum;
	}
	if (threadIdx.x == 0) {
		params[1] = carry;
		params[2] = vals_side;
		gstart[carry] = params[0];
		if (rec_count)
			*rec_count = carry;
	}
}

__global__ __launch_bounds__(SV_THREADS) void survey_group_kernel(const uint64_t *keys, const uint32_t *vals, const btbbx_hit *hits,
								    const uint32_t *params, uint32_t cap, const uint32_t *tiles,
								    uint64_t total_bits, uint32_t n_streams, uint32_t max_length,
								    btbbx_pkt_in entry, uint32_t clk_div, uint32_t clk_phase,
								    SurveyChannels table, int identity,
								    uint32_t *gstart, uint32_t *chan, btbbx_hit *hits_out, btbbx_pkt_in *pin)
{
	__shared__ uint32_t lds[SV_WAVES];
	const uint32_t tid = threadIdx.x, n = params[0];
	uint32_t carry = tiles[blockIdx.x];
	for (uint32_t k = 0; k < SV_GRP_TILE / SV_THREADS; k++) {
		const uint32_t i = blockIdx.x * SV_GRP_TILE + k * SV_THREADS + tid;
		const bool first = sv_first_of_lap(keys, i, n);
		uint32_t sum;
		const uint32_t ex = block_exclusive_scan<SV_WAVES>(first ? 1u : 0u, lds, sum);
		const uint32_t gid = carry + ex + (first ? 1u : 0u) - 1u;         // (i < n: some record at or before i is a first one)
		carry += sum;
		btbbx_hit h;
		h.offset = SV_PAD_OFFSET;
		h.lap = 0;
		h.ac_errors = 0;
		h.reserved = 0;
		h.stream = 0;
		btbbx_pkt_in p = entry;
		p.length = 0;
		uint32_t word = 3, bit = 0;                                        // (word 3 of a group's four: never read)
		if (i < n) {
			h = hits[vals[i]];
			if (first)
				gstart[gid] = i;
			p.clkn = entry.clkn + (uint32_t)((h.offset + clk_phase) / clk_div);
			if (h.stream < n_streams) {
				const uint32_t ch = identity ? h.stream : table.ch[h.stream];
				word = ch >> 5;
				bit = 1u << (ch & 31);
				// the captured length, as gather_kernel computes it
				const uint64_t avail = h.offset < total_bits ? total_bits - h.offset : 0;
				uint32_t len = avail < max_length ? (uint32_t)avail : max_length;
				p.length = len > BTBBX_MAX_SYMBOLS ? BTBBX_MAX_SYMBOLS : len;
			} else {
				h.offset = SV_PAD_OFFSET;                                 // a stream that does not exist: no symbols, no channel
				h.stream = 0;
			}
		}
		if (i < n) {
			hits_out[i] = h;
			pin[i] = p;
		}
		// channel map: a wave whose records all belong to one group (the waves of a large piconet) sends three atomics
		const uint64_t active = __ballot(i < n);
		const uint32_t g0 = __shfl(gid, 0, 64);
		if (active == ~0ULL && __ballot(gid == g0) == ~0ULL) {
			uint32_t m0 = word == 0 ? bit : 0, m1 = word == 1 ? bit : 0, m2 = word == 2 ? bit : 0;
#pragma unroll
			for (int d = 32; d >= 1; d >>= 1) {
				m0 |= __shfl_xor(m0, d, 64);
				m1 |= __shfl_xor(m1, d, 64);
				m2 |= __shfl_xor(m2, d, 64);
			}
			if ((tid & 63) < 3) {
				const uint32_t m = (tid & 63) == 0 ? m0 : (tid & 63) == 1 ? m1 : m2;
				if (m)
					atomicOr(&chan[(size_t)g0 * 4 + (tid & 63)], m);
			}
		} else if (i < n && bit) {
			atomicOr(&chan[(size_t)gid * 4 + word], bit);
		}
	}
}

// ---- 3b. the packets a walk can touch ------------------------------------------------------------------
// A packet without a header is never walked (it only marks its channel), and one piconet may own a million of them: the
// header-bearing packets are compacted, in sorted order, into widx[]; wpos[i] = how many of them lie before record i, so
// group g walks widx[wpos[gstart[g]] .. wpos[gstart[g + 1]]) and never looks at the others.

__global__ __launch_bounds__(SV_THREADS) void survey_wmark_kernel(const uint8_t *present, const uint32_t *params, uint32_t *wtiles)
{
	__shared__ uint32_t count;
	const uint32_t tid = threadIdx.x, n = params[0];
	if (tid == 0)
		count = 0;
	__syncthreads();
	uint32_t mine = 0;
	for (uint32_t k = 0; k < SV_GRP_TILE / SV_THREADS; k++) {
		const uint32_t i = blockIdx.x * SV_GRP_TILE + k * SV_THREADS + tid;
		mine += i < n && present[i] ? 1u : 0u;
	}
	if (mine)
		atomicAdd(&count, mine);
	__syncthreads();
	if (tid == 0)
		wtiles[blockIdx.x] = count;
}

// one workgroup: tile counts -> exclusive prefix sums; wpos[n] = all header-bearing packets
__global__ __launch_bounds__(SV_THREADS) void survey_wtiles_kernel(uint32_t *wtiles, uint32_t n_tiles, const uint32_t *params, uint32_t *wpos)
{
	__shared__ uint32_t lds[SV_WAVES];
	uint32_t carry = 0;
	for (uint32_t base = 0; base < n_tiles; base += SV_THREADS) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t v = i < n_tiles ? wtiles[i] : 0;
		uint32_t sum;
		const uint32_t ex = block_exclusive_scan<SV_WAVES>(v, lds, sum);
		if (i < n_tiles)
			wtiles[i] = carry + ex;
		carry += sum;
	}
	if (threadIdx.x == 0)
		wpos[params[0]] = carry;
}

__global__ __launch_bounds__(SV_THREADS) void survey_wlist_kernel(const uint8_t *present, const uint32_t *params, const uint32_t *wtiles,
								    uint32_t *wpos, uint32_t *widx)
{
	__shared__ uint32_t lds[SV_WAVES];
	const uint32_t tid = threadIdx.x, n = params[0];
	uint32_t carry = wtiles[blockIdx.x];
	for (uint32_t k = 0; k < SV_GRP_TILE / SV_THREADS; k++) {
		const uint32_t i = blockIdx.x * SV_GRP_TILE + k * SV_THREADS + tid;
		const bool has = i < n && present[i];
		uint32_t sum;
		const uint32_t at = carry + block_exclusive_scan<SV_WAVES>(has ? 1u : 0u, lds, sum);
		carry += sum;
		if (i < n) {
			wpos[i] = at;
			if (has)
				widx[at] = i;                           // (at < n: fewer header-bearing packets than packets before and at i)
		}
	}
}

// ---- 4. the walk ------------------------------------------------------------------------------------

// One wave per piconet, lane c = candidate "CLK1-6 of the first packet was c".  Trial rows are loaded as they lie
// (lane c reads trial c) SV_BATCH packets at a time, none of them depending on the piconet's state; the rotation by
// the packet's distance from the first packet is a lane permutation once the state is known.  Only header-bearing packets
// are visited (widx, above): per 64 of them one load of their indices and clocks.
__global__ __launch_bounds__(SV_THREADS) void survey_walk_kernel(const uint32_t *params, uint32_t rec_cap, const uint32_t *gstart,
								   const uint32_t *chan, const btbbx_hit *hits, const uint32_t *vals,
								   const btbbx_pkt_in *pin, const uint32_t *wpos, const uint32_t *widx, const uint32_t *trials,
								   btbbx_survey_rec *recs, int16_t *candidates)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t g = blockIdx.x * SV_WAVES + (threadIdx.x >> 6);
	const uint32_t n_groups = params[1];
	if (g >= n_groups || g >= rec_cap)
		return;
	const uint32_t start = gstart[g], end = gstart[g + 1];

	int cand = 0;                                     // clock6_candidates[lane] of a new piconet object
	uint32_t flags = SVF_LAP_VALID;
	uint32_t first_pkt_time = 0, n_walked = 0, n_resets = 0;
	int packets_observed = 0, total_observed = 0;
	uint32_t settled_by = 0, settled_after = 0, settled_at = 0xffffffffu, uap = 0, clk_offset = 0;

	const uint32_t wfirst = wpos[start], wend = wpos[end];
	for (uint32_t base = wfirst; base < wend && !settled_by; base += 64) {
		const bool ok = base + lane < wend;
		const uint32_t my_idx = ok ? widx[base + lane] : 0;
		const uint32_t my_clkn = ok ? pin[my_idx].clkn : 0;
		uint64_t todo = __ballot(ok);
		while (todo && !settled_by) {
			uint32_t row[SV_BATCH];
			int which[SV_BATCH];
#pragma unroll
			for (int k = 0; k < SV_BATCH; k++) {
				which[k] = -1;
				row[k] = 0;
				if (todo) {
					which[k] = __builtin_ctzll(todo);
					todo &= todo - 1;
					row[k] = trials[(size_t)__shfl(my_idx, which[k], 64) * 64 + lane];
				}
			}
#pragma unroll
			for (int k = 0; k < SV_BATCH; k++) {
				if (which[k] < 0 || settled_by)
					continue;
				const uint32_t clkn = __shfl(my_clkn, which[k], 64);
				n_walked++;
				const bool opening = !(flags & SVF_GOT_FIRST);
				if (opening)
					first_pkt_time = clkn;
				if (packets_observed >= SV_MAX_PATTERN) {         // "Oops. More hops than we can remember."
					flags &= ~(SVF_GOT_FIRST | SVF_UAP_VALID | SVF_CLK6_VALID);
					packets_observed = 0;
					n_resets++;
					continue;
				}
				packets_observed++;
				total_observed++;
				const uint32_t rot = (clkn - first_pkt_time) & 63;
				const uint32_t t = __shfl(row[k], (lane + rot) & 63, 64);
				const int t_uap = (int)(t & 0xff);
				const int rv = (int)(int16_t)(t >> 16);
				const bool live = opening || cand >= 0;
				const bool checked = live && (opening || t_uap == cand);
				const bool kept = checked && (rv == 1 || rv == 2);
				const uint64_t proven = __ballot(checked && !kept && rv != 0);
				const uint32_t winner = proven ? (uint32_t)__builtin_ctzll(proven) : 64u;
				if (live && lane < winner)
					cand = kept ? t_uap : -1;
				if (winner < 64) {                                  // "Correct CRC!"
					uap = (uint32_t)__shfl(t_uap, winner, 64);
					clk_offset = (winner - (first_pkt_time & 0x3f)) & 0x3f;
					settled_by = 2;
				} else {
					flags |= SVF_GOT_FIRST;
					const uint64_t survivors = __ballot(kept);
					const uint32_t left = __popcll(survivors);
					if (left == 1) {
						const uint32_t only = (uint32_t)__builtin_ctzll(survivors);
						uap = (uint32_t)__shfl(t_uap, only, 64);
						clk_offset = (only - (first_pkt_time & 0x3f)) & 0x3f;
						settled_by = 1;
					} else if (left == 0) {
						flags &= ~(SVF_GOT_FIRST | SVF_UAP_VALID | SVF_CLK6_VALID);
						packets_observed = 0;
						n_resets++;
					}
				}
				if (settled_by) {
					flags |= SVF_CLK6_VALID | SVF_UAP_VALID;
					settled_after = (uint32_t)total_observed;
					total_observed = 0;
					settled_at = vals[__shfl(my_idx, which[k], 64)];
				}
			}
		}
	}

	if (candidates)
		candidates[(size_t)g * 64 + lane] = (int16_t)cand;
	if (lane == 0) {
		const btbbx_hit h0 = hits[start];
		const uint32_t m0 = chan[(size_t)g * 4], m1 = chan[(size_t)g * 4 + 1], m2 = chan[(size_t)g * 4 + 2];
		btbbx_survey_rec r;
		r.lap = h0.lap;
		r.flags = flags;
		r.uap = (uint8_t)uap;
		r.clk_offset = (uint8_t)clk_offset;
		r.used_channels = (uint8_t)(__popc(m0) + __popc(m1) + __popc(m2));
		r.settled_by = (uint8_t)settled_by;
#pragma unroll
		for (int b = 0; b < 10; b++) {
			const uint32_t m = b < 4 ? m0 : b < 8 ? m1 : m2;
			r.afh_map[b] = (uint8_t)(m >> (8 * (b & 3)));
		}
		r.first_stream = h0.stream;
		r.n_packets = end - start;
		r.n_walked = n_walked;
		r.n_resets = n_resets;
		r.settled_after = settled_after;
		r.settled_hit = settled_at;
		r.packets_observed = packets_observed;
		r.total_packets_observed = total_observed;
		r.first_pkt_time = first_pkt_time;
		r.first_offset = h0.offset;
		recs[g] = r;
	}
}

#include "survey_jobs.h"
#include "follow.h"

// ---- C ABI ------------------------------------------------------------------------------------------

extern "C" size_t btbbx_survey_scratch_bytes(uint32_t cap)
{
	return survey_layout(cap).total;
}

static uint32_t bits_of(uint64_t v)
{
	uint32_t b = 0;
	while (v) {
		b++;
		v >>= 1;
	}
	return b;
}

static int survey_check_args(const char *who, uint64_t n_words, uint32_t n_streams, const uint8_t *channels, const btbbx_pkt_in *entry,
			     uint32_t clk_div, uint32_t clk_phase)
{
	if (!n_streams || !n_words || n_words > (1ULL << 34)) {
		set_error("%s: no streams, no words or offsets beyond 2^40", who);
		return BTBBX_E_ARG;
	}
	if (!entry || !clk_div || clk_phase >= clk_div) {
		set_error("%s: no entry state, clk_div = 0 or clk_phase >= clk_div", who);
		return BTBBX_E_ARG;
	}
	if (!channels && n_streams > 79) {
		set_error("%s: %u streams need a channel table (BR/EDR has channels 0..78)", who, n_streams);
		return BTBBX_E_ARG;
	}
	if (channels) {
		if (n_streams > SV_CHAN_STREAMS) {
			set_error("%s: a channel table covers at most %u streams", who, SV_CHAN_STREAMS);
			return BTBBX_E_ARG;
		}
		for (uint32_t s = 0; s < n_streams; s++)
			if (channels[s] > 78) {
				set_error("%s: channels[%u] = %u is not a BR/EDR channel (0..78)", who, s, channels[s]);
				return BTBBX_E_ARG;
			}
	}
	return BTBBX_OK;
}

extern "C" int btbbx_survey_hits_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
					const btbbx_hit *d_hits, const uint32_t *d_count, uint32_t cap, const uint8_t *channels,
					const btbbx_pkt_in *entry, uint32_t clk_div, uint32_t clk_phase, uint32_t max_length,
					btbbx_survey_rec *d_recs, uint32_t rec_cap, uint32_t *d_rec_count, int16_t *d_candidates,
					void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
	int rc = survey_check_args("btbbx_survey_hits_device", n_words, n_streams, channels, entry, clk_div, clk_phase);
	if (rc)
		return rc;
	const SurveyLayout L = survey_layout(cap);
	if (!d_words || !d_rec_count || (cap && !d_hits) || (cap && rec_cap && !d_recs) || !d_scratch || scratch_bytes < L.total) {
		set_error("btbbx_survey_hits_device: null pointer, or scratch of %zu bytes needed and %zu given", L.total, scratch_bytes);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_scratch & 15) || ((uintptr_t)d_hits & 15) || ((uintptr_t)d_recs & 7) || ((uintptr_t)d_words & 7) ||
	    ((uintptr_t)d_rec_count & 3) || ((uintptr_t)d_count & 3) || ((uintptr_t)d_candidates & 1)) {
		set_error("btbbx_survey_hits_device: misaligned pointer (scratch and hits 16 bytes, records and words 8)");
		return BTBBX_E_ARG;
	}
	if (n_streams > 1 && pitch_words < n_words) {
		set_error("btbbx_survey_hits_device: pitch_words < n_words");
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	hipStream_t q = (hipStream_t)hip_stream;
	if (!cap) {
		HIP_TRY(hipMemsetAsync(d_rec_count, 0, sizeof(uint32_t), q));
		return BTBBX_OK;
	}
	char *s = (char *)d_scratch;
	uint32_t *params = (uint32_t *)(s + L.params);
	uint64_t *keys[2] = {(uint64_t *)(s + L.keys[0]), (uint64_t *)(s + L.keys[1])};
	uint32_t *vals[2] = {(uint32_t *)(s + L.vals[0]), (uint32_t *)(s + L.vals[1])};
	uint32_t *hist = (uint32_t *)(s + L.hist), *tot = (uint32_t *)(s + L.tot), *tiles = (uint32_t *)(s + L.tiles);
	uint32_t *gstart = (uint32_t *)(s + L.gstart), *chan = (uint32_t *)(s + L.chan), *lengths = (uint32_t *)(s + L.lengths);
	btbbx_hit *shits = (btbbx_hit *)(s + L.hits);
	btbbx_pkt_in *pin = (btbbx_pkt_in *)(s + L.pin);
	uint64_t *packets = (uint64_t *)(s + L.packets);
	btbbx_trial *trials = (btbbx_trial *)(s + L.trials);
	uint8_t *present = (uint8_t *)(s + L.present);
	uint32_t *wtiles = (uint32_t *)(s + L.wtiles), *wpos = (uint32_t *)(s + L.wpos), *widx = (uint32_t *)(s + L.widx);

	HIP_TRY(hipMemsetAsync(chan, 0, (size_t)cap * 16, q));
	const uint32_t cap_blocks = (cap + SV_THREADS - 1) / SV_THREADS;
	hipLaunchKernelGGL(survey_key_kernel, dim3(cap_blocks), dim3(SV_THREADS), 0, q, d_hits, d_count, cap, params, keys[0], vals[0]);

	// digits from the least significant: stream, offset, LAP -- only those that can differ
	RadixPass passes[12];
	int n_passes = 0;
	for (uint32_t b = 0; b < bits_of(n_streams - 1); b += 8)
		passes[n_passes++] = {1, b};
	for (uint32_t b = 0; b < bits_of(n_words * 64 - 1) && b < 40; b += 8)
		passes[n_passes++] = {0, b};
	for (uint32_t b = 40; b < 64; b += 8)
		passes[n_passes++] = {0, b};
	const RadixBufs bufs = {{keys[0], keys[1]}, {vals[0], vals[1]}, hist, tot, params, cap};
	const int cur = radix_sort_passes(bufs, d_hits, passes, n_passes, 0, q);

	hipLaunchKernelGGL(survey_mark_kernel, dim3(L.grp_tiles), dim3(SV_THREADS), 0, q, keys[cur], params, tiles);
	hipLaunchKernelGGL(survey_tiles_kernel, dim3(1), dim3(SV_THREADS), 0, q, tiles, L.grp_tiles, params, gstart, d_rec_count, (uint32_t)cur);
	SurveyChannels table;
	memset(&table, 0, sizeof(table));
	if (channels)
		memcpy(table.ch, channels, n_streams);
	hipLaunchKernelGGL(survey_group_kernel, dim3(L.grp_tiles), dim3(SV_THREADS), 0, q, keys[cur], vals[cur], d_hits, params, cap, tiles,
			   n_words * 64, n_streams, max_length, *entry, clk_div, clk_phase, table, channels ? 0 : 1, gstart, chan, shits, pin);
	HIP_TRY(hipGetLastError());

	// (launched for cap, worked for the list's length: params[0])
	rc = launch_gather(d_words, n_words, pitch_words, shits, cap, params, max_length, packets, lengths, q);
	if (rc)
		return rc;
	rc = launch_trials(packets, pin, cap, params, trials, q);
	if (rc)
		return rc;
	rc = launch_header_flags(packets, lengths, cap, params, present, q);
	if (rc)
		return rc;
	hipLaunchKernelGGL(survey_wmark_kernel, dim3(L.grp_tiles), dim3(SV_THREADS), 0, q, present, params, wtiles);
	hipLaunchKernelGGL(survey_wtiles_kernel, dim3(1), dim3(SV_THREADS), 0, q, wtiles, L.grp_tiles, params, wpos);
	hipLaunchKernelGGL(survey_wlist_kernel, dim3(L.grp_tiles), dim3(SV_THREADS), 0, q, present, params, wtiles, wpos, widx);

	const uint32_t walkers = rec_cap < cap ? rec_cap : cap;
	if (walkers)
		hipLaunchKernelGGL(survey_walk_kernel, dim3((walkers + SV_WAVES - 1) / SV_WAVES), dim3(SV_THREADS), 0, q, params, rec_cap,
				   gstart, chan, shits, vals[cur], pin, wpos, widx, (const uint32_t *)trials, d_recs, d_candidates);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

// The ordered LAP_ANY scan in front of a host-level survey: one hit per 1024 offsets + slack, again with room for every match
// when more were found (as btbbx_scan_host does); the count is read back, and the survey's scratch is sized from it.
// *block: the count (word 0; word 1 is free for the piconet count), the hit list 256 bytes behind it.
static int survey_scan_list(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, uint64_t search_bits,
			    int max_ac_errors, hipStream_t q, char **block_out, uint32_t *dev_cap_out, uint32_t *count_out)
{
	uint64_t guess = search_bits / 1024 * n_streams + 4096;
	uint32_t dev_cap = guess > 0xfffffff0ULL ? 0xfffffff0u : (uint32_t)guess;
	uint32_t count = 0;
	char *block = nullptr;
	for (int pass = 0; pass < 2; pass++) {
		const size_t hit_bytes = sv_up((size_t)dev_cap * sizeof(btbbx_hit));
		const size_t order_bytes = sv_up(btbbx_scan_ordered_scratch_bytes(search_bits, n_streams, BTBBX_LAP_ANY, dev_cap));
		block = (char *)scope_hits(256 + hit_bytes + order_bytes);
		if (!block)
			return BTBBX_E_NOMEM;
		HIP_TRY(hipMemsetAsync(block, 0, 2 * sizeof(uint32_t), q));
		int rc = btbbx_scan_ordered_device(d_words, n_words, pitch_words, n_streams, search_bits, BTBBX_LAP_ANY, max_ac_errors,
						   (btbbx_hit *)(block + 256), dev_cap, (uint32_t *)block, block + 256 + hit_bytes, order_bytes, q);
		if (rc)
			return rc;
		HIP_TRY(hipMemcpyAsync(&count, block, sizeof(count), hipMemcpyDeviceToHost, q));
		HIP_TRY(hipStreamSynchronize(q));
		if (count <= dev_cap)
			break;
		dev_cap = count;
	}
	*block_out = block;
	*dev_cap_out = dev_cap;
	*count_out = count;
	return BTBBX_OK;
}

extern "C" int64_t btbbx_survey_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				     uint64_t search_bits, int max_ac_errors, const uint8_t *channels,
				     uint32_t clkn0, uint32_t clk_div, uint32_t clk_phase,
				     btbbx_survey_rec *recs, uint64_t rec_cap, int16_t *candidates)
{
	btbbx_pkt_in entry;
	memset(&entry, 0, sizeof(entry));
	entry.clkn = clkn0;
	entry.flags = 1u << 0;                                  // BTBB_WHITENED: what btbb_find_ac leaves (init_packet)
	int rc = survey_check_args("btbbx_survey_host", n_words, n_streams, channels, &entry, clk_div, clk_phase);
	if (rc)
		return rc;
	if (n_streams == 1)
		pitch_words = n_words;
	if (!words || (!recs && rec_cap) || pitch_words < n_words || search_bits + 63 > n_words * 64) {
		set_error("btbbx_survey_host: null pointer, pitch_words < n_words or search_bits + 63 > 64 n_words");
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	if (!search_bits)
		return 0;
	CallScope scope;
	hipStream_t q = scope_stream();
	const uint64_t cap_words = (uint64_t)(n_streams - 1) * pitch_words + n_words;
	uint64_t *d_words = (uint64_t *)scope_device((size_t)(cap_words + 2) * 8);
	if (!d_words)
		return BTBBX_E_NOMEM;
	HIP_TRY(hipMemcpyAsync(d_words, words, (size_t)cap_words * 8, hipMemcpyHostToDevice, q));

	char *block = nullptr;
	uint32_t dev_cap = 0, count = 0;
	rc = survey_scan_list(d_words, n_words, pitch_words, n_streams, search_bits, max_ac_errors, q, &block, &dev_cap, &count);
	if (rc)
		return rc;
	const uint32_t have = std::min(count, dev_cap);
	if (!have)
		return 0;
	// records, candidates and the survey's scratch: one block for the life of the call
	const uint32_t dev_recs = (uint32_t)std::min<uint64_t>(rec_cap, have);
	const size_t survey_bytes = sv_up(btbbx_survey_scratch_bytes(have));
	const size_t rec_bytes = sv_up((size_t)dev_recs * sizeof(btbbx_survey_rec));
	const size_t cand_bytes = candidates ? sv_up((size_t)dev_recs * 64 * sizeof(int16_t)) : 0;
	char *work = nullptr;
	if (hipMalloc((void **)&work, survey_bytes + rec_bytes + cand_bytes + 256) != hipSuccess) {
		(void)hipGetLastError();
		set_error("btbbx_survey_host: %zu bytes of device memory for %u hits not available", survey_bytes + rec_bytes + cand_bytes, have);
		return BTBBX_E_NOMEM;
	}
	btbbx_survey_rec *d_recs = (btbbx_survey_rec *)(work + survey_bytes);
	int16_t *d_cand = candidates ? (int16_t *)(work + survey_bytes + rec_bytes) : nullptr;
	uint32_t *d_rec_count = (uint32_t *)block + 1;
	uint32_t n_piconets = 0;
	rc = btbbx_survey_hits_device(d_words, n_words, pitch_words, n_streams, (const btbbx_hit *)(block + 256), (const uint32_t *)block, have,
				      channels, &entry, clk_div, clk_phase, BTBBX_MAX_SYMBOLS, d_recs, dev_recs, d_rec_count, d_cand, work,
				      survey_bytes, q);
	hipError_t e = hipSuccess;
	if (!rc) {
		e = hipMemcpyAsync(&n_piconets, d_rec_count, sizeof(n_piconets), hipMemcpyDeviceToHost, q);
		if (e == hipSuccess)
			e = hipStreamSynchronize(q);
		const uint64_t n = std::min<uint64_t>(n_piconets, dev_recs);
		if (e == hipSuccess && n)
			e = hipMemcpyAsync(recs, d_recs, (size_t)n * sizeof(btbbx_survey_rec), hipMemcpyDeviceToHost, q);
		if (e == hipSuccess && n && candidates)
			e = hipMemcpyAsync(candidates, d_cand, (size_t)n * 64 * sizeof(int16_t), hipMemcpyDeviceToHost, q);
	}
	const hipError_t f = hipStreamSynchronize(q);
	(void)hipFree(work);
	if (rc)
		return rc;
	HIP_TRY(e);
	HIP_TRY(f);
	return (int64_t)n_piconets;
}

// ---- job builder and clock acquisition ----------------------------------------------------------------

extern "C" int btbbx_survey_clock_jobs_device(const btbbx_survey_rec *d_recs, const uint32_t *d_rec_count, uint32_t rec_cap,
					      const void *d_survey_scratch, size_t survey_scratch_bytes, uint32_t cap,
					      const uint8_t *channels, uint32_t n_streams, uint32_t flags, uint32_t max_obs,
					      btbbx_clock_job *d_jobs, uint32_t job_cap, uint32_t *d_n_jobs, uint32_t *d_job_rec,
					      int32_t *d_index_offsets, uint8_t *d_channels, uint32_t *d_obs_hits,
					      uint32_t obs_cap, uint32_t *d_n_obs, void *hip_stream)
{
	const char *who = "btbbx_survey_clock_jobs_device";
	const SurveyLayout L = survey_layout(cap);
	if (!d_recs || !d_jobs || !d_n_jobs || !d_survey_scratch || !d_index_offsets || !d_channels) {
		set_error("%s: null pointer (records, jobs, job count, scratch or an observation array)", who);
		return BTBBX_E_ARG;
	}
	if (survey_scratch_bytes < L.total || obs_cap < cap) {
		set_error("%s: the survey's scratch has %zu bytes for %u hits (%zu given), and its observations need %u entries (%u given)", who,
			  L.total, cap, survey_scratch_bytes, cap, obs_cap);
		return BTBBX_E_ARG;
	}
	if (!max_obs || max_obs > 1024 || !job_cap || (flags & ~(BTBBX_JOBS_AFH | BTBBX_JOBS_ALIASED))) {
		set_error("%s: max_obs %u outside 1..1024, job_cap %u, or unknown bits in flags 0x%x", who, max_obs, job_cap, flags);
		return BTBBX_E_ARG;
	}
	if (!n_streams || (!channels && n_streams > 79) || (channels && n_streams > SV_CHAN_STREAMS)) {
		set_error("%s: %u streams (1..79 without a channel table, up to %u with one)", who, n_streams, SV_CHAN_STREAMS);
		return BTBBX_E_ARG;
	}
	for (uint32_t s = 0; channels && s < n_streams; s++)
		if (channels[s] > 78) {
			set_error("%s: channels[%u] = %u is not a BR/EDR channel (0..78)", who, s, channels[s]);
			return BTBBX_E_ARG;
		}
	if (((uintptr_t)d_survey_scratch & 15) || ((uintptr_t)d_recs & 3) || ((uintptr_t)d_rec_count & 3) || ((uintptr_t)d_jobs & 3) ||
	    ((uintptr_t)d_n_jobs & 3) || ((uintptr_t)d_job_rec & 3) || ((uintptr_t)d_index_offsets & 3) || ((uintptr_t)d_obs_hits & 3) ||
	    ((uintptr_t)d_n_obs & 3)) {
		set_error("%s: misaligned pointer (scratch 16 bytes, everything else but the channels 4)", who);
		return BTBBX_E_ARG;
	}
	int rc = ctx_require();
	if (rc)
		return rc;
	hipStream_t q = (hipStream_t)hip_stream;
	if (!cap) {                                             // (the survey of an empty list launched nothing: its scratch is not valid)
		HIP_TRY(hipMemsetAsync(d_n_jobs, 0, sizeof(uint32_t), q));
		if (d_n_obs)
			HIP_TRY(hipMemsetAsync(d_n_obs, 0, sizeof(uint32_t), q));
		return BTBBX_OK;
	}
	const char *s = (const char *)d_survey_scratch;
	const uint32_t *params = (const uint32_t *)(s + L.params), *gstart = (const uint32_t *)(s + L.gstart);
	const uint32_t *wpos = (const uint32_t *)(s + L.wpos), *widx = (const uint32_t *)(s + L.widx);
	SurveyChannels table;
	memset(&table, 0, sizeof(table));
	if (channels)
		memcpy(table.ch, channels, n_streams);
	hipLaunchKernelGGL(acquire_slots_kernel, dim3(1), dim3(AQ_SLOT_THREADS), 0, q, (const uint32_t *)d_recs, d_rec_count, rec_cap, cap, params,
			   gstart, wpos, max_obs, d_jobs, job_cap, d_n_jobs, d_job_rec, d_n_obs);
	// (launched for every job there can be: one per record, one per hit)
	const uint32_t waves = std::min(job_cap, std::min(rec_cap, cap));
	if (waves)
		hipLaunchKernelGGL(acquire_fill_kernel, dim3((waves + SV_WAVES - 1) / SV_WAVES), dim3(SV_THREADS), 0, q, (const uint32_t *)d_recs, cap,
				   params, gstart, wpos, widx, (const btbbx_pkt_in *)(s + L.pin), (const btbbx_hit *)(s + L.hits),
				   (const uint32_t *)(s + L.vals[0]), (const uint32_t *)(s + L.vals[1]), table, channels ? 0 : 1, flags, max_obs, d_jobs,
				   job_cap, d_n_jobs, d_index_offsets, d_channels, d_obs_hits, obs_cap);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

// What btbbx_follow_host appends to the chain of btbbx_acquire_host (null: the chain alone).
struct FollowOut {
	btbbx_hit *hits;
	btbbx_follow_pkt *follow;
	btbbx_pkt_out *pkts;
	uint64_t hit_cap;
	uint64_t *n_hits;
	btbbx_follow_sum *sums;
};

// The chain of btbbx_acquire_host / btbbx_follow_host (`who`).  With `fo` every stored record's job is worked, whatever job_cap
// the caller has room for, job_rec / results may be null, and btbbx_follow_hits_device runs behind the batch reversal.
static int64_t acquire_run(const char *who, const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			   uint64_t search_bits, int max_ac_errors, const uint8_t *channels,
			   uint32_t clkn0, uint32_t clk_div, uint32_t clk_phase,
			   btbbx_survey_rec *recs, uint64_t rec_cap, int16_t *clk6_candidates,
			   uint32_t flags, uint32_t max_obs,
			   btbbx_clock_job *jobs, uint32_t *job_rec, btbbx_clock_result *results, uint64_t job_cap,
			   uint64_t *n_jobs, uint32_t *candidates, uint32_t cand_cap, const FollowOut *fo)
{
	btbbx_pkt_in entry;
	memset(&entry, 0, sizeof(entry));
	entry.clkn = clkn0;
	entry.flags = 1u << 0;                                  // BTBB_WHITENED: what btbb_find_ac leaves (init_packet)
	int rc = survey_check_args(who, n_words, n_streams, channels, &entry, clk_div, clk_phase);
	if (rc)
		return rc;
	if (n_streams == 1)
		pitch_words = n_words;
	if (!words || (!recs && rec_cap) || pitch_words < n_words || search_bits + 63 > n_words * 64) {
		set_error("%s: null pointer, pitch_words < n_words or search_bits + 63 > 64 n_words", who);
		return BTBBX_E_ARG;
	}
	if (!n_jobs || (!fo && job_cap && (!job_rec || !results)) || !max_obs || max_obs > 1024 || (flags & ~(BTBBX_JOBS_AFH | BTBBX_JOBS_ALIASED))) {
		set_error("%s: no n_jobs, job_rec or results, max_obs %u outside 1..1024, or unknown bits in flags 0x%x", who, max_obs, flags);
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	*n_jobs = 0;
	if (fo)
		*fo->n_hits = 0;
	const uint64_t work_cap = fo ? rec_cap : job_cap;        // jobs worked on the device
	if (!search_bits)
		return 0;
	CallScope scope;
	hipStream_t q = scope_stream();
	const uint64_t cap_words = (uint64_t)(n_streams - 1) * pitch_words + n_words;
	uint64_t *d_words = (uint64_t *)scope_device((size_t)(cap_words + 2) * 8);
	if (!d_words)
		return BTBBX_E_NOMEM;
	HIP_TRY(hipMemcpyAsync(d_words, words, (size_t)cap_words * 8, hipMemcpyHostToDevice, q));
	char *block = nullptr;
	uint32_t dev_cap = 0, count = 0;
	rc = survey_scan_list(d_words, n_words, pitch_words, n_streams, search_bits, max_ac_errors, q, &block, &dev_cap, &count);
	if (rc)
		return rc;
	const uint32_t have = std::min(count, dev_cap);
	if (fo)
		*fo->n_hits = count;
	if (!have)
		return 0;
	// One block for the survey's scratch, its records, and the builder's outputs; a second one, once the number of jobs is
	// known, for the batch reversal (about 8 KiB of scratch per job).
	const uint32_t dev_recs = (uint32_t)std::min<uint64_t>(rec_cap, have);
	const uint32_t dev_jobs = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(work_cap, dev_recs));
	size_t at = 0;
	auto take = [&](size_t bytes) { const size_t here = at; at += sv_up(bytes); return here; };
	const size_t survey_bytes = btbbx_survey_scratch_bytes(have);
	const size_t o_scr = take(survey_bytes), o_recs = take((size_t)dev_recs * sizeof(btbbx_survey_rec));
	const size_t o_c6 = take(clk6_candidates ? (size_t)dev_recs * 64 * sizeof(int16_t) : 0), o_cnt = take(2 * sizeof(uint32_t));
	const size_t o_jobs = take((size_t)dev_jobs * sizeof(btbbx_clock_job)), o_jrec = take((size_t)dev_jobs * sizeof(uint32_t));
	const size_t o_off = take((size_t)have * sizeof(int32_t)), o_ch = take(have);
	// the follow stage's outputs and its one intermediate (d_in)
	const size_t o_fin = take(fo ? (size_t)have * sizeof(btbbx_pkt_in) : 0), o_ffol = take(fo ? (size_t)have * sizeof(btbbx_follow_pkt) : 0);
	const size_t o_fout = take(fo ? (size_t)have * sizeof(btbbx_pkt_out) : 0), o_fsum = take(fo ? (size_t)dev_recs * sizeof(btbbx_follow_sum) : 0);
	char *work = nullptr, *batch = nullptr;
	if (hipMalloc((void **)&work, at) != hipSuccess) {
		(void)hipGetLastError();
		set_error("%s: %zu bytes of device memory for %u hits not available", who, at, have);
		return BTBBX_E_NOMEM;
	}
	btbbx_survey_rec *d_recs = (btbbx_survey_rec *)(work + o_recs);
	int16_t *d_c6 = clk6_candidates ? (int16_t *)(work + o_c6) : nullptr;
	uint32_t *d_rec_count = (uint32_t *)block + 1, *d_n_jobs = (uint32_t *)(work + o_cnt);
	btbbx_clock_job *d_jobs = (btbbx_clock_job *)(work + o_jobs);
	btbbx_clock_result *d_res = nullptr;
	uint32_t counts[2] = {0, 0}, n_piconets = 0;             // jobs, observations
	uint64_t stored = 0;
	hipError_t e = hipSuccess;
	rc = btbbx_survey_hits_device(d_words, n_words, pitch_words, n_streams, (const btbbx_hit *)(block + 256), (const uint32_t *)block, have,
				      channels, &entry, clk_div, clk_phase, BTBBX_MAX_SYMBOLS, d_recs, dev_recs, d_rec_count, d_c6, work + o_scr,
				      survey_bytes, q);
	if (!rc && dev_recs) {
		rc = btbbx_survey_clock_jobs_device(d_recs, d_rec_count, dev_recs, work + o_scr, survey_bytes, have, channels, n_streams, flags,
						    max_obs, d_jobs, dev_jobs, d_n_jobs, (uint32_t *)(work + o_jrec), (int32_t *)(work + o_off),
						    (uint8_t *)(work + o_ch), nullptr, have, d_n_jobs + 1, q);
	}
	// The one place the chain comes to the host: the batch reversal's scratch follows the number of jobs, which is read back
	// together with the number of piconets (btbbx_survey_host reads that one at the same point).
	if (!rc && dev_recs)
		e = hipMemcpyAsync(counts, d_n_jobs, sizeof(counts), hipMemcpyDeviceToHost, q);
	if (!rc && e == hipSuccess)
		e = hipMemcpyAsync(&n_piconets, d_rec_count, sizeof(n_piconets), hipMemcpyDeviceToHost, q);
	if (!rc && e == hipSuccess)
		e = hipStreamSynchronize(q);
	stored = work_cap ? std::min<uint64_t>(counts[0], dev_jobs) : 0;
	if (!rc && e == hipSuccess && stored) {
		const uint32_t nj = (uint32_t)stored;
		const size_t want_cand = candidates ? (size_t)nj * cand_cap * sizeof(uint32_t) : 0;
		const size_t batch_bytes = btbbx_hop_reversal_batch_scratch_bytes(nj, cand_cap);
		size_t bat = 0;
		auto more = [&](size_t bytes) { const size_t here = bat; bat += sv_up(bytes); return here; };
		const size_t o_bs = more(batch_bytes), o_res = more((size_t)nj * sizeof(btbbx_clock_result)), o_cand = more(want_cand);
		if (hipMalloc((void **)&batch, bat) != hipSuccess) {
			(void)hipGetLastError();
			set_error("%s: %zu bytes of device memory for %u jobs not available", who, bat, nj);
			rc = BTBBX_E_NOMEM;
		}
		if (!rc)
			d_res = (btbbx_clock_result *)(batch + o_res);
		// the caller's candidate slots go in first, so that the slots no job writes come back as they were
		if (!rc && want_cand)
			e = hipMemcpyAsync(batch + o_cand, candidates, want_cand, hipMemcpyHostToDevice, q);
		if (!rc && e == hipSuccess)
			rc = btbbx_hop_reversal_batch_device(d_jobs, d_n_jobs, nj, (const int32_t *)(work + o_off), (const uint8_t *)(work + o_ch), have,
							     d_res, want_cand ? (uint32_t *)(batch + o_cand) : nullptr,
							     cand_cap, batch + o_bs, batch_bytes, q);
		const size_t nj_out = (size_t)std::min<uint64_t>(nj, job_cap);           // (= nj without the follow stage)
		if (!rc && e == hipSuccess && results && nj_out)
			e = hipMemcpyAsync(results, d_res, nj_out * sizeof(btbbx_clock_result), hipMemcpyDeviceToHost, q);
		if (!rc && e == hipSuccess && want_cand)
			e = hipMemcpyAsync(candidates, batch + o_cand, want_cand, hipMemcpyDeviceToHost, q);
		if (!rc && e == hipSuccess && jobs)
			e = hipMemcpyAsync(jobs, d_jobs, (size_t)nj * sizeof(btbbx_clock_job), hipMemcpyDeviceToHost, q);
		if (!rc && e == hipSuccess && job_rec && nj_out)
			e = hipMemcpyAsync(job_rec, work + o_jrec, nj_out * sizeof(uint32_t), hipMemcpyDeviceToHost, q);
	}
	if (fo && !rc && e == hipSuccess) {
		// behind the reversal on the same stream: no job stored means no job table at all (stages 0 and 1)
		const uint32_t nj = (uint32_t)stored;
		btbbx_pkt_out *d_out = (btbbx_pkt_out *)(work + o_fout);
		e = hipMemsetAsync(d_out, 0, (size_t)have * sizeof(btbbx_pkt_out), q);  // (the decoder leaves alone what it does not assign)
		if (e == hipSuccess)
			rc = btbbx_follow_hits_device(d_words, n_words, pitch_words, n_streams, (const btbbx_hit *)(block + 256), (const uint32_t *)block,
						      have, d_recs, d_rec_count, dev_recs, nj ? d_jobs : nullptr,
						      nj ? (const uint32_t *)(work + o_jrec) : nullptr, nj ? d_res : nullptr, nj ? d_n_jobs : nullptr, nj,
						      channels, &entry, clk_div, clk_phase, BTBBX_MAX_SYMBOLS, (btbbx_pkt_in *)(work + o_fin),
						      (btbbx_follow_pkt *)(work + o_ffol), d_out, nullptr, (btbbx_follow_sum *)(work + o_fsum), q);
		const size_t n_out = (size_t)std::min<uint64_t>(have, fo->hit_cap), n_sums = (size_t)std::min<uint64_t>(n_piconets, dev_recs);
		if (!rc && e == hipSuccess && n_out)
			e = hipMemcpyAsync(fo->hits, block + 256, n_out * sizeof(btbbx_hit), hipMemcpyDeviceToHost, q);
		if (!rc && e == hipSuccess && n_out)
			e = hipMemcpyAsync(fo->follow, work + o_ffol, n_out * sizeof(btbbx_follow_pkt), hipMemcpyDeviceToHost, q);
		if (!rc && e == hipSuccess && n_out && fo->pkts)
			e = hipMemcpyAsync(fo->pkts, d_out, n_out * sizeof(btbbx_pkt_out), hipMemcpyDeviceToHost, q);
		if (!rc && e == hipSuccess && n_sums)
			e = hipMemcpyAsync(fo->sums, work + o_fsum, n_sums * sizeof(btbbx_follow_sum), hipMemcpyDeviceToHost, q);
	}
	if (!rc && e == hipSuccess) {
		const uint64_t n = std::min<uint64_t>(n_piconets, dev_recs);
		if (n)
			e = hipMemcpyAsync(recs, d_recs, (size_t)n * sizeof(btbbx_survey_rec), hipMemcpyDeviceToHost, q);
		if (e == hipSuccess && n && clk6_candidates)
			e = hipMemcpyAsync(clk6_candidates, d_c6, (size_t)n * 64 * sizeof(int16_t), hipMemcpyDeviceToHost, q);
	}
	const hipError_t f = hipStreamSynchronize(q);
	(void)hipFree(work);
	if (batch)
		(void)hipFree(batch);
	if (rc)
		return rc;
	HIP_TRY(e);
	HIP_TRY(f);
	*n_jobs = counts[0];
	return (int64_t)n_piconets;
}

extern "C" int64_t btbbx_acquire_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				      uint64_t search_bits, int max_ac_errors, const uint8_t *channels,
				      uint32_t clkn0, uint32_t clk_div, uint32_t clk_phase,
				      btbbx_survey_rec *recs, uint64_t rec_cap, int16_t *clk6_candidates,
				      uint32_t flags, uint32_t max_obs,
				      btbbx_clock_job *jobs, uint32_t *job_rec, btbbx_clock_result *results, uint64_t job_cap,
				      uint64_t *n_jobs, uint32_t *candidates, uint32_t cand_cap)
{
	return acquire_run("btbbx_acquire_host", words, n_words, pitch_words, n_streams, search_bits, max_ac_errors, channels, clkn0, clk_div,
			   clk_phase, recs, rec_cap, clk6_candidates, flags, max_obs, jobs, job_rec, results, job_cap, n_jobs, candidates, cand_cap,
			   nullptr);
}

// ---- following ------------------------------------------------------------------------------------------

extern "C" int btbbx_follow_hits_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
					const btbbx_hit *d_hits, const uint32_t *d_count, uint32_t cap,
					const btbbx_survey_rec *d_recs, const uint32_t *d_rec_count, uint32_t rec_cap,
					const btbbx_clock_job *d_jobs, const uint32_t *d_job_rec, const btbbx_clock_result *d_results,
					const uint32_t *d_n_jobs, uint32_t job_cap,
					const uint8_t *channels, const btbbx_pkt_in *entry, uint32_t clk_div, uint32_t clk_phase,
					uint32_t max_length, btbbx_pkt_in *d_in, btbbx_follow_pkt *d_follow, btbbx_pkt_out *d_out,
					uint32_t *d_lengths, btbbx_follow_sum *d_sums, void *hip_stream)
{
	const char *who = "btbbx_follow_hits_device";
	if (!d_words || !d_hits || !d_recs || !d_in || !d_follow || !d_out || !d_sums || !entry) {
		set_error("%s: null pointer (words, hits, records, entry state or an output)", who);
		return BTBBX_E_ARG;
	}
	if (job_cap && (!d_jobs || !d_job_rec || !d_results)) {
		set_error("%s: job_cap = %u without jobs, their records or their results", who, job_cap);
		return BTBBX_E_ARG;
	}
	if (!cap || !rec_cap) {
		set_error("%s: cap = %u, rec_cap = %u", who, cap, rec_cap);
		return BTBBX_E_ARG;
	}
	int rc = survey_check_args(who, n_words, n_streams, channels, entry, clk_div, clk_phase);
	if (rc)
		return rc;
	if (((uintptr_t)d_words & 7) || ((uintptr_t)d_hits & 7) || ((uintptr_t)d_out & 7) || ((uintptr_t)d_count & 3) || ((uintptr_t)d_recs & 3) ||
	    ((uintptr_t)d_rec_count & 3) || ((uintptr_t)d_jobs & 3) || ((uintptr_t)d_job_rec & 3) || ((uintptr_t)d_results & 3) ||
	    ((uintptr_t)d_n_jobs & 3) || ((uintptr_t)d_in & 3) || ((uintptr_t)d_follow & 3) || ((uintptr_t)d_lengths & 3) || ((uintptr_t)d_sums & 3)) {
		set_error("%s: misaligned pointer (words, hits and decoded packets 8 bytes, everything else 4)", who);
		return BTBBX_E_ARG;
	}
	if (n_streams > 1 && pitch_words < n_words) {
		set_error("%s: pitch_words < n_words", who);
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	hipStream_t q = (hipStream_t)hip_stream;
	SurveyChannels table;
	memset(&table, 0, sizeof(table));
	if (channels)
		memcpy(table.ch, channels, n_streams);
	// (launched for the caps, worked for the counts)
	const uint32_t rec_blocks = (uint32_t)(((uint64_t)rec_cap + FW_THREADS - 1) / FW_THREADS);
	const uint32_t hit_blocks = (uint32_t)(((uint64_t)cap + FW_THREADS - 1) / FW_THREADS);
	hipLaunchKernelGGL(follow_stage_kernel, dim3(rec_blocks), dim3(FW_THREADS), 0, q, (const uint32_t *)d_recs, d_rec_count, rec_cap, d_job_rec,
			   d_results, d_n_jobs, job_cap, d_sums);
	hipLaunchKernelGGL(follow_clock_kernel, dim3(hit_blocks), dim3(FW_THREADS), 0, q, d_hits, d_count, cap, (const uint32_t *)d_recs, d_rec_count,
			   rec_cap, d_jobs, d_results, (const btbbx_follow_sum *)d_sums, table, channels ? 0 : 1, n_streams, *entry, clk_div, clk_phase,
			   d_in, d_follow);
	HIP_TRY(hipGetLastError());
	// the decoder is btbbx_decode_hits_counted_device's; without a count in HBM its form for cap packets
	rc = d_count ? btbbx_decode_hits_counted_device(d_words, n_words, pitch_words, d_hits, d_in, d_count, cap, max_length, d_out, d_lengths, q)
		     : btbbx_decode_hits_device(d_words, n_words, pitch_words, d_hits, d_in, cap, max_length, d_out, d_lengths, q);
	if (rc)
		return rc;
	hipLaunchKernelGGL(follow_tally_kernel, dim3(hit_blocks), dim3(FW_THREADS), 0, q, (const btbbx_follow_pkt *)d_follow,
			   (const btbbx_pkt_out *)d_out, d_count, cap, d_sums);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

extern "C" int64_t btbbx_follow_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				     uint64_t search_bits, int max_ac_errors, const uint8_t *channels,
				     uint32_t clkn0, uint32_t clk_div, uint32_t clk_phase,
				     btbbx_survey_rec *recs, uint64_t rec_cap, uint32_t flags, uint32_t max_obs,
				     uint32_t *job_rec, btbbx_clock_result *results, uint64_t job_cap, uint64_t *n_jobs,
				     btbbx_hit *hits, btbbx_follow_pkt *follow, btbbx_pkt_out *pkts, uint64_t hit_cap, uint64_t *n_hits,
				     btbbx_follow_sum *sums)
{
	if (!rec_cap || !recs || !sums || !n_jobs || !n_hits || (hit_cap && (!hits || !follow))) {
		set_error("btbbx_follow_host: rec_cap = 0, or no recs, sums, n_jobs, n_hits, hits or follow");
		return BTBBX_E_ARG;
	}
	const FollowOut fo = {hits, follow, pkts, hit_cap, n_hits, sums};
	return acquire_run("btbbx_follow_host", words, n_words, pitch_words, n_streams, search_bits, max_ac_errors, channels, clkn0, clk_div,
			   clk_phase, recs, rec_cap, nullptr, flags, max_obs, nullptr, job_rec, results, job_cap, n_jobs, nullptr, 0, &fo);
}
