// le_csa2.h -- LE channel selection algorithm #2 (included by le.hip, behind le_track.h): for every connection the tracking timed,
// the absolute connEventCounter of its first event -- the one of the 65 536 hypotheses under which most events lie on the channel
// the algorithm predicts --, the prediction for every packet, and which of the two algorithms explains the connection.  The
// contract is in include/btbbx.h (btbbx_le_csa2_device), the reasoning in DESIGN 3.8.3.  All arithmetic is integer arithmetic.
// The stage reads what the tracking wrote (its records, not its scratch):
//
//   1. le_csa2_base_kernel      one workgroup: N and K; the prefix sums of n_events over the TIMED connections: every connection's
//      first entry in the event table
//   2. le_csa2_event_kernel     one lane per candidate: a member stores (n_e mod 2^16, C_e) at its connection's base + its event
//   3. le_csa2_score_kernel     work item = (connection, block of 1024 hypotheses), taken from a grid of fixed size that strides over
//      K x 64; four hypotheses per lane, the events staged through LDS in tiles, expected() tabulated in LDS for the window of
//      counters the block meets in the tile; the block's best score, its smallest c0 and the best score of the others go to scratch
//   4. le_csa2_verdict_kernel   one wave per connection: the 64 partials folded with the tie rule, the events off the prediction
//      tallied, the record
//   5. le_csa2_pkt_kernel       one lane per candidate: the per-packet record
//
// The kernels are extern "C": their symbols carry no parameter types, so the substrings by which the resource tests tell the
// kernel families apart (a btbbx_le_track_pkt parameter would mangle into one) stay out of them.
// Nothing here synchronises or reads back but the host wrapper.
#pragma once
#include "le_track.h"

#define LC_BLOCKS      64u                 // hypothesis blocks per connection
#define LC_PER_LANE    4u                  // hypotheses per lane: 65 536 / LC_BLOCKS / LE_THREADS
#define LC_PER_BLOCK   (LC_PER_LANE * LE_THREADS)   // hypotheses per block
#define LC_TILE        512u                // events staged in LDS per round
#define LC_SPAN        3072u               // the counters a tile's events may span and still be looked up in the window
#define LC_BASE_ROUND  (8u * LE_THREADS)   // connections per round of the base kernel's scan
#define LC_MAP37       0x1fffffffffULL

static_assert(LC_BLOCKS * LC_PER_LANE * LE_THREADS == 65536u, "the blocks cover the 16-bit counter");
static_assert(sizeof(btbbx_le_csa2) == 24 && offsetof(btbbx_le_csa2, n_off) == 4 && offsetof(btbbx_le_csa2, n_second) == 8 &&
	      offsetof(btbbx_le_csa2, channel_id) == 12 && offsetof(btbbx_le_csa2, counter0) == 14 && offsetof(btbbx_le_csa2, flags) == 16 &&
	      offsetof(btbbx_le_csa2, reserved) == 20, "btbbx_le_csa2 layout (libbtbb_amd.LE_CSA2_DTYPE)");
static_assert(sizeof(btbbx_le_csa2_pkt) == 8 && offsetof(btbbx_le_csa2_pkt, prn) == 2 && offsetof(btbbx_le_csa2_pkt, unmapped) == 4 &&
	      offsetof(btbbx_le_csa2_pkt, expected) == 5 && offsetof(btbbx_le_csa2_pkt, on_hop) == 6 && offsetof(btbbx_le_csa2_pkt, reserved) == 7,
	      "btbbx_le_csa2_pkt layout (libbtbb_amd.LE_CSA2_PKT_DTYPE)");

// params[0] = candidates worked on (N), [1] = connections stored (K); ebase: K + 1 entries; etab: one entry per event;
// part: LC_BLOCKS entries per connection (best S, its smallest c0, the best S of the block's others, 0)
struct LcLayout {
	size_t params, ebase, etab, part, total;
};

static LcLayout le_csa2_layout(uint32_t cand_cap, uint32_t conn_cap)
{
	LcLayout L;
	const size_t c = cand_cap ? cand_cap : 1, k = conn_cap ? conn_cap : 1;
	size_t at = 0;
	auto take = [&](size_t bytes) { const size_t here = at; at += ld_up(bytes); return here; };
	L.params = take(256);
	L.ebase = take((k + 1) * 4);
	L.etab = take(c * 4);
	L.part = take(k * LC_BLOCKS * sizeof(uint4));
	L.total = at;
	return L;
}

__device__ __forceinline__ uint32_t lc_channel_id(uint32_t aa) { return (aa >> 16) ^ (aa & 0xffffu); }

// rule 3: three rounds of (reverse the bits of each byte, multiply by 17 and add the channel identifier) between two XORs
__device__ __forceinline__ uint32_t lc_prn(uint32_t counter, uint32_t chid)
{
	uint32_t x = counter ^ chid;
#pragma unroll
	for (int r = 0; r < 3; r++) {
		const uint32_t v = __brev(x);                       // (byte 0 reversed in bits 24..31, byte 1 in bits 16..23)
		x = (v >> 24) | ((v >> 8) & 0xff00u);
		x = (17u * x + chid) & 0xffffu;
	}
	return x ^ chid;
}

// rule 4 with the table of used channels found by counting bits (the verdict and the packets; the scoring pass keeps it in LDS)
__device__ __forceinline__ uint32_t lc_expected(uint32_t prn, unsigned long long map, uint32_t n_used, uint32_t flags, uint32_t &unmapped)
{
	unmapped = prn % 37u;
	if ((map >> unmapped) & 1)
		return unmapped;
	if ((flags & BTBBX_LE_CSA2_REMAP) && n_used)
		return lt_nth_bit(map, (n_used * prn) >> 16);
	return 0xff;
}

// the connection's map and n_used (the popcount of the map's 37 bits, which is what the tracking stored as n_used), and whether
// its track is TIMED
__device__ __forceinline__ bool lc_track(const btbbx_le_track *tracks, uint32_t g, unsigned long long &map, uint32_t &n_used)
{
	map = tracks[g].map_mask & LC_MAP37;
	n_used = (uint32_t)__popcll(map);
	return (reinterpret_cast<const uint32_t *>(tracks + g)[10] >> 24) & BTBBX_LE_TRACK_TIMED;
}

// ---- 1. event bases -----------------------------------------------------------------------------------------------------

// ebase[g] = the events of the TIMED connections in front of g, ebase[K] = all of them; never beyond N (a member opens at most
// one event, so the sums of a list the tracking wrote stay below it; records from elsewhere are cut there)
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_csa2_base_kernel(const uint32_t *d_cand_count, uint32_t cand_cap,
									     const uint32_t *d_conn_count, uint32_t conn_cap,
									     const btbbx_le_track *tracks, uint32_t *params, uint32_t *ebase)
{
	__shared__ unsigned long long lds[LT_WAVES];
	const uint32_t tid = threadIdx.x, nh = *d_cand_count, kh = *d_conn_count;
	const uint32_t n = nh < cand_cap ? nh : cand_cap, k = kh < conn_cap ? kh : conn_cap;
	if (tid == 0) {
		params[0] = n;
		params[1] = k;
	}
	unsigned long long carry = 0;
	for (uint32_t base = 0; base < k; base += LC_BASE_ROUND) {     // (uniform over the workgroup)
		uint32_t v[8];
		unsigned long long mine = 0;
#pragma unroll
		for (uint32_t j = 0; j < 8; j++) {
			const uint32_t g = base + tid * 8 + j;
			v[j] = 0;
			if (g < k && ((reinterpret_cast<const uint32_t *>(tracks + g)[10] >> 24) & BTBBX_LE_TRACK_TIMED))
				v[j] = tracks[g].n_events;
			mine += v[j];
		}
		unsigned long long total;
		unsigned long long run = carry + lt_block_scan64(mine, lds, total);
#pragma unroll
		for (uint32_t j = 0; j < 8; j++) {
			const uint32_t g = base + tid * 8 + j;
			if (g < k)
				ebase[g] = run < n ? (uint32_t)run : n;
			run += v[j];
		}
		carry += total;
	}
	if (tid == 0)
		ebase[k] = carry < n ? (uint32_t)carry : n;
}

// ---- 2. event table -----------------------------------------------------------------------------------------------------

// rule 1: a member stores its event's relative counter and channel; every member of an event stores the same word
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_csa2_event_kernel(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts,
									      const uint32_t *params, const uint32_t *ebase, uint32_t *etab)
{
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x;
	if (i >= params[0])
		return;
	const uint32_t g = reinterpret_cast<const uint2 *>(cands + i)[2].y;
	const uint4 p = reinterpret_cast<const uint4 *>(pkts)[i];          // rank, event, counter, channel | ...
	if (g >= params[1] || p.x == 0xffffffffu)
		return;
	const uint32_t base = ebase[g], count = ebase[g + 1] - base;
	if (p.y < count)
		etab[base + p.y] = (p.z & 0xffffu) | ((p.w & 0xffu) << 16);
}

// ---- 3. scoring ---------------------------------------------------------------------------------------------------------

// two (best key, runner-up) pairs of disjoint hypothesis sets -> the pair of their union; key = S << 32 | (0xffff - c0), so the
// larger key is the larger score, ties the smaller c0, and the loser's score is a candidate for the runner-up
__device__ __forceinline__ void lc_merge(unsigned long long &top, uint32_t &second, unsigned long long o_top, uint32_t o_second)
{
	const unsigned long long lo = top < o_top ? top : o_top;
	top = top < o_top ? o_top : top;
	second = second > o_second ? second : o_second;
	second = second > (uint32_t)(lo >> 32) ? second : (uint32_t)(lo >> 32);
}

__device__ __forceinline__ void lc_wave_merge(unsigned long long &top, uint32_t &second)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		const unsigned long long o_top = lt_shfl_xor64(top, d);
		const uint32_t o_second = __shfl_xor(second, d);
		lc_merge(top, second, o_top, o_second);
	}
}

// rule 5.  Work item w = connection w / 64, hypotheses c0 = 1024 (w mod 64) + 4 thread + r, r in 0..3.  The events come through LDS in
// tiles of LC_TILE.  With d_e = (n_e - n_first) mod 2^16, n_first the tile's first n_e, hypothesis 1024 b + j meets event e at the
// counter 1024 b + n_first + j + d_e: the block needs expected() on a WINDOW of 1024 + span counters only, span = the tile's largest
// d_e.  So a tile costs a lane (1024 + span) / 256 evaluations of rules 3 and 4 for the window and, per event, a quarter of an LDS
// read of four events (d_e | C_e << 16, worked out by the lanes that stage the tile; the same words for all lanes: a broadcast), two
// reads of the window -- the four bytes at j + d_e .. j + d_e + 3, the shift d_e mod 4 being the same for all lanes -- and four
// compares.  span is taken from the tile's last event (the events lie in time order) and cut at LC_SPAN; an event with a larger
// d_e -- behind a long gap in the capture, or in a list that is not in time order -- is evaluated directly in a second loop, which
// runs only for a tile that has one: four times rules 3 and 4 per lane
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_csa2_score_kernel(const uint32_t *params, const btbbx_le_conn *conns,
									      const btbbx_le_track *tracks, const uint32_t *ebase,
									      const uint32_t *etab, uint32_t flags, uint4 *part)
{
	__shared__ uint32_t window[(LC_PER_BLOCK + LC_SPAN) / 4 + 2];       // bytes; one dword of slack for the read behind the last
	__shared__ uint32_t ev[LC_TILE];
	__shared__ __attribute__((aligned(16))) uint32_t near[LC_TILE];
	__shared__ unsigned long long wave_top[LT_WAVES];
	__shared__ uint32_t wave_second[LT_WAVES];
	__shared__ uint8_t used[40];
	const uint32_t tid = threadIdx.x;
	const unsigned long long items = (unsigned long long)params[1] * LC_BLOCKS;
	for (unsigned long long w = blockIdx.x; w < items; w += gridDim.x) {
		const uint32_t g = (uint32_t)(w / LC_BLOCKS), block0 = (uint32_t)(w % LC_BLOCKS) * LC_PER_BLOCK, first = block0 + LC_PER_LANE * tid;
		unsigned long long map;
		uint32_t n_used;
		if (!lc_track(tracks, g, map, n_used))
			continue;                                       // (uniform over the workgroup)
		const uint32_t chid = lc_channel_id(conns[g].access_address);
		const uint32_t base = ebase[g], count = ebase[g + 1] - base;
		const bool remap = (flags & BTBBX_LE_CSA2_REMAP) && n_used;
		auto expected_of = [&](uint32_t counter) {              // rule 4, the table of used channels in LDS
			const uint32_t prn = lc_prn(counter & 0xffffu, chid), un = prn % 37u;
			if ((map >> un) & 1)
				return un;
			return remap ? (uint32_t)used[(n_used * prn) >> 16] : 0xffu;
		};
		__syncthreads();                                        // the work item before this one is done with the LDS
		if (tid < 37 && ((map >> tid) & 1))
			used[__popcll(map & ((1ULL << tid) - 1))] = (uint8_t)tid;
		uint32_t s[LC_PER_LANE];
#pragma unroll
		for (uint32_t r = 0; r < LC_PER_LANE; r++)
			s[r] = 0;
		for (uint32_t t0 = 0; t0 < count; t0 += LC_TILE) {
			const uint32_t m = count - t0 < LC_TILE ? count - t0 : LC_TILE, m4 = (m + 3) & ~3u;
			const uint32_t n_first = etab[base + t0] & 0xffffu, d_last = ((etab[base + t0 + m - 1] & 0xffffu) - n_first) & 0xffffu;
			const uint32_t span = d_last < LC_SPAN ? d_last : LC_SPAN;
			if (t0)
				__syncthreads();                                // the tile before this one is done with
			// near[i] = d_e | C_e << 16 for an event inside the window; for one beyond it, and for the padding to a multiple of four,
			// a word that matches nothing (no expected() is 0xfe)
			int far = 0;
			for (uint32_t i = tid; i < m4; i += LE_THREADS) {
				uint32_t word = 0xfeu << 16;
				if (i < m) {
					const uint32_t v = etab[base + t0 + i], d = ((v & 0xffffu) - n_first) & 0xffffu;
					ev[i] = v;
					if (d <= span)
						word = d | (v & 0xffff0000u);
					else
						far = 1;
				}
				near[i] = word;
			}
			far = __syncthreads_or(far);                            // (the first tile: used[] as well)
			for (uint32_t k = tid; k < LC_PER_BLOCK + span; k += LE_THREADS)
				reinterpret_cast<uint8_t *>(window)[k] = (uint8_t)expected_of(block0 + n_first + k);
			__syncthreads();
			for (uint32_t i = 0; i < m4; i += 4) {                  // four events at a time: their LDS reads are in flight together
				const uint4 q = *reinterpret_cast<const uint4 *>(near + i);
				const uint32_t words[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
				for (int u = 0; u < 4; u++) {
					const uint32_t v = __builtin_amdgcn_readfirstlane(words[u]), ch = v >> 16, d = v & 0xffffu, at = tid + (d >> 2);
					const uint32_t four = __builtin_amdgcn_alignbyte(window[at + 1], window[at], d & 3u);
#pragma unroll
					for (uint32_t r = 0; r < LC_PER_LANE; r++)
						s[r] += ((four >> (8 * r)) & 0xffu) == ch ? 1u : 0u;
				}
			}
			if (!far)
				continue;                                       // (uniform over the workgroup)
			for (uint32_t i = 0; i < m; i++) {
				const uint32_t v = __builtin_amdgcn_readfirstlane(ev[i]);
				if ((((v & 0xffffu) - n_first) & 0xffffu) <= span)
					continue;
#pragma unroll
				for (uint32_t r = 0; r < LC_PER_LANE; r++)
					s[r] += expected_of(first + r + v) == v >> 16 ? 1u : 0u;
			}
		}
		unsigned long long top = ((unsigned long long)s[0] << 32) | (0xffffu - first);
		uint32_t second = 0;
#pragma unroll
		for (uint32_t r = 1; r < LC_PER_LANE; r++)
			lc_merge(top, second, ((unsigned long long)s[r] << 32) | (0xffffu - (first + r)), 0);
		lc_wave_merge(top, second);
		if ((tid & 63) == 0) {
			wave_top[tid >> 6] = top;
			wave_second[tid >> 6] = second;
		}
		__syncthreads();
		if (tid == 0) {
			for (uint32_t k = 1; k < LT_WAVES; k++)
				lc_merge(top, second, wave_top[k], wave_second[k]);
			part[w] = make_uint4((uint32_t)(top >> 32), 0xffffu - ((uint32_t)top & 0xffffu), second, 0);
		}
	}
}

// ---- 4. verdict ---------------------------------------------------------------------------------------------------------

// one wave per connection, one partial per lane: the winner with the tie rule; the runner-up -- the other blocks' best scores and
// what the winner's block found beside it --; the events whose prediction under the winner is known and differs; the record
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_csa2_verdict_kernel(const uint32_t *params, const btbbx_le_conn *conns,
										const btbbx_le_track *tracks, const uint32_t *ebase,
										const uint32_t *etab, const uint4 *part, uint32_t flags,
										btbbx_le_csa2 *sel)
{
	const uint32_t lane = threadIdx.x & 63, g = blockIdx.x * LT_WAVES + (threadIdx.x >> 6);
	if (g >= params[1])
		return;
	unsigned long long map;
	uint32_t n_used;
	const bool timed = lc_track(tracks, g, map, n_used);
	const uint32_t chid = lc_channel_id(conns[g].access_address);
	uint32_t n_on = 0, n_off = 0, second = 0, counter0 = 0, out_flags = 0;
	if (timed) {
		const uint4 p = part[(size_t)g * LC_BLOCKS + lane];
		unsigned long long top = ((unsigned long long)p.x << 32) | (0xffffu - (p.y & 0xffffu));
		second = p.z;
		lc_wave_merge(top, second);
		n_on = (uint32_t)(top >> 32);
		counter0 = 0xffffu - ((uint32_t)top & 0xffffu);
		const uint32_t base = ebase[g], count = ebase[g + 1] - base;
		for (uint32_t e = lane; e < count; e += 64) {
			const uint32_t v = etab[base + e];
			uint32_t unmapped;
			const uint32_t expected = lc_expected(lc_prn((counter0 + v) & 0xffffu, chid), map, n_used, flags, unmapped);
			n_off += expected != 0xffu && expected != (v >> 16) ? 1u : 0u;
		}
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1)
			n_off += __shfl_xor(n_off, d);
		out_flags = BTBBX_LE_CSA2_EVALUATED;
		if (n_on > second)
			out_flags |= BTBBX_LE_CSA2_UNIQUE | (n_on > tracks[g].n_on_hop ? BTBBX_LE_CSA2_PREFERRED : 0u);
	}
	if (lane)
		return;
	uint2 *out = reinterpret_cast<uint2 *>(sel + g);
	out[0] = make_uint2(n_on, n_off);
	out[1] = make_uint2(second, chid | (counter0 << 16));
	out[2] = make_uint2(out_flags, 0);
}

// ---- 5. packets ---------------------------------------------------------------------------------------------------------

// rule 6 (and the records of rules 1 and 2): one lane per candidate
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_csa2_pkt_kernel(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts,
									    const uint32_t *params, const btbbx_le_track *tracks,
									    const btbbx_le_csa2 *sel, uint32_t flags, btbbx_le_csa2_pkt *sel_pkts)
{
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x;
	if (i >= params[0])
		return;
	const uint32_t g = reinterpret_cast<const uint2 *>(cands + i)[2].y;
	const uint4 p = reinterpret_cast<const uint4 *>(pkts)[i];
	uint2 out = make_uint2(0xffffffffu, 0xffffffffu);
	if (g < params[1] && p.x != 0xffffffffu) {
		const uint2 s = reinterpret_cast<const uint2 *>(sel + g)[1];     // n_second; channel_id | counter0 << 16
		out = make_uint2(0, 0xffffu);                                    // not EVALUATED: counter 0, prn 0, 0xff, 0xff, 0, 0
		if (reinterpret_cast<const uint32_t *>(sel + g)[4] & BTBBX_LE_CSA2_EVALUATED) {
			unsigned long long map;
			uint32_t n_used, unmapped;
			lc_track(tracks, g, map, n_used);
			const uint32_t counter = ((s.y >> 16) + p.z) & 0xffffu, prn = lc_prn(counter, s.y & 0xffffu);
			const uint32_t expected = lc_expected(prn, map, n_used, flags, unmapped);
			out = make_uint2(counter | (prn << 16), unmapped | (expected << 8) | (expected == (p.w & 0xffu) ? 1u << 16 : 0u));
		}
	}
	reinterpret_cast<uint2 *>(sel_pkts)[i] = out;
}

// ---- host side ----------------------------------------------------------------------------------------------------------

extern "C" size_t btbbx_le_csa2_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap)
{
	return le_csa2_layout(cand_cap, conn_cap).total;
}

// the five launches of one run
static int le_csa2_launch(const btbbx_le_cand *d_cands, const uint32_t *d_count, uint32_t cap, const btbbx_le_conn *d_conns,
			  const uint32_t *d_conn_count, uint32_t conn_cap, const btbbx_le_track *d_tracks, const btbbx_le_track_pkt *d_pkts,
			  uint32_t flags, btbbx_le_csa2 *d_sel, btbbx_le_csa2_pkt *d_sel_pkts, void *d_scratch, hipStream_t q)
{
	const LcLayout L = le_csa2_layout(cap, conn_cap);
	char *s = (char *)d_scratch;
	uint32_t *params = (uint32_t *)(s + L.params), *ebase = (uint32_t *)(s + L.ebase), *etab = (uint32_t *)(s + L.etab);
	uint4 *part = (uint4 *)(s + L.part);
	const dim3 per_cand((cap + LE_THREADS - 1) / LE_THREADS), wg(LE_THREADS);
	// the work items live in device memory (K x 64): a grid that fills the machine strides over them
	const uint32_t score_grid = (uint32_t)std::min<uint64_t>((uint64_t)conn_cap * LC_BLOCKS, 8ull * (uint32_t)std::max(ctx().num_cus, 1));
	flags &= BTBBX_LE_CSA2_REMAP;
	hipLaunchKernelGGL(le_csa2_base_kernel, dim3(1), wg, 0, q, d_count, cap, d_conn_count, conn_cap, d_tracks, params, ebase);
	hipLaunchKernelGGL(le_csa2_event_kernel, per_cand, wg, 0, q, d_cands, d_pkts, params, ebase, etab);
	hipLaunchKernelGGL(le_csa2_score_kernel, dim3(score_grid), wg, 0, q, params, d_conns, d_tracks, ebase, etab, flags, part);
	hipLaunchKernelGGL(le_csa2_verdict_kernel, dim3((conn_cap + LT_WAVES - 1) / LT_WAVES), wg, 0, q, params, d_conns, d_tracks, ebase, etab,
			   part, flags, d_sel);
	hipLaunchKernelGGL(le_csa2_pkt_kernel, per_cand, wg, 0, q, d_cands, d_pkts, params, d_tracks, d_sel, flags, d_sel_pkts);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

extern "C" int btbbx_le_csa2_device(const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
				    const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
				    const btbbx_le_track *d_tracks, const btbbx_le_track_pkt *d_pkts, uint32_t flags,
				    btbbx_le_csa2 *d_sel, btbbx_le_csa2_pkt *d_sel_pkts,
				    void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
	const char *who = "btbbx_le_csa2_device";
	const LcLayout L = le_csa2_layout(cand_cap, conn_cap);
	if (!d_cands || !d_cand_count || !d_conns || !d_conn_count || !d_tracks || !d_pkts || !d_sel || !d_sel_pkts || !d_scratch ||
	    scratch_bytes < L.total) {
		set_error("%s: null pointer, or scratch of %zu bytes needed and %zu given", who, L.total, scratch_bytes);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_cands & 7) || ((uintptr_t)d_conns & 7) || ((uintptr_t)d_tracks & 7) || ((uintptr_t)d_pkts & 7) ||
	    ((uintptr_t)d_sel & 7) || ((uintptr_t)d_sel_pkts & 7) || ((uintptr_t)d_scratch & 7) || ((uintptr_t)d_cand_count & 3) ||
	    ((uintptr_t)d_conn_count & 3)) {
		set_error("%s: misaligned pointer (records and scratch 8 bytes, the counters 4)", who);
		return BTBBX_E_ARG;
	}
	const int rc = ctx_require();
	if (rc)
		return rc;
	if (!cand_cap || !conn_cap)
		return BTBBX_OK;
	return le_csa2_launch(d_cands, d_cand_count, cand_cap, d_conns, d_conn_count, conn_cap, d_tracks, d_pkts, flags, d_sel, d_sel_pkts,
			      d_scratch, (hipStream_t)hip_stream);
}
