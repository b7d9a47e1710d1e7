// le_cfind.h -- promiscuous discovery of LE Coded PHY connections: the access address and the CRCInit of every coded data-channel
// packet of a capture, neither of them given.  The contract is include/btbbx.h ("promiscuous LE Coded connection discovery", rules
// 1..12); tests/_le_cfind.py states it in Python.  The coded scan (le_coded.h) finds a packet whose access address it is told; here
// the address is what block 1 of the packet decodes to, and the 336-symbol match is counted against THAT address.
//
//   1. le_cfind_scan_kernel     the tile frame of le_coded_scan_kernel and its address-free pre-filter (bitslice.h le_coded_filter);
//      behind it, per survivor, a second address-free bound: the exact mismatches of the 80 preamble symbols plus the equal pairs
//      among the 128 pairs of the 64 address groups.  What passes leaves as a 16-byte pre-record (offset, stream, the bound)
//   2. le_cfind_decode_kernel   eight lanes per pre-record, lane = trellis state: block 1, the exact count against the re-encoded
//      decoded address, offenses, CI, block 2 to the lag step, header and fit, the rest of block 2, header_moved, dewhitening and
//      the CRC register run backwards.  Survivors are ranked by a ballot into the candidate list
//
// The candidates have the shape of btbbx_le_cand, so btbbx_le_discover_group_device (le_discover.h) groups them unchanged.
// This header is a translation unit's worth (le_cfind.hip includes it and nothing else of the LE family): no kernel of le.hip or
// le_coded.hip shares a compilation with it (DESIGN 3.8.10 records what new neighbours did once).
#pragma once
#include "tile_scan.h"
#include "le_record.h"
#include <algorithm>

#define LCF_THREADS 256
#define LCF_TILE_WORDS (2 * LCF_THREADS)         // two words (128 offsets) per lane and tile
#define LCF_HALO_WORDS 6                         // a lane reads its two words and the six behind them: 128 + 335 symbols
#define LCF_RING 128                             // per-wave ring of pre-records (entries)
#define LCF_GROUP 8                              // lanes per pre-record: one per trellis state
#define LCF_RECS 8                               // pre-records per workgroup (one wave)
#define LCF_WORDS 66                             // decision words per state: N <= 2083 steps, 32 per word
#define LCF_INF (1u << 24)                       // an unreachable state's metric
#define LCF_LAG_STEP (16 + BTBBX_LE_CODED_LAG)   // the step behind which the provisional header is read
#define LCF_PREAMBLE 0x3c3c3c3cu                 // 0 0 1 1 1 1 0 0, symbol k = bit k

struct LeCfindScanArgs {
	const uint64_t *words;
	uint64_t n_words;
	uint64_t pitch_words;
	uint64_t search_bits;
	uint32_t tiles_per_stream;
	uint32_t n_streams;
	uint32_t max_err;
	const uint16_t *phys;
	uint4 *pre;
	uint32_t pre_cap;
	uint32_t *pre_count;
};

// ---- 1. the scan ------------------------------------------------------------------------------------------------------

// the equal pairs (k, k + 2), k mod 4 in {0, 1}, of a dword of window symbols whose groups of four start at bit 0
__device__ __forceinline__ uint32_t lcf_equal_pairs(uint32_t w)
{
	return ~(w ^ (w >> 2)) & 0x33333333u;
}

// Frame, fetch, chains and ring as le_coded_scan_kernel.  A tile of a stream on an advertising channel is skipped by the whole
// wave (rule 1), its successor's fetch already under way.  The pre-filter runs with the run-time limit as it is.  A survivor's
// eleven funnel-shifted window dwords give the second bound: popcount(preamble ^ 0 0 1 1 1 1 0 0 ...) over symbols 0..79, and,
// over symbols 80..335, the pairs that ANY mapped address makes unequal and the window has equal (a group is 0011 or 1100).  The two
// terms count over disjoint symbols and each is at most the mismatches rule 4 counts there, whatever address block 1 decodes to:
// bound <= rule 4's count, so bound > max_errors loses no candidate.
__global__ __launch_bounds__(LCF_THREADS) void le_cfind_scan_kernel(LeCfindScanArgs a)
{
	__shared__ uint4 ring_mem[LCF_THREADS / 64][LCF_RING];
	const uint32_t tid = threadIdx.x, lane = tid & 63;
	const uint32_t tiles_per_stream = a.tiles_per_stream;
	uint32_t stream = 0, t = blockIdx.x;
	while (t >= tiles_per_stream && stream < a.n_streams) {
		t -= tiles_per_stream;
		stream++;
	}
	const uint32_t lw = tid * 2;
	uint4 *ring = ring_mem[tid >> 6];
	uint32_t q_head = 0, q_tail = 0;                // wave-uniform, free running
	auto flush = [&](uint32_t n) {                  // the n <= 64 oldest entries -> the pre-record list
		uint32_t base = 0;
		if (lane == 0)
			base = atomicAdd(a.pre_count, n);
		base = __builtin_amdgcn_readfirstlane(base);
		if (lane < n && base < a.pre_cap && lane < a.pre_cap - base)
			a.pre[base + lane] = ring[(q_head + lane) & (LCF_RING - 1)];
		q_head += n;
	};
	auto stage = [&](bool hit, uint32_t s, uint64_t offset, uint32_t bound) {
		const uint64_t mask = __ballot(hit);
		if (!mask)
			return;
		if (q_tail - q_head + 64 > LCF_RING)
			flush(64);
		if (hit) {
			const uint32_t slot = q_tail + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
			uint4 rec;
			rec.x = (uint32_t)offset;
			rec.y = (uint32_t)(offset >> 32);
			rec.z = s;
			rec.w = bound;
			ring[slot & (LCF_RING - 1)] = rec;
		}
		q_tail += (uint32_t)__popcll(mask);
	};
	u32x4 nx[4];
	auto fetch = [&](uint32_t ft, uint32_t fstream) {   // the lane's eight words of tile ft: zero behind the stream's end
		uint32_t bytes = 0;                             // wave-uniform
		const uint64_t *tp = a.words;
		if (fstream < a.n_streams) {
			const uint64_t first = (uint64_t)ft * LCF_TILE_WORDS;
			tp = a.words + (uint64_t)fstream * a.pitch_words + first;
			const uint64_t left = first < a.n_words ? a.n_words - first : 0;
			bytes = (uint32_t)(left < LCF_TILE_WORDS + LCF_HALO_WORDS ? left : LCF_TILE_WORDS + LCF_HALO_WORDS) * 8u;
		}
		const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t *>(tp), 0, (int)bytes, 0x00020000);
#pragma unroll
		for (int u = 0; u < 4; u++)
			nx[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(lw * 8u + 16u * u), 0, 0);
	};
	fetch(t, stream);
	while (stream < a.n_streams) {
		const uint64_t word0 = (uint64_t)t * LCF_TILE_WORDS + lw;
		uint32_t D[16], m[4];
#pragma unroll
		for (int u = 0; u < 4; u++) {
			D[4 * u] = nx[u].x;
			D[4 * u + 1] = nx[u].y;
			D[4 * u + 2] = nx[u].z;
			D[4 * u + 3] = nx[u].w;
		}
		const uint32_t this_stream = stream;
		t += gridDim.x;
		while (t >= tiles_per_stream && stream < a.n_streams) {
			t -= tiles_per_stream;
			stream++;
		}
		fetch(t, stream);                               // the next tile's words are loaded while this one is worked on
		if (le_channel_index(a.phys[this_stream]) >= 37)    // rule 1, wave-uniform: an advertising channel yields no candidate
			continue;
		le_coded_filter(D, a.max_err, m);
#pragma unroll
		for (int c = 0; c < 4; c++) {
			const uint64_t first_off = word0 * 64 + 32u * c;
			m[c] &= first_off >= a.search_bits ? 0u
				: (a.search_bits - first_off >= 32 ? 0xffffffffu : ((1u << (uint32_t)(a.search_bits - first_off)) - 1u));
		}
		// survivors: one offset of every chain per pass, passes until no lane of the wave has one left
		for (;;) {
			uint32_t any = 0;
#pragma unroll
			for (int c = 0; c < 4; c++)
				any |= m[c];
			if (!__ballot(any != 0))
				break;
#pragma unroll
			for (int c = 0; c < 4; c++) {
				if (!__ballot(m[c] != 0))
					continue;
				const uint32_t p = (uint32_t)__builtin_ctz(m[c] | 0x80000000u);
				uint32_t W[11];
#pragma unroll
				for (int q = 0; q < 11; q++)
					W[q] = alignbit(D[c + q + 1], D[c + q], p);
				uint32_t e = (uint32_t)__popc(W[0] ^ LCF_PREAMBLE) + (uint32_t)__popc(W[1] ^ LCF_PREAMBLE) +
					     (uint32_t)__popc((W[2] ^ LCF_PREAMBLE) & 0xffffu);
				e += (uint32_t)__popc(lcf_equal_pairs(W[2]) & 0xffff0000u) + (uint32_t)__popc(lcf_equal_pairs(W[10]) & 0xffffu);
#pragma unroll
				for (int q = 3; q < 10; q++)
					e += (uint32_t)__popc(lcf_equal_pairs(W[q]));
				const bool hit = m[c] != 0 && e <= a.max_err;
				m[c] &= m[c] - 1;
				stage(hit, this_stream, word0 * 64 + 32u * c + p, e);
			}
		}
		while (q_tail - q_head >= 64)
			flush(64);
	}
	while (q_tail != q_head)
		flush(q_tail - q_head < 64 ? q_tail - q_head : 64);
}

// ---- 2. the trellis, the candidate ------------------------------------------------------------------------------------

struct LeCfindDecodeArgs {
	const uint64_t *words;
	uint64_t n_words;
	uint64_t pitch_words;
	const uint4 *pre;
	const uint32_t *pre_count;
	uint32_t pre_cap;
	const uint16_t *phys;
	uint32_t max_len;
	uint32_t max_err;
	uint2 *cands;                                   // btbbx_le_cand, moved as three 8-byte words
	uint4 *info;                                    // btbbx_le_coded_cand_info, or null
	uint32_t cand_cap;
	uint32_t *cand_count;
};

// The decoder's mapping (le_coded.h le_coded_decode_kernel): eight lanes per pre-record, lane = state s' = b1 | b2 << 1 | b3 << 2
// AFTER the step, predecessors (s' >> 1) | x << 2 in the lanes src0 and src1 of the group; the two transitions into s' send
// complementary symbols, so one branch metric is formed and the other is S minus it; x = 0 survives on equal sums.  Decisions go 32
// steps per word into LDS (2112 bytes per pre-record), the path's bits into 264 more.  A group stays in the kernel to its end but
// works only while `live`: it goes dead at the first rule that fails, in the order block 1, rule 4's exact count (the group's first
// six lanes take 64 symbols each against the re-encoded decoded address), offenses and CI, block 2 to the lag step, header and fit,
// the rest of block 2 and its trace-back, header_moved, and at last the CRCInit.  The CRC runs backwards over the dewhitened octets
// with 3.8.1's inverse table (crc_inv[T[i] >> 16] = T[i] << 8 | i: the state before an octet d is (s << 8 ^ crc_inv[s >> 16]) ^ d),
// one look-up per octet where the bit-serial walk takes eight dependent steps of four instructions; the table is 1 KiB of LDS next
// to 19 KiB of decisions and limits nothing.  One lane walks trace-backs and CRC, as in the decoder.  All lanes meet at the end:
// a ballot ranks the survivors, the wave's lane 0 adds their number to the counter once.
__global__ __launch_bounds__(LCF_GROUP * LCF_RECS) void le_cfind_decode_kernel(LeCfindDecodeArgs a)
{
	__shared__ uint32_t dec[LCF_RECS][LCF_WORDS][LCF_GROUP];
	__shared__ uint32_t path[LCF_RECS][LCF_WORDS];
	__shared__ uint32_t crc_inv[256];
	__shared__ uint16_t wh_tab[128];
	const uint32_t tid = threadIdx.x;
	const uint32_t have = *a.pre_count, n = have < a.pre_cap ? have : a.pre_cap;
	if ((uint64_t)blockIdx.x * LCF_RECS >= n)           // (the grid is sized by pre_cap: a workgroup without work builds no table)
		return;
	for (uint32_t k = tid; k < 256; k += LCF_GROUP * LCF_RECS) {
		const uint32_t s = le_crc_tab_entry(k);
		crc_inv[s >> 16] = (s << 8) | k;
	}
	for (uint32_t k = tid; k < 128; k += LCF_GROUP * LCF_RECS)
		wh_tab[k] = le_wh_tab_entry(k);
	__syncthreads();
	const uint32_t g = tid / LCF_GROUP, st = tid % LCF_GROUP;
	// the workgroup's pre-records, eight at a time (wave-uniform trip count; the wave meets behind every eight)
	for (uint64_t i0 = (uint64_t)blockIdx.x * LCF_RECS; i0 < n; i0 += (uint64_t)gridDim.x * LCF_RECS) {
	const uint64_t i = i0 + g;
	bool live = i < n;
	const uint4 pr = live ? a.pre[i] : make_uint4(0, 0, 0, 0);
	const uint64_t offset = ((uint64_t)pr.y << 32) | pr.x;
	const uint32_t stream = pr.z;
	const uint64_t *w = a.words + (uint64_t)stream * a.pitch_words;
	const uint64_t n_words = a.n_words;
	auto sym64 = [&](uint64_t bit) -> uint64_t {       // 64 symbols from `bit`, zeros past the stream's end
		const uint64_t wi = bit >> 6;
		const uint32_t sh = (uint32_t)(bit & 63);
		const uint64_t lo = wi < n_words ? w[wi] : 0;
		const uint64_t hi = sh && wi + 1 < n_words ? w[wi + 1] : 0;
		return (lo >> sh) | (sh ? hi << (64 - sh) : 0);
	};
	// the symbols of the transition from (s' >> 1), b3 = 0, with input b = s' & 1
	const uint32_t in_b = st & 1u, r1 = (st >> 1) & 1u, r2 = (st >> 2) & 1u;
	const uint32_t a0 = in_b ^ r1 ^ r2, a1 = in_b ^ r2;
	const uint32_t e2 = a0 | (a1 << 1);                                       // a0 is sent first
	const uint32_t e8 = (a0 ? 0x3u : 0xcu) | ((a1 ? 0x3u : 0xcu) << 4);      // 1 -> 1 1 0 0, 0 -> 0 0 1 1, first symbol in bit 0
	const uint32_t first_lane = tid - st;
	const uint32_t src0 = first_lane | (st >> 1), src1 = src0 | 4u;
	uint32_t metric = 0, acc = 0;
	// steps [t0, t1) of a block whose first symbol is at `base`; the decision word in progress is stored at the last step too
	auto forward = [&](uint64_t base, uint32_t S, uint32_t t0, uint32_t t1) {
		const uint32_t e = S == 8 ? e8 : e2, smask = S == 8 ? 0xffu : 3u;
		uint32_t t = t0;
		while (t < t1) {
			uint64_t chunk = sym64(base + (uint64_t)S * t);
			const uint32_t stop = min(t + 64u / S, t1);
			for (; t < stop; t++) {
				const uint32_t bm0 = (uint32_t)__popc(((uint32_t)chunk & smask) ^ e);
				chunk >>= S;
				const uint32_t c0 = (uint32_t)__shfl((int)metric, (int)src0) + bm0;
				const uint32_t c1 = (uint32_t)__shfl((int)metric, (int)src1) + (S - bm0);
				const uint32_t d = c1 < c0 ? 1u : 0u;
				metric = d ? c1 : c0;
				if ((t & 31) == 0)
					acc = 0;
				acc |= d << (t & 31);
				if ((t & 31) == 31 || t + 1 == t1)
					dec[g][t >> 5][st] = acc;
			}
		}
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
		__builtin_amdgcn_wave_barrier();
	};
	// the path that ends in state s after step T: its first `keep` input bits -> path[g]
	auto trace = [&](uint32_t s, uint32_t T, uint32_t keep) {
		uint32_t wacc = 0;
		for (uint32_t t = T; t-- > 0;) {
			const uint32_t x = (dec[g][t >> 5][s] >> (t & 31)) & 1u;
			if (t < keep) {
				wacc |= (s & 1u) << (t & 31);
				if ((t & 31) == 0) {
					path[g][t >> 5] = wacc;
					wacc = 0;
				}
			}
			s = (s >> 1) | (x << 2);
		}
	};
	uint32_t aa = 0, ci = 0, metric1 = 0, metric2 = 0, errors = 0, S = 0, N = 0, h0 = 0, h1 = 0, lag_header = 0, init = 0, ch = 0;
	if (live) {
		// rule 3: block 1
		ch = le_channel_index(a.phys[stream]);
		metric = st ? LCF_INF : 0u;
		forward(offset + 80, 8, 0, 37);
		metric1 = (uint32_t)__shfl((int)metric, (int)first_lane);
		if (st == 0) {
			trace(0, 37, 34);
			aa = path[g][0];
			ci = path[g][1] & 3u;
		}
		aa = (uint32_t)__shfl((int)aa, (int)first_lane);
		ci = (uint32_t)__shfl((int)ci, (int)first_lane);
		// rule 4: lane q < 6 of the group counts window symbols 64 q .. 64 q + 63 (the sixth: sixteen) against preamble + mapped,
		// coded AA': octet k of the pattern is the preamble's for k < 10 and the two mapped coded bits of address bit k - 10 behind it
		const uint32_t g0 = aa ^ (aa << 1) ^ (aa << 2) ^ (aa << 3), g1 = aa ^ (aa << 2) ^ (aa << 3);
		uint64_t pat = 0;
#pragma unroll
		for (uint32_t b = 0; b < 8; b++) {
			const uint32_t k = 8u * st + b, bit = (k - 10u) & 31u;
			const uint32_t code = (((g0 >> bit) & 1u) ? 0x3u : 0xcu) | ((((g1 >> bit) & 1u) ? 0x3u : 0xcu) << 4);
			pat |= (uint64_t)(k < 10 ? 0x3cu : code) << (8u * b);
		}
		const uint64_t valid = st < 5 ? ~0ull : st == 5 ? 0xffffull : 0ull;
		errors = st < 6 ? (uint32_t)__popcll((sym64(offset + 64u * st) ^ pat) & valid) : 0u;
		errors += (uint32_t)__shfl_xor((int)errors, 1);
		errors += (uint32_t)__shfl_xor((int)errors, 2);
		errors += (uint32_t)__shfl_xor((int)errors, 4);
		// rules 4, 5, 6
		live = errors <= a.max_err && le_data_offenses(aa) == 0 && ci < 2;
	}
	if (live) {
		// rule 7: block 2 up to the lag step, the provisional header; rule 8
		S = ci == 0 ? 8u : 2u;
		const uint64_t base2 = offset + 376;
		metric = st ? LCF_INF : 0u;
		forward(base2, S, 0, LCF_LAG_STEP);
		uint32_t best = (metric << 3) | st;                     // smallest metric, then smallest state
		best = min(best, (uint32_t)__shfl_xor((int)best, 1));
		best = min(best, (uint32_t)__shfl_xor((int)best, 2));
		best = min(best, (uint32_t)__shfl_xor((int)best, 4));
		if (st == 0) {
			trace(best & 7u, LCF_LAG_STEP, 16);
			lag_header = path[g][0] & 0xffffu;
		}
		lag_header = (uint32_t)__shfl((int)lag_header, (int)first_lane);
		const uint32_t wt = wh_tab[(ch & 0x3fu) | 0x40u];
		h0 = (lag_header ^ wt) & 0xffu;
		h1 = ((lag_header >> 8) ^ wh_tab[wt >> 8]) & 0xffu;
		N = 8u * (h1 + 5u) + 3u;
		live = (h0 & 3u) != 0 && (h0 & 0xe0u) == 0 && h1 <= a.max_len && offset + 376 + (uint64_t)S * N <= n_words * 64;
	}
	if (live) {
		// rule 9: the rest of the forward pass, the path from state 0
		forward(offset + 376, S, LCF_LAG_STEP, N);
		metric2 = (uint32_t)__shfl((int)metric, (int)first_lane);
		uint32_t moved = 0;
		if (st == 0) {
			trace(0, N, N - 3);
			moved = (path[g][0] & 0xffffu) != lag_header ? 1u : 0u;
			if (!moved) {
				// rule 10: dewhiten the 2 + L + 3 octets in place, then the register backwards from the received CRC
				uint8_t *oct = reinterpret_cast<uint8_t *>(path[g]);
				const uint32_t pdu = 2u + h1;
				uint32_t ws = (ch & 0x3fu) | 0x40u;
				for (uint32_t k = 0; k < pdu + 3; k++) {
					const uint32_t wt = wh_tab[ws];
					oct[k] = (uint8_t)(oct[k] ^ wt);
					ws = wt >> 8;
				}
				uint32_t s = (uint32_t)oct[pdu] | ((uint32_t)oct[pdu + 1] << 8) | ((uint32_t)oct[pdu + 2] << 16);
				for (uint32_t k = pdu; k-- > 0;)
					s = ((s << 8) ^ crc_inv[s >> 16]) ^ oct[k];
				init = __builtin_bitreverse32(s) >> 8;          // reflected register -> CRCInit as the spec writes it
			}
		}
		live = (uint32_t)__shfl((int)moved, (int)first_lane) == 0;
	}
	// rules 11 and 12
	const bool emit = live && st == 0;
	const uint64_t mask = __ballot(emit);
	if (!mask)
		continue;
	uint32_t base = 0;
	if (tid == 0)
		base = atomicAdd(a.cand_count, (uint32_t)__popcll(mask));
	base = __builtin_amdgcn_readfirstlane(base);
	const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
	if (emit && slot < a.cand_cap) {
		uint2 *out = a.cands + 3 * (size_t)slot;
		out[0] = make_uint2(pr.x, pr.y);
		out[1] = make_uint2(aa, init);
		out[2] = make_uint2(stream | (h0 << 16) | (h1 << 24), ch);  // conn = the channel index until grouping
		if (a.info)
			a.info[slot] = make_uint4(376u + S * N, metric2, metric1 | (errors << 16) | (ci << 24), S);
	}
	}
}

// ---- host side ----------------------------------------------------------------------------------------------------

static_assert(sizeof(btbbx_le_coded_cand_info) == 16 && offsetof(btbbx_le_coded_cand_info, metric2) == 4 &&
	      offsetof(btbbx_le_coded_cand_info, metric1) == 8 && offsetof(btbbx_le_coded_cand_info, errors) == 10 &&
	      offsetof(btbbx_le_coded_cand_info, ci) == 11 && offsetof(btbbx_le_coded_cand_info, s) == 12,
	      "btbbx_le_coded_cand_info: 16 bytes (libbtbb_amd LE_CODED_CAND_INFO_DTYPE)");
static_assert(sizeof(btbbx_le_cand) == 24 && offsetof(btbbx_le_cand, access_address) == 8 && offsetof(btbbx_le_cand, crc_init) == 12 &&
	      offsetof(btbbx_le_cand, stream) == 16 && offsetof(btbbx_le_cand, header0) == 18 && offsetof(btbbx_le_cand, length) == 19 &&
	      offsetof(btbbx_le_cand, conn) == 20, "btbbx_le_cand layout");

#define LCF_MAX_PRE 0xfffffff0u

static int le_cfind_check_args(const char *who, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, uint64_t search_bits, uint32_t max_len,
			       int max_errors)
{
	if (max_errors < 0 || max_errors > BTBBX_LE_CODED_MAX_ERRORS) {
		set_error("%s: max_errors must be 0..%d", who, BTBBX_LE_CODED_MAX_ERRORS);
		return BTBBX_E_ARG;
	}
	if (max_len > 255) {
		set_error("%s: max_len must be 0..255", who);
		return BTBBX_E_ARG;
	}
	return check_scan_args(who, BTBBX_LE_CODED_PATTERN, n_words, pitch_words, n_streams, search_bits);
}

extern "C" size_t btbbx_le_cfind_scratch_bytes(uint32_t pre_cap)
{
	return (size_t)pre_cap * sizeof(uint4);
}

// both kernels; *d_pre_count is cleared here (the decoder reads the pre-records it counts), *d_cand_count is added to
static int le_cfind_launch(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, uint64_t search_bits,
			   const uint16_t *d_phys, uint32_t max_len, int max_errors, btbbx_le_cand *d_cands, btbbx_le_coded_cand_info *d_info,
			   uint32_t cand_cap, uint32_t *d_cand_count, uint32_t *d_pre_count, void *d_scratch, uint32_t pre_cap, hipStream_t q)
{
	HIP_TRY(hipMemsetAsync(d_pre_count, 0, sizeof(uint32_t), q));
	if (search_bits == 0)
		return BTBBX_OK;
	LeCfindScanArgs a;
	a.words = d_words;
	a.n_words = n_words;
	a.pitch_words = n_streams > 1 ? pitch_words : n_words;
	a.search_bits = search_bits;
	a.n_streams = n_streams;
	a.max_err = (uint32_t)max_errors;
	a.phys = d_phys;
	a.pre = (uint4 *)d_scratch;
	a.pre_cap = pre_cap;
	a.pre_count = d_pre_count;
	TileGrid g;
	const int rc = tile_grid("btbbx_le_cfind_scan_device", search_bits, n_words, n_streams, LCF_TILE_WORDS, ctx().num_cus, &g);
	if (rc)
		return rc;
	a.tiles_per_stream = (uint32_t)g.tiles_per_stream;
	hipLaunchKernelGGL(le_cfind_scan_kernel, dim3(g.grid), dim3(LCF_THREADS), 0, q, a);
	HIP_TRY(hipGetLastError());
	LeCfindDecodeArgs d;
	d.words = d_words;
	d.n_words = n_words;
	d.pitch_words = a.pitch_words;
	d.pre = a.pre;
	d.pre_count = d_pre_count;
	d.pre_cap = pre_cap;
	d.phys = d_phys;
	d.max_len = max_len;
	d.max_err = (uint32_t)max_errors;
	d.cands = (uint2 *)d_cands;
	d.info = (uint4 *)d_info;
	d.cand_cap = cand_cap;
	d.cand_count = d_cand_count;
	// at most 32 workgroups per CU, each striding over the pre-records: a grid by pre_cap alone is millions of empty workgroups
	const uint32_t need = (pre_cap + LCF_RECS - 1) / LCF_RECS, most = (uint32_t)ctx().num_cus * 32u;
	hipLaunchKernelGGL(le_cfind_decode_kernel, dim3(need < most ? need : most), dim3(LCF_GROUP * LCF_RECS), 0, q, d);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

extern "C" int btbbx_le_cfind_scan_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
					  uint64_t search_bits, const uint16_t *d_phys_channel, uint32_t max_len, int max_errors,
					  btbbx_le_cand *d_cands, btbbx_le_coded_cand_info *d_info, uint32_t cand_cap, uint32_t *d_cand_count,
					  uint32_t *d_pre_count, void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
	const char *who = "btbbx_le_cfind_scan_device";
	int rc = le_cfind_check_args(who, n_words, pitch_words, n_streams, search_bits, max_len, max_errors);
	if (rc)
		return rc;
	if (!d_words || !d_phys_channel || !d_cand_count || !d_pre_count || (!d_cands && cand_cap)) {
		set_error("%s: null pointer", who);
		return BTBBX_E_ARG;
	}
	if (!d_scratch || scratch_bytes < sizeof(uint4)) {
		set_error("%s: scratch of at least %zu bytes needed (btbbx_le_cfind_scratch_bytes(pre_cap), pre_cap >= 1) and %zu given", who,
			  sizeof(uint4), scratch_bytes);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_words & 7) || ((uintptr_t)d_cands & 7) || ((uintptr_t)d_info & 15) || ((uintptr_t)d_cand_count & 3) ||
	    ((uintptr_t)d_pre_count & 3) || ((uintptr_t)d_phys_channel & 1) || ((uintptr_t)d_scratch & 15)) {
		set_error("%s: misaligned pointer (words and candidates 8 bytes, info and scratch 16, the counters 4, channels 2)", who);
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	const size_t room = scratch_bytes / sizeof(uint4);
	return le_cfind_launch(d_words, n_words, pitch_words, n_streams, search_bits, d_phys_channel, max_len, max_errors, d_cands, d_info, cand_cap,
			       d_cand_count, d_pre_count, d_scratch, room > LCF_MAX_PRE ? LCF_MAX_PRE : (uint32_t)room, (hipStream_t)hip_stream);
}

static size_t lcf_up(size_t x) { return (x + 255) & ~(size_t)255; }

// btbbx_le_discover_host's chain (le_host.h le_disc_host_chain) with the coded scan in it: copy in, scan -- again with room when
// the pre-record list or the candidate list was short --, the unchanged grouping, copy out
extern "C" int64_t btbbx_le_cfind_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				       uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, int max_errors, uint32_t min_count,
				       btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap, uint64_t *n_cands_out)
{
	const char *who = "btbbx_le_cfind_host";
	int rc = le_cfind_check_args(who, n_words, pitch_words, n_streams, search_bits, max_len, max_errors);
	if (rc)
		return rc;
	if (!words || !phys_channel || (!conns && conn_cap) || (!cands && cand_cap)) {
		set_error("%s: null pointer", who);
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	if (n_cands_out)
		*n_cands_out = 0;
	if (n_streams == 1)
		pitch_words = n_words;
	CallScope scope;
	hipStream_t q = scope_stream();
	const uint64_t cap_words = (uint64_t)(n_streams - 1) * pitch_words + n_words;
	const size_t words_bytes = lcf_up((size_t)(cap_words + 1) * 8);
	char *dblock = (char *)scope_device(words_bytes + 2 * (size_t)n_streams);
	if (!dblock)
		return BTBBX_E_NOMEM;
	const uint64_t *d_words = (const uint64_t *)dblock;
	uint16_t *d_phys = (uint16_t *)(dblock + words_bytes);
	HIP_TRY(hipMemcpyAsync(dblock, words, (size_t)cap_words * 8, hipMemcpyHostToDevice, q));
	HIP_TRY(hipMemcpyAsync(d_phys, phys_channel, 2 * (size_t)n_streams, hipMemcpyHostToDevice, q));
	// first guesses: noise leaves a pre-record at 1e-8 of the offsets at max_errors 63 and next to no candidate
	const uint64_t guess = search_bits / 4096 * n_streams + 4096;
	uint32_t pre_cap = guess > LCF_MAX_PRE ? LCF_MAX_PRE : (uint32_t)guess, dev_cap = pre_cap;
	uint32_t counts[2] = {0, 0};                            // pre-records, candidates
	char *block = nullptr;
	size_t pre_bytes = 0, cand_bytes = 0, scratch_bytes = 0;
	uint32_t dev_conns = 0;
	for (int pass = 0; pass < 3; pass++) {
		pre_bytes = lcf_up(btbbx_le_cfind_scratch_bytes(pre_cap));
		cand_bytes = lcf_up((size_t)dev_cap * sizeof(btbbx_le_cand));
		scratch_bytes = lcf_up(btbbx_le_discover_scratch_bytes(dev_cap));
		dev_conns = (uint32_t)std::min<uint64_t>(conn_cap, dev_cap);
		block = (char *)scope_hits(256 + pre_bytes + cand_bytes + scratch_bytes + lcf_up((size_t)dev_conns * sizeof(btbbx_le_conn)));
		if (!block)
			return BTBBX_E_NOMEM;
		HIP_TRY(hipMemsetAsync(block, 0, 4 * sizeof(uint32_t), q));
		rc = le_cfind_launch(d_words, n_words, pitch_words, n_streams, search_bits, d_phys, max_len, max_errors,
				     (btbbx_le_cand *)(block + 256 + pre_bytes), nullptr, dev_cap, (uint32_t *)block + 1, (uint32_t *)block, block + 256,
				     pre_cap, q);
		if (rc)
			return rc;
		HIP_TRY(hipMemcpyAsync(counts, block, sizeof(counts), hipMemcpyDeviceToHost, q));
		HIP_TRY(hipStreamSynchronize(q));
		if (counts[0] <= pre_cap && counts[1] <= dev_cap)
			break;
		// (a short pre-record list hid candidates: the candidate count of this pass is a lower bound then, and a third pass may follow)
		pre_cap = std::max(pre_cap, std::min(counts[0], LCF_MAX_PRE));
		dev_cap = std::max(dev_cap, counts[1]);
	}
	const uint32_t count = counts[1], have = std::min(count, dev_cap);
	if (n_cands_out)
		*n_cands_out = count;
	if (!have)
		return 0;
	uint32_t *d_count = (uint32_t *)block + 1, *d_conn_count = (uint32_t *)block + 2;
	btbbx_le_cand *d_cands = (btbbx_le_cand *)(block + 256 + pre_bytes);
	btbbx_le_conn *d_conns = (btbbx_le_conn *)(block + 256 + pre_bytes + cand_bytes + scratch_bytes);
	rc = btbbx_le_discover_group_device(d_cands, d_count, dev_cap, min_count, d_conns, dev_conns, d_conn_count, block + 256 + pre_bytes + cand_bytes,
					    scratch_bytes, q);
	if (rc)
		return rc;
	uint32_t n_conns = 0;
	HIP_TRY(hipMemcpyAsync(&n_conns, d_conn_count, sizeof(uint32_t), hipMemcpyDeviceToHost, q));
	HIP_TRY(hipStreamSynchronize(q));
	const uint64_t nc = std::min<uint64_t>(n_conns, dev_conns), nk = std::min<uint64_t>(have, cand_cap);
	if (nc)
		HIP_TRY(hipMemcpyAsync(conns, d_conns, (size_t)nc * sizeof(btbbx_le_conn), hipMemcpyDeviceToHost, q));
	if (nk)
		HIP_TRY(hipMemcpyAsync(cands, d_cands, (size_t)nk * sizeof(btbbx_le_cand), hipMemcpyDeviceToHost, q));
	HIP_TRY(hipStreamSynchronize(q));
	return (int64_t)n_conns;
}
