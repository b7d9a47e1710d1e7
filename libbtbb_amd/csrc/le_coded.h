// le_coded.h -- Bluetooth LE Coded PHY (Core v5.x Vol 6 Part B 2.2, 3.1, 3.2, 3.3): the search for preamble + coded access
// address over whole captures and the Viterbi decoder behind it.  The contract is include/btbbx.h ("LE Coded PHY scan", rules
// 1..8); tests/_le_coded.py states the air format literally.
//
// Air format: 80 preamble symbols (ten times 0 0 1 1 1 1 0 0), FEC block 1 (AA 32 bits LSB first, CI 2 bits, TERM1 3 zero bits;
// always S = 8: 296 symbols), FEC block 2 (PDU, CRC-24, TERM2 3 zero bits: N = 8 (L + 5) + 3 bits at S = 8 or 2 symbols per bit).
// CRC, then whitening (PDU and CRC only), then the rate-1/2 K = 4 encoder (a0 = b ^ b1 ^ b2 ^ b3, a1 = b ^ b2 ^ b3, a0 first,
// state 0 at the start of each block), then at S = 8 the mapper 0 -> 0011, 1 -> 1100.
//
// This header is a translation unit's worth (le_coded.hip includes it and nothing else of the LE family), so that no kernel of
// le.hip shares a compilation with it.
#pragma once
#include "tile_scan.h"
#include "le_record.h"
#include <algorithm>

#define LEC_THREADS 256
#define LEC_TILE_WORDS (2 * LEC_THREADS)         // two words (128 offsets) per lane and tile, as le_scan_kernel
#define LEC_HALO_WORDS 6                         // a lane reads its two words and the six behind them: 128 + 335 symbols
#define LEC_RING 128                             // per-wave hit ring (entries)
#define LEC_PAT_DWORDS 11                        // 336 pattern symbols: ten dwords and sixteen bits

// the 336 symbols preamble + mapped, coded AA (encoder from state 0, no CI), symbol k = bit k & 31 of dword k >> 5
static void le_coded_pattern(uint32_t aa, uint32_t *pat)
{
	for (int q = 0; q < LEC_PAT_DWORDS; q++)
		pat[q] = 0;
	uint32_t k = 0;
	auto put = [&](uint32_t sym) {
		pat[k >> 5] |= (sym & 1u) << (k & 31);
		k++;
	};
	for (int i = 0; i < 80; i++)
		put((0x3cu >> (i & 7)) & 1u);                   // 0 0 1 1 1 1 0 0
	uint32_t b1 = 0, b2 = 0, b3 = 0;
	for (int i = 0; i < 32; i++) {
		const uint32_t b = (aa >> i) & 1u;
		const uint32_t a[2] = { b ^ b1 ^ b2 ^ b3, b ^ b2 ^ b3 };
		for (int j = 0; j < 2; j++)
			for (int s = 0; s < 4; s++)
				put(a[j] ? (0x3u >> s) : (0xcu >> s));  // 1 -> 1 1 0 0, 0 -> 0 0 1 1
		b3 = b2;
		b2 = b1;
		b1 = b;
	}
}

struct LeCodedScanArgs {
	const uint64_t *words;
	uint64_t n_words;
	uint64_t pitch_words;
	uint64_t search_bits;
	uint32_t tiles_per_stream;
	uint32_t n_streams;
	uint32_t pat[LEC_PAT_DWORDS];
	uint32_t max_err;
	uint32_t aa;
	btbbx_hit *hits;
	uint32_t hit_cap;
	uint32_t *hit_count;
};

// The 1M scan's frame: one workgroup of 256 lanes works on a tile of 512 words of one stream at a time, a lane owns two
// consecutive words and reads the six behind them (sixteen dwords D[0..15]): chain c = the 32 offsets starting at dword c, whose
// 336-symbol windows lie in D[c .. c + 11].  The bit-sliced necessary condition (bitslice.h le_coded_filter: equal symbols
// among 160 pairs that the pattern of ANY access address makes unequal) runs for the four chains at once; survivors get the exact
// count popcount(window ^ pattern) over eleven funnel-shifted dwords.  Hits are ranked with a ballot and mbcnt into a per-wave ring
// and leave it 64 at a time, with one counter atomic per 64 hits.  Words behind the stream's end read as zero through the buffer
// descriptor's range check; offsets at or behind search_bits are masked in every tile (a few instructions against the filter's 900).
__global__ __launch_bounds__(LEC_THREADS) void le_coded_scan_kernel(LeCodedScanArgs a)
{
	__shared__ uint4 ring_mem[LEC_THREADS / 64][LEC_RING];
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
	auto flush = [&](uint32_t n) {                  // the n <= 64 oldest entries -> the global hit list
		uint32_t base = 0;
		if (lane == 0)
			base = atomicAdd(a.hit_count, n);
		base = __builtin_amdgcn_readfirstlane(base);
		if (lane < n && base + lane < a.hit_cap)
			reinterpret_cast<uint4 *>(a.hits)[base + lane] = ring[(q_head + lane) & (LEC_RING - 1)];
		q_head += n;
	};
	auto stage = [&](bool hit, uint32_t s, uint64_t offset, uint32_t nerr) {
		const uint64_t mask = __ballot(hit);
		if (!mask)
			return;
		if (q_tail - q_head + 64 > LEC_RING)
			flush(64);
		if (hit) {
			const uint32_t slot = q_tail + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
			uint4 rec;
			rec.x = (uint32_t)offset;
			rec.y = (uint32_t)(offset >> 32);
			rec.z = a.aa;                                   // the AA searched for
			rec.w = nerr | (s << 16);
			ring[slot & (LEC_RING - 1)] = rec;
		}
		q_tail += (uint32_t)__popcll(mask);
	};
	u32x4 nx[4];
	auto fetch = [&](uint32_t ft, uint32_t fstream) {   // the lane's eight words of tile ft: zero behind the stream's end
		uint32_t bytes = 0;                             // wave-uniform
		const uint64_t *tp = a.words;
		if (fstream < a.n_streams) {
			const uint64_t first = (uint64_t)ft * LEC_TILE_WORDS;
			tp = a.words + (uint64_t)fstream * a.pitch_words + first;
			const uint64_t left = first < a.n_words ? a.n_words - first : 0;
			bytes = (uint32_t)(left < LEC_TILE_WORDS + LEC_HALO_WORDS ? left : LEC_TILE_WORDS + LEC_HALO_WORDS) * 8u;
		}
		const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t *>(tp), 0, (int)bytes, 0x00020000);
#pragma unroll
		for (int u = 0; u < 4; u++)
			nx[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(lw * 8u + 16u * u), 0, 0);
	};
	fetch(t, stream);
	while (stream < a.n_streams) {
		const uint64_t word0 = (uint64_t)t * LEC_TILE_WORDS + lw;
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
				uint32_t e = (uint32_t)__popc((alignbit(D[c + 11], D[c + 10], p) ^ a.pat[10]) & 0xffffu);
#pragma unroll
				for (int q = 0; q < 10; q++)
					e += (uint32_t)__popc(alignbit(D[c + q + 1], D[c + q], p) ^ a.pat[q]);
				const bool hit = m[c] != 0 && e <= a.max_err;
				m[c] &= m[c] - 1;
				stage(hit, this_stream, word0 * 64 + 32u * c + p, e);
			}
		}
		while (q_tail - q_head >= 64)
			flush(64);
	}
	if (q_tail != q_head)
		flush(q_tail - q_head);
}

// ---- stage 2: the trellis, the record ---------------------------------------------------------------------------------

#define LEC_GROUP 8                              // lanes per hit: one per trellis state
#define LEC_HITS 8                               // hits per workgroup (one wave)
#define LEC_WORDS 66                             // decision words per state: N <= 2083 steps, 32 per word
#define LEC_INF (1u << 24)                       // an unreachable state's metric (a path's is at most 8 * 2083)

// Eight lanes per hit, lane = state s' = b1 | b2 << 1 | b3 << 2 AFTER the step; its predecessors (s' >> 1) | x << 2 are the
// lanes src0 (x = 0) and src1 of the same group, fixed for the kernel.  The two transitions into s' send complementary symbols
// (they differ in b3, which enters both a0 and a1), so a lane forms one branch metric with XOR and popcount and the other is
// S minus it.  A step: two cross-lane reads of the metrics, add, compare (x = 0 survives on equal sums), select; the decision
// bits go 32 steps per word into LDS (dec[hit][word][state]: 2112 bytes per hit), the symbols arrive 64 at a time.  Block 1
// (37 steps at S = 8), the lag trace-back at step 40 of block 2, the rest of the forward pass and the final trace-back run here
// one after the other; the group's first lane walks the trace-backs, writes the path's bits to LDS and hands them to le_record
// octet by octet.  Groups of one wave differ in N: each runs its own trip counts and leaves when it is done.
__global__ __launch_bounds__(LEC_GROUP * LEC_HITS) void le_coded_decode_kernel(const uint64_t *words, uint64_t n_words, uint64_t pitch_words,
									       const btbbx_hit *hits, const uint32_t *d_count, uint32_t cap,
									       const uint16_t *phys, uint32_t crc_init_reflected,
									       btbbx_le_pkt *out, btbbx_le_coded_info *info)
{
	__shared__ uint32_t dec[LEC_HITS][LEC_WORDS][LEC_GROUP];
	__shared__ uint32_t path[LEC_HITS][LEC_WORDS];
	__shared__ uint32_t crc_tab[256];
	__shared__ uint16_t wh_tab[128];
	const uint32_t tid = threadIdx.x;
	for (uint32_t k = tid; k < 256; k += LEC_GROUP * LEC_HITS)
		crc_tab[k] = le_crc_tab_entry(k);
	for (uint32_t k = tid; k < 128; k += LEC_GROUP * LEC_HITS)
		wh_tab[k] = le_wh_tab_entry(k);
	__syncthreads();
	const uint32_t n = min(*d_count, cap);
	const uint32_t g = tid / LEC_GROUP, st = tid % LEC_GROUP;
	const uint32_t i = blockIdx.x * LEC_HITS + g;
	if (i >= n)
		return;
	const btbbx_hit h = hits[i];
	const uint64_t *w = words + (uint64_t)h.stream * pitch_words;
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
	const uint32_t ws0 = (le_channel_index(phys[h.stream]) & 0x3fu) | 0x40u;

	// rule 3: block 1
	metric = st ? LEC_INF : 0u;
	forward(h.offset + 80, 8, 0, 37);
	const uint32_t metric1 = (uint32_t)__shfl((int)metric, (int)first_lane);
	uint32_t aa = 0, ci = 0;
	if (st == 0) {
		trace(0, 37, 34);
		aa = path[g][0];
		ci = path[g][1] & 3u;
	}
	ci = (uint32_t)__shfl((int)ci, (int)first_lane);
	const uint32_t S = ci == 0 ? 8u : ci == 1 ? 2u : 0u;   // rule 4
	uint32_t *io = reinterpret_cast<uint32_t *>(info + i);
	if (S == 0) {
		if (st == 0) {
			le_record([](uint32_t) { return 0u; }, [](uint32_t) { return false; }, 0, crc_tab, wh_tab, phys[h.stream], crc_init_reflected,
				  aa, h, out[i]);
			io[0] = 376;
			io[1] = 0;
			io[2] = metric1 | (ci << 16);
			io[3] = 0;
		}
		return;
	}
	// rule 5: block 2 up to the lag step, the provisional header
	const uint64_t base2 = h.offset + 376;
	metric = st ? LEC_INF : 0u;
	forward(base2, S, 0, 16 + BTBBX_LE_CODED_LAG);
	uint32_t best = (metric << 3) | st;                     // smallest metric, then smallest state
	best = min(best, (uint32_t)__shfl_xor((int)best, 1));
	best = min(best, (uint32_t)__shfl_xor((int)best, 2));
	best = min(best, (uint32_t)__shfl_xor((int)best, 4));
	uint32_t lag_header = 0, L = 0;
	if (st == 0) {
		trace(best & 7u, 16 + BTBBX_LE_CODED_LAG, 16);
		lag_header = path[g][0] & 0xffffu;
		const uint32_t wt = wh_tab[ws0];
		L = ((lag_header >> 8) ^ wh_tab[wt >> 8]) & 0xffu;
	}
	L = (uint32_t)__shfl((int)L, (int)first_lane);
	const uint32_t N = 8u * (L + 5u) + 3u;
	// rule 6: the rest of the forward pass, the path from state 0
	forward(base2, S, 16 + BTBBX_LE_CODED_LAG, N);
	const uint32_t metric2 = (uint32_t)__shfl((int)metric, (int)first_lane);
	if (st != 0)
		return;
	trace(0, N, N - 3);
	const uint32_t moved = (path[g][0] & 0xffffu) != lag_header ? 1u : 0u;
	const uint32_t symbols = 376u + S * N;
	const bool truncated = h.offset + symbols > n_words * 64;
	const uint32_t *bits = path[g];
	// rule 7
	le_record([&](uint32_t k) { return (bits[k >> 2] >> (8u * (k & 3u))) & 0xffu; }, [&](uint32_t) { return truncated; }, (int)(2u + L),
		  crc_tab, wh_tab, phys[h.stream], crc_init_reflected, aa, h, out[i]);
	io[0] = symbols;
	io[1] = metric2;
	io[2] = metric1 | (ci << 16) | (S << 24);
	io[3] = moved;
}

// ---- host side ----------------------------------------------------------------------------------------------------

static_assert(sizeof(btbbx_le_coded_info) == 16 && offsetof(btbbx_le_coded_info, metric2) == 4 && offsetof(btbbx_le_coded_info, metric1) == 8 &&
	      offsetof(btbbx_le_coded_info, ci) == 10 && offsetof(btbbx_le_coded_info, s) == 11 && offsetof(btbbx_le_coded_info, header_moved) == 12,
	      "btbbx_le_coded_info: 16 bytes (libbtbb_amd LE_CODED_INFO_DTYPE)");

static int le_coded_check_args(const char *who, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, uint64_t search_bits, int max_errors)
{
	if (max_errors < 0 || max_errors > BTBBX_LE_CODED_MAX_ERRORS) {
		set_error("%s: max_errors must be 0..%d", who, BTBBX_LE_CODED_MAX_ERRORS);
		return BTBBX_E_ARG;
	}
	return check_scan_args(who, BTBBX_LE_CODED_PATTERN, n_words, pitch_words, n_streams, search_bits);
}

static int le_coded_launch_scan(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, uint64_t search_bits,
				uint32_t aa, int max_errors, btbbx_hit *d_hits, uint32_t hit_cap, uint32_t *d_hit_count, hipStream_t q)
{
	if (search_bits == 0)
		return BTBBX_OK;
	LeCodedScanArgs a;
	a.words = d_words;
	a.n_words = n_words;
	a.pitch_words = n_streams > 1 ? pitch_words : n_words;
	a.search_bits = search_bits;
	a.n_streams = n_streams;
	le_coded_pattern(aa, a.pat);
	a.max_err = (uint32_t)max_errors;
	a.aa = aa;
	a.hits = d_hits;
	a.hit_cap = hit_cap;
	a.hit_count = d_hit_count;
	TileGrid g;
	const int rc = tile_grid("btbbx_le_coded_scan_device", search_bits, n_words, n_streams, LEC_TILE_WORDS, ctx().num_cus, &g);
	if (rc)
		return rc;
	a.tiles_per_stream = (uint32_t)g.tiles_per_stream;
	hipLaunchKernelGGL(le_coded_scan_kernel, dim3(g.grid), dim3(LEC_THREADS), 0, q, a);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

extern "C" int btbbx_le_coded_scan_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
					  uint64_t search_bits, uint32_t aa, int max_errors,
					  btbbx_hit *d_hits, uint32_t hit_cap, uint32_t *d_hit_count, void *hip_stream)
{
	int rc = le_coded_check_args("btbbx_le_coded_scan_device", n_words, pitch_words, n_streams, search_bits, max_errors);
	if (rc)
		return rc;
	if (!d_words || !d_hit_count || (!d_hits && hit_cap)) {
		set_error("btbbx_le_coded_scan_device: null pointer");
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_words & 7) || ((uintptr_t)d_hits & 15) || ((uintptr_t)d_hit_count & 3)) {
		set_error("btbbx_le_coded_scan_device: misaligned pointer (words 8, hits 16, count 4 bytes)");
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	return le_coded_launch_scan(d_words, n_words, pitch_words, n_streams, search_bits, aa, max_errors, d_hits, hit_cap, d_hit_count,
				    (hipStream_t)hip_stream);
}

// the decisions live in LDS (2112 bytes per hit): no caller scratch
extern "C" size_t btbbx_le_coded_scratch_bytes(uint32_t) { return 0; }

static int le_coded_launch_decode(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, const btbbx_hit *d_hits,
				  const uint32_t *d_count, uint32_t cap, const uint16_t *d_phys, uint32_t crc_init, btbbx_le_pkt *d_out,
				  btbbx_le_coded_info *d_info, hipStream_t q)
{
	if (cap == 0)
		return BTBBX_OK;
	hipLaunchKernelGGL(le_coded_decode_kernel, dim3((cap + LEC_HITS - 1) / LEC_HITS), dim3(LEC_GROUP * LEC_HITS), 0, q, d_words, n_words,
			   pitch_words, d_hits, d_count, cap, d_phys, le_reverse24(crc_init & 0xffffffu), d_out, d_info);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

extern "C" int btbbx_le_coded_decode_hits_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
						 const btbbx_hit *d_hits, const uint32_t *d_count, uint32_t cap,
						 const uint16_t *d_phys_channel, uint32_t crc_init,
						 btbbx_le_pkt *d_out, btbbx_le_coded_info *d_info,
						 void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
	(void)d_scratch;
	(void)scratch_bytes;
	const char *who = "btbbx_le_coded_decode_hits_device";
	if (cap && (!d_words || !d_hits || !d_count || !d_phys_channel || !d_out || !d_info)) {
		set_error("%s: null pointer", who);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_words & 7) || ((uintptr_t)d_hits & 7) || ((uintptr_t)d_count & 3) || ((uintptr_t)d_phys_channel & 1) ||
	    ((uintptr_t)d_out & 7) || ((uintptr_t)d_info & 3)) {
		set_error("%s: misaligned pointer (words, hits, records 8, count and info 4, channels 2 bytes)", who);
		return BTBBX_E_ARG;
	}
	if (n_words > (1ull << 40)) {
		set_error("%s: n_words exceeds 2^40", who);
		return BTBBX_E_ARG;
	}
	int rc = ctx_require();
	if (rc)
		return rc;
	return le_coded_launch_decode(d_words, n_words, pitch_words, d_hits, d_count, cap, d_phys_channel, crc_init, d_out, d_info,
				      (hipStream_t)hip_stream);
}

// btbbx_le_scan_host's chain with the coded scan and decoder in it
extern "C" int64_t btbbx_le_coded_scan_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
					    uint64_t search_bits, const uint16_t *phys_channel, uint32_t aa, uint32_t crc_init,
					    int max_errors, btbbx_le_pkt *pkts, btbbx_le_coded_info *info, uint64_t cap)
{
	int rc = le_coded_check_args("btbbx_le_coded_scan_host", n_words, pitch_words, n_streams, search_bits, max_errors);
	if (rc)
		return rc;
	if (!words || !phys_channel || ((!pkts || !info) && cap)) {
		set_error("btbbx_le_coded_scan_host: null pointer");
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	if (n_streams == 1)
		pitch_words = n_words;
	CallScope scope;
	hipStream_t q = scope_stream();
	const uint64_t cap_words = (uint64_t)(n_streams - 1) * pitch_words + n_words;
	const size_t words_bytes = ((size_t)(cap_words + 1) * 8 + 255) & ~(size_t)255;
	char *dblock = (char *)scope_device(words_bytes + 2 * (size_t)n_streams);
	if (!dblock)
		return BTBBX_E_NOMEM;
	const uint64_t *d_words = (const uint64_t *)dblock;
	uint16_t *d_phys = (uint16_t *)(dblock + words_bytes);
	HIP_TRY(hipMemcpyAsync(dblock, words, (size_t)cap_words * 8, hipMemcpyHostToDevice, q));
	HIP_TRY(hipMemcpyAsync(d_phys, phys_channel, 2 * (size_t)n_streams, hipMemcpyHostToDevice, q));
	// first guess as btbbx_le_scan_host; repeated with room for every match when more were found
	uint64_t guess = search_bits / 1024 * n_streams + 4096;
	if (guess > cap)
		guess = cap;
	uint32_t dev_cap = guess > 0xfffffff0ull ? 0xfffffff0u : (uint32_t)guess;
	uint32_t count = 0;
	char *block = nullptr;
	size_t rec_bytes = 0, order_bytes = 0, pkt_bytes = 0;
	for (int pass = 0; pass < 2; pass++) {
		rec_bytes = ((size_t)dev_cap * sizeof(btbbx_hit) + 255) & ~(size_t)255;
		order_bytes = dev_cap >= 2 ? (btbbx_order_hits_scratch_bytes(dev_cap) + 255) & ~(size_t)255 : 0;
		pkt_bytes = ((size_t)dev_cap * sizeof(btbbx_le_pkt) + 255) & ~(size_t)255;
		block = (char *)scope_hits(256 + rec_bytes + order_bytes + pkt_bytes + (size_t)dev_cap * sizeof(btbbx_le_coded_info));
		if (!block)
			return BTBBX_E_NOMEM;
		uint32_t *d_count = (uint32_t *)block;
		HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(uint32_t), q));
		rc = le_coded_launch_scan(d_words, n_words, pitch_words, n_streams, search_bits, aa, max_errors, (btbbx_hit *)(block + 256), dev_cap,
					  d_count, q);
		if (rc)
			return rc;
		HIP_TRY(hipMemcpyAsync(&count, d_count, sizeof(count), hipMemcpyDeviceToHost, q));
		HIP_TRY(hipStreamSynchronize(q));
		if (count <= dev_cap || cap == 0)
			break;
		dev_cap = count;
	}
	const uint32_t have = std::min(count, dev_cap);
	if (have) {
		uint32_t *d_count = (uint32_t *)block;
		btbbx_hit *d_hits = (btbbx_hit *)(block + 256);
		btbbx_le_pkt *d_pkts = (btbbx_le_pkt *)(block + 256 + rec_bytes + order_bytes);
		btbbx_le_coded_info *d_info = (btbbx_le_coded_info *)(block + 256 + rec_bytes + order_bytes + pkt_bytes);
		if (have >= 2) {
			rc = btbbx_order_hits_device(d_hits, d_count, dev_cap, block + 256 + rec_bytes, order_bytes, q);
			if (rc)
				return rc;
		}
		const uint32_t n = (uint32_t)std::min<uint64_t>(have, cap);
		rc = le_coded_launch_decode(d_words, n_words, pitch_words, d_hits, d_count, n, d_phys, crc_init, d_pkts, d_info, q);
		if (rc)
			return rc;
		HIP_TRY(hipMemcpyAsync(pkts, d_pkts, (size_t)n * sizeof(btbbx_le_pkt), hipMemcpyDeviceToHost, q));
		HIP_TRY(hipMemcpyAsync(info, d_info, (size_t)n * sizeof(btbbx_le_coded_info), hipMemcpyDeviceToHost, q));
		HIP_TRY(hipStreamSynchronize(q));
	}
	return (int64_t)count;
}
