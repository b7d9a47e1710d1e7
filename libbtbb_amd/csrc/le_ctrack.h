// le_ctrack.h -- tracking of LE Coded PHY connections: the duration of every coded candidate, the tracking's rule 3 taking that
// duration, and the chain around both.  The contract is include/btbbx.h ("LE Coded connection tracking", rules 1..4 and the
// changed rule 3); tests/_le_ctrack.py states it in Python.  The promiscuous coded discovery (le_cfind.h) leaves candidates that
// the 1M grouping sorts in place; the tracking (le_track.h) closes an event by the 1M duration 80 + 8 * length, which a coded
// packet exceeds 8 to 70 times, so every reply opens an event of its own.  Only rule 3 reads the duration:
//
//   1. le_ctrack_symbols_kernel   one lane per candidate of the list AS IT STANDS (sorted or not): block 1 of the coded decoder
//      (37 steps, 8 states) with the eight path metrics in registers, for the two CI bits alone -> 376 + S * N
//   2. le_ctrack_flag_kernel      le_track_flag_kernel with end = offset + symbols[vals[j - 1]]; le_track_launch enqueues it in
//      place of its own flag pass, its other thirteen kernels run unchanged
//
// This header is a translation unit's worth (le_ctrack.hip includes it and nothing else of the LE family): no kernel of le.hip,
// le_coded.hip or le_cfind.hip shares a compilation with it.  What it needs of the tracking is le_slots.h (no kernel in it) and
// le_track_run, a host function of le.hip.
#pragma once
#include "le_slots.h"
#include <algorithm>
#include <string.h>

#define LCT_THREADS 256
#define LCT_INF (1u << 24)                       // an unreachable state's metric
#define LCT_FIRST_KEPT 34                        // the first step whose decisions the trace-back to the CI reads

// ---- 1. the duration ----------------------------------------------------------------------------------------------------

struct LeCtrackSymbolsArgs {
	const uint64_t *words;
	uint64_t n_words;
	uint64_t pitch_words;
	uint32_t n_streams;
	const btbbx_le_cand *cands;
	const uint32_t *count;
	uint32_t cap;
	uint32_t *symbols;
};

// One lane per candidate.  Block 1 is the 296 symbols from o + 80: six stream words from word (o + 80) >> 6 on (a word at or
// past n_words reads as 0, so does every word of a candidate whose stream is out of range), funnel-shifted by (o + 80) & 63 into
// five words whose byte t & 7 of word t >> 3 is step t's eight symbols.  The two transitions into a state send complementary
// symbols (le_cfind_decode_kernel says why), so a step forms the distances of its two half-bytes to 0 0 1 1 once and every branch
// metric is a sum of two of {d, 4 - d}.  All loops are unrolled: metrics and words are named registers, nothing is indexed.
// The CI is bits 32 and 33 of the path that ends in state 0 after step 36.  The state after step 33 is b33 | b32 << 1 | b31 << 2,
// and it is reached from state 0 by the decisions of steps 36, 35 and 34 alone: those 24 bits are all that is kept of the 296
// decisions (a lane per candidate needs no LDS for them, and no second pass).  Every lane of a wave runs the same 37 steps.
__global__ __launch_bounds__(LCT_THREADS) void le_ctrack_symbols_kernel(LeCtrackSymbolsArgs a)
{
	const uint32_t have = *a.count, n = have < a.cap ? have : a.cap;
	const uint64_t i = (uint64_t)blockIdx.x * LCT_THREADS + threadIdx.x;
	if (i >= n)
		return;
	const uint2 *rec = reinterpret_cast<const uint2 *>(a.cands + i);
	const uint2 ra = rec[0], rc = rec[2];
	const uint64_t offset = ((uint64_t)ra.y << 32) | ra.x;
	const uint32_t stream = rc.x & 0xffffu, length = rc.x >> 24;
	const bool in_range = stream < a.n_streams;                 // rule 1
	const uint64_t first = offset + 80, wi = first >> 6;
	const uint32_t sh = (uint32_t)(first & 63);
	const uint64_t *w = a.words + (in_range ? (uint64_t)stream * a.pitch_words : 0);
	uint64_t raw[6], blk[5];
#pragma unroll
	for (int k = 0; k < 6; k++)
		raw[k] = in_range && wi + k < a.n_words ? w[wi + k] : 0;
#pragma unroll
	for (int k = 0; k < 5; k++)
		blk[k] = (raw[k] >> sh) | (sh ? raw[k + 1] << (64 - sh) : 0);
	uint32_t m[8], kept = 0;
#pragma unroll
	for (int s = 0; s < 8; s++)
		m[s] = s ? LCT_INF : 0u;
#pragma unroll
	for (int t = 0; t < 37; t++) {
		const uint32_t r = (uint32_t)(blk[t >> 3] >> (8 * (t & 7))) & 0xffu;
		// distance of the first and the second four symbols to a coded 0 (0 0 1 1, first symbol in bit 0); to a coded 1: 4 less it
		const uint32_t d0 = (uint32_t)__popc((r & 0xfu) ^ 0xcu), d1 = (uint32_t)__popc((r >> 4) ^ 0xcu);
		uint32_t nm[8];
#pragma unroll
		for (int s = 0; s < 8; s++) {
			// into state s (after the step) from (s >> 1) with b3 = 0: a0 = b ^ b1 ^ b2, a1 = b ^ b2; from (s >> 1) | 4 both flip
			const int b = s & 1, b1 = (s >> 1) & 1, b2 = (s >> 2) & 1;
			const int a0 = b ^ b1 ^ b2, a1 = b ^ b2;
			const uint32_t bm0 = (a0 ? 4u - d0 : d0) + (a1 ? 4u - d1 : d1);
			const uint32_t c0 = m[s >> 1] + bm0, c1 = m[(s >> 1) | 4] + (8u - bm0);
			const bool x = c1 < c0;                             // x = 0 survives on equal sums
			nm[s] = x ? c1 : c0;
			if (t >= LCT_FIRST_KEPT)
				kept |= (x ? 1u : 0u) << (8 * (t - LCT_FIRST_KEPT) + s);
		}
#pragma unroll
		for (int s = 0; s < 8; s++)
			m[s] = nm[s];
	}
	uint32_t s = 0;
#pragma unroll
	for (int t = 36; t >= LCT_FIRST_KEPT; t--)
		s = (s >> 1) | (((kept >> (8 * (t - LCT_FIRST_KEPT) + s)) & 1u) << 2);
	const uint32_t ci = ((s >> 1) & 1u) | ((s & 1u) << 1);         // rule 2: bit 32, bit 33
	const uint32_t steps = 8u * (length + 5u) + 3u;                 // rule 3
	const uint32_t S = ci == 0 ? 8u : ci == 1 ? 2u : 0u;
	a.symbols[i] = in_range ? 376u + S * steps : 0u;
}

// ---- 2. the flag pass with durations --------------------------------------------------------------------------------------

// le_track_flag_kernel (le_track.h), rule 3 for every slot against the slot in front of it, with the predecessor's duration read
// from symbols[] at the predecessor's list index: one more dword per slot that does not open its connection, nothing else differs
__global__ __launch_bounds__(LCT_THREADS) void le_ctrack_flag_kernel(const btbbx_le_cand *cands, const uint64_t *keys, const uint32_t *vals,
								     const uint32_t *params, const uint16_t *phys, uint32_t n_streams, uint32_t ifs_bits,
								     const uint32_t *symbols, uint32_t tile_slots, uint32_t *info, uint32_t *tiles)
{
	__shared__ uint32_t count;
	const uint32_t tid = threadIdx.x, n = params[0], k = params[1];
	if (tid == 0)
		count = 0;
	__syncthreads();
	uint32_t mine = 0;
	for (uint32_t r = 0; r < tile_slots / LCT_THREADS; r++) {
		const uint32_t j = blockIdx.x * tile_slots + r * LCT_THREADS + tid;
		if (j >= n)
			break;
		const uint32_t c = (uint32_t)keys[j];
		uint32_t v = 0xff;
		if (c < k) {
			const LdCand me = ld_load(cands, vals[j]);
			uint32_t ch, chp;
			lt_member_of(me.c, phys, n_streams, k, ch);
			bool open = j == 0 || (uint32_t)keys[j - 1] != c;
			if (!open) {
				const uint32_t pi = vals[j - 1];
				const LdCand p = ld_load(cands, pi);
				lt_member_of(p.c, phys, n_streams, k, chp);
				const uint64_t off = ((uint64_t)me.a.y << 32) | me.a.x, end = (((uint64_t)p.a.y << 32) | p.a.x) + symbols[pi];
				open = ch != chp || off > end + ifs_bits;
			}
			v = ch | (open ? LT_INFO_EVENT : 0u);
			mine += open ? 1u : 0u;
		}
		info[j] = v;
	}
	if (mine)
		atomicAdd(&count, mine);
	__syncthreads();
	if (tid == 0)
		tiles[blockIdx.x] = count;
}

// ---- host side ------------------------------------------------------------------------------------------------------------

static_assert(LCT_THREADS == LT_THREADS, "the stand-in runs on the flag pass's grid");
static_assert(sizeof(btbbx_le_cand) == 24 && offsetof(btbbx_le_cand, stream) == 16 && offsetof(btbbx_le_cand, length) == 19 &&
	      offsetof(btbbx_le_cand, conn) == 20, "btbbx_le_cand layout");

// le.hip (le_track.h): btbbx_le_track_device's checks and launches, with a stand-in for the flag pass
int le_track_run(const char *who, const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
		 const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
		 const uint16_t *d_phys_channel, uint32_t n_streams,
		 uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
		 btbbx_le_track *d_tracks, btbbx_le_track_pkt *d_pkts,
		 void *d_scratch, size_t scratch_bytes, void *hip_stream, const LtFlagStandIn *stand_in);

extern "C" int btbbx_le_ctrack_symbols_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
					      const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
					      uint32_t *d_symbols, void *hip_stream)
{
	const char *who = "btbbx_le_ctrack_symbols_device";
	if (n_streams == 0 || n_streams > 65535 || pitch_words < n_words || n_words > (1ull << 40)) {
		set_error("%s: n_streams must be 1..65535, pitch_words >= n_words and n_words <= 2^40", who);
		return BTBBX_E_ARG;
	}
	if (cand_cap && (!d_words || !d_cands || !d_cand_count || !d_symbols)) {
		set_error("%s: null pointer", who);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_words & 7) || ((uintptr_t)d_cands & 7) || ((uintptr_t)d_symbols & 3) || ((uintptr_t)d_cand_count & 3)) {
		set_error("%s: misaligned pointer (words and candidates 8 bytes, symbols and the counter 4)", who);
		return BTBBX_E_ARG;
	}
	const int rc = ctx_require();
	if (rc)
		return rc;
	if (cand_cap == 0)
		return BTBBX_OK;
	LeCtrackSymbolsArgs a;
	a.words = d_words;
	a.n_words = n_words;
	a.pitch_words = n_streams > 1 ? pitch_words : n_words;
	a.n_streams = n_streams;
	a.cands = d_cands;
	a.count = d_cand_count;
	a.cap = cand_cap;
	a.symbols = d_symbols;
	const uint32_t grid = (uint32_t)(((uint64_t)cand_cap + LCT_THREADS - 1) / LCT_THREADS);
	hipLaunchKernelGGL(le_ctrack_symbols_kernel, dim3(grid), dim3(LCT_THREADS), 0, (hipStream_t)hip_stream, a);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

static void le_ctrack_enqueue_flag(const LtFlagPass &p, const void *user)
{
	hipLaunchKernelGGL(le_ctrack_flag_kernel, dim3(p.n_tiles), dim3(LCT_THREADS), 0, p.q, p.cands, p.keys, p.vals, p.params, p.phys, p.n_streams,
			   p.ifs_bits, (const uint32_t *)user, p.tile_slots, p.info, p.tiles);
}

extern "C" int btbbx_le_ctrack_device(const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
				      const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
				      const uint16_t *d_phys_channel, uint32_t n_streams, const uint32_t *d_symbols,
				      uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
				      btbbx_le_track *d_tracks, btbbx_le_track_pkt *d_pkts,
				      void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
	const char *who = "btbbx_le_ctrack_device";
	if (!d_symbols || ((uintptr_t)d_symbols & 3)) {
		set_error("%s: d_symbols is null or not 4-byte aligned", who);
		return BTBBX_E_ARG;
	}
	const LtFlagStandIn stand_in = {le_ctrack_enqueue_flag, d_symbols};
	return le_track_run(who, d_cands, d_cand_count, cand_cap, d_conns, d_conn_count, conn_cap, d_phys_channel, n_streams, unit_bits, ifs_bits,
			    jitter_bits, flags, d_tracks, d_pkts, d_scratch, scratch_bytes, hip_stream, &stand_in);
}

static size_t lct_up(size_t x) { return (x + 255) & ~(size_t)255; }

// what the chain keeps on the device behind the counters, as offsets into its block
struct LctHostLayout {
	size_t pre, cands, group, conns, symbols, track, tracks, pkts, csa2, sel, sel_pkts, total;
};

static LctHostLayout le_ctrack_host_layout(uint32_t pre_cap, uint32_t dev_cap, uint32_t dev_conns, bool with_sel)
{
	LctHostLayout L;
	size_t at = 256;
	auto take = [&](size_t bytes) { const size_t here = at; at += lct_up(bytes); return here; };
	L.pre = take(btbbx_le_cfind_scratch_bytes(pre_cap));
	L.cands = take((size_t)dev_cap * sizeof(btbbx_le_cand));
	L.group = take(btbbx_le_discover_scratch_bytes(dev_cap));
	L.conns = take((size_t)dev_conns * sizeof(btbbx_le_conn));
	L.symbols = take((size_t)dev_cap * sizeof(uint32_t));
	L.track = take(btbbx_le_track_scratch_bytes(dev_cap, dev_conns));
	L.tracks = take((size_t)dev_conns * sizeof(btbbx_le_track));
	L.pkts = take((size_t)dev_cap * sizeof(btbbx_le_track_pkt));
	L.csa2 = take(with_sel ? btbbx_le_csa2_scratch_bytes(dev_cap, dev_conns) : 0);
	L.sel = take(with_sel ? (size_t)dev_conns * sizeof(btbbx_le_csa2) : 0);
	L.sel_pkts = take(with_sel ? (size_t)dev_cap * sizeof(btbbx_le_csa2_pkt) : 0);
	L.total = at;
	return L;
}

// btbbx_le_cfind_host's chain over the exported device entries -- copy in, the coded scan repeated with room, the grouping --, then
// the durations of the SORTED list, the tracking that takes them and channel selection #2 on the same stream, and the copy-out of
// btbbx_le_csa2_host
extern "C" int64_t btbbx_le_ctrack_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
					uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, int max_errors,
					uint32_t min_count, btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands,
					uint64_t cand_cap, uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits,
					uint32_t jitter_bits, uint32_t flags, btbbx_le_track *tracks, btbbx_le_track_pkt *pkts,
					btbbx_le_csa2 *sel, btbbx_le_csa2_pkt *sel_pkts, uint32_t *symbols)
{
	const char *who = "btbbx_le_ctrack_host";
	if (max_errors < 0 || max_errors > BTBBX_LE_CODED_MAX_ERRORS || max_len > 255) {
		set_error("%s: max_errors must be 0..%d and max_len 0..255", who, BTBBX_LE_CODED_MAX_ERRORS);
		return BTBBX_E_ARG;
	}
	int rc = check_scan_args(who, BTBBX_LE_CODED_PATTERN, n_words, pitch_words, n_streams, search_bits);
	if (rc)
		return rc;
	if (unit_bits < 2 || jitter_bits >= unit_bits / 2) {
		set_error("%s: unit_bits must be >= 2 and jitter_bits < unit_bits / 2", who);
		return BTBBX_E_ARG;
	}
	if (!words || !phys_channel || ((!conns || !tracks) && conn_cap) || (!cands && cand_cap)) {
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
	const size_t words_bytes = lct_up((size_t)(cap_words + 1) * 8);
	char *dblock = (char *)scope_device(words_bytes + 2 * (size_t)n_streams);
	if (!dblock)
		return BTBBX_E_NOMEM;
	const uint64_t *d_words = (const uint64_t *)dblock;
	uint16_t *d_phys = (uint16_t *)(dblock + words_bytes);
	HIP_TRY(hipMemcpyAsync(dblock, words, (size_t)cap_words * 8, hipMemcpyHostToDevice, q));
	HIP_TRY(hipMemcpyAsync(d_phys, phys_channel, 2 * (size_t)n_streams, hipMemcpyHostToDevice, q));
	// the first guesses of btbbx_le_cfind_host
	const uint64_t guess = search_bits / 4096 * n_streams + 4096;
	uint32_t pre_cap = guess > 0xfffffff0ull ? 0xfffffff0u : (uint32_t)guess, dev_cap = pre_cap, dev_conns = 0;
	uint32_t counts[2] = {0, 0};                            // pre-records, candidates
	char *block = nullptr;
	LctHostLayout L;
	for (int pass = 0; pass < 3; pass++) {
		dev_conns = (uint32_t)std::min<uint64_t>(conn_cap, dev_cap);
		L = le_ctrack_host_layout(pre_cap, dev_cap, dev_conns, sel != nullptr);
		block = (char *)scope_hits(L.total);
		if (!block)
			return BTBBX_E_NOMEM;
		HIP_TRY(hipMemsetAsync(block, 0, 4 * sizeof(uint32_t), q));
		rc = btbbx_le_cfind_scan_device(d_words, n_words, pitch_words, n_streams, search_bits, d_phys, max_len, max_errors,
						(btbbx_le_cand *)(block + L.cands), nullptr, dev_cap, (uint32_t *)block + 1, (uint32_t *)block, block + L.pre,
						btbbx_le_cfind_scratch_bytes(pre_cap), q);
		if (rc)
			return rc;
		HIP_TRY(hipMemcpyAsync(counts, block, sizeof(counts), hipMemcpyDeviceToHost, q));
		HIP_TRY(hipStreamSynchronize(q));
		if (counts[0] <= pre_cap && counts[1] <= dev_cap)
			break;
		pre_cap = std::max(pre_cap, std::min(counts[0], 0xfffffff0u));
		dev_cap = std::max(dev_cap, counts[1]);
	}
	const uint32_t count = counts[1], have = std::min(count, dev_cap);
	if (n_cands_out)
		*n_cands_out = count;
	if (!have)
		return 0;
	uint32_t *d_count = (uint32_t *)block + 1, *d_conn_count = (uint32_t *)block + 2;
	btbbx_le_cand *d_cands = (btbbx_le_cand *)(block + L.cands);
	btbbx_le_conn *d_conns = (btbbx_le_conn *)(block + L.conns);
	uint32_t *d_symbols = (uint32_t *)(block + L.symbols);
	btbbx_le_track *d_tracks = (btbbx_le_track *)(block + L.tracks);
	btbbx_le_track_pkt *d_pkts = (btbbx_le_track_pkt *)(block + L.pkts);
	rc = btbbx_le_discover_group_device(d_cands, d_count, dev_cap, min_count, d_conns, dev_conns, d_conn_count, block + L.group,
					    btbbx_le_discover_scratch_bytes(dev_cap), q);
	if (rc)
		return rc;
	uint32_t n_conns = 0;
	HIP_TRY(hipMemcpyAsync(&n_conns, d_conn_count, sizeof(uint32_t), hipMemcpyDeviceToHost, q));
	rc = btbbx_le_ctrack_symbols_device(d_words, n_words, pitch_words, n_streams, d_cands, d_count, dev_cap, d_symbols, q);
	if (rc)
		return rc;
	HIP_TRY(hipStreamSynchronize(q));
	const uint64_t nc = std::min<uint64_t>(n_conns, dev_conns), nk = std::min<uint64_t>(have, cand_cap);
	if (nc) {
		rc = btbbx_le_ctrack_device(d_cands, d_count, dev_cap, d_conns, d_conn_count, dev_conns, d_phys, n_streams, d_symbols, unit_bits, ifs_bits,
					    jitter_bits, flags, d_tracks, d_pkts, block + L.track, btbbx_le_track_scratch_bytes(dev_cap, dev_conns), q);
		if (!rc && sel)
			rc = btbbx_le_csa2_device(d_cands, d_count, dev_cap, d_conns, d_conn_count, dev_conns, d_tracks, d_pkts, flags,
						  (btbbx_le_csa2 *)(block + L.sel), (btbbx_le_csa2_pkt *)(block + L.sel_pkts), block + L.csa2,
						  btbbx_le_csa2_scratch_bytes(dev_cap, dev_conns), q);
		if (rc) {
			(void)hipStreamSynchronize(q);
			return rc;
		}
		HIP_TRY(hipMemcpyAsync(conns, d_conns, (size_t)nc * sizeof(btbbx_le_conn), hipMemcpyDeviceToHost, q));
		HIP_TRY(hipMemcpyAsync(tracks, d_tracks, (size_t)nc * sizeof(btbbx_le_track), hipMemcpyDeviceToHost, q));
		if (pkts && nk)
			HIP_TRY(hipMemcpyAsync(pkts, d_pkts, (size_t)nk * sizeof(btbbx_le_track_pkt), hipMemcpyDeviceToHost, q));
		if (sel)
			HIP_TRY(hipMemcpyAsync(sel, block + L.sel, (size_t)nc * sizeof(btbbx_le_csa2), hipMemcpyDeviceToHost, q));
		if (sel && sel_pkts && nk)
			HIP_TRY(hipMemcpyAsync(sel_pkts, block + L.sel_pkts, (size_t)nk * sizeof(btbbx_le_csa2_pkt), hipMemcpyDeviceToHost, q));
	} else {
		if (pkts)
			memset(pkts, 0xff, (size_t)nk * sizeof(btbbx_le_track_pkt));
		if (sel && sel_pkts)
			memset(sel_pkts, 0xff, (size_t)nk * sizeof(btbbx_le_csa2_pkt));
	}
	if (nk) {
		HIP_TRY(hipMemcpyAsync(cands, d_cands, (size_t)nk * sizeof(btbbx_le_cand), hipMemcpyDeviceToHost, q));
		if (symbols)
			HIP_TRY(hipMemcpyAsync(symbols, d_symbols, (size_t)nk * sizeof(uint32_t), hipMemcpyDeviceToHost, q));
	}
	HIP_TRY(hipStreamSynchronize(q));
	return (int64_t)n_conns;
}
