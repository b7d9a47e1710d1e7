// scan_known.h -- scan_known_lap_kernel: the scan for one known LAP.  A piece of scan.hip.
#pragma once
#include "scan_core.h"

// ---- known LAP --------------------------------------------------------------------------

// Known-LAP hits are staged in a per-wave LDS ring and flushed 64 at a time: one global
// counter atomic per 64 hits (a single counter word saturates near 88 M atomics/s on this
// chip, which a dense hit stream would otherwise run into).
#define KRING 128
#ifndef KL_WORDS
#define KL_WORDS 2                             // consecutive stream words per lane and tile (tile = KL_WORDS x 256 words; a power of two); the
#endif                                         // next tile's words are loaded while this one is worked on (0.466 against 0.4865 ms, round 3)
#define KL_SELECT_LIMIT 1                      // limits up to here: one survivor per lane and pass (scan_known_lap_kernel)
struct KnownHit { uint32_t off_lo, off_hi, stream_err; };      // 12 bytes per staged hit

// LIMIT = max_ac_errors when it is 0 .. 4 (the count <= limit compare of the filters then folds into a few
// and / andn of the count planes; with the limit in a register it is sixteen instructions with SGPR masks), -1 = any
// CLS = bit 23 of the LAP (the barker class of its sync word), -1 = not specialised
// ORD: the ordered scan's form -- hits leave through the segment slots (a template flag: the code that fills them costs the plain form
// eight registers, one wave per SIMD, if it is only branched around)
template <int LIMIT, int CLS, bool MSB, bool ORD = false>
// (round 6: the ORD form at 65 VGPRs = seven waves per SIMD; forced to 64 / eight by amdgpu_waves_per_eu: no difference, 0.540-0.542 against 0.538-0.544 ms per chain step)
__global__ __launch_bounds__(256) void scan_known_lap_kernel(ScanArgs a)
{
	__shared__ KnownHit ring_mem[4][KRING];
	__shared__ uint32_t slot_cnt[4][64];                   // (ordered scan, segment slots: hits per tile tag of a batch ...
	__shared__ uint16_t slot_code[4][64][4];               //  ... and up to four of their 12-bit offsets inside the segment)
	if (a.gate && *a.gate == 0)
		return;
	const uint32_t tid = threadIdx.x;
	const uint32_t lane = tid & 63;
	KnownHit *ring = ring_mem[tid >> 6];
	constexpr bool ord = ORD;
	uint32_t ac_lo = (uint32_t)a.syncword, ac_hi = (uint32_t)(a.syncword >> 32);
	asm volatile("" : "+v"(ac_lo), "+v"(ac_hi));          // (an SGPR operand halves the issue rate of the XORs in the survivor pass)
	// the planes of the filter are XORed with all-ones where the sync word has a 1: sixteen masks, kept in
	// VGPRs on purpose -- they are wave-uniform, and a VALU instruction with an SGPR source issues at half rate
	// (tools/valu_rate.hip: 4.2 against 2.5 cycles)
	uint32_t flip[16];
#pragma unroll
	for (int k = 0; k < 16; k++) {
		flip[k] = (((k < 8 ? ac_lo : ac_hi) >> (24 + (k & 7))) & 1) ? 0xffffffffu : 0u;   // plane k = sync-word bit 24 + k (k < 8), 48 + k (k >= 8)
		asm volatile("" : "+v"(flip[k]));
	}
	const int limit = LIMIT >= 0 ? LIMIT : (a.max_err < 0 ? -1 : a.max_err);
	if (limit < 0)
		return;
	const bool wide = limit >= 2;               // launch-uniform choice of the pre-filter
#ifdef SCAN_PROFILE
	// phases: 0 = wait for the tile's words, 1 = bit-sliced filter, 2 = survivor passes + hit staging, 3 = ring flush + tile cursor,
	// 4 = issuing the next tile's loads
	__shared__ uint32_t kl_prof[4][32];
	const uint32_t prof_off = (uint32_t)(uintptr_t)(lds_u32_t *)&kl_prof[tid >> 6][0];
	if (lane < 32)
		kl_prof[tid >> 6][lane] = 0;
	uint64_t prof_t;
	asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(prof_t) : : "memory");
#endif
	uint32_t q_head = 0, q_tail = 0;                // wave-uniform, free running

	auto flush = [&](uint32_t n) {                  // n <= 64 oldest entries -> global hit list
		uint32_t base = 0;
		if (lane == 0)
			base = atomicAdd(a.hit_count, n);
		base = __builtin_amdgcn_readfirstlane(base);
		if (lane < n) {
			const KnownHit k = ring[(q_head + lane) & (KRING - 1)];
			const uint32_t idx = base + lane;
			if (idx < a.hit_cap) {
				btbbx_hit h;
				h.offset = ((uint64_t)k.off_hi << 32) | k.off_lo;
				h.lap = a.lap;
				h.ac_errors = (uint8_t)(k.stream_err & 0xff);
				h.reserved = 0;
				h.stream = (uint16_t)(k.stream_err >> 8);
				a.hits[idx] = h;
				count_bucket(a, h.stream, h.offset);
			}
		}
		q_head += n;
	};
	// Ordered scan (round 6, as in scan_slide_kernel<..., ORD>): a SEGMENT = 4096 offsets = the 64 words of a tile one wave owns
	// (a tile is 2 x 256 words: two segments per wave).  Hits wait in the ring as before, but leave it at a tile end only -- every
	// hit of a segment is then in the batch --, ranked by offset inside their segment, into the segment's own slots.
	uint32_t iter = 0, ring_first_iter = 0;         // wave-uniform: tiles this wave has worked on; the tile of the oldest ring entry
	auto stage = [&](bool hit, uint32_t stream, uint64_t offset, uint32_t nerr) {
		const uint64_t mask = __ballot(hit);
		if (!mask)
			return;
		if (a.first) {                              // first-match mode: atomicMin, hits are sparse
			if (hit)
				emit_hit(a, stream, offset, a.lap, nerr);
			return;
		}
		if (q_tail - q_head + 64 > KRING) {
			if (ord) {                              // more than 64 hits in a wave's tile(s): a stream of sync words -- the general ordering redoes the call
				*a.irregular = 1u;
				return;
			}
			flush(64);
		}
		if (q_tail == q_head)
			ring_first_iter = iter;
		if (hit) {
			const uint32_t slot = q_tail + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
					__builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
			// (ordered scan: bits 24 .. 31 = the segment's tag inside the batch, KL_WORDS per tile: a wave's run of a tile starts at a
			// multiple of 64 KL_WORDS words, so the segment number's low bits tell which)
			const uint32_t tag = ((iter * KL_WORDS) | ((uint32_t)(offset >> 12) & (KL_WORDS - 1u))) & 0xffu;
			KnownHit k = { (uint32_t)offset, (uint32_t)(offset >> 32), (stream << 8) | nerr | (ord ? tag << 24 : 0u) };
			ring[slot & (KRING - 1)] = k;
		}
		q_tail += (uint32_t)__popcll(mask);
	};
	auto to_slots = [&](bool final) {               // at a tile end: the whole ring (<= 128 entries) into the segment slots
		const uint32_t n = q_tail - q_head;
		if (n == 0 || (n < 48 && !final))
			return;
		uint32_t *cnt = slot_cnt[tid >> 6];
		uint16_t (*codes)[4] = slot_code[tid >> 6];
		const bool tags_ok = iter - ring_first_iter < 64 / KL_WORDS;      // KL_WORDS tags per tile, 64 counters: no two segments of the batch share one
		// (one round of 64 entries at a time and nothing kept between the rounds: the kernel's 64 registers are its eight waves per SIMD)
		bool fast = tags_ok;
		if (tags_ok) {
			cnt[lane] = 0;
#pragma unroll 1
			for (uint32_t r = 0; r < n; r += 64)
				if (r + lane < n) {
					const KnownHit e = ring[(q_head + r + lane) & (KRING - 1)];
					const uint32_t key = (e.stream_err >> 24) & 63u;
					const uint32_t idx = atomicAdd(&cnt[key], 1u);
					if (idx < 4)
						codes[key][idx] = (uint16_t)(e.off_lo & 0xfffu);
				}
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
			if (__ballot(*(volatile __attribute__((address_space(3))) const uint32_t *)&cnt[lane] > 4u))
				fast = false;
		}
#pragma unroll 1
		for (uint32_t r = 0; r < n; r += 64) {
			const bool have = r + lane < n;
			const KnownHit e = ring[(q_head + r + lane) & (KRING - 1)];
			uint32_t count = 0, rank = 0;
			if (fast) {
				if (have) {
					const uint32_t key = (e.stream_err >> 24) & 63u, mine = e.off_lo & 0xfffu;
					count = *(volatile __attribute__((address_space(3))) const uint32_t *)&cnt[key];
					for (uint32_t j = 0; j < count; j++)
						rank += codes[key][j] < mine ? 1u : 0u;
				}
			} else {                                // a sparse stream (a batch over 32 tiles or more) or a crowded segment: every entry against every other
#pragma unroll 1
				for (uint32_t j = 0; j < n; j++) {
					const KnownHit o = ring[(q_head + j) & (KRING - 1)];          // (wave-uniform address: a broadcast)
					const bool same = ((o.stream_err ^ e.stream_err) & 0xffff00u) == 0 && o.off_hi == e.off_hi && (o.off_lo >> 12) == (e.off_lo >> 12);
					count += same ? 1u : 0u;
					rank += same && o.off_lo < e.off_lo ? 1u : 0u;
				}
			}
			const uint32_t stream = (e.stream_err >> 8) & 0xffffu;
			const uint32_t seg = stream * a.segs_per_stream + (uint32_t)((((uint64_t)e.off_hi << 32) | e.off_lo) >> 12);
			uint4 out;
			out.x = e.off_lo;
			out.y = e.off_hi;
			out.z = a.lap;
			out.w = (e.stream_err & 0xffu) | (stream << 16);
			const bool spill = have && rank >= a.seg_slot_n;
			if (have && !spill)
				a.seg_slots[(uint64_t)seg * a.seg_slot_n + rank] = (uint64_t)(e.off_lo & 0xfffu) | ((uint64_t)(a.lap & 0xffffffu) << 12) | ((uint64_t)(e.stream_err & 0xffu) << 36);
			if (have && rank + 1 == count)
				a.seg_cnt[seg] = (uint16_t)count;
			const uint64_t om = __ballot(spill);
			if (om) {
				uint32_t base = 0;
				if (lane == 0)
					base = atomicAdd(a.ovf_count, (uint32_t)__popcll(om));
				base = __builtin_amdgcn_readfirstlane(base);
				const uint32_t at = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(om >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)om, 0));
				if (spill) {
					if (at < a.ovf_cap) {
						reinterpret_cast<uint4 *>(a.ovf_recs)[at] = out;
						a.ovf_meta[at] = make_uint2(seg, rank);
					} else {
						*a.irregular = 1u;
					}
				}
			}
		}
		q_head += n;
	};

	// division-free (stream, tile) cursor, as in the LAP_ANY kernel
	// (32-bit tile numbers: the launcher refuses more; 64-bit compares of wave-uniform values would run on the VALU)
	const uint32_t tiles_per_stream = (uint32_t)a.tiles_per_stream;
	uint32_t stream = 0;
	uint32_t t = blockIdx.x;
	while (t >= tiles_per_stream && stream < a.n_streams) {
		t -= tiles_per_stream;
		stream++;
	}
	// A tile is KL_WORDS x 256 words and a lane owns KL_WORDS CONSECUTIVE words of it (round 6, late; rounds 1-5: words 256 apart),
	// so the filter's planes are shared all along the lane's run of 2 * KL_WORDS halves: 8 x (2 * KL_WORDS + 1) funnel shifts per
	// tile instead of 8 x 3 x KL_WORDS, and one halo word per lane instead of one per word.  The next tile's words are loaded while
	// this one is worked on: the counters had 43 % of the wave-cycles in s_waitcnt with eight waves per SIMD taking turns at their
	// loads (profiles/r03_chain/pmc_known_before.json).
	constexpr int NCH = 2 * KL_WORDS;                   // chains (32-offset halves) per lane and tile
	const uint32_t lw = tid * KL_WORDS;                 // the lane's first word in a tile
	uint64_t nw[KL_WORDS + 1];                          // the lane's words of the next tile and the word behind them
	static_assert(KL_WORDS == 2, "fetch_run: one 16-byte and one 8-byte buffer load per lane");
	const uint32_t lw_bytes = lw * 8u;
	auto fetch = [&](uint32_t ft, uint32_t fstream) { fetch_run<KL_WORDS * 256>(a, ft, fstream, lw_bytes, nw); };
	fetch(t, stream);
	// The first tile's words are waited for HERE: with these loads still counted as pending at the loop head the compiler waits for
	// "everything in flight" (s_waitcnt vmcnt(0)) in front of the filter of EVERY tile -- right behind the next tile's loads, which
	// undid the prefetch (rounds 3-6: 15-25 % of a wave's time in that wait, profiles/r06_known).
#pragma unroll
	for (int u = 0; u <= KL_WORDS; u++)
		asm volatile("" : "+v"(nw[u]));
	while (stream < a.n_streams) {
		// word index and validity of this tile's offsets from the (wave-uniform) tile number: nothing per lane is carried
		// from the fetch but the words themselves.  Chain c = offsets 32 c .. 32 c + 31 of the lane's run; its windows lie in D[c .. c + 2].
		const uint64_t word0 = (uint64_t)t * (KL_WORDS * 256) + lw;
		uint32_t D[NCH + 2], m[NCH];
#pragma unroll
		for (int u = 0; u <= KL_WORDS; u++) {
			D[2 * u] = (uint32_t)nw[u];
			D[2 * u + 1] = (uint32_t)(nw[u] >> 32);
		}
		const bool ragged = t >= a.full_tiles;          // wave-uniform: offsets beyond the search length are cut out BEHIND the filter
		const uint32_t this_stream = stream;
		t += gridDim.x;
		while (t >= tiles_per_stream && stream < a.n_streams) {
			t -= tiles_per_stream;
			stream++;
		}
		fetch(t, stream);
		PROF_MARK(4);
#ifdef SCAN_PROFILE
#pragma unroll
		for (int k = 0; k < NCH + 2; k++)
			asm volatile("" : "+v"(D[k]));                  // this tile's words have arrived
		PROF_MARK(0);
#endif
		__builtin_amdgcn_s_setprio(0);                  // bit-sliced filter: lowest (see PRIO_FILTER above)
		if constexpr (MSB) {
#pragma unroll
			for (int k = 0; k < NCH + 2; k++)
				D[k] = msb_dword(D[k]);
		}
		{	// (pair_planes above: the planes of D[c + 1] : D[c + 2] are the upper planes of chain c and the lower ones of chain c + 1)
			uint32_t P[2][8];
			if (wide)
				pair_planes<0>(D[0], D[1], P[0]);
			else
				pair_planes<4>(D[0], D[1], P[0]);
#pragma unroll
			for (int c = 0; c < NCH; c++) {
				pair_planes<0>(D[c + 1], D[c + 2], P[(c + 1) & 1]);
				m[c] = (wide ? top16_filter<CLS>(P[c & 1], P[(c + 1) & 1], flip, limit)
					     : top12_filter<CLS>(P[c & 1], P[(c + 1) & 1], flip, limit));
			}
		}
		if (ragged) {                                   // (as four validity masks in front of the filter: a register copy and an AND per chain of every tile)
			asm volatile("" ::: "memory");              // (keeps the compiler from flattening the branch into selects)
#pragma unroll
			for (int c = 0; c < NCH; c++) {
				const uint64_t first_off = word0 * 64 + 32u * c;
				m[c] &= first_off >= a.search_bits ? 0u
					: (a.search_bits - first_off >= 32 ? 0xffffffffu : ((1u << (uint32_t)(a.search_bits - first_off)) - 1u));
			}
		}
#ifdef SCAN_PROFILE
#pragma unroll
		for (int c = 0; c < NCH; c++)
			PROF_PIN(m[c]);
		PROF_MARK(1);
#endif
		__builtin_amdgcn_s_setprio(3);                  // survivors, hit staging, flush and the next tile's loads: highest
		// Limits 0 and 1 (few survivors: the filter passes 2.6e-4 / 1.5e-5 of the offsets): ONE survivor per lane and pass -- the
		// next one of whichever chain holds one; a pass that looks at one offset of every chain costs NCH checks
		// for a small fraction of a survivor per lane.  4 GiB at limit 0: 1.85 -> 1.71 ms; at limit 2 nothing (2.52 / 2.50), at
		// limit 4 the lane's survivors queue up (3.14 -> 3.91): the every-chain pass stays for limits of 2 and more.
		if constexpr (LIMIT >= 0 && LIMIT <= KL_SELECT_LIMIT) {
		for (;;) {
			uint32_t mm = m[NCH - 1], da = D[NCH - 1], db = D[NCH], dc = D[NCH + 1], ci = NCH - 1;   // the lane's first chain that holds a survivor
#pragma unroll
			for (int c = NCH - 2; c >= 0; c--) {
				const bool s = m[c] != 0;
				mm = s ? m[c] : mm;
				da = s ? D[c] : da;
				db = s ? D[c + 1] : db;
				dc = s ? D[c + 2] : dc;
				ci = s ? (uint32_t)c : ci;
			}
			if (!__ballot(mm != 0))
				break;
			const uint32_t p1 = lowest_bit(mm);             // (-1 for no survivor: see check() below)
			const int e1 = __popc(alignbit(db, da, p1) ^ ac_lo) + __popc(alignbit(dc, db, p1) ^ ac_hi);          // :433
			const bool hit1 = mm != 0 && e1 <= limit;
			const uint32_t rest = mm & (mm - 1);
#pragma unroll
			for (int c = 0; c < NCH; c++)
				m[c] = ci == (uint32_t)c ? rest : m[c];
			if (__ballot(hit1))
				stage(hit1, this_stream, word0 * 64 + 32u * ci + p1, (uint32_t)e1);
		}
		} else {
		// wave-uniform survivor loop.  First pass: one offset of every chain (a wave's 64 lanes practically always hold a survivor in
		// each of the NCH chains).  Further passes: a chain has a second survivor in some lane in one tile of eight, so a chain that
		// is empty wave-wide is skipped (the ballots are the loop's exit test as well) instead of running its check for nobody.
		uint32_t p[NCH];
		int e[NCH];
		bool hit[NCH];
		auto check = [&](int c) {
			p[c] = lowest_bit(m[c]);                        // (-1 for an empty chain: the funnel shifts below take its low five bits, and `hit` is masked)
			e[c] = __popc(alignbit(D[c + 1], D[c], p[c]) ^ ac_lo)
				+ __popc(alignbit(D[c + 2], D[c + 1], p[c]) ^ ac_hi);          // :433
			hit[c] = m[c] != 0 && e[c] <= limit;
			m[c] &= m[c] - 1;
		};
		{
			uint32_t any = 0;
#pragma unroll
			for (int c = 0; c < NCH; c++)
				any |= m[c];
			if (__ballot(any != 0)) {
				bool anyhit = false;
#pragma unroll
				for (int c = 0; c < NCH; c++) {
					check(c);
					anyhit |= hit[c];
				}
				if (__ballot(anyhit)) {
#pragma unroll
					for (int c = 0; c < NCH; c++)
						stage(hit[c], this_stream, word0 * 64 + 32u * c + p[c], (uint32_t)e[c]);
				}
				for (;;) {
					uint64_t live[NCH], anyl = 0;
#pragma unroll
					for (int c = 0; c < NCH; c++) {
						live[c] = __ballot(m[c] != 0);
						anyl |= live[c];
					}
					if (!anyl)
						break;
#pragma unroll
					for (int c = 0; c < NCH; c++) {
						if (!live[c])
							continue;
						check(c);
						stage(hit[c], this_stream, word0 * 64 + 32u * c + p[c], (uint32_t)e[c]);
					}
				}
			}
		}
		}
		PROF_MARK(2);
		iter++;
		if (ord) {
			to_slots(false);
		} else {
			while (q_tail - q_head >= 64)
				flush(64);
		}
		PROF_MARK(3);
	}
	if (ord) {
		to_slots(true);
	} else if (q_tail != q_head) {
		flush(q_tail - q_head);
	}
#ifdef SCAN_PROFILE
	if (lane < 32)
		atomicAdd(&g_scan_prof[lane], (unsigned long long)kl_prof[tid >> 6][lane]);
#endif
}
