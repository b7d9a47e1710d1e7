// scan_lap_any.h -- scan_lap_any_kernel: LAP_ANY with tables for five errors (syndrome from two tables in LDS, a bitmap in L2 per
// survivor).  A piece of scan.hip.
#pragma once
#include "scan_core.h"

__global__ __launch_bounds__(SCAN_THREADS) void scan_lap_any_kernel(ScanArgs a)
{
	extern __shared__ uint32_t lds[];

	const uint32_t tid = threadIdx.x;
	const uint32_t lane = tid & 63;
	const uint32_t wave = tid >> 6;
	const uint32_t slot_off = LDS_OFF_PARK + CAND_BYTES * (wave * 64 * PARK_SLOTS + lane * PARK_SLOTS);
	const uint32_t ring_off = LDS_OFF_QUEUE + CAND_BYTES * wave * QRING;
	uint32_t kdiff = a.t.kdiff;
	asm volatile("" : "+v"(kdiff));           // keep it in a VGPR: a VALU op with an SGPR source issues at half rate

	// tile order: one contiguous eighth of the tiles per XCD, its workgroups interleaved (scan_core.h)
	TILE_ORDER(a, first_tile, tile_step, n_mine)

	// tables -> LDS, 16 bytes per lane per step, coalesced
	{
		char *ldsb = reinterpret_cast<char *>(lds);
		const uint4 *srcA = reinterpret_cast<const uint4 *>(a.t.tabA);
		const uint4 *srcB = reinterpret_cast<const uint4 *>(a.t.tabB);
		uint4 *dA = reinterpret_cast<uint4 *>(ldsb + LDS_OFF_TABA);
		uint4 *dB = reinterpret_cast<uint4 *>(ldsb + LDS_OFF_TABB);
		for (uint32_t i = tid; i < LDS_TABA_WORDS / 4; i += SCAN_THREADS) dA[i] = srcA[i];
		for (uint32_t i = tid; i < LDS_TABB_WORDS / 4; i += SCAN_THREADS) dB[i] = srcB[i];
	}
	__syncthreads();
#ifdef SCAN_PROFILE
	const uint32_t prof_off = LDS_OFF_PROF + 128u * (tid >> 6);
	if ((tid & 63) < 32)
		lds_st(prof_off + 4u * (tid & 63), 0u);
	uint64_t prof_t;
	asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(prof_t) : : "memory");
#endif

	// Candidate = passed the bitmap in L2 (a quarter of the survivors with tables for five errors).  Three stages:
	//  1. park: one DS write into a private slot of the lane -- no atomics and no ballots in
	//     the survivor loop (a lane with all slots full verifies in place: adversarial input);
	//  2. compact: at a tile end, once enough lanes hold one, the parked codes are packed
	//     into the wave's ring with ballot + mbcnt;
	//  3. verify: the exact reference rule, 64 ring entries at a time (full wave, and the
	//     compiler merges the 64 hit-counter atomics into one).
	// code = (tile iteration << 12) | (lane that owns the word << 6) | offset in the word
	uint32_t n_parked = 0;
	uint32_t q_head = 0, q_tail = 0;          // wave-uniform ring cursors (free running)
	CODE_WORD_CLOSURE(SCAN_THREADS, 64, (void)0);
	// hits: up to 64 pending records per wave in registers, written 1 KiB at a time behind one counter atomic (scan_core.h)
	HIT_QUEUE_CLOSURES();
	auto park = [&](uint32_t code, uint32_t wlo, uint32_t whi) {
		if (n_parked < PARK_SLOTS) {
			const u32x4 rec = {code, wlo, whi, 0u};
			lds_st4(slot_off + CAND_BYTES * n_parked, rec);
			n_parked++;
		} else {                                  // all slots taken (adversarial input): verify in place
			uint32_t stream, lap, nerr;
			const uint64_t word = code_word(code, stream);
			if (verify_lap_any(a, ((uint64_t)whi << 32) | wlo, lap, nerr))
				emit_hit(a, stream, word * 64 + (code & 63), lap, nerr);
		}
	};
	auto drain = [&](uint32_t n) {
		PROF_MARK(17);
		bool hit = false;
		uint32_t stream = 0, lap = 0, nerr = 0;
		uint64_t offset = 0;
		if (lane < n) {
			const u32x4 rec = lds_ld4(ring_off + CAND_BYTES * ((q_head + lane) & (QRING - 1)));
			const uint32_t code = rec.x;
			const uint64_t w = ((uint64_t)rec.z << 32) | rec.y;
			offset = code_word(code, stream) * 64 + (code & 63);
			hit = verify_lap_any(a, w, lap, nerr);
		}
		push_hits(hit, stream, offset, lap, nerr);
		q_head += n;
		PROF_MARK(18);
	};
	auto compact = [&](bool final) {
		for (uint32_t k = 0; k < PARK_SLOTS; k++) {
			const uint64_t have = __ballot(n_parked > k);
			if (!have)
				break;
			if (n_parked > k) {
				const uint32_t slot = q_tail + __builtin_amdgcn_mbcnt_hi((uint32_t)(have >> 32),
						__builtin_amdgcn_mbcnt_lo((uint32_t)have, 0));
				const uint32_t from = slot_off + CAND_BYTES * k, to = ring_off + CAND_BYTES * (slot & (QRING - 1));
				lds_st4(to, lds_ld4(from));
			}
			q_tail += __popcll(have);
			while (q_tail - q_head >= 64)       // keeps the ring below 128 entries
				drain(64);
		}
		n_parked = 0;
		if (final && q_tail != q_head)
			drain(q_tail - q_head);
	};

	// tile cursor without divisions: uniform (stream, tile-in-stream) stepped per tile
	// (32-bit: the launcher refuses launches with 2^32 tiles or more, and 64-bit compares of wave-uniform
	// values run on the VALU -- the SALU has none)
	struct Cursor { uint32_t stream; uint32_t t; };
	const uint32_t tiles_per_stream = (uint32_t)a.tiles_per_stream;
	Cursor cur = {a.n_streams, 0};               // stream == n_streams: nothing (left) to do
	uint32_t handed = 0;                          // tiles handed out so far
	if (n_mine) {
		cur.stream = a.n_streams > 1 ? first_tile / tiles_per_stream : 0;
		cur.t = first_tile - cur.stream * tiles_per_stream;
	}
	auto advance = [&](Cursor &c) {
		if (++handed >= n_mine) {
			c.stream = a.n_streams;
			return;
		}
		// (no wrap: the launcher keeps the tile count below 2^20 x grid size)
		c.t += tile_step;
		while (c.t >= tiles_per_stream && c.stream < a.n_streams) {
			c.t -= tiles_per_stream;
			c.stream++;
		}
	};
	// a tile whose 1024 words + halo word and 65536 offsets are all in range needs no masks
	auto tile_full = [&](uint32_t tt) {                         // (one scalar compare; the launcher did the 64-bit arithmetic)
		return tt < a.full_tiles;
	};
	// front set (tables for five errors, round 6): window positions of the second check stream behind offset 63 reach 23 bits into
	// the word after next -- its low dword comes along
	const bool front = a.t.slide4b_bitmap != nullptr;          // launch-uniform
	auto load_pair = [&](const Cursor &c, uint64_t &lo, uint64_t &hi, uint32_t &far) {
		lo = hi = 0;
		far = 0;
		if (c.stream >= a.n_streams)
			return;
		const uint64_t *tp = a.words + (uint64_t)c.stream * a.pitch_words + (uint64_t)c.t * SCAN_THREADS;   // uniform
		if (tile_full(c.t)) {
			lo = stream_ld(tp + tid);
			hi = stream_ld(tp + tid + 1);
		} else {
			const uint64_t w = (uint64_t)c.t * SCAN_THREADS + tid;
			lo = w < a.n_words ? stream_ld(tp + tid) : 0;
			hi = w + 1 < a.n_words ? stream_ld(tp + tid + 1) : 0;
		}
		if (front) {
			const uint64_t w = (uint64_t)c.t * SCAN_THREADS + tid;
			far = w + 2 < a.n_words ? *reinterpret_cast<const uint32_t *>(tp + tid + 2) : 0u;
		}
	};

	// Each trip of the main loop works on UNROLL tiles at once (independent words in the same
	// lane): with one workgroup of 16 waves per CU (the tables fill the LDS) this is what keeps
	// enough independent LDS chains in flight to cover the DS latency.
	constexpr int UNROLL = SCAN_UNROLL;
	Cursor tc[UNROLL];
	uint64_t lo[UNROLL], hi[UNROLL];
	uint32_t far[UNROLL];
#pragma unroll
	for (int u = 0; u < UNROLL; u++) {
		tc[u] = cur;
		load_pair(cur, lo[u], hi[u], far[u]);
		advance(cur);
	}

	for (uint32_t it = 0; tc[0].stream < a.n_streams; it += UNROLL) {
		// software prefetch of the next tiles: the loads fly while these are processed
		Cursor nc[UNROLL];
		uint64_t nlo[UNROLL], nhi[UNROLL];
		uint32_t nfar[UNROLL];
#pragma unroll
		for (int u = 0; u < UNROLL; u++) {
			nc[u] = cur;
			load_pair(cur, nlo[u], nhi[u], nfar[u]);
			advance(cur);
		}

		uint32_t d[UNROLL][4], m[UNROLL][2], cls[UNROLL][2];
		uint32_t c2[UNROLL][3] = {};                             // the second check stream (front set), positions 0 .. 95 of the lane's word
#pragma unroll
		for (int u = 0; u < UNROLL; u++) {
			d[u][0] = (uint32_t)lo[u]; d[u][1] = (uint32_t)(lo[u] >> 32);
			d[u][2] = (uint32_t)hi[u]; d[u][3] = (uint32_t)(hi[u] >> 32);
			if (a.msb) {
#pragma unroll
				for (int k = 0; k < 4; k++)
					d[u][k] = msb_dword(d[u][k]);
			}
			// offsets of this word that lie inside [0, search_bits)
			uint32_t validA = 0xffffffffu, validB = 0xffffffffu;
			if (tc[u].stream >= a.n_streams) {
				validA = validB = 0;
			} else if (!tile_full(tc[u].t)) {
				const uint64_t first_off = ((uint64_t)tc[u].t * SCAN_THREADS + tid) * 64;
				const uint64_t valid = first_off >= a.search_bits ? 0ULL
					: (a.search_bits - first_off >= 64 ? FULL_MASK : ((1ULL << (a.search_bits - first_off)) - 1));
				validA = (uint32_t)valid;
				validB = (uint32_t)(valid >> 32);
			}
			barker32(d[u][1], d[u][2], validA, m[u][0], cls[u][0]);    // offsets 0..31: window bits 57.. in d1:d2
			barker32(d[u][2], d[u][3], validB, m[u][1], cls[u][1]);    // offsets 32..63
			if (front) {
				const uint32_t d4 = a.msb ? msb_dword(far[u]) : far[u];
				c2[u][0] = slide32<SLIDE4B_TAPS>(d[u][0], d[u][1], d[u][2]);
				c2[u][1] = slide32<SLIDE4B_TAPS>(d[u][1], d[u][2], d[u][3]);
				c2[u][2] = slide32<SLIDE4B_TAPS>(d[u][2], d[u][3], d4);
			}
#ifdef SCAN_PROFILE
			PROF_PIN(m[u][0]); PROF_PIN(m[u][1]);
			if (u == UNROLL - 1) PROF_MARK(14);
#endif
		}

		// Survivor loop: runs while any lane of the wave has survivors; each pass takes one
		// survivor of every 32-offset half in flight (2 * UNROLL independent chains).  The LDS
		// reads of all chains are issued before any result is used.
		// Lanes without a survivor in a chain (45 % of them, measured) read along: their ffbl is ~0, so
		// they form some in-range table address from offset 31, and `m >> p` -- bit 0 set exactly for
		// a lane that has a survivor -- masks their bitmap bit afterwards.  Switching them off in the
		// exec mask instead (a v_cmp, an s_and_saveexec, a skip branch and an s_or per group of reads)
		// was 3 % slower: the loop is bound by instruction issue, not by LDS bank conflicts
		// (profiles/r02_cut).  The bitmap in L2 is still read under exec.
#pragma unroll
		for (int u = 0; u < UNROLL; u++) {
			PROF_PIN(m[u][0]);
			PROF_PIN(m[u][1]);
		}
		PROF_MARK(0);
		for (uint32_t pass = 1;; pass++) {
			uint32_t any = 0;
#pragma unroll
			for (int u = 0; u < UNROLL; u++)
				any |= m[u][0] | m[u][1];
			if (!__ballot(any != 0))
				break;
			uint32_t p[UNROLL][2], t1[UNROLL][2], t2[UNROLL][2], bw[UNROLL][2], proj[UNROLL][2];
			Probe q[UNROLL][2];
#pragma unroll
			for (int u = 0; u < UNROLL; u++)
#pragma unroll
				for (int h = 0; h < 2; h++) {
					p[u][h] = lowest_bit(m[u][h]);
					q[u][h] = probe_addr(d[u][h], d[u][h + 1], d[u][h + 2], cls[u][h], kdiff, p[u][h]);
					t1[u][h] = lds_ld(LDS_OFF_TABA + q[u][h].offA);
					t2[u][h] = lds_ld(LDS_OFF_TABB + q[u][h].offB);
				}
			uint32_t anybit = 0, bit[UNROLL][2], live[UNROLL][2], i2[UNROLL][2];
			// front set (round 6): 24 positions of the second check stream at the survivor's offset, one dword of a 2 MiB set in L2 per
			// survivor (the four chains' loads in flight together); only its members (22 %) go on to the bitmap over the syndrome.
			// (Sending the front-set loads of pass k + 1 behind the bitmap loads of pass k -- a two-stage pipeline, 107 VGPRs --
			// changed nothing: 7.40 against 7.28 ms per GiB; the kernel runs at the two tables' probe rates, 236 G/s out of the L2 and
			// 88 G/s for the 8 MiB one, not at their latency.  profiles/r06_init5)
			bool go[UNROLL][2];
			if (front) {
				uint32_t v1[UNROLL][2], w1[UNROLL][2];
#pragma unroll
				for (int u = 0; u < UNROLL; u++)
#pragma unroll
					for (int h = 0; h < 2; h++) {
						v1[u][h] = alignbit(c2[u][h + 1], c2[u][h], p[u][h]);
						w1[u][h] = 0;
						if (m[u][h])
							w1[u][h] = a.t.slide4b_bitmap[(v1[u][h] >> 5) & ((1u << (SLIDE4B_BITS - 5)) - 1)];
					}
#pragma unroll
				for (int u = 0; u < UNROLL; u++)
#pragma unroll
					for (int h = 0; h < 2; h++)
						go[u][h] = (int32_t)(w1[u][h] << (v1[u][h] & 31)) < 0;      // (words bit-reversed: member = sign; 0 for an empty chain)
			} else {
#pragma unroll
				for (int u = 0; u < UNROLL; u++)
#pragma unroll
					for (int h = 0; h < 2; h++)
						go[u][h] = m[u][h] != 0;
			}
#pragma unroll
			for (int u = 0; u < UNROLL; u++)
#pragma unroll
				for (int h = 0; h < 2; h++) {
					proj[u][h] = xor3(q[u][h].x, t1[u][h], t2[u][h]);
					// tables for five errors: every value of any set that fits the LDS is a sum of five columns, so the
					// survivors (round 6: those the front set lets through) probe the 2^26-bit bitmap in L2 / Infinity Cache right here
					i2[u][h] = (proj[u][h] * 0x9E3779B1u) >> a.t.bitmap2_shift;
					bw[u][h] = 0;
					if (go[u][h])
						bw[u][h] = a.t.bitmap2[i2[u][h] >> 5];
				}
#pragma unroll
			for (int u = 0; u < UNROLL; u++)
#pragma unroll
				for (int h = 0; h < 2; h++) {
					// only bit 0 counts: (bitmap word >> index) & (m >> p), p = ~0 for m == 0: 0 >> 31
					live[u][h] = m[u][h] >> p[u][h];
					bit[u][h] = bw[u][h] >> (i2[u][h] & 31);
					anybit = BITOP3(bit[u][h], live[u][h], anybit, 0xea);   // anybit |= bit & live, one instruction
					m[u][h] &= m[u][h] - 1;
				}
			if (anybit & 1) {
#pragma unroll
				for (int u = 0; u < UNROLL; u++)
#pragma unroll
					for (int h = 0; h < 2; h++)
						if (bit[u][h] & live[u][h] & 1)  // rare: rebuild the window of this offset and keep it with the code
							park(((it + u) << 12) | (lane << 6) | (h << 5) | (p[u][h] & 31),
							     alignbit(d[u][h + 1], d[u][h], p[u][h]), alignbit(d[u][h + 2], d[u][h + 1], p[u][h]));
			}
			PROF_MARK(pass < 13 ? pass : 13);
		}

		// wave-uniform: compact (and verify) once enough lanes hold a candidate
		PROF_MARK(16);
		if (__popcll(__ballot(n_parked != 0)) >= 24 || __ballot(n_parked >= PARK_SLOTS))
			compact(false);
		PROF_MARK(17);
#ifdef SCAN_PROFILE
#pragma unroll
		for (int u = 0; u < UNROLL; u++) {
			PROF_PIN(nlo[u]);
			PROF_PIN(nhi[u]);
		}
#endif
		PROF_MARK(19);
#pragma unroll
		for (int u = 0; u < UNROLL; u++) {
			tc[u] = nc[u];
			lo[u] = nlo[u];
			hi[u] = nhi[u];
			far[u] = nfar[u];
		}
	}
	compact(true);
	flush_hits();
#ifdef SCAN_PROFILE
	if (lane < 32)
		atomicAdd(&g_scan_prof[lane], (unsigned long long)lds_ld(prof_off + 4u * lane));
#endif
}
