// packet_trials.h -- piece of packet.hip: the 64-clock trial kernels (trials_linear_kernel: throughput, trials_wide_kernel: latency)
// and uap_table_kernel.  Restate try_clock (:1178) + crc_check (:708) of bluetooth_packet.c for every (packet, clock).
#pragma once

// ---- kernels --------------------------------------------------------------------------------

// The throughput shape for large batches (BASELINE config 5: 10^6 detected packets).  What a trial's crc_check
// spends its time on when it is run as written (do_crc_check above) -- FEC 2/3 over up to 183 blocks, whitening, a CRC over up to 343 bytes
// -- does not depend on the clock candidate except through two XORs:
//   * FEC 2/3 is undone BEFORE whitening (:898-958), so the decoded bits, and which block fails first, are
//     properties of the packet;
//   * the CRC register is GF(2)-linear:  reg(seed, data ^ whitening, L bytes)
//         = A^L(seed)  ^  reg(0, data, L)  ^  reg(0, whitening, L),
//     the first from g_il (eight 16-bit terms selected by the UAP), the last from g_pw.
// So a workgroup first works out, once per packet, the decoded bytes of the two FEC 2/3 layouts (payload at
// 122, DV data at 202), their first failing block, the HV1 verdict, and reg(0, data, 4i) for every fourth
// byte count of the three data layouts (raw, FEC at 122, FEC at 202) -- and a DM / DH / FHS trial is then a
// payload header, a length, a handful of table reads and a compare.  EV4 (which scans for the first byte
// count whose CRC is zero) still walks bytes, but bytes that are already decoded.
// a word of LDS as it is now (another lane of the wave may just have changed it): a volatile read through a generic
// pointer is a FLAT load, which waits on both memory counters -- and with it on every prefetched word still in flight
__device__ __forceinline__ uint32_t lds_now(const uint32_t *p)
{
	return *(volatile __attribute__((address_space(3))) const uint32_t *)p;
}

#define TL_THREADS 512                  // two workgroups per CU, 32 packets per batch, 74 KiB of LDS each (one 1024-thread workgroup,
                                        // 64 packets, 126 KiB: 0.930 against 0.921-0.926 ms per 2^20 packets, profiles/r05_trials)
#define TL_PACKETS (TL_THREADS / 16)
#define TL_WGS_PER_CU (1024 / TL_THREADS)
#define TL_TRIALS  (TL_PACKETS * 64)
#define TL_A_BLOCKS 183                     // DM5: 228 bytes = 1824 bits
#define TL_A_BYTES  232                     // >= 229, multiple of 4
#define TL_B_BLOCKS 10                      // DV: 12 bytes
#define TL_B_BYTES  16
#ifdef TL_PROFILE
__device__ unsigned long long g_tl_prof[16];
// per-workgroup counters in LDS (global atomics here would sit in the same in-order queue as the loads the
// kernel waits for, and the profile would show their latency instead of the kernel's)
#define TL_PROF_START __shared__ uint32_t tl_acc[16]; if (threadIdx.x < 16) tl_acc[threadIdx.x] = 0; uint64_t tl_t = __builtin_readcyclecounter()
#define TL_PROF(k) do { const uint64_t n_ = __builtin_readcyclecounter(); if (tid == 0) tl_acc[k] += (uint32_t)(n_ - tl_t); tl_t = n_; } while (0)
#define TL_PROF_END do { __syncthreads(); if (tid < 16) atomicAdd(&g_tl_prof[tid], (unsigned long long)tl_acc[tid]); } while (0)
#else
#define TL_PROF_START do { } while (0)
#define TL_PROF(k) do { } while (0)
#define TL_PROF_END do { } while (0)
#endif
#define TL_AFAIL(p) lds_now(&a_fail[p])
__global__ __launch_bounds__(TL_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void trials_linear_kernel(const uint64_t *packets, const btbbx_pkt_in *in,
							     uint32_t n_packets, btbbx_trial *trials, const uint32_t *d_count)
{
	if (d_count)                                        // the list's length lives in HBM: n_packets is its capacity
		n_packets = min(n_packets, *d_count);
	__shared__ uint64_t pk[TL_PACKETS][BTBBX_PKT_WORDS + 1];
	__shared__ __attribute__((aligned(8))) btbbx_pkt_in pin[TL_PACKETS];
	__shared__ uint32_t hdr_ut[TL_PACKETS];
	__shared__ uint16_t clk_ut[64];
	__shared__ __attribute__((aligned(16))) uint16_t pw20[64];   // register after the 20 whitening bytes of an FHS attempt
	__shared__ __attribute__((aligned(16))) uint16_t lin[LIN_MAXLEN * 16];
	__shared__ __attribute__((aligned(16))) uint16_t advw[7 * 2 * 256];
	__shared__ uint16_t order[TL_TRIALS];
	__shared__ uint32_t t_info[TL_TRIALS];            // per trial: try_clock's return value | type << 8 | UAP << 16
	__shared__ int16_t t_rv[TL_TRIALS];
	__shared__ uint32_t pk_sort[TL_PACKETS];          // per packet: type key | varies with the clock << 4 | rank among its like << 8
	__shared__ uint32_t type_base[18];                // first trial slot of every type; [17] = packets whose type varies with the clock
	// per packet
	// (a10 is dead behind step 2a, the barrier that follows it separates it from step 2c: its rows are then the packet's p4a and
	// p4c rows.  93 dwords per row: odd, so the rows of consecutive packets start in different banks.)
	__shared__ uint16_t a10[TL_PACKETS][TL_A_BLOCKS + 3];       // decoded 10-bit groups, payload at 122
	static_assert(TL_A_BYTES / 4 + LIN_MAXLEN / 4 <= TL_A_BLOCKS + 3, "p4a and p4c of a packet lie in its a10 row");
	__shared__ uint16_t b10[TL_PACKETS][TL_B_BLOCKS + 2];       // ... DV data at 202
	__shared__ uint32_t a_bytes[TL_PACKETS][TL_A_BYTES / 4], b_bytes[TL_PACKETS][TL_B_BYTES / 4];
	__shared__ uint32_t a_fail[TL_PACKETS], b_fail[TL_PACKETS]; // first undecodable block
	__shared__ uint16_t p4b[TL_PACKETS][TL_B_BYTES / 4];
	auto p4a = [&](uint32_t p) { return &a10[p][0]; };
	auto p4c = [&](uint32_t p) { return &a10[p][TL_A_BYTES / 4]; };
	__shared__ int8_t hv_rv[TL_PACKETS];
	__shared__ uint16_t chunk_reg[TL_PACKETS][20];
	const uint32_t tid = threadIdx.x, lane = tid & 63;
	TL_PROF_START;
	// tables once per workgroup (the workgroups are persistent: each takes every gridDim.x-th batch)
	for (uint32_t i = tid; i < LIN_MAXLEN * 2; i += TL_THREADS)
		reinterpret_cast<uint4 *>(lin)[i] = reinterpret_cast<const uint4 *>(g_lin)[i];
	for (uint32_t i = tid; i < 7 * 2 * 256 / 8; i += TL_THREADS)
		reinterpret_cast<uint4 *>(advw)[i] = reinterpret_cast<const uint4 *>(g_advw)[i];
	chain_lds_init();                                       // ends with a barrier
	if (tid >= 64 && tid < 128) {
		const uint32_t wb = (uint32_t)wh_bits(wh_start(tid - 64, 0), 18);
		// bits 12, 13: the clock's rank among the FOUR clocks that whiten the type field alike (the 64 clocks map onto the
		// sixteen 4-bit values four times each -- an affine map of full rank; tables.cpp checks it on the host): with that,
		// where a trial stands in type order is arithmetic (step 1b below)
		const uint32_t wt = (wb >> 3) & 0xf;
		uint32_t crank = 0;
		for (uint32_t k = 0; k < 16; k++) {
			const uint64_t mk = __ballot(wt == k);
			if (wt == k)
				crank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mk >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mk, 0));
		}
		clk_ut[tid - 64] = (uint16_t)(uap_from_hec(wb & 0x3ff, wb >> 10) | (wt << 8) | (crank << 12));
		const uint32_t v = (uint32_t)wh_bits(wh_start(tid - 64, 18), 7);
		uint32_t x = 0;
		for (int j = 0; j < 7; j++)
			if ((v >> j) & 1)
				x ^= lin[20 * 16 + 8 + j];
		pw20[tid - 64] = (uint16_t)x;
	}
	const uint32_t n_batches = (n_packets + TL_PACKETS - 1) / TL_PACKETS;
	// a batch is 16 x 51 packet words + 16 x 2 words of btbbx_pkt_in, four per thread; the next batch's words fly
	// while this one is worked on (all of them the same kind of guarded load: anything the compiler has to merge
	// with an old value, or may re-issue at its use, ends up waited for right behind the prefetch)
	constexpr uint32_t PK_ELEMS = TL_PACKETS * (BTBBX_PKT_WORDS + 1), IN_ELEMS = TL_PACKETS * sizeof(btbbx_pkt_in) / 8;
	constexpr uint32_t PER_THREAD = (PK_ELEMS + IN_ELEMS + TL_THREADS - 1) / TL_THREADS;
	static_assert(sizeof(btbbx_pkt_in) == 16, "two words per btbbx_pkt_in");
	uint64_t pre[PER_THREAD];
	// every load unconditional, from a clamped address (validity is applied when the words go to LDS)
	// (round 4: the element -> (packet, word) arithmetic of the two lambdas is done where it is used -- `tv` is opaque to the
	// compiler --: hoisted out of the batch loop it is a dozen registers that live in scratch, and a reload from scratch counts
	// on the same in-order counter as the prefetched words)
	auto fetch = [&](uint32_t b) {
		const uint32_t f = b * TL_PACKETS, have = b < n_batches ? (n_packets - f < TL_PACKETS ? n_packets - f : TL_PACKETS) : 0;
		uint32_t tv = tid;
		asm volatile("" : "+v"(tv));
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++) {
			const uint32_t i = tv + TL_THREADS * k;
			const uint32_t p = i / (BTBBX_PKT_WORDS + 1), w = i % (BTBBX_PKT_WORDS + 1), e = i - PK_ELEMS;
			const uint64_t *src = packets;
			if (i < PK_ELEMS) {
				if (p < have && w < BTBBX_PKT_WORDS)
					src = packets + (uint64_t)(f + p) * BTBBX_PKT_WORDS + w;
			} else if (e < 2 * have) {
				src = reinterpret_cast<const uint64_t *>(in) + (uint64_t)f * 2 + e;
			}
			pre[k] = *src;
		}
	};
	// the prefetched words of batch b go to LDS (and the per-batch counters are reset)
	auto stage_in = [&](uint32_t b) {
		const uint32_t f = b * TL_PACKETS, have = b < n_batches ? (n_packets - f < TL_PACKETS ? n_packets - f : TL_PACKETS) : 0;
		uint32_t tv = tid;
		asm volatile("" : "+v"(tv));
#pragma unroll
		for (uint32_t k = 0; k < PER_THREAD; k++) {
			const uint32_t i = tv + TL_THREADS * k;
			const uint32_t p = i / (BTBBX_PKT_WORDS + 1), w = i % (BTBBX_PKT_WORDS + 1);
			if (i < PK_ELEMS)
				pk[p][w] = (p < have && w < BTBBX_PKT_WORDS) ? pre[k] : 0;
			else if (i < PK_ELEMS + IN_ELEMS)
				reinterpret_cast<uint64_t *>(pin)[i - PK_ELEMS] = pre[k];
		}
		if (tid < TL_PACKETS) {
			a_fail[tid] = TL_A_BLOCKS;
			b_fail[tid] = TL_B_BLOCKS;
		}
	};
	fetch(blockIdx.x);
	stage_in(blockIdx.x);
	fetch(blockIdx.x + gridDim.x);
	for (uint32_t batch = blockIdx.x; batch < n_batches; batch += gridDim.x) {
	const uint32_t first = batch * TL_PACKETS;
	const uint32_t mine = n_packets - first < TL_PACKETS ? n_packets - first : TL_PACKETS;

	__syncthreads();                                        // this batch is in LDS, the previous batch's results are read
	TL_PROF(0);

	// 1. try_clock (:1178-1195).  uap_from_hec (:693-705) and the type field are GF(2)-linear in the 18 header
	// bits and unwhitening XORs a clock-dependent constant onto them, so try_clock(c) = U(header) ^ U(whitening
	// bits of c): one U per packet here, one per clock in clk_ut (as in uap_table_kernel), one XOR per trial below.
	// Wrong candidate clocks turn the 4 type bits into noise, so the 64 trials of a packet spread over all
	// sixteen decoders: the trial numbers are counting-sorted by type (LDS atomics) and step 3 walks them in
	// that order, a wave's 64 consecutive entries being trials of ONE type except at the few type boundaries.
	// (Trials are independent of each other -- the one cross-trial dependency of the reference, EV4 reading
	// the llid / flow a previous trial left, cannot change a result, see do_EV4 -- so their order is free.)
	// 1b. (round 5) The trial numbers in type order WITHOUT a sort over the 4096 trials.  The type of trial (packet, clock)
	// is the packet's four raw type bits XOR four whitening bits that depend on the clock alone, and every 4-bit value is the
	// whitening of exactly four clocks: a packet whose type varies with the clock (whitened, header FEC 1/3 decodable) puts
	// exactly FOUR trials into EVERY type.  So type t starts at slot 4 nvar t + 64 x (packets of fixed type < t), the trial of
	// varying packet number r and clock c is slot base[type] + 4 r + (rank of c among its four), and the 64 trials of a
	// fixed-type packet (not whitened, or FEC 1/3 failed: SURVEY Q5) lie together behind them.  One wave ranks the packets of a batch;
	// rounds 2-4 counted every trial into its type with an LDS atomic (sixteen counters, 4096 atomics per batch) and scattered
	// the trial numbers in a second pass behind a scan of the counters.
	static_assert(TL_PACKETS <= 64, "one wave ranks the packets of a batch");
	if (tid < 64) {
		const bool live = tid < mine;
		uint32_t h = 0;
		if (live) {
			uint32_t dis;
			const uint32_t hdr = header_fec13(pk[tid], dis);
			h = uap_from_hec(hdr & 0x3ff, hdr >> 10) | (((hdr >> 3) & 0xf) << 8) | ((dis < 4 ? 1u : 0u) << 16);
			hdr_ut[tid] = h;
		}
		const bool fec_ok = (h & 0x10000u) != 0;
		const bool var = live && fec_ok && (pin[live ? tid : 0].flags & F_WHITENED);
		const uint32_t key = !live ? 0u : fec_ok ? (h >> 8) & 0xfu : (uint32_t)pin[tid].type & 0xfu;
		const uint64_t vm = __ballot(var);
		const uint32_t nvar = (uint32_t)__popcll(vm);
		uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(vm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)vm, 0));
		const bool fixed = live && !var;
		uint32_t cf = 0;                                    // lane k: packets of fixed type k
		if (__ballot(fixed)) {
			for (uint32_t k = 0; k < 16; k++) {
				const uint64_t fm = __ballot(fixed && key == k);
				if (fixed && key == k)
					rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(fm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fm, 0));
				if (lane == k)
					cf = (uint32_t)__popcll(fm);
			}
		}
		// (the scan of wave_scan.h, written out: as a call this kernel comes out with other code, profiles/r08_packet)
		uint32_t incl = cf;
#pragma unroll
		for (int dd = 1; dd < 16; dd <<= 1) {
			const uint32_t up = __shfl_up(incl, dd);
			if (lane >= (uint32_t)dd)
				incl += up;
		}
		if (lane < 16)
			type_base[lane] = 4u * nvar * lane + 64u * (incl - cf);
		if (lane == 17)
			type_base[17] = nvar;
		if (tid < TL_PACKETS)
			pk_sort[tid] = key | ((var ? 1u : 0u) << 4) | (rank << 8);
	}
	// 2a. FEC 2/3 of both layouts: sixteen threads per packet (one quarter of a wave), sixteen blocks of the
	// payload layout per round, and no further round once a block of the packet has failed -- nothing behind
	// the first undecodable block can matter to any trial, and in the noise behind a short packet half of
	// all blocks fail.  HV1 verdict (:1131-1150).
	static_assert(TL_THREADS == 16 * TL_PACKETS, "sixteen threads per packet");
	// 32-bit words of the payload layout that lie in front of the packet's first undecodable block (+ the one it starts in)
	auto a_words = [&](uint32_t p) {
		const uint32_t blocks = TL_AFAIL(p) < TL_A_BLOCKS ? TL_AFAIL(p) : TL_A_BLOCKS, n = (blocks * 10 + 31) / 32 + 1;
		return n < TL_A_BYTES / 4 ? n : (uint32_t)(TL_A_BYTES / 4);
	};
	{
		const uint32_t p = tid >> 4, sub = tid & 15;
		if (p < mine) {
			uint32_t d;
			if (sub < TL_B_BLOCKS) {
				if (!fec23_block(pk_bits32(pk[p], 202 + 15 * sub, 15), d))
					atomicMin(&b_fail[p], sub);
				b10[p][sub] = (uint16_t)d;
			}
#pragma unroll 1
			for (uint32_t k0 = 0; k0 < TL_A_BLOCKS; k0 += 16) {
				const uint32_t k = k0 + sub;
				if (k < TL_A_BLOCKS) {
					if (!fec23_block(pk_bits32(pk[p], 122 + 15 * k, 15), d))
						atomicMin(&a_fail[p], k);
					a10[p][k] = (uint16_t)d;
				}
				// the sixteen lanes are in one wave and a wave's LDS operations complete in order: its
				// atomics above are done when this read is served
				__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
				if (TL_AFAIL(p) < k0 + 16)
					break;
			}
			// the decoded bits as bytes, four per thread and step, as far as they decode: by the same sixteen
			// lanes, which wrote every 10-bit group these words are made of (same wave: in order)
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
			auto word_from = [&](const uint16_t *src, uint32_t nblk, uint32_t word) {
				const uint32_t bit = 32 * word, k0 = bit / 10, sh = bit % 10;    // bits 32 word .. 32 word + 31 of the groups
				uint64_t acc = 0;
				for (uint32_t j = 0; j < 5; j++)
					acc |= (uint64_t)(k0 + j < nblk ? src[k0 + j] : 0) << (10 * j);
				return (uint32_t)(acc >> sh);
			};
			if (sub < TL_B_BYTES / 4)
				b_bytes[p][sub] = word_from(b10[p], TL_B_BLOCKS, sub);
			const uint32_t need = a_words(p);
			for (uint32_t word = sub; word < need; word += 16)
				a_bytes[p][word] = word_from(a10[p], TL_A_BLOCKS, word);
		}
	}
	if (tid >= 128 && tid < 128 + mine) {
		const uint32_t p = tid - 128;
		int rv = 1;
		if ((int)pin[p].length - 122 >= 240) {
			uint32_t total = 0;
			for (int i = 0; i < 4; i++) {
				uint32_t dis;
				(void)fec13(pk_bits(pk[p], 122 + 60 * i, 60), 20, dis);
				total += dis;
			}
			rv = total < 20 ? 2 : 0;
		}
		hv_rv[p] = (int8_t)rv;
	}
	__syncthreads();
	TL_PROF(1);
	const uint32_t total = mine * 64;
	for (uint32_t i = tid; i < total; i += TL_THREADS) {
		const uint32_t p = i >> 6;
		const uint32_t h = hdr_ut[p];
		uint32_t uap = pin[p].uap, type = pin[p].type, ret = 0;     // FEC 1/3 failure: nothing changes
		const uint32_t ps = pk_sort[p], cu = clk_ut[lane];
		if (h & 0x10000u) {
			const uint32_t v = (h ^ ((pin[p].flags & F_WHITENED) ? (cu & 0xfffu) : 0u)) & 0xffff;
			uap = ret = v & 0xff;
			type = v >> 8;
		}
		t_info[i] = ret | (type << 8) | (uap << 16);
		// where this trial stands in type order (step 1b)
		const uint32_t slot = (ps & 0x10u) ? type_base[type & 15] + 4u * (ps >> 8) + (cu >> 12)
						   : type_base[type & 15] + 4u * type_base[17] + 64u * (ps >> 8) + lane;
		order[slot] = (uint16_t)i;
	}
	// 2c. reg(0, data, 4 i) for the three layouts (raw: 86 words, FEC at 122: 58, FEC at 202: 4), in chunks of
	// eight words = twenty chunks per packet: (i) every chunk from 0, all in parallel, storing the register in front
	// of each of its words; (ii) per layout the chunk starts, start' = adv32(start) ^ chunk (a dozen dependent
	// steps instead of 86).  reg(0, data, 4 q) is then (register stored for word q) ^ (the chunk's start carried
	// 4 (q mod 8) bytes forward, two reads of advw) -- put together by the trial that asks for it.
	// task t -> (packet, chunk slot r, layout, chunk j, words): raw and DV chunks first (12 per packet), then the
	// payload-layout chunks, of which a packet needs only those in front of its first failing block
	auto chunk_of = [&](uint32_t t, uint32_t &p, uint32_t &r, uint32_t &layout, uint32_t &j, uint32_t &nwords) {
		if (t < mine * 12) {
			p = t / 12;
			j = t % 12;
			if (j < 11) { layout = 0; r = j; nwords = j < 10 ? 8 : LIN_MAXLEN / 4 - 80; }
			else { layout = 2; r = 19; j = 0; nwords = TL_B_BYTES / 4; }
		} else {
			// chunk-major: chunk 0 of every packet, then chunk 1 of every packet, ... -- a packet needs only the chunks in front of its
			// first failing block, so the tasks that have work lie at the front of the list and the second round of TL_THREADS
			// tasks (640 tasks on 512 threads) is empty for everything but full-length DM3 / DM5 payloads (round 6; packet-major
			// left a quarter of the threads a full chunk each in that round: 0.924-0.931 against 0.873 ms per 2^20 packets, all types
			// 0.862 against 0.823 -- profiles/r06_trials; the EV4 scan, taken out as a probe, is 2 % of the batch)
			const uint32_t u = t - mine * 12;
			j = mine == TL_PACKETS ? u / TL_PACKETS : u / mine;
			p = u - j * mine;
			layout = 1;
			r = 11 + j;
			const uint32_t need = a_words(p);
			nwords = need > 8 * j ? (need - 8 * j < 8 ? need - 8 * j : 8) : 0;
		}
	};
	auto data_word = [&](uint32_t p, uint32_t layout, uint32_t i) {
		return layout == 0 ? pk_bits32(pk[p], 122 + 32 * i, 32) : layout == 1 ? a_bytes[p][i] : b_bytes[p][i];
	};
	// the (up to) eight words of a chunk, all loaded before any is used: one LDS round trip, not eight.  The raw
	// payload starts at symbol 122 = dword 3, bit 26 of the packet row, so its words are funnel shifts by 26 of
	// nine consecutive dwords
	auto chunk_words = [&](uint32_t p, uint32_t layout, uint32_t j, uint32_t nwords, uint32_t (&w8)[8]) {
		if (layout == 0) {
			const uint32_t *d = reinterpret_cast<const uint32_t *>(pk[p]) + 3 + 8 * j;
			uint32_t raw[9];
#pragma unroll
			for (uint32_t i = 0; i < 9; i++)
				raw[i] = i <= nwords ? d[i] : 0;
#pragma unroll
			for (uint32_t i = 0; i < 8; i++)
				w8[i] = __builtin_amdgcn_alignbit(raw[i + 1], raw[i], 26);
		} else {
#pragma unroll
			for (uint32_t i = 0; i < 8; i++)
				w8[i] = i < nwords ? data_word(p, layout, 8 * j + i) : 0;
		}
	};
	for (uint32_t t = tid; t < mine * 20; t += TL_THREADS) {
		uint32_t p, r, layout, j, nwords, crc = 0;
		chunk_of(t, p, r, layout, j, nwords);
		if (!nwords)
			continue;
		uint32_t w8[8];
		chunk_words(p, layout, j, nwords, w8);
		uint16_t *dst = layout == 0 ? p4c(p) : layout == 1 ? p4a(p) : p4b[p];
#pragma unroll
		for (uint32_t i = 0; i < 8; i++)
			if (i < nwords) {
				dst[8 * j + i] = (uint16_t)crc;                // the register in front of word i, from 0 at the chunk start
				crc = crc_word(crc, w8[i]);
			}
		chunk_reg[p][r] = (uint16_t)crc;
	}
	__syncthreads();
	TL_PROF(8);
	if (tid >= 64 && tid < 64 + 3 * mine) {
		const uint32_t p = (tid - 64) / 3, layout = (tid - 64) % 3;
		const uint32_t r0 = layout == 0 ? 0 : layout == 1 ? 11 : 19;
		const uint32_t n = layout == 0 ? 11 : layout == 1 ? (a_words(p) + 7) / 8 : 1;
		uint32_t start = 0;
		for (uint32_t j = 0; j < n; j++) {
			const uint32_t c = chunk_reg[p][r0 + j];
			chunk_reg[p][r0 + j] = (uint16_t)start;
			start = g_lds.adv32[0][start & 0xff] ^ g_lds.adv32[1][start >> 8] ^ c;
		}
	}
	__syncthreads();
	TL_PROF(4);

	// 3. crc_check (:708-769) in type order
	for (uint32_t kk = tid; kk < total; kk += TL_THREADS) {
		const uint32_t i = order[kk], p = i >> 6, clock = i & 63;
		const uint32_t info = t_info[i], type = (info >> 8) & 0xff, uap = (info >> 16) & 0xff;
		const bool wht = pin[p].flags & F_WHITENED;
		const int size = (int)pin[p].length - 122;
		const uint32_t seed = crc_seed(uap);
		// what seed and whitening contribute to the register after L bytes: the terms of row L that the
		// seed's eight bits and the seven first whitening bits of this clock select
		const uint32_t sel = (seed >> 8) | (wht ? (uint32_t)wh_bits(wh_start(clock, 18), 7) << 8 : 0u);
		auto seed_row20 = [&](uint32_t sd) {                   // the seed's terms of row 20 alone (FHS tries other clocks)
			const uint4 r0 = reinterpret_cast<const uint4 *>(lin)[40];
			const uint32_t r[4] = {r0.x, r0.y, r0.z, r0.w};
			uint32_t x = 0;
#pragma unroll
			for (int bit = 0; bit < 8; bit++)
				x ^= (0u - ((sd >> (8 + bit)) & 1)) & (r[bit >> 1] >> (16 * (bit & 1)));
			return x & 0xffff;
		};
		auto lin_terms = [&](uint32_t L) {
			uint32_t x = 0;
#pragma unroll
			for (int half = 0; half < 2; half++) {             // (both 16-byte halves of the row asked for together: 115 VGPRs; one at a time -- rounds 4-6a --
			                                                   //  was 1-2 % slower: 0.861 / 0.817 against 0.853 / 0.795 ms, profiles/r06_trials)
				const uint4 q = reinterpret_cast<const uint4 *>(lin)[2 * L + half];
				const uint32_t r[4] = {q.x, q.y, q.z, q.w};
				const uint32_t sl = sel >> (8 * half);
#pragma unroll
				for (int bit = 0; bit < 8; bit++)
					x ^= (0u - ((sl >> bit) & 1)) & (r[bit >> 1] >> (16 * (bit & 1)));
			}
			return x & 0xffff;
		};
		// reg(0, data, L) from the every-fourth-byte table and up to three more bytes
		auto data_reg = [&](int layout, uint32_t L) {
			const uint32_t q = L >> 2, r = L & 3;
			uint32_t crc, w;
			if (layout == 0) { crc = p4c(p)[q]; w = r ? pk_bits32(pk[p], 122 + 32 * q, 32) : 0; }
			else if (layout == 1) { crc = p4a(p)[q]; w = r ? a_bytes[p][q] : 0; }
			else { crc = p4b[p][q]; w = r ? b_bytes[p][q] : 0; }
			// + the chunk's start register carried to word q
			const uint32_t start = chunk_reg[p][(layout == 0 ? 0u : layout == 1 ? 11u : 19u) + (q >> 3)], iw = q & 7;
			crc ^= iw ? (uint32_t)(advw[((iw - 1) * 2) * 256 + (start & 0xff)] ^ advw[((iw - 1) * 2 + 1) * 256 + (start >> 8)]) : start;
			for (uint32_t j = 0; j < r; j++)
				crc = crc_byte(crc, (w >> (8 * j)) & 0xff);
			return crc;
		};
		auto crc_is_zero = [&](int layout, uint32_t L) {
			return (data_reg(layout, L) ^ lin_terms(L)) == 0;
		};
		int rv = 1;
		switch (type) {
		case 2: {                                               // fhs (:783-818)
			if (size < 240) { rv = 1; break; }
			if (a_fail[p] < 16) { rv = 0; break; }
			const uint32_t x = data_reg(1, 20) ^ seed_row20(seed);   // zero register <=> x == reg(0, whitening of the attempt, 20)
			rv = 0;
			if (!wht) {
				if (x == 0) rv = 1000;
			} else {
				// attempt 0 is the trial's own clock, attempts 1..32 are clocks 32..63: their registers in four
				// 16-byte reads (not unrolled: the kernel sits at its 128-VGPR ceiling)
				uint32_t hit = x == pw20[clock];
				const uint32_t xx = x | (x << 16);
#pragma unroll 1
				for (int v = 0; v < 4; v++) {
					const uint4 q = reinterpret_cast<const uint4 *>(&pw20[32])[v];
					const uint32_t d0 = q.x ^ xx, d1 = q.y ^ xx, d2 = q.z ^ xx, d3 = q.w ^ xx;
					hit |= ((d0 & 0xffff) == 0) | ((d0 >> 16) == 0) | ((d1 & 0xffff) == 0) | ((d1 >> 16) == 0)
					     | ((d2 & 0xffff) == 0) | ((d2 >> 16) == 0) | ((d3 & 0xffff) == 0) | ((d3 >> 16) == 0);
				}
				if (hit) rv = 1000;
			}
			break;
		}
		case 3: case 8: case 10: case 14:                       // DM (:898-958)
		case 4: case 11: case 15: {                             // DH (:962-1011)
			const bool fec = type == 3 || type == 8 || type == 10 || type == 14;
			const int layout = !fec ? 0 : (type == 8 ? 2 : 1);
			const int psize = type == 8 ? size - 80 : size;
			const int hb = (type == 3 || type == 8 || type == 4) ? 1 : 2;
			const int hbits = 8 * hb;
			const uint32_t fail = layout == 2 ? b_fail[p] : a_fail[p];
			rv = 0;
			if (psize < hbits) break;                           // decode_payload_header (:821-895) gives up
			uint32_t raw;
			if (fec) {
				if (psize < (hb == 2 ? 30 : 15)) break;
				if (fail < (uint32_t)hb) break;
				raw = (layout == 2 ? b_bytes[p][0] : a_bytes[p][0]) & ((1u << hbits) - 1);
			} else {
				raw = pk_bits32(pk[p], 122, hbits);
			}
			const uint32_t ph = raw ^ (wht ? (uint32_t)wh_bits(wh_start(clock, 18), hbits) : 0u);
			int plen = hb == 2 ? (int)((ph >> 3) & 0x3ff) + 4 : (int)((ph >> 3) & 0x1f) + 3;
			int cap;
			switch (type) {
			case 3:  cap = 20;  break;
			case 4:  cap = 30;  break;
			case 8:  cap = 12;  break;
			case 10: cap = 125; break;
			case 11: cap = 187; break;
			case 14: cap = 228; break;
			default: cap = 343; break;
			}
			if (plen > cap) plen = cap;
			const int nbits = plen * 8;
			if (nbits > psize) { rv = 1; break; }
			if (fec && fail < (uint32_t)(nbits + 9) / 10) break; // a block of the payload does not decode
			rv = crc_is_zero(layout, (uint32_t)plen) ? 10 : 2;
			break;
		}
		case 12: {                                              // EV4 (:1044-1097)
			// iterations b = 0 .. B-1 of the reference's block loop get past its two checks
			uint32_t B = size >= 15 ? (uint32_t)size / 15 : 0;
			if (B > 98) B = 98;
			if (B > a_fail[p]) B = a_fail[p];
			const uint32_t lmax = B ? 5 * (B - 1) / 4 : 0;        // bytes L-1 with ceil(4 L / 5) <= B - 1 are reached
			uint32_t crc = seed, idx = wh_start(clock, 18);
			rv = B == 98 ? 2 : 1;
			// Four bytes per step, and the register after EACH of them from ten independent table reads (the
			// same slicing as crc_word: the 16-bit register is used up by the first two bytes) -- the scan for
			// the first zero register is a chain of up to 121 dependent steps otherwise, and with the trials
			// sorted by type the EV4 waves are what the other fifteen wait for at the barrier.
			for (uint32_t L0 = 0; L0 < lmax; L0 += 4) {
				const uint32_t w = a_bytes[p][L0 >> 2] ^ (wht ? (uint32_t)wh_bits(idx, 32) : 0u);
				idx = idx + 32 >= 127 ? idx + 32 - 127 : idx + 32;
				const uint32_t x0 = (crc ^ w) & 0xff, x1 = ((crc ^ w) >> 8) & 0xff, b2 = (w >> 16) & 0xff, b3 = w >> 24;
				const uint32_t c1 = (crc >> 8) ^ g_lds.crc[x0];
				const uint32_t c2 = g_lds.crc_z[0][x0] ^ g_lds.crc[x1];
				const uint32_t c3 = g_lds.crc_z[1][x0] ^ g_lds.crc_z[0][x1] ^ g_lds.crc[b2];
				const uint32_t c4 = g_lds.crc_z[2][x0] ^ g_lds.crc_z[1][x1] ^ g_lds.crc_z[0][b2] ^ g_lds.crc[b3];
				// byte counts L0 + 1 .. L0 + 4; a zero register counts from 2 bytes on and up to lmax
				const bool z1 = c1 == 0 && L0 + 1 >= 2 && L0 + 1 <= lmax, z2 = c2 == 0 && L0 + 2 <= lmax;
				const bool z3 = c3 == 0 && L0 + 3 <= lmax, z4 = c4 == 0 && L0 + 4 <= lmax;
				if (z1 || z2 || z3 || z4) { rv = 10; break; }
				crc = c4;
			}
			break;
		}
		case 5: rv = hv_rv[p]; break;                           // HV1
		default: rv = 1; break;                                 // EV3 / EV5 always map to 1, the rest is not checked
		}
		if (rv == 0 && type != 2 && type != 3 && type != 5)
			rv = 1;
		t_rv[i] = (int16_t)rv;
	}
	__syncthreads();
	TL_PROF(5);
	// The next batch moves in and the one after that is requested BEFORE this batch's results are stored: gfx9
	// counts loads and stores in one in-order counter, so a wait for prefetched words that comes after the
	// stores also waits for the stores (47 % of the kernel when it was written the other way round).
	stage_in(batch + gridDim.x);
	fetch(batch + 2 * gridDim.x);
	// 4. out, in (packet, clock) order (the t_* arrays are not touched before the barrier at the loop top)
	static_assert(sizeof(btbbx_trial) == 4, "one dword per trial");
	for (uint32_t i = tid; i < total; i += TL_THREADS)
		reinterpret_cast<uint32_t *>(trials)[(uint64_t)first * 64 + i] =
			(t_info[i] & 0xffff) | ((uint32_t)(uint16_t)t_rv[i] << 16);
	TL_PROF(6);
	}
	TL_PROF_END;
}

// Two other shapes of this kernel were built and measured in round 4 and are NOT in the source (kept as text in
// profiles/r04_trials/, both bit-exact on every GPU test):
//   * trials_wave_kernel: a WAVE owns four packets from first word to last result, no workgroup barrier at all.  It does
//     what it was built for -- SQ_WAIT_ANY 72 % -> 43 % of the wave-cycles, VALU-active 9.6 % -> 22 % -- and is slower,
//     1.33 against 0.94 ms per 2^20 packets: 780 VALU wave-instructions per packet against 421 (pmc_*.json there).  A
//     sort over the 256 trials of four packets leaves four types in every pass of 64 (the workgroup-wide sort over 4096
//     leaves one), so the DM/DH, FHS and EV4 code runs in every pass with a quarter of the lanes; the one-lane-per-
//     packet steps are issued by every wave instead of one in sixteen; 80 chunk tasks on 64 lanes are two passes.
//   * trials_hybrid_kernel: the packet-local phases wave-local as above, the type sort workgroup-wide as here, three
//     barriers per batch instead of six: 1.10 ms (the redundant one-lane steps and the second chunk pass cost more than
//     the three barriers saved).
// What stayed: the a_fail reads below no longer go through a generic pointer (lds_now: a volatile generic read is a
// FLAT load, which waits for every prefetched word in flight): 0.957 -> 0.944 ms; the index arithmetic of fetch / stage_in is
// kept out of the batch loop's preheader and the FEC loop rolled (13 spilled registers -> none); every wave works the type
// bases out for itself, which takes thread 0's sixteen dependent LDS steps and their barrier off the path.  The last two
// are within the noise (0.927-0.938 ms; 670 -> 689 M packets/s on random packets of every type, profiles/r04_trials/
// trials_ab2.txt): the kernel waits on the dependent LDS steps of its phases, not on these.
// Small batches (a handful of packets from a live receiver): one workgroup per (packet, clock),
// lane 0 runs the trial.  64 x n waves spread over the CUs, none of them serialising different packet
// types, so the call takes as long as the longest single trial -- the lane-per-clock kernel above is
// the throughput shape, this one the latency shape.
__global__ __launch_bounds__(64) void trials_wide_kernel(const uint64_t *packets, const btbbx_pkt_in *in,
							  uint32_t n_packets, btbbx_trial *trials, const uint32_t *d_count)
{
	chain_lds_init();
	if (d_count)
		n_packets = min(n_packets, *d_count);
	const uint32_t pkt = blockIdx.x >> 6, clock = blockIdx.x & 63;
	if (threadIdx.x || pkt >= n_packets)
		return;
	const btbbx_pkt_in pi = in[pkt];
	PState s;
	s.w = packets + (uint64_t)pkt * BTBBX_PKT_WORDS;
	s.length = (int)pi.length;
	pstate_enter(s, pi);
	pstate_blank_out(s);
	uint32_t dis;
	const uint32_t hdr = header_fec13(s.w, dis);
	const uint32_t uap = do_try_clock(s, clock, hdr, dis);
	const int rv = do_crc_check<false>(s, clock);
	btbbx_trial t;
	t.uap = (uint8_t)uap;
	t.type = (uint8_t)s.type;
	t.rv = (int16_t)rv;
	trials[(uint64_t)pkt * 64 + clock] = t;
}

// The HEC-only half of the brute force (config 5 of BASELINE.json: "64 whitening seeds x HEC
// check"): table[p * 64 + c] = try_clock(c)'s return value | packet_type(c) << 8, 0 when the FEC 1/3
// of the header fails.  uap_from_hec (:693-705) and the type field are GF(2)-linear in the 18
// header bits, and unwhitening XORs a clock-dependent constant onto them, so
//     UAP(c) = U(header) ^ U(whitening bits of c),
// one LFSR run per packet and a 64-entry constant table instead of 64 runs.  The kernel is then
// pure data movement: 8 useful bytes in (the header symbols 68..121 sit in word 1 of a packed
// packet), 128 bytes out per packet.  A wave takes 64 packets; lane L first decodes packet L,
// then the wave writes 8 x 1 KiB: in store j lane L emits the 8 clocks 8 (L & 7).. of packet
// 8 j + (L >> 3), fetching that packet's value with one lane-to-lane read.
__global__ __launch_bounds__(256) void uap_table_kernel(const uint64_t *packets, const btbbx_pkt_in *in, uint32_t n,
							 uint4 *table)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t pkt0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 64;
	if (pkt0 >= n)
		return;
	uint32_t ut = 0;                               // U | type << 8 | fec ok << 16 | whitened << 17
	if (pkt0 + lane < n) {
		const uint32_t p = pkt0 + lane;
		uint32_t dis;
		const uint32_t hdr = fec13((packets[(uint64_t)p * BTBBX_PKT_WORDS + 1] >> 4) & ((1ULL << 54) - 1), 18, dis);
		const uint32_t wht = in ? (in[p].flags & F_WHITENED) : 1u;
		ut = uap_from_hec(hdr & 0x3ff, hdr >> 10) | (((hdr >> 3) & 0xf) << 8) | ((dis < 4 ? 1u : 0u) << 16) | (wht << 17);
	}
	uint32_t wc[4] = {0, 0, 0, 0};                 // this lane's 8 clocks, two 16-bit entries per word
#pragma unroll
	for (int k = 0; k < 8; k++) {
		const uint32_t wb = (uint32_t)wh_bits_const(wh_start_const(8 * (lane & 7) + k, 0), 18);
		const uint32_t e = uap_from_hec(wb & 0x3ff, wb >> 10) | (((wb >> 3) & 0xf) << 8);
		wc[k >> 1] |= e << (16 * (k & 1));
	}
#pragma unroll
	for (int j = 0; j < 8; j++) {
		const uint32_t src = 8 * j + (lane >> 3);
		const uint32_t v = (uint32_t)__shfl((int)ut, (int)src);
		const uint32_t both = (v & 0xffff) * 0x10001u;
		const uint32_t okm = 0u - ((v >> 16) & 1u), whm = 0u - ((v >> 17) & 1u);
		uint4 o;
		o.x = (both ^ (wc[0] & whm)) & okm;
		o.y = (both ^ (wc[1] & whm)) & okm;
		o.z = (both ^ (wc[2] & whm)) & okm;
		o.w = (both ^ (wc[3] & whm)) & okm;
		if (pkt0 + src < n)
			table[(uint64_t)(pkt0 + src) * 8 + (lane & 7)] = o;
	}
}
