// scan_core.h -- what the kernels of scan.hip share: the launch arguments (ScanArgs), the SCAN_PROFILE marks and the device
// primitives -- hit records, stream loads, LDS accessors, the exact rule (verify_lap_any), the barker filter (barker32), the
// sliding check stream (slide32), and what the two LAP_ANY kernels have in common: XCD tile order, candidate code, pending-hit queue.
#pragma once
#include "tile_scan.h"

#define FULL_MASK 0xffffffffffffffffULL

struct ScanArgs {
	const uint64_t *words;
	uint64_t n_words;        // valid words per stream
	uint64_t pitch_words;    // distance between streams
	uint64_t search_bits;    // offsets [0, search_bits) are tested
	uint64_t tiles_per_stream;
	uint64_t n_tiles;
	uint32_t xcd_tiles;      // LAP_ANY: tiles per XCD share (0 = plain round robin over workgroups)
	uint32_t ring_margin;    // scan_slide_kernel: free ring entries below which the pass loop is left for a drain
	uint32_t full_tiles;     // leading tiles of a stream whose words, halo word and offsets are all in range
	uint32_t n_streams;
	uint32_t msb;            // the words hold their symbols MSB first in every byte (BTBBX_FMT_PACKED_MSB): converted in registers
	uint32_t lap;            // known-LAP mode
	uint64_t syncword;       // known-LAP mode
	int max_err;
	btbbx_hit *hits;
	uint32_t hit_cap;
	uint32_t *hit_count;
	unsigned long long *first;   // first-match mode (atomicMin target) or nullptr
	// btbbx_scan_ordered_device: every record written is also counted in the bucket the ordering (sort.hip) will put it in
	// -- the list then needs no histogram pass -- bucket = (stream * bucket_mul + offset) >> bucket_shift; null = off
	uint32_t *bucket_cnt;
	uint64_t bucket_mul;
	uint32_t bucket_shift;
	// btbbx_scan_ordered_device, LAP_ANY with tables for <= 2 errors (scan_slide_kernel<..., ORD>; the ordering itself: sort.hip
	// "segment slots"): a SEGMENT = the 63 words of a tile one wave owns.  All hits of a segment come out of ONE drain of ONE wave,
	// which ranks them by offset among themselves and stores each in the segment's own slots -- plain stores, no counter, no
	// atomic; hits ranked beyond the slots go to an overflow list with (segment, rank).  null = off.
	uint64_t *seg_slots;         // [segments][seg_slot_n]: offset inside the segment (12 bits) | lap << 12 | ac_errors << 36 -- the segment says the rest
	uint16_t *seg_cnt;           // hits of the segment (all of them, also those in the overflow list); zeroed by the caller
	uint32_t seg_slot_n;
	uint32_t segs_per_stream;    // tiles_per_stream x waves per tile
	btbbx_hit *ovf_recs;         // overflow list: records ...
	uint2 *ovf_meta;             // ... and their (segment, rank)
	uint32_t ovf_cap;
	uint32_t *ovf_count;
	uint32_t *irregular;         // set when a hit left outside a drain (a ring without room: a stream of sync words) or the overflow list is full:
	                             // the caller falls back to the general ordering
	const uint32_t *gate;        // the fallback launch itself: returns at once unless *gate != 0
	ScanTables t;
};

// Debug build (-DSCAN_PROFILE): where the LAP_ANY kernel's wave time goes.  Lane 0 of every wave adds the
// s_memtime ticks since its previous mark to a per-wave counter in LDS (global atomics here would stall the
// very loads the loop waits for); the counters go out once at the end and the launcher prints the table.
//   0 = tile loads + barker filter, 1..13 = survivor pass k, 16 = loop exit, 17 = compaction,
//   18 = exact checks, 19 = wait for the prefetched words
#ifdef SCAN_PROFILE
__device__ unsigned long long g_scan_prof[32];
#define PROF_MARK(k) do { uint64_t now_; __builtin_amdgcn_sched_barrier(0); \
		asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_) : : "memory"); __builtin_amdgcn_sched_barrier(0); \
		if (lane == 0) __hip_atomic_fetch_add(reinterpret_cast<lds_u32_t *>(prof_off + 4u * (k)), (uint32_t)(now_ - prof_t), \
						      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); prof_t = now_; } while (0)
#define PROF_PIN(x) asm volatile("" : "+v"(x))
#else
#define PROF_MARK(k) do { (void)(k); } while (0)
#define PROF_PIN(x) do { } while (0)
#endif

__device__ __forceinline__ void count_bucket(const ScanArgs &a, uint32_t stream, uint64_t offset)
{
	if (a.bucket_cnt)
		atomicAdd(&a.bucket_cnt[((uint64_t)stream * a.bucket_mul + offset) >> a.bucket_shift], 1u);
}

__device__ __forceinline__ void emit_hit(const ScanArgs &a, uint32_t stream, uint64_t offset,
					 uint32_t lap, uint32_t nerr)
{
	if (a.first) {
		unsigned long long v = ((unsigned long long)offset << 32) | ((unsigned long long)(lap & 0xffffff) << 8) | nerr;
		atomicMin(a.first, v);
		return;
	}
	uint32_t idx = atomicAdd(a.hit_count, 1u);
	if (idx < a.hit_cap) {
		btbbx_hit h;
		h.offset = offset;
		h.lap = lap;
		h.ac_errors = (uint8_t)nerr;
		h.reserved = 0;
		h.stream = (uint16_t)stream;
		a.hits[idx] = h;
		count_bucket(a, stream, offset);
	}
}

// (Stream words are read once; loading them non-temporally so that they do not push the L2-resident tables of the
// >= 4-error kernels out of the cache changed nothing: 12.0 against 12.06 ms per GiB at five errors, round 3; round 6, the two-level
// form for four errors: 7 % fewer fabric reads, 3 % slower -- profiles/r06_init4.)
__device__ __forceinline__ uint64_t stream_ld(const uint64_t *p)
{
	return *p;
}
// MSB-first bytes (first received symbol in bit 7, the order a radio front end delivers) -> the library's LSB-first dword:
// reverse the dword's 32 bits, put the four bytes back in order (v_bfrev_b32 + v_perm_b32).  The scan kernels do this to the
// four dwords of a lane behind a wave-uniform branch -- in the filter phase, which runs in the other waves' gaps -- instead of
// a conversion pass over the capture in HBM (4 GiB read + 4 GiB written before a 4 GiB scan).
__device__ __forceinline__ uint32_t msb_dword(uint32_t x)
{
	return __builtin_bswap32(__brev(x));
}
__device__ __forceinline__ uint64_t load_word(const uint64_t *base, uint64_t j, uint64_t n_words)
{
	return j < n_words ? stream_ld(base + j) : 0ULL;
}

// The exact acceptance rule of promiscuous_packet_search for one offset that passed the
// barker filter (bluetooth_packet.c:387-416).
// The kernel has no static __shared__, so the dynamic LDS allocation starts at LDS byte 0
// and table addresses are plain byte offsets: every DS access below is `base + offset:imm`
// with the table base folded into the 16-bit immediate.
typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
__device__ __forceinline__ uint32_t lds_ld(uint32_t byte_off) { return *reinterpret_cast<lds_u32_t *>(byte_off); }
__device__ __forceinline__ void lds_st(uint32_t byte_off, uint32_t v) { *reinterpret_cast<lds_u32_t *>(byte_off) = v; }
typedef __attribute__((address_space(3))) uint16_t lds_u16_t;
__device__ __forceinline__ uint32_t lds_ld16(uint32_t byte_off) { return *reinterpret_cast<lds_u16_t *>(byte_off); }
// lanes whose 16-bit entry x, shifted LEFT by sh & 15, is negative as a 16-bit number: the fast-rate left shift (see
// scan_slide_kernel) and the 16-bit compare, both as written here (from C the compiler widens the test to v_bfe_u32 + v_cmp_ne_u32)
__device__ __forceinline__ uint64_t sign16_after_shl(uint32_t x, uint32_t sh)
{
	uint32_t r;
	uint64_t m;
	asm("v_lshlrev_b16 %1, %2, %3\n\tv_cmp_gt_i16_e64 %0, 0, %1" : "=s"(m), "=&v"(r) : "v"(sh), "v"(x));
	return m;
}
typedef __attribute__((address_space(3))) u32x4 lds_u32x4_t;
__device__ __forceinline__ u32x4 lds_ld4(uint32_t byte_off) { return *reinterpret_cast<lds_u32x4_t *>(byte_off); }
__device__ __forceinline__ void lds_st4(uint32_t byte_off, u32x4 v) { *reinterpret_cast<lds_u32x4_t *>(byte_off) = v; }
// a ring record as four dword stores (the compiler pairs them into two ds_write2_b32): its dwords come from registers that
// are not neighbours, and one 16-byte store first copies them into four that are -- vector instructions of a one-lane event
__device__ __forceinline__ void lds_st_rec(uint32_t byte_off, u32x4 v)
{
	lds_st(byte_off, v.x);
	lds_st(byte_off + 4u, v.y);
	lds_st(byte_off + 8u, v.z);
	lds_st(byte_off + 12u, v.w);
}
// ... as written here: where several branches store to one slot the compiler hoists slot + 4 / 8 / 12 out of them as three
// registers and stores four single dwords per branch (scan_slide_kernel's append of a trip's notes)
__device__ __forceinline__ void lds_st_rec2(uint32_t byte_off, uint32_t x, uint32_t y, uint32_t z, uint32_t w)
{
	asm volatile("ds_write2_b32 %0, %1, %2 offset1:1\n\tds_write2_b32 %0, %3, %4 offset0:2 offset1:3"
		     : : "v"(byte_off), "v"(x), "v"(y), "v"(z), "v"(w) : "memory");
}

// w = the 64-symbol window at `offset` (the kernel keeps it with the candidate: by the time a
// batch is verified the stream words have long left the L2, and re-reading them cost 40 % extra
// HBM traffic).
// TWO: the tables hold patterns of two errors or fewer (scan_slide_kernel's one-level form, the only caller that says so: the
// launcher gives it no other tables).  context.cpp builds no second-level bitmap for them, so there is no test for one; a slot
// holds two error positions, not five; and each of the two high syndrome bits is ONE v_bcnt of the XOR of the window's masked
// halves instead of two chained ones (the drain's vector instructions by cause: profiles/r08_drain).  Its syndrome tables are
// the three SYN3 tables at LDS byte `syn3_off` (below), not tabA / tabB in global memory: a drain is a chain of dependent
// loads at the wave's highest priority, and with the tables in LDS it waits for one round trip to the L2 (the pattern table)
// instead of two -- 0.3 to 0.6 % of a launch beside the same rule with global tables, ahead in eight rotations of nine
// (profiles/r08_drain; the drains are 4.8 % of a launch, 2.5 of them the pattern look-up).
// SYN3: tabA and tabB (window bits 34 .. 44 and 45 .. 56, 24 KiB) cut again into three tables of 8 + 8 + 7 bits, 2.5 KiB -- the
// syndrome is linear in the window, tabB affine (it carries the class-0 constant, which stays in the last table alone).
#define SYN3_WORDS 640u
#define SYN3_BYTES (4u * SYN3_WORDS)
static_assert(TABA_FIRST == 34 && TABA_BITS == 11 && TABB_BITS == 12, "the SYN3 tables are cut for window bits 34 .. 56 as 8 + 8 + 7");
__device__ __forceinline__ uint32_t syn3_entry(const ScanTables &t, uint32_t i)
{
	if (i < 256u)
		return t.tabA[i];                                                      // window bits 34 .. 41
	if (i < 512u)
		return t.tabA[((i - 256u) & 7u) << 8] ^ t.tabB[(i - 256u) >> 3] ^ t.tabB[0];   // 42 .. 44 (tabA) and 45 .. 49 (tabB, linear part)
	return t.tabB[(i - 512u) << 5];                                            // 50 .. 56, with tabB's constant
}
// The two-error form in pieces, for a caller that sends the pattern look-up and reads its answer later (scan_slide_kernel's
// split drain); verify_lap_any<.., TWO> is these pieces in a row.  lap_syndrome2 = the syndrome of the window, and the window
// with its barker bits corrected; hslot_of = the first slot of a syndrome's probe sequence; slot_errors2 = a matching slot's
// error positions taken out of the window, their count returned.
__device__ __forceinline__ uint64_t lap_syndrome2(const ScanArgs &a, uint64_t w, uint64_t &sw, uint32_t syn3_off)
{
	const uint32_t win = (uint32_t)(w >> 57);
	const uint32_t cls = __popc(win ^ BARKER1) <= 1 ? 1u : 0u;
	sw = (w & LOW57) | ((uint64_t)(cls ? BARKER1 : BARKER0) << 57);
	const uint64_t low = w & LOW57;
	const uint32_t hi = (uint32_t)(low >> 32);                                 // window bits 32 .. 56; a table index as a byte offset
	const uint32_t s_lo = (uint32_t)low ^ lds_ld(syn3_off + (hi & 0x3fcu)) ^ lds_ld(syn3_off + 1024u + ((hi >> 8) & 0x3fcu))
			      ^ lds_ld(syn3_off + 2048u + ((hi >> 16) & 0x1fcu)) ^ (cls ? a.t.kdiff : 0u);
	const uint32_t l0 = (uint32_t)low, l1 = (uint32_t)(low >> 32);
	const uint32_t f0 = (l0 & (uint32_t)a.t.hi_mask[0]) ^ (l1 & (uint32_t)(a.t.hi_mask[0] >> 32));
	const uint32_t f1 = (l0 & (uint32_t)a.t.hi_mask[1]) ^ (l1 & (uint32_t)(a.t.hi_mask[1] >> 32));
	const uint32_t s_hi = ((uint32_t)(a.t.kclass[cls] >> 32) ^ (__popc(f0) & 1) ^ ((__popc(f1) & 1) << 1)) & 3;
	return ((uint64_t)s_hi << 32) | s_lo;
}
__device__ __forceinline__ uint64_t hslot_of(const ScanTables &t, uint64_t syn)
{
	return ((((uint32_t)syn ^ (uint32_t)(syn >> 32)) * 0x9E3779B1u) >> (32 - __popcll(t.hmask))) & t.hmask;
}
__device__ __forceinline__ bool hslot_matches(uint64_t slot, uint64_t syn)
{
	return (slot & 0x3ffffffffULL) == syn;
}
__device__ __forceinline__ uint32_t slot_errors2(uint64_t slot, uint64_t &sw)
{
	// a stored pattern has a first position (0 .. 57) and a second one or 63; bit 63 of the window is a barker bit
	// that the LAP does not read, so "no second error" needs no select, only the count does
	const uint32_t p0 = (uint32_t)(slot >> 34) & 63, p1 = (uint32_t)(slot >> 40) & 63;
	sw ^= (1ULL << p0) | (1ULL << p1);
	return p1 != 63 ? 2u : 1u;
}
__device__ __forceinline__ uint32_t lap_of(uint64_t sw)
{
	return (uint32_t)(sw >> 34) & 0xffffff;
}
template <bool LDS_TABLES = true, bool TWO = false>
__device__ __forceinline__ bool verify_lap_any(const ScanArgs &a, uint64_t w, uint32_t &lap, uint32_t &nerr_out, uint32_t syn3_off = 0)
{
	if constexpr (TWO) {
		uint64_t sw;
		const uint64_t syn = lap_syndrome2(a, w, sw, syn3_off);
		uint32_t nerr = 0;
		if (syn) {
			uint64_t h = hslot_of(a.t, syn);
			for (;;) {
				const uint64_t slot = a.t.hslots[h];
				if (slot == HSLOT_EMPTY)
					return false;                         // no pattern -> ac_errors = 0xff -> reject
				if (hslot_matches(slot, syn)) {
					nerr = slot_errors2(slot, sw);
					break;
				}
				h = (h + 1) & a.t.hmask;
			}
		}
		lap = lap_of(sw);
		nerr_out = nerr;
		return (int)nerr <= a.max_err;
	} else {
		uint32_t win = (uint32_t)(w >> 57);
		uint32_t cls = __popc(win ^ BARKER1) <= 1 ? 1u : 0u;
		uint64_t sw = (w & LOW57) | ((uint64_t)(cls ? BARKER1 : BARKER0) << 57);
		// syndrome of (sw ^ pn): linear in the low 57 window bits plus a class constant.  The low 32
		// bits come from the LDS tables exactly as in the probe; bits 32 and 33 are two parities.  (The
		// byte tables in global memory cost eight divergent loads per candidate, which is what bounded
		// the scan for tables built for three or more errors.)
		const uint64_t low = w & LOW57;
		const uint32_t ia = (uint32_t)(low >> TABA_FIRST) & ((1u << TABA_BITS) - 1), ib = (uint32_t)(low >> (TABA_FIRST + TABA_BITS));
		const uint32_t s_lo = (uint32_t)low ^ (LDS_TABLES ? lds_ld(LDS_OFF_TABA + (ia << 2)) : a.t.tabA[ia])
				      ^ (LDS_TABLES ? lds_ld(LDS_OFF_TABB + (ib << 2)) : a.t.tabB[ib]) ^ (cls ? a.t.kdiff : 0u);
		const uint32_t s_hi = ((uint32_t)(a.t.kclass[cls] >> 32) ^ (__popcll(low & a.t.hi_mask[0]) & 1)
				       ^ ((__popcll(low & a.t.hi_mask[1]) & 1) << 1)) & 3;
		const uint64_t syn = ((uint64_t)s_hi << 32) | s_lo;
		if (a.t.bitmap2) {
			const uint32_t i2 = (s_lo * 0x9E3779B1u) >> a.t.bitmap2_shift;
			if (!((a.t.bitmap2[i2 >> 5] >> (i2 & 31)) & 1))
				return false;
		}
		uint32_t nerr = 0;
		if (syn) {
			uint64_t h = ((((uint32_t)syn ^ (uint32_t)(syn >> 32)) * 0x9E3779B1u) >> (32 - __popcll(a.t.hmask))) & a.t.hmask;
			for (;;) {
				uint64_t slot = a.t.hslots[h];
				if (slot == HSLOT_EMPTY)
					return false;                         // no pattern -> ac_errors = 0xff -> reject
				if ((slot & 0x3ffffffffULL) == syn) {
					uint64_t err = 0;
#pragma unroll
					for (int i = 0; i < 5; i++) {
						uint32_t pos = (uint32_t)(slot >> (34 + 6 * i)) & 63;
						if (pos != 63)
							err |= 1ULL << pos;
					}
					sw ^= err;
					nerr = __popcll(err);
					break;
				}
				h = (h + 1) & a.t.hmask;
			}
		}
		lap = (uint32_t)(sw >> 34) & 0xffffff;
		nerr_out = nerr;
		return (int)nerr <= a.max_err;
	}
}

// ---- LAP_ANY ----------------------------------------------------------------------------

// Barker pre-filter for the 32 offsets whose 7-bit window (LAP MSB + 6 barker bits,
// bluetooth_packet.c:378-385) lives in dh:dm: bit k of the window at offset p is bit
// (p + 25 + k) of dh:dm.  Counts mismatches against BARKER1 = 0b0100111 with a carry-save
// adder of v_bitop3 full adders (inverted planes folded into the truth tables):
//   count in {0,1} -> BARKER_DISTANCE <= 1, corrected to BARKER1 (class 1)
//   count in {6,7} -> BARKER_DISTANCE <= 1, corrected to BARKER0 (class 0)
__device__ __forceinline__ void barker32(uint32_t dm, uint32_t dh, uint32_t valid, uint32_t &pass, uint32_t &cls)
{
	const uint32_t s0 = alignbit(dh, dm, 25), s1 = alignbit(dh, dm, 26), s2 = alignbit(dh, dm, 27);
	const uint32_t s3 = alignbit(dh, dm, 28), s4 = alignbit(dh, dm, 29), s5 = alignbit(dh, dm, 30);
	const uint32_t s6 = alignbit(dh, dm, 31);
	// mismatch planes: m0 = ~s0, m1 = ~s1, m2 = ~s2, m3 = s3, m4 = s4, m5 = ~s5, m6 = s6
	const uint32_t a = BITOP3(s0, s1, s2, 0x69);       // m0 ^ m1 ^ m2
	const uint32_t ca = BITOP3(s0, s1, s2, 0x17);      // maj(m0, m1, m2)
	const uint32_t b = BITOP3(s3, s4, s5, 0x69);       // m3 ^ m4 ^ m5
	const uint32_t cb = BITOP3(s3, s4, s5, 0xd4);      // maj(s3, s4, ~s5)
	const uint32_t cc = BITOP3(a, b, s6, 0xe8);        // carry of the ones column
	// count = ones + 2 (ca + cb + cc): it is 0 or 1 iff the three carries are all clear, 6 or 7 iff they are all set -- one
	// "all three equal" instead of the twos and fours planes and their comparison (third session of round 6: seven instead of
	// eight three-input instructions per 32 offsets)
	pass = BITOP3(ca, cb, cc, 0x81) & valid;
	cls = BITOP3(ca, cb, cc, 0x01);                    // all clear: count in {0, 1}
}

// (scan_lap_any_kernel, tables for five errors)  One survivor costs about 17 VALU + 2 DS instructions:
//   syndrome_low32 = w[31:0] ^ tabA[w[44:34]] ^ tabB[w[56:45]] ^ (class ? kdiff : 0)
// for the window w at offset p of the dword triple (e0,e1,e2), then a probe of the second-level
// bitmap in L2 with a hash of it.  The stages are separate functions so that the survivor loop
// can issue the LDS reads of its two chains back to back, each under the exec mask of the
// lanes that really have a survivor: the DS pipe (shared by the 16 waves of the CU) then
// only pays bank conflicts for useful lanes.
// Instruction choice follows tools/valu_rate.hip: two-operand logic/shift ops and v_bitop3
// issue at full rate on gfx950, v_bfe/v_alignbit/v_lshl_add/v_and_or at half rate.
struct Probe { uint32_t x, offA, offB; };

__device__ __forceinline__ Probe probe_addr(uint32_t e0, uint32_t e1, uint32_t e2, uint32_t cls,
					    uint32_t kdiff, uint32_t p)
{
	Probe r;
	const uint32_t wlo = alignbit(e1, e0, p);
	const uint32_t whi = alignbit(e2, e1, p);
	// whi = window bits 32..63: bits 34..44 sit at 2..12 -- already the byte offset of a u32 entry
	r.offA = whi & (((1u << TABA_BITS) - 1) << 2);
	r.offB = (whi >> (TABA_FIRST - 32 + TABA_BITS - 2)) & (((1u << TABB_BITS) - 1) << 2);
	const uint32_t cmask = (uint32_t)__builtin_amdgcn_sbfe(cls, p, 1);     // 0 or ~0
	r.x = BITOP3(cmask, kdiff, wlo, 0x6a);                                 // wlo ^ (cmask & kdiff)
	return r;
}

// Wave priorities (s_setprio) by phase of a trip.  The four waves of a SIMD otherwise run in step -- all in the
// VALU-dense pre-filter, then all waiting on LDS round trips in the survivor loop -- and compete for the same unit.
// With the pre-filter lowest, the loop above it and the candidate handling (the longest latencies: LDS batches,
// global probes, hit stores) highest, a wave in a latency-bound phase issues as soon as it can and the pre-filter of
// the others fills the gaps: 4.55 -> 4.18 ms.  Measured (filter / loop / candidates): 0/2/3 and 0/1/3 4.17-4.18,
// 1/2/3 4.20, 3/1/0 4.23, 2/0/3 4.24, 1/0/1 and 0/3/3 4.29, 1/0/0 4.42; a fixed priority per wave (no phases): 4.54-4.58.
#ifndef PRIO_FILTER
#define PRIO_FILTER 0
#define PRIO_LOOP 2
#define PRIO_CAND 3
#endif
struct SlideTapList { int n; int k[32]; };
template <uint64_t TAPS>
constexpr SlideTapList slide_tap_list()
{
	SlideTapList l = {0, {0}};
	for (int k = 0; k < 64; k++)
		if ((TAPS >> k) & 1)
			l.k[l.n++] = k;
	return l;
}
// 32 positions of the sliding check stream (slide.h): bit b = parity of the stream bits b + k over the taps k,
// stream bit i = bit i of e2:e1:e0.  Taps and shifts are compile-time constants (a funnel shift by a
// run-time amount costs more, see 3.2 of NOTEBOOK.md).
template <uint64_t TAPS>
__device__ __forceinline__ uint32_t slide32(uint32_t e0, uint32_t e1, uint32_t e2)
{
	constexpr SlideTapList taps = slide_tap_list<TAPS>();
	uint32_t plane[32];
#pragma unroll
	for (int i = 0; i < taps.n; i++) {
		const int k = taps.k[i];
		if (k == 0)
			plane[i] = e0;
		else if (k < 32)
			plane[i] = alignbit(e1, e0, k);
		else if (k == 32)
			plane[i] = e1;
		else
			plane[i] = alignbit(e2, e1, k - 32);
	}
	uint32_t acc = plane[0];
#pragma unroll
	for (int i = 1; i + 1 < taps.n; i += 2)
		acc = xor3(acc, plane[i], plane[i + 1]);
	if ((taps.n & 1) == 0)
		acc ^= plane[taps.n - 1];
	return acc;
}

// ---- what scan_lap_any_kernel and scan_slide_kernel share ----------------------------------
//
// Three pieces of text both kernels had word for word.  They are MACROS that expand to the former statements and closures,
// because every other form changed tuned code: as functions or a struct (by value, by reference, results in a struct) they
// gave scan_slide_kernel other operand orders and register numbers and four of its forms six more instructions, and
// scan_lap_any_kernel up to a quarter more instructions (profiles/r09_scan has the table).  The expansions use the kernels'
// own names: a, lane, wave, first_tile, tile_step.

// Tile order.  The dispatcher is observed to place workgroup b on XCD b % 8 (not a contract: a
// different placement costs L2 sharing, never correctness).  Each XCD gets one contiguous
// eighth of the tiles and its 32 workgroups walk it interleaved, so that the halo word of a
// tile -- the first word of the next tile -- is found in the L2 the neighbour workgroup just
// filled instead of being fetched from HBM a second time by another XCD.
// Declares first_tile, tile_step, n_mine: this workgroup's tiles are first_tile + k * tile_step, k < n_mine.
#define TILE_ORDER(a, first_tile, tile_step, n_mine) \
	uint32_t first_tile = blockIdx.x, tile_step = gridDim.x, n_mine; \
	if (a.xcd_tiles) { \
		const uint32_t xcd = blockIdx.x & 7, lo_t = xcd * a.xcd_tiles; \
		const uint32_t hi_t = min((uint64_t)lo_t + a.xcd_tiles, a.n_tiles); \
		tile_step = gridDim.x >> 3; \
		first_tile = lo_t + (blockIdx.x >> 3); \
		n_mine = first_tile < hi_t ? (hi_t - first_tile + tile_step - 1) / tile_step : 0; \
	} else { \
		n_mine = first_tile < a.n_tiles ? (uint32_t)((a.n_tiles - first_tile + tile_step - 1) / tile_step) : 0; \
	}

// Candidate code = (tile iteration << 12) | (lane that owns the word << 6) | offset in the word, for a wave that owns
// WAVE_WORDS_ consecutive words of a tile of TILE_WORDS_.  Declares code_word(code, stream): the word's number inside its
// stream; NOTE_TILE_ is a statement that sees t, the tile's number inside its stream.
// `it` -> tile.  The launcher keeps tile numbers below 2^32 (iterations < 2^20, grid <= CUs),
// so this is one 32-bit division and only for multi-stream launches -- the 64-bit div + mod
// that used to sit here cost about 2000 cycles per batch of 64 candidates.
#define CODE_WORD_CLOSURE(TILE_WORDS_, WAVE_WORDS_, NOTE_TILE_) \
	auto code_word = [&](uint32_t code, uint32_t &stream) { \
		const uint32_t tile = first_tile + (code >> 12) * tile_step; \
		uint32_t t = tile; \
		stream = 0; \
		if (a.n_streams > 1) { \
			stream = tile / (uint32_t)a.tiles_per_stream; \
			t = tile - stream * (uint32_t)a.tiles_per_stream; \
		} \
		NOTE_TILE_; \
		return (uint64_t)t * TILE_WORDS_ + wave * WAVE_WORDS_ + ((code >> 6) & 63); \
	}

// Hits of a verified batch are not written one batch at a time: a single counter word in
// global memory takes ~140 M atomics/s, which capped the scan as soon as batches became
// frequent (tables for >= 3 errors: 750 k batches per GiB).  Each wave keeps up to 64 pending
// hit records in registers (one per lane), appends new ones with ds_permute (a lane-to-lane
// push through the LDS crossbar, no LDS memory), and reserves + writes 64 at a time.
// Declares pend (wave-uniform) and, for lane k < pend, h_off = offset low, h_hi = offset high | stream << 16, h_lap =
// lap << 8 | errors; flush_hits() and push_hits(hit, stream, offset, lap, nerr).  First-match mode (a.first): atomicMin,
// hits go out one by one.  In push_hits, lanes without a hit push to a lane outside [pend, pend + c), whose result is ignored.
#define HIT_QUEUE_CLOSURES() \
	uint32_t pend = 0; \
	uint32_t h_off = 0, h_hi = 0, h_lap = 0; \
	auto flush_hits = [&]() { \
		if (pend == 0) \
			return; \
		uint32_t base = 0; \
		if (lane == 0) \
			base = atomicAdd(a.hit_count, pend); \
		base = __builtin_amdgcn_readfirstlane(base); \
		const uint32_t idx = base + lane; \
		if (lane < pend && idx < a.hit_cap) { \
			uint4 rec; \
			rec.x = h_off; \
			rec.y = h_hi & 0xffff; \
			rec.z = h_lap >> 8; \
			rec.w = (h_lap & 0xff) | (h_hi & 0xffff0000u); \
			reinterpret_cast<uint4 *>(a.hits)[idx] = rec; \
			count_bucket(a, h_hi >> 16, ((uint64_t)(h_hi & 0xffff) << 32) | h_off); \
		} \
		pend = 0; \
	}; \
	auto push_hits = [&](bool hit, uint32_t stream, uint64_t offset, uint32_t lap, uint32_t nerr) { \
		if (a.first) { \
			if (hit) \
				emit_hit(a, stream, offset, lap, nerr); \
			return; \
		} \
		const uint64_t m = __ballot(hit); \
		if (!m) \
			return; \
		const uint32_t c = (uint32_t)__popcll(m); \
		if (pend + c > 64) \
			flush_hits(); \
		const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0)); \
		const int dst = (int)((hit ? pend + rank : (pend ? 0u : c)) << 2); \
		const uint32_t r_off = (uint32_t)__builtin_amdgcn_ds_permute(dst, (int)(uint32_t)offset); \
		const uint32_t r_hi = (uint32_t)__builtin_amdgcn_ds_permute(dst, (int)((uint32_t)(offset >> 32) | (stream << 16))); \
		const uint32_t r_lap = (uint32_t)__builtin_amdgcn_ds_permute(dst, (int)((lap << 8) | nerr)); \
		if (lane - pend < c) { \
			h_off = r_off; \
			h_hi = r_hi; \
			h_lap = r_lap; \
		} \
		pend += c; \
	}
