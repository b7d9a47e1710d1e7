// scan_slide.h -- scan_slide_kernel, the headline kernel (LAP_ANY with tables for <= 4 errors), its tuning constants and its two
// cuts.  A piece of scan.hip.
#pragma once
#include <type_traits>
#include "scan_core.h"

// ---- LAP_ANY, sliding checks (tables for <= 4 errors; two cuts of one kernel: SlideStd / Slide4 below) ----
//
// The kernel of the headline path (promiscuous_packet_search, bluetooth_packet.c:368-420).  Per trip of
// TILES tiles: the bit-sliced barker filter (barker32) and the check stream (slide32, slide.h) for both
// halves of the lane's words, then the lock-step survivor loop -- eight vector instructions and ONE read of the
// 2^SLIDE_BITS-bit candidate set in LDS per survivor (chains as shift registers, round 5).  A candidate goes straight to
// the wave's ring in LDS (the membership compare's lane mask + mbcnt, no atomics; the one-level form notes it in a register and appends a trip's notes at once, round 7); the exact reference rule (verify_lap_any, syndrome tables read
// through L2; the one-level form's syndrome tables in LDS, round 8; its pattern look-up sent at a trip's end and read in the next trip, round 9) runs on ring batches of up to 64.  The ring and those 2.5 KiB are the only LDS besides the set, so TWO workgroups
// fit a CU: 2 x 768 threads = 6 waves per SIMD at <= 80 VGPRs (78.5 KiB of LDS each; a wave owns 63 words of a tile of 756).  Measured on one box,
// 4 GiB, ms per launch (profiles/r03_ab/): one 1024-thread workgroup per CU (4 waves per SIMD) 4.12, 2 x 1024
// (8 waves, 64 VGPRs, spills outside the loop) 3.82-3.90, 2 x 768 3.59, 2 x 896 / 832 / 704 / 640 (waves that do
// not divide evenly over the four SIMDs) 4.4-5.6; the 2^20-bit set (128 KiB, one workgroup per CU only) 3.81.
// Candidates ranked beyond the ring's free entries are checked in place, never dropped (a stream made of sync
// words: tests/test_gpu_scan.py adversarial cases).
// Geometry and tuning (every A/B behind these values is in profiles/: r03_ab, r05_scan).
#define SLIDE_TILES 2                      // tiles a wave works on per trip (2 * SLIDE_TILES chains per lane); 1: +15 %, 3 (80 VGPRs): +1 %
#define SLIDE4_TILES 3                     // ... of the two-level form (tables for three and four errors; 2: +2.5 %, 4: +20 %)
#define SLIDE_WGS 2                        // workgroups per CU the kernel is cut for
#define SLIDE_THREADS 768                  // workgroup size = words per tile (a multiple of 256: whole waves per SIMD); 2 x 1024: +2.5 % (round 5, spills); round 6,
                                           // the ordered form at 64 registers without a spill: 3.24 against 3.01 ms -- eight waves per SIMD are SLOWER (profiles/r06_order)
#define SLIDE_FIXED 6                      // passes run before the first "anything left?" test of a trip (5: +2 %, 7: +1 %)
#define SLIDE_DRAIN_AT 60u                 // 64-entry ring: entries at which a trip end drains it (32 / 48 / 56 / 60: 3.56 / 3.48 / 3.46 / 3.455 ms; round 6 on
                                           // the 63-word kernel: 32 +1.5 %, 40 and 48 nothing -- profiles/r06_scan/ab_b3_drain_threshold.txt)
#define SLIDE_DRAIN_AT_ORD 40u             // ... of the ordered form (see its drain)
// The split drain (round 9, profiles/r16_split_drain).  Five rotations of seven builds on one box, ms per launch, parent 2.6152 (its runs 0.5 % apart):
#ifndef SLIDE_SPLIT_AT
#define SLIDE_SPLIT_AT 0                   // where the trip BEHIND a drain_issue finishes the batch: 0 = at its head, in front of the filter; 1 = between filter
#endif                                     // and passes; 2 = at its end, in front of its append.  One slot sent: 2.6026 / 2.6016 / 2.6090; two: 2.5890 / 2.6053 / 2.6055
#ifndef SLIDE_SPLIT_SLOTS
#define SLIDE_SPLIT_SLOTS 2                // slots a drain_issue sends per lane: h alone, or h and h + 1 in one 16-byte load (see the figures above)
#endif
// Round 6 measured three more forms of this kernel and dropped them (profiles/r06_scan; the source with the switches is kept there as text):
//   * the fixed passes without compare, scalar OR and branch -- the sign of (set word << index) shifted into a hit register per chain, one look
//     at the registers behind the last pass, the candidate's record carrying its survivor's ordinal for the drain to turn into an offset:
//     bit-exact, 17 % fewer scalar instructions, 5.4 % MORE vector instructions, +10 % time (3.21 against 2.92 ms; fully unrolled 3.03).  The
//     launch follows its vector instruction count; scalar instructions and branches are not what it waits for.
//   * a drain's hits written straight behind one counter atomic each (no pending records in registers: 66 VGPRs): 4.10 ms -- 322 k
//     returning atomics on one address serialise (SQ_WAIT_ANY 2.7 x).
//   * two chains per word walking towards each other (6.09 passes instead of 6.99): not built -- tools/lockstep_model.py prices it at +34 % per
//     chain and pass (64-bit survivor masks, 82 check bits per chain) for -13 % passes.
// Round 7 (profiles/r07_events): the one-level form's passes only NOTE a candidate -- one v_or under the chain's lane mask and two or
//   three scalar ORs -- and the trip appends its notes to the ring once, behind the sparse tail: one rank, one address, one code for
//   the wave, two ds_write2_b32 per chain under lane masks kept on the scalar side.  "No candidate events at all" (timing only) put
//   the ceiling at 7.8 % (2.538 against 2.753 ms); the change is worth 2.7 % (2.698 -> 2.626 ms; 1 540 -> 1 511 M vector and
//   842 -> 775 M scalar instructions per launch) over six alternating pairs on one box, bit-exact -- short of the 3 % in every pair
//   it was specified to reach.  Three forms were timed: what the launch paid for was the VECTOR instructions of the append, not the scalar work moved out of the priority-2 loop (13 + one
//   compare per chain seen: -1.1 %; 9 + a compare: -1.9 %; 6 and no compare: -2.8 %); four lane masks instead of two cost ten
//   v_readlane of spilled scalars per trip and were not timed.  v_add_co_u32 (m - 1 with "m was not zero" as its carry) issues at the
//   slow rate, 4.3 cycles against 2.6 for v_add_u32: the sparse tail keeps its compares.
// Round 8 (profiles/r08_drain): what is behind a trip's notes, taken apart by timing-only builds of the parent (2.629 ms, its three
//   runs 0.5 % apart): no drain at all -4.8 %; drains without the hit queue -0.55 %; no drain and an append that only moves the tail
//   another -4.2 % (it also frees the raw dwords and the notes' masks); a drain without its pattern look-up -2.5 %, without
//   its syndrome tables as well -1.3 % more.  Skipping a lane's second candidate, and the round-5 "no filter" build, both came out
//   SLOWER than the parent (+6 %, +4.5 %): they measure another register allocation, not the work left out.  Built: the exact rule in
//   a form for tables of two errors or fewer (verify_lap_any<.., TWO>: no second-level bitmap, two error positions per slot, one
//   v_bcnt per high syndrome bit) with its syndrome tables in LDS as three small ones (SYN3, 2.5 KiB in the 4 KiB two workgroups leave
//   of a CU) -- a drain is 110 vector instructions for 136, ten fewer scalar registers spilled (16 for 26) and none of the six v_readlane of spilled scalars left in a drain's
//   exact rule: 1 510.6 -> 1 498.0 M vector instructions per launch, 2.6245 -> 2.5984 ms (-1.0 %, every one of six pairs, three times the
//   parent's spread of 0.32 %; on a noisier box -1.4 % inside a spread of 1.6 %).  Not built: the second note (no ceiling could be
//   measured, the count says <= 0.8 %), the hit queue (0.55 % is its whole cost), the append ranked once per two trips (the first
//   trip's raw dwords would have to live through the second).  Probing two slots per round trip, and pattern tables of a quarter
//   to sixteen times the slots, changed nothing: the look-up's 2.5 % is one dependent round trip to the L2 per drain and the loop around it.
// Round 9 (profiles/r16_split_drain): the drain in two.  Priced first, on the parent: the probe's slot read from LDS instead of the
//   pattern table in L2 (timing only) -1.9 % (2.6270 -> 2.5762 ms, the parent's three runs 0.27 % apart) and 230 M fewer wave cycles of
//   SQ_WAIT_ANY per launch = 710 per drain: a drain waits for about two round trips to the L2, not one -- sixty lanes probe at once, two
//   thirds of them false candidates that read on until an empty slot, and at a load of 0.05 one of them meets a taken slot in nine batches of ten.
//   Built: a trip end that drains only SENDS the look-up (drain_issue) and the next trip's tile loads leave behind it; the trip behind
//   it reads the answer (drain, second half).  With one slot sent the gain was 0.4 to 0.6 % wherever the second half ran (head / behind the
//   filter / end of the trip: the second probe still waited); with slots h and h + 1 sent in one 16-byte load and the second half at
//   the trip's head -1.0 % in the rotation of all seven forms and, as the tree, 2.6151 -> 2.5762 ms (-1.5 %, every one of six pairs:
//   -1.1 to -1.9 %; the parent's six runs were 0.9 % apart in that job, so the gain is 1.6 spreads, not the three the round asked for),
//   SQ_WAIT_ANY 3 075 -> 2 862 M, wave cycles 7 763 -> 7 592 M (-2.2 %, what the LDS switch reached), vector instructions 1 497.96 ->
//   1 493.17 M (no exec mask around the syndrome and the look-up: lanes without a record send one too).  73 VGPRs for 65 (71 with one slot sent), six waves per SIMD as before.
// The kernel's two cuts.
// SlideStd: tables for <= 2 errors (0.3 % of the survivors are members of the set).  Two workgroups per CU around a 2^19-bit set; six
//   passes run blind, a candidate the ring has no room for is checked in place.
// Slide4: tables for three and four errors (slide.h), where 3 % / 32 % of the survivors are members of any set the LDS can hold.  ONE
//   workgroup per CU around a 2^20-bit set (the whole LDS: 128 KiB + 2 KiB of ring per wave); its members look a second check
//   stream up in a set in L2 before they count as candidates (LEVEL2); the pass loop watches the ring's room and is left for
//   drains (DENSE: the room test in every pass costs the sparse case 4 %, the in-place path costs a dense case a factor of three).
//   INVERT: the chains run on the complemented check stream -- an idle chain indexes 0 or 1, which are members of the set for four
//   errors while their complements are not (context.cpp stores the set accordingly).
// Measured, ms per GiB (tools/init_sweep.py, profiles/r05_init4): three errors 1.72-1.75 (SlideStd in a dense form, rounds 3-4) ->
// 1.42-1.44; four errors 2.78-2.84 (a probe kernel: three table reads per survivor, 58 % of them to L2) -> 2.09-2.13.
struct SlideStd {
	static constexpr int BITS = SLIDE_BITS, THREADS = SLIDE_THREADS, WGS = SLIDE_WGS;
	static constexpr uint64_t TAPS = SLIDE_TAPS, TAPS_B = 0;
	static constexpr bool LEVEL2 = false, INVERT = false, DENSE = false;
	static constexpr bool TWO_ERRORS = true;   // its tables hold patterns of <= 2 errors (scan.hip launches it with no others): verify_lap_any's lighter form
};
struct Slide4 {
	static constexpr int BITS = SLIDE4_BITS, THREADS = 1024, WGS = 1;
	static constexpr uint64_t TAPS = SLIDE4_TAPS, TAPS_B = SLIDE4B_TAPS;
	static constexpr bool LEVEL2 = true, INVERT = true, DENSE = true;
	static constexpr bool TWO_ERRORS = false;
};
template <class CFG> struct SlideGeom {
	static constexpr uint32_t SET_WORDS = 1u << (CFG::BITS - 5), SET_BYTES = 4u * SET_WORDS;
	static constexpr uint32_t WAVES_PER_EU = CFG::WGS * CFG::THREADS / 256;
#ifdef SCAN_PROFILE
	static constexpr uint32_t RING = 64;                                    // (the phase counters need 2 KiB of the two-level form's full LDS)
#else
	static constexpr uint32_t RING = CFG::WGS == 2 ? 64 : 128;               // ring entries per wave
#endif
	static constexpr uint32_t LANE_WORDS = 63;                              // words of a tile a wave owns (see the kernel)
	static constexpr uint32_t TILE_WORDS = CFG::THREADS / 64 * LANE_WORDS;
	static constexpr uint32_t RING_END = SET_BYTES + CAND_BYTES * (CFG::THREADS / 64) * RING;
	static constexpr uint32_t SYN3_OFF = RING_END;                          // (one-level form) the exact rule's syndrome tables, scan_core.h SYN3
	static constexpr uint32_t PROF_OFF = SYN3_OFF + (CFG::TWO_ERRORS ? SYN3_BYTES : 0u);
#ifdef SCAN_PROFILE
	static constexpr uint32_t LDS_BYTES = PROF_OFF + 128u * (CFG::THREADS / 64);     // 32 phase counters per wave
#else
	static constexpr uint32_t LDS_BYTES = PROF_OFF;
#endif
	static_assert((uint64_t)LDS_BYTES * CFG::WGS <= 160u * 1024u, "the workgroups a CU is cut for must fit its 160 KiB of LDS");
};

// MSB: the words hold their symbols MSB first in every byte (BTBBX_FMT_PACKED_MSB); a template flag, not a run-time branch: the
// branch alone cost the LSB path 1 % here and 7 % in scan_known_lap_kernel (the words' registers become merge points)
// ORD: hits leave through the segment slots (ScanArgs::seg_slots) instead of the appended list
template <class CFG, int TILES, bool MSB, bool ORD = false>
__global__ __launch_bounds__(CFG::THREADS) __attribute__((amdgpu_waves_per_eu(SlideGeom<CFG>::WAVES_PER_EU, SlideGeom<CFG>::WAVES_PER_EU)))
void scan_slide_kernel(ScanArgs a)
{
	extern __shared__ uint32_t lds[];
	if (a.gate && *a.gate == 0)
		return;
	constexpr uint32_t RING = SlideGeom<CFG>::RING;
	// ABS (third session of round 6, the one-level form): a chain is walked by ABSOLUTE positions -- p = v_ffbl of what is left of
	// its mask, index = the untouched 64-bit check register >> p, mask &= mask - 1 -- instead of the pair of shift registers
	// below.  The same instructions per survivor (v_add + v_and for v_lshrrev + v_and), but no marker to plant per chain and trip,
	// no v_ffbh per candidate event (p IS the offset) and nothing loop-carried but the mask: 2.893 -> 2.879 ms over six
	// alternating pairs (profiles/r06_shift).  The two-level form keeps the shift registers: its events run a pass behind.
	constexpr bool ABS = !CFG::LEVEL2;
	constexpr uint32_t THREADS = CFG::THREADS, SET_WORDS = SlideGeom<CFG>::SET_WORDS, SET_BYTES = SlideGeom<CFG>::SET_BYTES;

	const uint32_t tid = threadIdx.x;
	const uint32_t lane = tid & 63;
	const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform: ring addresses stay on the SALU
	// A wave owns LANE_WORDS = 63 consecutive words of a tile; its lane 63 works on the NEXT wave's first word, only so that
	// lane 62 gets the check bits behind its own word (positions 64 .. 95) from a neighbour like every other lane.  (With 64
	// words per wave those eighteen bits of lane 63 came from the scalar unit: two readlanes and 22 scalar shifts / XORs per
	// tile and check stream -- 5 % of the instructions a wave issues per trip, for one lane; a lane in 64 idles instead.)
	constexpr uint32_t LANE_WORDS = SlideGeom<CFG>::LANE_WORDS, TILE_WORDS = SlideGeom<CFG>::TILE_WORDS;
	const uint32_t wid = wave * LANE_WORDS + lane;                       // this lane's word in a tile
	uint32_t live = lane != 63 ? 0xffffffffu : 0u;                       // offsets of the lane's word that are its own
	asm volatile("" : "+v"(live));
	const uint32_t ring_off = SET_BYTES + CAND_BYTES * wave * RING;

	// tile order: one contiguous eighth of the tiles per XCD, its workgroups interleaved (scan_core.h)
	TILE_ORDER(a, first_tile, tile_step, n_mine)

	{	// candidate set -> LDS byte 0, 16 bytes per lane per step, as 16-bit entries, every entry bit-reversed: the member bit of
		// index i is bit 15 - (i & 15) of entry i >> 4, so that a LEFT shift by i brings it to the entry's sign bit -- "member" is
		// then one signed 16-bit compare, whose result (a lane mask in scalar registers) is also the ballot the candidate path
		// needs.  Sixteen bits, not thirty-two (rounds 5-6a): on gfx950 v_lshlrev_b32 issues at the slow rate (4.1 cycles per wave,
		// like v_alignbit) while v_lshlrev_b16 and the RIGHT shifts issue at the fast one (2.3-2.5; tools/valu_rate.hip,
		// profiles/r06_scan/valu_rate_shifts.txt) -- one left shift per survivor.
		const uint4 *src = reinterpret_cast<const uint4 *>(CFG::LEVEL2 ? a.t.slide4_bitmap : a.t.slide_bitmap);
		uint4 *dst = reinterpret_cast<uint4 *>(lds);
		auto rev16 = [](uint32_t x) { const uint32_t r = __brev(x); return (r >> 16) | (r << 16); };   // both halves reversed in place
		for (uint32_t i = tid; i < SET_WORDS / 4; i += THREADS) {
			const uint4 v = src[i];
			dst[i] = make_uint4(rev16(v.x), rev16(v.y), rev16(v.z), rev16(v.w));
		}
	}
	constexpr uint32_t SYN3_OFF = SlideGeom<CFG>::SYN3_OFF;
	if constexpr (CFG::TWO_ERRORS) {
		// the exact rule's syndrome tables, in the 4 KiB two workgroups of this cut leave of a CU's LDS: a drain then waits for
		// one round trip to the L2 (the pattern table), not two
		for (uint32_t i = tid; i < SYN3_WORDS; i += THREADS)
			lds_st(SYN3_OFF + 4u * i, syn3_entry(a.t, i));
	}
	__syncthreads();

#ifdef SCAN_PROFILE
	// phases: 0 = tile loads + barker filter + check stream, 1 .. 13 = survivor pass k, 16 = loop exit, 18 = ring drain,
	// 19 = hand-over to the next trip
	const uint32_t prof_off = SlideGeom<CFG>::PROF_OFF + 128u * wave;
	if (lane < 32)
		lds_st(prof_off + 4u * lane, 0u);
	uint64_t prof_t;
	asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(prof_t) : : "memory");
#endif
	uint32_t q_head = 0, q_tail = 0;          // wave-uniform ring cursors (free running)
	// code = (tile iteration << 12) | (lane that owns the word << 6) | offset in the word
	uint32_t code_tile = 0;                       // (set by code_word: the tile's number inside its stream)
	CODE_WORD_CLOSURE(TILE_WORDS, LANE_WORDS, code_tile = t);
	// hits: up to 64 pending records per wave in registers, written 1 KiB at a time behind one counter atomic (scan_core.h)
	HIT_QUEUE_CLOSURES();
	// One-level form (round 9): the drain in two.  drain_issue, at the trip end: records, windows, syndromes, and the pattern
	// look-up SENT -- every lane's, also a lane without a record (rec = 0 gives a slot inside the table like any other, and no
	// exec mask is formed); the ring is free again at once.  drain(p_n, the second half), a trip later (SLIDE_SPLIT_AT): the
	// slot's answer, the error decode, the LAP and the hits.  Carried per lane: code, the corrected window's high dword (the LAP
	// is its bits 2 .. 25), the syndrome and the slot in flight; wave-uniform: p_n, the batch's size, 0 = no batch pending (a
	// batch has an entry).  The two-level form and (placement E) the ordered form drain in one go: drain(n, whole).
	static_assert(SLIDE_SPLIT_AT >= 0 && SLIDE_SPLIT_AT <= 2, "head, behind the filter, or end of the trip");
	constexpr bool SPLIT = !CFG::DENSE && !(ORD && SLIDE_SPLIT_AT == 2);     // (E: the ordered form's ranking borrows the ring, which the passes have written to by then)
	static_assert(!SPLIT || CFG::TWO_ERRORS, "the split drain has no test of a second-level bitmap");
	uint32_t p_n = 0;
	uint32_t p_code = 0, p_swhi = 0, p_synlo = 0, p_synhi = 0;
	uint64_t p_slot = 0, p_slot2 = 0;
	auto drain_issue = [&](uint32_t n) {
		u32x4 rec = {0u, 0u, 0u, 0u};
		if (lane < n)
			rec = lds_ld4(ring_off + CAND_BYTES * ((q_head + lane) & (RING - 1)));
		p_code = rec.x;
		const uint64_t w = ((uint64_t)alignbit(rec.w, rec.z, p_code) << 32) | alignbit(rec.z, rec.y, p_code);   // (shift = the low five bits)
		uint64_t sw;
		const uint64_t syn = lap_syndrome2(a, w, sw, SYN3_OFF);
#if SLIDE_SPLIT_SLOTS == 2
		{	// slots h and h + 1 in one 16-byte load (the table has one slot behind its end that repeats slot 0: context.cpp)
			typedef uint64_t slot_pair_t __attribute__((ext_vector_type(2), aligned(8)));
			const slot_pair_t two = *reinterpret_cast<const slot_pair_t *>(a.t.hslots + hslot_of(a.t, syn));
			p_slot = two.x;
			p_slot2 = two.y;
		}
#else
		p_slot = a.t.hslots[hslot_of(a.t, syn)];
#endif
		p_swhi = (uint32_t)(sw >> 32);
		p_synlo = (uint32_t)syn;
		p_synhi = (uint32_t)(syn >> 32);
		p_n = n;
		q_head += n;
	};
	const std::false_type whole;
	const std::true_type second_half;
	auto drain = [&](uint32_t n, auto half) {    // the n <= 64 oldest ring entries through the exact rule, or the batch drain_issue sent through the rest of it
		constexpr bool SECOND = decltype(half)::value;
		bool hit = false;
		uint32_t stream = 0, lap = 0, nerr = 0;
		uint64_t offset = 0;
		u32x4 rec = {0u, 0u, 0u, 0u};
		if constexpr (SECOND)
			rec.x = p_code;
		else if (lane < n)
			rec = lds_ld4(ring_off + CAND_BYTES * ((q_head + lane) & (RING - 1)));
		const uint32_t code = rec.x;
		const uint64_t word = code_word(code, stream);
		if (lane < n) {
			if constexpr (SECOND) {
				offset = word * 64 + (code & 63);
				const uint64_t syn = ((uint64_t)p_synhi << 32) | p_synlo;
				uint64_t sw = (uint64_t)p_swhi << 32;
				bool found = true;
				if (syn) {
					uint64_t slot = p_slot;
#if SLIDE_SPLIT_SLOTS == 2
					if (slot != HSLOT_EMPTY && !hslot_matches(slot, syn))
						slot = p_slot2;
#endif
					if (slot != HSLOT_EMPTY && !hslot_matches(slot, syn)) {      // a displaced pattern (16 slots per pattern: rare): the probe goes on, waiting
						uint64_t h = hslot_of(a.t, syn) + (SLIDE_SPLIT_SLOTS - 1);
						do {
							h = (h + 1) & a.t.hmask;
							slot = a.t.hslots[h];
						} while (slot != HSLOT_EMPTY && !hslot_matches(slot, syn));
					}
					if (slot == HSLOT_EMPTY)
						found = false;                    // no pattern -> ac_errors = 0xff -> reject
					else
						nerr = slot_errors2(slot, sw);
				}
				lap = lap_of(sw);
				hit = found && (int)nerr <= a.max_err;
			} else {
				const uint64_t w = ((uint64_t)alignbit(rec.w, rec.z, code) << 32) | alignbit(rec.z, rec.y, code);   // (shift = the low five bits)
				offset = word * 64 + (code & 63);
				hit = verify_lap_any<false, CFG::TWO_ERRORS>(a, w, lap, nerr, SYN3_OFF);
			}
		}
		if constexpr (ORD) {
			// A drain takes whole trips, so every hit of a segment (tile iteration code >> 12 of this wave) is in this batch: its
			// rank = the hits of the same tile with a smaller code (lane, offset) -- one scalar trip per hit of the batch --, its
			// place = slot `rank` of the segment.  The hit with the highest rank stores the segment's count.
			const uint64_t hm = __ballot(hit);
			if (hm) {
				uint32_t rank = 0, count = 0;
				// The ring is empty now (its records sit in registers) and lends its kilobyte: a hit counter per tile iteration of the
				// batch -- ring entries are in trip order, so the iterations run from the oldest entry's (even) one to the newest's -- and
				// room for four 12-bit codes per tile.  A hit's count = its tile's counter, its rank = the codes of its tile below its own.
				// (One scalar trip per hit of the batch over all lanes instead -- 300 instructions per drain -- cost the launch 8 %.)
				// A batch that spans 64 iterations or more (a sparse stream: few hits) or a tile with more than four hits: that loop.
				const uint32_t it_mine = code >> 12;
				const uint32_t it_lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)it_mine) & ~1u;
				const uint32_t it_hi = (uint32_t)__builtin_amdgcn_readlane((int)it_mine, (int)(n - 1)) | 1u;
				bool fast = it_hi - it_lo < 64u;
				if (fast) {
					const uint32_t key = (it_mine - it_lo) & 63u;
					lds_st(ring_off + 4u * lane, 0u);
					uint32_t idx = 0;
					if (hit) {
						idx = __hip_atomic_fetch_add(reinterpret_cast<lds_u32_t *>(ring_off + 4u * key), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
						if (idx < 4u)
							*reinterpret_cast<__attribute__((address_space(3))) uint16_t *>(ring_off + 256u + 8u * key + 2u * idx) = (uint16_t)(code & 0xfffu);
					}
					asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
					if (hit)
						count = lds_ld(ring_off + 4u * key);
					if (__ballot(count > 4u)) {
						fast = false;
					} else if (hit) {
						const uint32_t lo2 = lds_ld(ring_off + 256u + 8u * key), hi2 = lds_ld(ring_off + 260u + 8u * key);
						const uint32_t mine = code & 0xfffu;
						rank = ((lo2 & 0xffffu) < mine ? 1u : 0u);                      // (entry 0 always exists; the own entry is not below itself)
						rank += count > 1u && (lo2 >> 16) < mine ? 1u : 0u;
						rank += count > 2u && (hi2 & 0xffffu) < mine ? 1u : 0u;
						rank += count > 3u && (hi2 >> 16) < mine ? 1u : 0u;
					}
				}
				if (!fast) {
					rank = count = 0;
					for (uint64_t r = hm; r; r &= r - 1) {
						const uint32_t cj = (uint32_t)__builtin_amdgcn_readlane((int)code, (int)__builtin_ctzll(r));
						const bool same = (code ^ cj) < 4096u;
						count += same ? 1u : 0u;
						rank += same && cj < code ? 1u : 0u;
					}
				}
				const uint32_t seg = stream * a.segs_per_stream + code_tile * (THREADS / 64) + wave;
				uint4 out;
				out.x = (uint32_t)offset;
				out.y = (uint32_t)(offset >> 32);
				out.z = lap;
				out.w = nerr | (stream << 16);
				const bool spill = hit && rank >= a.seg_slot_n;
				if (hit && !spill)       // (code & 0xfff = lane << 6 | offset in the word = the offset inside the wave's 63 words)
					a.seg_slots[(uint64_t)seg * a.seg_slot_n + rank] = (uint64_t)(code & 0xfffu) | ((uint64_t)lap << 12) | ((uint64_t)nerr << 36);
				if (hit && rank + 1 == count)
					a.seg_cnt[seg] = (uint16_t)count;            // (<= 4032 offsets per segment)
				const uint64_t om = __ballot(spill);
				if (om) {                                            // more hits in 4032 offsets than a segment has slots: rare
					uint32_t base = 0;
					if (lane == 0)
						base = atomicAdd(a.ovf_count, (uint32_t)__popcll(om));
					base = __builtin_amdgcn_readfirstlane(base);
					const uint32_t idx = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(om >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)om, 0));
					if (spill) {
						if (idx < a.ovf_cap) {
							reinterpret_cast<uint4 *>(a.ovf_recs)[idx] = out;
							a.ovf_meta[idx] = make_uint2(seg, rank);
						} else {
							*a.irregular = 1u;
						}
					}
				}
			}
		} else {
			push_hits(hit, stream, offset, lap, nerr);
		}
		if constexpr (SECOND)
			p_n = 0;
		else
			q_head += n;
	};

	// The tile cursor carries its tile's address along (one 64-bit scalar add per tile; the products stream x pitch and tile x
	// words are formed again only when it crosses into the next stream), and a lane's word is that address + a byte offset
	// it computes once: `global_load ... v_off, s[base]` -- no 64-bit vector address arithmetic per load (round 5: the scalar
	// unit's instructions are not free, they take about two issue cycles each from the same wave).
	struct Cursor { uint32_t stream; uint32_t t; const uint64_t *tp; };
	const uint32_t tiles_per_stream = (uint32_t)a.tiles_per_stream;
	Cursor cur = {a.n_streams, 0, a.words};      // stream == n_streams: nothing (left) to do
	uint32_t handed = 0;
	auto tile_address = [&](const Cursor &c) { return a.words + (uint64_t)c.stream * a.pitch_words + (uint64_t)c.t * TILE_WORDS; };
	if (n_mine) {
		cur.stream = a.n_streams > 1 ? first_tile / tiles_per_stream : 0;
		cur.t = first_tile - cur.stream * tiles_per_stream;
		cur.tp = tile_address(cur);
	}
	// (the product is formed again at every tile -- two scalar multiplies: hoisted, it lived in a spilled SGPR pair and came back
	// through two v_readlane per tile, vector instructions on the path of every trip)
	auto step_words = [&]() {
		uint32_t ts = tile_step;
		asm volatile("" : "+s"(ts));
		return (uint64_t)ts * TILE_WORDS;
	};
	auto advance = [&](Cursor &c) {
		if (++handed >= n_mine) {
			c.stream = a.n_streams;
			return;
		}
		c.t += tile_step;
		c.tp += step_words();
		if (c.t >= tiles_per_stream) {
			while (c.t >= tiles_per_stream && c.stream < a.n_streams) {
				c.t -= tiles_per_stream;
				c.stream++;
			}
			c.tp = tile_address(c);
		}
	};
	auto tile_full = [&](uint32_t tt) { return tt < a.full_tiles; };
	uint32_t voff = wid * 8u;                                            // this lane's word in a tile, in bytes
	asm volatile("" : "+v"(voff));
	// A lane's two words (its own and the one behind it) come through a BUFFER descriptor over the tile: base = the cursor's tile
	// address, extent = the words of the stream that are left there, so the hardware's range check returns zero for a word
	// behind the stream's end (checked per dword) -- one 16-byte load from a 32-bit lane offset, no 64-bit vector address, no
	// zero-initialised destination, no exec mask for the ragged tile.  (Third session of round 6: the global loads cost seven
	// vector instructions per tile -- four v_mov, a v_mov_b64, a v_lshl_add_u64 -- on the path of every full tile.)
	auto load_pair = [&](const Cursor &c, uint64_t &lo, uint64_t &hi) {
		uint32_t bytes = 0;                                                  // wave-uniform
		if (c.stream < a.n_streams) {
			bytes = (TILE_WORDS + 2u) * 8u;                                  // (a full tile: its words and two behind it are in range)
			if (!tile_full(c.t)) {
				const uint64_t first = (uint64_t)c.t * TILE_WORDS;
				const uint64_t left = first < a.n_words ? a.n_words - first : 0;
				bytes = (uint32_t)(left < TILE_WORDS + 2u ? left : TILE_WORDS + 2u) * 8u;
			}
		}
		const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t *>(c.tp), 0, (int)bytes, 0x00020000);
		const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)voff, 0, 0);
		lo = ((uint64_t)v.y << 32) | v.x;
		hi = ((uint64_t)v.w << 32) | v.z;
	};

	Cursor tc[TILES];
	uint64_t lo[TILES], hi[TILES];
#pragma unroll
	for (int u = 0; u < TILES; u++) {
		tc[u] = cur;
		load_pair(cur, lo[u], hi[u]);
		advance(cur);
	}

	for (uint32_t it = 0; tc[0].stream < a.n_streams; it += TILES) {
		if constexpr (SPLIT && SLIDE_SPLIT_AT == 0) {
			if (p_n)
				drain(p_n, second_half);                      // (still at PRIO_CAND from the trip end)
		}
		__builtin_amdgcn_s_setprio(PRIO_FILTER);
		uint32_t d[TILES][4], m[TILES][2], c[TILES][3];
		uint32_t c2[TILES][CFG::LEVEL2 ? 3 : 1];                 // (two-level form) the second check stream, positions as c
#pragma unroll
		for (int u = 0; u < TILES; u++) {
			d[u][0] = (uint32_t)lo[u]; d[u][1] = (uint32_t)(lo[u] >> 32);
			d[u][2] = (uint32_t)hi[u]; d[u][3] = (uint32_t)(hi[u] >> 32);
			if constexpr (MSB) {
#pragma unroll
				for (int k = 0; k < 4; k++)
					d[u][k] = msb_dword(d[u][k]);
			}
			uint32_t cls_unused;
			barker32(d[u][1], d[u][2], live, m[u][0], cls_unused);      // offsets 0..31: window bits 57.. in d1:d2
			barker32(d[u][2], d[u][3], live, m[u][1], cls_unused);      // offsets 32..63
			// offsets beyond the search length (the last tile of a stream only): cut out of the masks BEHIND the filter -- as two
			// validity masks in front of it they were two register copies per tile on the path of every full tile
			if (tc[u].stream >= a.n_streams) {
				m[u][0] = m[u][1] = 0;
			} else if (!tile_full(tc[u].t)) {
				const uint64_t first_off = ((uint64_t)tc[u].t * TILE_WORDS + wid) * 64;
				const uint64_t valid = first_off >= a.search_bits ? 0ULL
					: (a.search_bits - first_off >= 64 ? FULL_MASK : ((1ULL << (a.search_bits - first_off)) - 1));
				m[u][0] &= (uint32_t)valid;
				m[u][1] &= (uint32_t)(valid >> 32);
			}
			c[u][0] = slide32<CFG::TAPS>(d[u][0], d[u][1], d[u][2]);
			c[u][1] = slide32<CFG::TAPS>(d[u][1], d[u][2], d[u][3]);
			if constexpr (CFG::INVERT) {
				c[u][0] = ~c[u][0];
				c[u][1] = ~c[u][1];
			}
			// positions 64..95 = the first check dword of the next lane's word (lane 63 has no offsets of its own, see above)
			c[u][2] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((lane + 1) << 2), (int)c[u][0]);
			if constexpr (CFG::LEVEL2) {
				c2[u][0] = slide32<CFG::TAPS_B>(d[u][0], d[u][1], d[u][2]);
				c2[u][1] = slide32<CFG::TAPS_B>(d[u][1], d[u][2], d[u][3]);
				c2[u][2] = (uint32_t)__builtin_amdgcn_ds_bpermute((int)((lane + 1) << 2), (int)c2[u][0]);
			}
		}

		// A chain (32 offsets) as a pair of shift registers: its survivor mask and the 50 check bits its indices are cut from,
		// both moved down to the survivor in hand (one v_lshrrev_b64 instead of a funnel shift per survivor, no "m - 1").  Bit
		// 63 is a marker: its distance from the top is the offset the chain stands at, which only a candidate event asks for.
		uint64_t C[TILES][2];
#pragma unroll
		for (int u = 0; u < TILES; u++)
#pragma unroll
			for (int h = 0; h < 2; h++)
				C[u][h] = ((uint64_t)(ABS ? c[u][h + 1] : (c[u][h + 1] | 0x80000000u)) << 32) | c[u][h];
		struct Stage { uint32_t v[TILES][2], bw[TILES][2]; };
		auto any_left = [&]() {
			uint32_t any = 0;
#pragma unroll
			for (int u = 0; u < TILES; u++)
				any |= m[u][0] | m[u][1];
			return __ballot(any != 0) != 0;
		};
		uint32_t pos2[TILES][2];                     // (two-level form) where the chains stood when their pending look-ups were sent
		auto event_chain = [&](int u, int h, uint64_t cm) {    // append one chain's candidates of one pass (lanes cm) to the wave's ring
			const bool cand = __builtin_amdgcn_inverse_ballot_w64(cm);
			// ring entries left for this chain; candidates ranked beyond them (a stream made of
			// sync words: tests/test_gpu_scan.py adversarial cases) go through the exact rule in place
			const uint32_t room = RING - (q_tail - q_head);
			uint32_t in_wave;                       // (asm: the compiler turns `popcount == 1` into a 64-bit VECTOR compare)
			asm("s_bcnt1_i32_b64 %0, %1" : "=s"(in_wave) : "s"(cm) : "scc");
			const uint32_t n = min(in_wave, room);
			if (cand) {
				uint32_t lane6 = lane << 6;
				asm volatile("" : "+v"(lane6));         // (otherwise four loop-invariant code bases sit in VGPRs through the pass loop)
				// the marker planted above the chain's check bits has moved down by exactly the offsets passed
				uint32_t pos;
				if constexpr (ABS)
					pos = pos2[u][h];                   // (a candidate's chain was not empty: 0 .. 31)
				else if constexpr (CFG::LEVEL2)
					pos = pos2[u][h];
				else
					asm("v_ffbh_u32 %0, %1" : "=v"(pos) : "v"((uint32_t)(C[u][h] >> 32)));
				// the record carries the three stream dwords the window lies in; the drain cuts it out (for sixty
				// candidates at once) instead of this branch (for one)
				const uint32_t code = pos | lane6 | (((it + u) << 12) | (h << 5));
				const u32x4 rec = {code, d[u][h], d[u][h + 1], d[u][h + 2]};
				if (in_wave == 1 && room) {
					// one candidate in the wave (nine events in ten): its slot is the ring tail, no ranking
					lds_st_rec(ring_off + CAND_BYTES * (q_tail & (RING - 1)), rec);
				} else {
					const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(cm >> 32),
							__builtin_amdgcn_mbcnt_lo((uint32_t)cm, 0));
					if (rank < room) {
						lds_st_rec(ring_off + CAND_BYTES * ((q_tail + rank) & (RING - 1)), rec);
					} else {
						uint32_t stream, lap, nerr, cold = code;
						asm volatile("" : "+v"(cold));      // keeps the tile -> stream division of this cold path out of every trip
						const uint64_t word = code_word(cold, stream);
						const uint32_t wlo = alignbit(rec.z, rec.y, pos), whi = alignbit(rec.w, rec.z, pos);
						if (verify_lap_any<false, CFG::TWO_ERRORS>(a, ((uint64_t)whi << 32) | wlo, lap, nerr, SYN3_OFF)) {
							if constexpr (ORD)
								*a.irregular = 1u;          // a hit outside the drains: its segment cannot be ranked here
							else
								emit_hit(a, stream, word * 64 + (cold & 63), lap, nerr);
						}
					}
				}
			}
			q_tail += n;
		};
		auto events = [&](const uint64_t (&cms)[TILES][2]) {   // ... every chain's (the two-level form)
#pragma unroll
			for (int u = 0; u < TILES; u++)
#pragma unroll
				for (int h = 0; h < 2; h++)
					if (cms[u][h])
						event_chain(u, h, cms[u][h]);
		};
		// One-level form (round 7): a pass only NOTES its candidates -- one dword per lane: where the chain stood and which chain -- and
		// the trip appends them once behind the tail (append_noted): one rank, one ring address, one code, and per chain one record
		// store under that chain's lanes, instead of rank, room, address and store per chain and pass inside the priority-2 loop.
		// A lane holds one note: a chain whose candidates meet a lane that already has one goes through event_chain as before.
		static_assert(CFG::DENSE || TILES == 2, "a note's tile bit is OR-ed into the trip's (even) tile iteration");
		uint64_t noted = 0;                          // lanes that hold a note ...
		uint64_t noted_h = 0, noted_u = 0;           // ... of an upper half / of the trip's second tile (a chain's lanes on the scalar side: no compare)
		uint32_t note;
		asm volatile("" : "=v"(note));               // (no instruction: a lane's note is read only while its bit of `noted` is set)
		auto note_events = [&](const uint64_t (&cms)[TILES][2]) {
#pragma unroll
			for (int u = 0; u < TILES; u++)
#pragma unroll
				for (int h = 0; h < 2; h++) {
					const uint64_t cm = cms[u][h];
					if (!cm)
						continue;
					if (cm & noted) {
						event_chain(u, h, cm);
						continue;
					}
					// the note = the candidate's code without lane and trip: offset in the half, half (bit 5), tile of the trip (bit 12)
					// (asm: one v_or under the chain's lane mask; as C the compiler may make it a select over all lanes)
					if (__builtin_amdgcn_inverse_ballot_w64(cm))
						asm volatile("v_or_b32 %0, %1, %2" : "+v"(note) : "i"((uint32_t)(h << 5) | (uint32_t)(u << 12)), "v"(pos2[u][h]));
					noted |= cm;
					if (h)
						noted_h |= cm;
					if (u)
						noted_u |= cm;
				}
		};
		auto append_noted = [&]() {                  // the trip's notes -> ring, in one go (the order inside a trip is free: the drain ranks by code)
			if (!noted)
				return;
			const uint32_t room = RING - (q_tail - q_head);
			uint32_t in_wave;
			asm("s_bcnt1_i32_b64 %0, %1" : "=s"(in_wave) : "s"(noted) : "scc");
			const uint32_t n = min(in_wave, room);
			if (__builtin_amdgcn_inverse_ballot_w64(noted)) {
				const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(noted >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)noted, 0));
				const uint32_t code = note | (lane << 6) | (it << 12);
				const uint32_t slot = ring_off + CAND_BYTES * ((q_tail + rank) & (RING - 1));
				auto lanes_of = [&](int u, int h) {
					return (h ? noted_h : noted & ~noted_h) & (u ? noted_u : ~noted_u);
				};
				if (in_wave <= room) {
#pragma unroll
					for (int u = 0; u < TILES; u++)
#pragma unroll
						for (int h = 0; h < 2; h++) {
							const uint64_t mine = lanes_of(u, h);
							if (mine) {
								asm volatile("" : : "s"(mine));         // (a scalar branch around the chain, not one more term of its lane mask)
								if (__builtin_amdgcn_inverse_ballot_w64(mine))
									lds_st_rec2(slot, code, d[u][h], d[u][h + 1], d[u][h + 2]);
							}
						}
				} else {
					// a ring with fewer free entries than the trip has notes (a stream made of sync words): those ranked beyond them go
					// through the exact rule in place, as in event_chain
					uint32_t y = 0, z = 0, w = 0;
#pragma unroll
					for (int u = 0; u < TILES; u++)
#pragma unroll
						for (int h = 0; h < 2; h++)
							if (__builtin_amdgcn_inverse_ballot_w64(lanes_of(u, h))) {
								y = d[u][h]; z = d[u][h + 1]; w = d[u][h + 2];
							}
					if (rank < room) {
						lds_st_rec2(slot, code, y, z, w);
					} else {
						uint32_t stream, lap, nerr, cold = code;
						asm volatile("" : "+v"(cold));
						const uint64_t word = code_word(cold, stream);
						const uint32_t wlo = alignbit(z, y, cold), whi = alignbit(w, z, cold);      // (shift = the low five bits)
						if (verify_lap_any<false, CFG::TWO_ERRORS>(a, ((uint64_t)whi << 32) | wlo, lap, nerr, SYN3_OFF)) {
							if constexpr (ORD)
								*a.irregular = 1u;
							else
								emit_hit(a, stream, word * 64 + (cold & 63), lap, nerr);
						}
					}
				}
			}
			q_tail += n;
		};
		// (An empty chain shifts itself out: its index becomes 0 or 1, which no table set contains -- context.cpp asserts it --,
		// so a lane without a survivor never looks like a candidate and the test needs no "this lane has one" term.)
		auto step = [&](int u, int h, Stage &g) {       // next survivor of a chain: index, set read in flight
			const uint32_t p = lowest_bit(m[u][h]);     // ~0 for an empty chain
			if constexpr (ABS) {
				g.v[u][h] = (uint32_t)(C[u][h] >> (p & 63));      // (an empty chain: bit 63 alone = index 0 or 1)
				g.bw[u][h] = lds_ld16((g.v[u][h] >> 3) & (SET_BYTES - 2));
				m[u][h] &= m[u][h] - 1u;
				pos2[u][h] = p;
			} else {
				m[u][h] >>= p & 31;
				C[u][h] >>= p & 63;
				g.v[u][h] = (uint32_t)C[u][h];
				g.bw[u][h] = lds_ld16((g.v[u][h] >> 3) & (SET_BYTES - 2));
				m[u][h] &= ~1u;
			}
		};
		auto member = [&](int u, int h, const Stage &g) {   // lanes whose index is in the set (the compare's own mask: no ballot)
			return sign16_after_shl(g.bw[u][h], g.v[u][h]);
		};
		// Two-level form: a third of the survivors are members of the LDS set; they alone (exec mask) look their SLIDE4B_BITS
		// positions of the second check stream up in the set in L2 -- one dword each, the four chains' loads in flight together.
		// The position comes from the chain's marker, as in a candidate event.  The look-ups of a pass are sent at its end and
		// looked at in the NEXT pass, behind that pass's own steps (level2_take): the L2's answer has a pass to arrive in.
		// (No "this chain has no member in any lane" shortcut: a branch per chain makes the compiler wait for the loads at
		// every merge -- 1.9 against 1.43 ms per GiB with tables for three errors, where a third of the chain-passes could skip.)
		uint32_t v2[TILES][2], w2[TILES][2] = {};            // (w2: a lane without a look-up in flight keeps a stale word; `sent` masks its answer)
		uint64_t sent[TILES][2], any_sent = 0;               // lanes with a look-up in flight, per chain
		auto level2_send = [&](const uint64_t (&cms)[TILES][2]) {
			any_sent = 0;
#pragma unroll
			for (int u = 0; u < TILES; u++)
#pragma unroll
				for (int h = 0; h < 2; h++) {
					sent[u][h] = cms[u][h];
					any_sent |= cms[u][h];
					asm("v_ffbh_u32 %0, %1" : "=v"(pos2[u][h]) : "v"((uint32_t)(C[u][h] >> 32)));
					v2[u][h] = alignbit(c2[u][h + 1], c2[u][h], pos2[u][h]);
					if (__builtin_amdgcn_inverse_ballot_w64(cms[u][h]))
						w2[u][h] = a.t.slide4b_bitmap[(v2[u][h] >> 5) & ((1u << (SLIDE4B_BITS - 5)) - 1)];
				}
		};
		auto level2_take = [&]() {
			if (!any_sent)
				return;
			uint64_t cms[TILES][2], any = 0;
#pragma unroll
			for (int u = 0; u < TILES; u++)
#pragma unroll
				for (int h = 0; h < 2; h++) {
					cms[u][h] = sent[u][h] & __ballot((int32_t)(w2[u][h] << (v2[u][h] & 31)) < 0);
					any |= cms[u][h];
				}
			any_sent = 0;
			if (any)
				events(cms);
		};
		auto pass = [&]() {
			Stage g;
#pragma unroll
			for (int u = 0; u < TILES; u++)
#pragma unroll
				for (int h = 0; h < 2; h++)
					step(u, h, g);
			// (the compiler knows nothing about the latency of the shift and compare written as asm in member(): without this it
			// slips each set read behind the previous chain's compare and waits for the reads one at a time)
			__builtin_amdgcn_sched_barrier(0);
			uint64_t cms[TILES][2], any = 0;
#pragma unroll
			for (int u = 0; u < TILES; u++)
#pragma unroll
				for (int h = 0; h < 2; h++) {
					cms[u][h] = member(u, h, g);
					any |= cms[u][h];
				}
			if constexpr (CFG::LEVEL2) {
				level2_take();                           // the previous pass's look-ups, then this pass's are sent
				// ("any member in the wave" formed HERE and on the scalar unit by name: carried across level2_take's branches the
				// compiler re-formed it from the six lane masks with twelve VECTOR instructions per pass)
				static_assert(!CFG::LEVEL2 || TILES == 3, "the scalar OR below is written for six chains");
				uint64_t any2;
				asm("s_or_b64 %0, %1, %2\n\ts_or_b64 %0, %0, %3\n\ts_or_b64 %0, %0, %4\n\ts_or_b64 %0, %0, %5\n\ts_or_b64 %0, %0, %6"
				    : "=&s"(any2) : "s"(cms[0][0]), "s"(cms[0][1]), "s"(cms[1][0]), "s"(cms[1][1]), "s"(cms[TILES - 1][0]), "s"(cms[TILES - 1][1]) : "scc");
				if (any2)
					level2_send(cms);
			} else if (any) {                            // some lane of the wave holds a candidate (half of the passes)
				note_events(cms);
			}
		};
		// Behind the fixed passes a handful of the wave's 2 * TILES * 64 chains still hold survivors (0.8 % have seven or more):
		// a pass then looks at the chains one by one and skips those that are empty wave-wide (the same ballots are the
		// loop's exit test), instead of paying the full pass for two or three lanes.
		auto sparse_tail = [&]() {
			uint64_t live[TILES][2], anyl = 0;

#pragma unroll
			for (int u = 0; u < TILES; u++)
#pragma unroll
				for (int h = 0; h < 2; h++) {
					live[u][h] = __ballot(m[u][h] != 0);
					anyl |= live[u][h];
				}
			while (anyl) {
				Stage g;
				uint64_t cms[TILES][2], anyc = 0;
				anyl = 0;
#pragma unroll
				for (int u = 0; u < TILES; u++)
#pragma unroll
					for (int h = 0; h < 2; h++) {
						cms[u][h] = 0;
						if (!live[u][h])
							continue;
						step(u, h, g);
						cms[u][h] = member(u, h, g);
						anyc |= cms[u][h];
						live[u][h] = __ballot(m[u][h] != 0);
						anyl |= live[u][h];
					}
				if (anyc)
					note_events(cms);
			}
		};
#ifdef SCAN_PROFILE
#pragma unroll
		for (int u = 0; u < TILES; u++) {
			PROF_PIN(m[u][0]); PROF_PIN(m[u][1]); PROF_PIN(c[u][0]); PROF_PIN(c[u][1]); PROF_PIN(c[u][2]);
		}
#endif
		PROF_MARK(0);
		uint32_t pass_no = 1;
		if constexpr (!CFG::DENSE) {
			if constexpr (SPLIT && SLIDE_SPLIT_AT == 1) {
				if (p_n) {
					__builtin_amdgcn_s_setprio(PRIO_CAND);
					drain(p_n, second_half);
				}
			}
			__builtin_amdgcn_s_setprio(PRIO_LOOP);
#pragma unroll 1
			for (int k = 0; k < SLIDE_FIXED; k++) { // practically every trip needs these (TILES * 128 chains of ~4 survivors)
				pass();
				PROF_MARK(pass_no < 13 ? pass_no : 13);
				pass_no++;
			}
			sparse_tail();
			if constexpr (SPLIT && SLIDE_SPLIT_AT == 2) {
				if (p_n) {
					__builtin_amdgcn_s_setprio(PRIO_CAND);
					drain(p_n, second_half);
				}
			}
			append_noted();
			PROF_MARK(pass_no < 13 ? pass_no : 13);
			__builtin_amdgcn_s_setprio(PRIO_CAND);
			PROF_MARK(16);
			// (ORD: drained at 40, which costs nothing measurable -- profiles/r06_scan -- and leaves every trip room for 24 candidates
			// where it has 4.5: a hit verified in place, outside the drains, then only happens to streams made of sync words)
			if (q_tail - q_head >= (RING == 64 ? (ORD ? SLIDE_DRAIN_AT_ORD : SLIDE_DRAIN_AT) : 64u)) {
				if constexpr (SPLIT)
					drain_issue(q_tail - q_head > 64 ? 64 : q_tail - q_head);       // (the batch before it was finished in this trip)
				else
					drain(q_tail - q_head > 64 ? 64 : q_tail - q_head, whole);
			}
		} else {
			// The pass loop is left when the ring gets short of room (a.ring_margin entries: what a pass may add), drained at
			// the one site behind it and re-entered; candidates that still find no room are checked in place.  (With the
			// drain inside the pass loop its hit registers would be loop-carried through every pass.)
			for (;;) {
				__builtin_amdgcn_s_setprio(PRIO_LOOP);
				bool more = true;
				while (q_tail - q_head + a.ring_margin <= RING) {
					if (!any_left()) {
						more = false;
						break;
					}
					pass();
					PROF_MARK(pass_no < 13 ? pass_no : 13);
					pass_no++;
				}
				if constexpr (CFG::LEVEL2)
					level2_take();                       // (the look-ups of the last pass)
				__builtin_amdgcn_s_setprio(PRIO_CAND);
				PROF_MARK(16);
				if (more || q_tail - q_head >= 32u)
					drain(q_tail - q_head > 64 ? 64 : q_tail - q_head, whole);
				if (!more)
					break;
			}
		}
		(void)pass_no;
		PROF_MARK(18);
#pragma unroll
		for (int u = 0; u < TILES; u++) {
			// no software prefetch: the other five waves of the SIMD cover the loads, and the eight registers it took are
			// worth more (round 5: 3.35 against 3.38 ms; round 6 again, the loads issued right behind the filter and checked in
			// the ISA to be waited for only at the next trip's head, 77 VGPRs: 3.03-3.06 against 2.93-2.95 -- profiles/r06_scan)
			tc[u] = cur;
			load_pair(cur, lo[u], hi[u]);
			advance(cur);
		}
		PROF_MARK(19);
	}
	if constexpr (SPLIT) {
		for (;;) {                                   // the batch the last trip sent, then what is left in the ring
			if (p_n)
				drain(p_n, second_half);
			if (q_tail == q_head)
				break;
			drain_issue(q_tail - q_head > 64 ? 64 : q_tail - q_head);
		}
	} else {
		while (q_tail != q_head)
			drain(q_tail - q_head > 64 ? 64 : q_tail - q_head, whole);
	}
	flush_hits();
#ifdef SCAN_PROFILE
	if (lane < 32)
		atomicAdd(&g_scan_prof[lane], (unsigned long long)lds_ld(prof_off + 4u * lane));
#endif
}
