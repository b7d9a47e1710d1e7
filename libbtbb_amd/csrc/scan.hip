// scan.hip -- sliding 64-bit access-code correlator for gfx950 (MI355X).
//
// Replaces the per-symbol loops of promiscuous_packet_search()
// (lib/src/bluetooth_packet.c:368-420) and find_known_lap() (:423-441) behind
// btbb_find_ac() (:444-464).  Input is the PACKED stream (1 bit per symbol); one
// lane owns the 64 bit-offsets that start in one 64-bit word.
//
// LAP_ANY, per lane and word (scan_slide_kernel; tables built for three and four errors: the same kernel in its two-level
// form, see SlideStd / Slide4 in scan_slide.h; for five errors: scan_lap_any_kernel, which computes the syndrome from two tables in LDS
// and probes a bitmap in L2 per survivor instead of step 2):
//   1. bit-sliced barker pre-filter: seven funnel-shifted copies of the stream give the
//      7-bit window (LAP MSB + 6 barker bits, :378-385) of all 32 offsets of a dword at
//      once; a carry-save adder counts mismatches against 0x27 and `count in {0,1,6,7}`
//      is BARKER_DISTANCE[window] <= 1.  1/8 of the offsets survive.
//   2. bit-sliced check stream (slide.h): the (64,30) code is cyclic, so ONE sparse parity check slides over the
//      window; 19 consecutive bits of the check stream at a survivor's offset are its candidate index.  A chain of 32
//      offsets is a pair of shift registers (survivor mask, check bits) moved down to the survivor in hand, so the
//      index is the low 19 bits: ONE read of a 2^19-bit set in LDS per survivor (the set = every index a window the
//      reference accepts can have: gen_syndrome :147-159 and the map of :161-185 are linear in the same code; it lies
//      there as bit-reversed 16-bit entries, membership is one fast-rate left shift and one signed compare).  0.30 % pass.
//   3. candidates go straight to a per-wave LDS ring and are verified up to 64 at a time with the
//      exact reference rule: full 34-bit syndrome, open-addressing lookup of the
//      error pattern, popcount <= max_ac_errors, LAP from the corrected word
//      (:396-416).  Results are therefore bit-exact, the set only prunes.
// Known LAP: a bit-sliced mismatch count of the top 16 (12 for max_ac_errors < 2) sync-word bits prunes (0.2 % left for
// max_ac_errors = 2), the survivors get the full popcount(window ^ syncword) of :433.
//
// scan_slide_kernel: two persistent 768-thread workgroups per CU (6 waves per SIMD; 64 KiB set + 12 KiB rings + 2.5 KiB syndrome tables of LDS
// each) stride over tiles of 756 words (63 per wave); scan_known_lap_kernel: 256-thread workgroups, tiles of 512 words.  Pure integer
// work, no MFMA; bound by VALU issue, not by HBM (DESIGN.md 3.1 and 6 say what it is bound by).
//
// One translation unit; the pieces it includes:
//   scan_core.h     ScanArgs, the SCAN_PROFILE marks, the device primitives every scan kernel uses (hit records and the pending-hit
//                   queue, LDS accessors, the XCD tile order and candidate code of the LAP_ANY kernels, verify_lap_any, barker32, slide32)
//   scan_lap_any.h  scan_lap_any_kernel (tables for five errors)
//   scan_slide.h    scan_slide_kernel, the headline kernel, with its tuning constants and its two cuts SlideStd / Slide4
//   scan_known.h    scan_known_lap_kernel
//   scan_launch.h   the prototypes of launch_scan and scan_slot_geometry (sort.hip calls them)
// This file: the device entries, the launcher, the symbol <-> packed format kernels.  The host-level wrappers (btbbx_scan_host ...,
// btbbx_shard_plan, btbbx_sort_hits) and check_scan_args are host code: scan_host.cpp.
#include <stdlib.h>
#include <string.h>
#include "scan_core.h"
#include "scan_lap_any.h"
#include "scan_slide.h"
#include "scan_known.h"
#include "scan_launch.h"

// ---- device entries -----------------------------------------------------------------------

extern "C" int btbbx_scan_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
				 uint32_t n_streams, uint64_t search_bits, uint32_t lap, int max_ac_errors,
				 btbbx_hit *d_hits, uint32_t hit_cap, uint32_t *d_hit_count, void *hip_stream)
{
	if (!d_words || !d_hit_count || (!d_hits && hit_cap)) {
		set_error("btbbx_scan_device: null pointer");
		return BTBBX_E_ARG;
	}
	return launch_scan(d_words, n_words, pitch_words, n_streams, search_bits, lap, max_ac_errors,
			   d_hits, hit_cap, d_hit_count, nullptr, (hipStream_t)hip_stream);
}

extern "C" int btbbx_scan_device_fmt(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
				     uint32_t n_streams, uint64_t search_bits, uint32_t lap, int max_ac_errors, int format,
				     btbbx_hit *d_hits, uint32_t hit_cap, uint32_t *d_hit_count, void *hip_stream)
{
	if (!d_words || !d_hit_count || (!d_hits && hit_cap) || (format != BTBBX_FMT_PACKED && format != BTBBX_FMT_PACKED_MSB)) {
		set_error("btbbx_scan_device_fmt: null pointer or a format that is not BTBBX_FMT_PACKED / BTBBX_FMT_PACKED_MSB");
		return BTBBX_E_ARG;
	}
	return launch_scan(d_words, n_words, pitch_words, n_streams, search_bits, lap, max_ac_errors,
			   d_hits, hit_cap, d_hit_count, nullptr, (hipStream_t)hip_stream, nullptr, 0, 0, format == BTBBX_FMT_PACKED_MSB);
}

extern "C" int btbbx_scan_first_device(const uint64_t *d_words, uint64_t n_words, uint64_t search_bits,
				       uint32_t lap, int max_ac_errors, uint64_t *d_first, void *hip_stream)
{
	if (!d_words || !d_first || search_bits >= (1ULL << 32)) {
		set_error("btbbx_scan_first_device: bad argument");
		return BTBBX_E_ARG;
	}
	return launch_scan(d_words, n_words, n_words, 1, search_bits, lap, max_ac_errors,
			   nullptr, 0, nullptr, reinterpret_cast<unsigned long long *>(d_first),
			   (hipStream_t)hip_stream);
}

// ---- launcher -----------------------------------------------------------------------------

// (scan_launch.h says what it returns.)  Known LAP: always slotted; LAP_ANY: the one-level form of scan_slide_kernel alone
bool scan_slot_geometry(uint64_t search_bits, uint32_t n_streams, uint32_t lap, uint32_t *segs_per_stream, uint64_t *n_segs)
{
	int table_errors = 0;
	ScanTables t;
	ctx_scan_snapshot(&t, &table_errors);
	const uint64_t search_words = (search_bits + 63) / 64;
	uint64_t per_stream;
	if (lap != BTBBX_LAP_ANY) {                        // known LAP: segments of 4096 offsets, eight per tile of 512 words
		per_stream = (search_words + 256ull * KL_WORDS - 1) / (256ull * KL_WORDS) * (4 * KL_WORDS);
	} else {
		if (table_errors > 2 || !t.slide_bitmap)
			return false;
		const uint64_t tiles = (search_words + SlideGeom<SlideStd>::TILE_WORDS - 1) / SlideGeom<SlideStd>::TILE_WORDS;
		per_stream = tiles * (SlideStd::THREADS / 64);
	}
	const uint64_t total = per_stream * n_streams;
	if (total >= (1ull << 31))
		return false;
	*segs_per_stream = (uint32_t)per_stream;
	*n_segs = total;
	return true;
}

#ifdef SCAN_PROFILE
// the phase counters of the launch just queued (scan_core.h), read back and printed as shares of the waves' time
static int scan_profile_print(const char *label, int n_phases)
{
	unsigned long long prof[32], total = 0;
	HIP_TRY(hipDeviceSynchronize());
	HIP_TRY(hipMemcpyFromSymbol(prof, HIP_SYMBOL(g_scan_prof), sizeof(prof)));
	for (int k = 0; k < 32; k++) total += prof[k];
	fprintf(stderr, "%s", label);
	for (int k = 0; k < n_phases; k++) fprintf(stderr, " %d:%.1f", k, 100.0 * (double)prof[k] / (double)(total ? total : 1));
	fprintf(stderr, "\n");
	return BTBBX_OK;
}
#endif

int launch_scan(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
		uint32_t n_streams, uint64_t search_bits, uint32_t lap, int max_ac_errors,
		btbbx_hit *d_hits, uint32_t hit_cap, uint32_t *d_hit_count,
		unsigned long long *d_first, hipStream_t stream, uint32_t *bucket_cnt, uint64_t bucket_mul,
		uint32_t bucket_shift, bool msb, const ScanSlots *slots, const uint32_t *gate)
{
	int rc = ctx_require();
	if (rc)
		return rc;
	rc = check_scan_args("btbbx_scan", 64, n_words, pitch_words, n_streams, search_bits);
	if (rc)
		return rc;
	if (search_bits == 0)
		return BTBBX_OK;
	if ((uintptr_t)d_hits & 15) {
		set_error("btbbx_scan: the hit buffer must be 16-byte aligned (records are written as one 16-byte store)");
		return BTBBX_E_ARG;
	}
	Ctx &c = ctx();
	ScanArgs a{};                                  // (the slot fields and the sync word: null / 0 unless set below)
	a.words = d_words;
	a.n_words = n_words;
	a.pitch_words = pitch_words;
	a.search_bits = search_bits;
	a.n_streams = n_streams;
	a.msb = msb ? 1u : 0u;
	a.lap = lap;
	a.max_err = max_ac_errors;
	a.hits = d_hits;
	a.hit_cap = hit_cap;
	a.hit_count = d_hit_count;
	a.first = d_first;
	a.bucket_cnt = bucket_cnt;
	a.bucket_mul = bucket_mul;
	a.bucket_shift = bucket_shift;
	a.gate = gate;
	if (slots) {
		a.seg_slots = slots->slots;
		a.seg_cnt = slots->cnt;
		a.seg_slot_n = slots->slot_n;
		a.segs_per_stream = slots->segs_per_stream;
		a.ovf_recs = slots->ovf_recs;
		a.ovf_meta = reinterpret_cast<uint2 *>(slots->ovf_meta);
		a.ovf_cap = slots->ovf_cap;
		a.ovf_count = slots->ovf_count;
		a.irregular = slots->irregular;
	}
	a.xcd_tiles = 0;
	a.ring_margin = 4;
	int table_errors = 0;
	ctx_scan_snapshot(&a.t, &table_errors);
	const uint64_t search_words = (search_bits + 63) / 64;
	if (lap == BTBBX_LAP_ANY) {
		// tables for <= 2 errors: the sliding-check kernel (1); for three and four: its two-level form (4: a 2^20-bit set in LDS, its members
		// looked up in a second set in L2, slide.h); for five every survivor probes a 2^26-bit bitmap in L2 (8: scan_lap_any_kernel)
		int run_variant = 1;
		if ((table_errors == 3 || table_errors == 4) && a.t.slide4_bitmap)
			run_variant = 4;
		else if (a.t.bitmap2 && table_errors >= 4)
			run_variant = 8;
		const uint32_t tile_words = run_variant == 1 ? SlideGeom<SlideStd>::TILE_WORDS : run_variant == 4 ? SlideGeom<Slide4>::TILE_WORDS : SCAN_THREADS;
		const uint32_t halo_words = run_variant == 8 ? 1 : 2;   // words behind a tile its last lane reads
		a.tiles_per_stream = (search_words + tile_words - 1) / tile_words;
		a.n_tiles = a.tiles_per_stream * n_streams;
		{	// tile t is full iff (t + 1) * tile_words + halo_words <= n_words and (t + 1) * tile_words * 64 <= search_bits
			const uint64_t by_words = n_words >= halo_words ? (n_words - halo_words) / tile_words : 0, by_bits = search_bits / (tile_words * 64ull);
			const uint64_t full = by_words < by_bits ? by_words : by_bits;
			a.full_tiles = full > 0xffffffffull ? 0xffffffffu : (uint32_t)full;
		}
		const uint64_t resident = (uint64_t)c.num_cus * (run_variant == 1 ? SLIDE_WGS : 1);
		uint64_t grid = a.n_tiles < resident ? a.n_tiles : resident;
		a.xcd_tiles = (grid % 8 == 0 && a.n_tiles >= grid) ? (uint32_t)((a.n_tiles + 7) / 8) : 0;
		if ((a.n_tiles + grid - 1) / grid >= (1u << 20) || (a.n_tiles >> 32)) {
			set_error("btbbx_scan: launch too large for the candidate encoding (split the stream)");
			return BTBBX_E_ARG;
		}
#ifdef SCAN_PROFILE
		static unsigned long long zero_prof[32];
		HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_scan_prof), zero_prof, sizeof(zero_prof)));
#endif
		if (slots && run_variant != 1) {
			set_error("btbbx_scan: internal: segment slots with a kernel that has none");
			return BTBBX_E_ARG;
		}
		switch (run_variant) {
		case 8:
			HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_lap_any_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SCAN_LDS_BYTES));
			hipLaunchKernelGGL(scan_lap_any_kernel, dim3((uint32_t)grid), dim3(SCAN_THREADS), SCAN_LDS_BYTES, stream, a);
			break;
		case 4: {
			a.ring_margin = 24u;
			constexpr uint32_t lds_bytes = SlideGeom<Slide4>::LDS_BYTES;
#define LAUNCH_SLIDE4(MSB_) do { \
			HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_slide_kernel<Slide4, SLIDE4_TILES, MSB_>), \
						    hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes)); \
			hipLaunchKernelGGL((scan_slide_kernel<Slide4, SLIDE4_TILES, MSB_>), dim3((uint32_t)grid), dim3(Slide4::THREADS), lds_bytes, stream, a); } while (0)
			if (msb) LAUNCH_SLIDE4(true); else LAUNCH_SLIDE4(false);
#undef LAUNCH_SLIDE4
			break;
		}
		case 1: {
			a.ring_margin = 24u;
			constexpr uint32_t lds_bytes = SlideGeom<SlideStd>::LDS_BYTES;
#define LAUNCH_SLIDE(MSB_, ORD_) do { \
			HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_slide_kernel<SlideStd, SLIDE_TILES, MSB_, ORD_>), \
						    hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes)); \
			hipLaunchKernelGGL((scan_slide_kernel<SlideStd, SLIDE_TILES, MSB_, ORD_>), dim3((uint32_t)grid), dim3(SLIDE_THREADS), lds_bytes, stream, a); } while (0)
			if (table_errors >= 3) {
				set_error("btbbx_scan: internal: the tables for %d errors lack their second-level set", table_errors);
				return BTBBX_E_ARG;
			}
			if (slots) {
				if (a.segs_per_stream != a.tiles_per_stream * (SLIDE_THREADS / 64) || d_first) {
					set_error("btbbx_scan: internal: segment slots laid out for another geometry");
					return BTBBX_E_ARG;
				}
				if (msb) LAUNCH_SLIDE(true, true); else LAUNCH_SLIDE(false, true);
			} else {
				if (msb) LAUNCH_SLIDE(true, false); else LAUNCH_SLIDE(false, false);
			}
#undef LAUNCH_SLIDE
			break;
		}
		default: set_error("btbbx_scan: internal: no LAP_ANY kernel for this table set"); return BTBBX_E_ARG;
		}
#ifdef SCAN_PROFILE
		rc = scan_profile_print("scan profile (% of wave time):", 20);
		if (rc)
			return rc;
#endif
	} else {
		a.syncword = host_gen_syncword(lap & 0xffffff);
		a.lap = lap;
		TileGrid g;
		rc = tile_grid("btbbx_scan", search_bits, n_words, n_streams, 256 * KL_WORDS, c.num_cus, &g);
		if (rc)
			return rc;
		a.tiles_per_stream = g.tiles_per_stream;
		a.n_tiles = g.n_tiles;
		a.full_tiles = g.full_tiles;
		if (slots && (a.segs_per_stream != a.tiles_per_stream * (4 * KL_WORDS) || d_first)) {
			set_error("btbbx_scan: internal: segment slots laid out for another geometry");
			return BTBBX_E_ARG;
		}
		const bool cls1 = ((a.syncword >> 57) & 1) != 0;          // = bit 23 of the LAP
#define LAUNCH_KNOWN__(L, C_, M_, O_) hipLaunchKernelGGL((scan_known_lap_kernel<L, C_, M_, O_>), dim3(g.grid), dim3(256), 0, stream, a)
#define LAUNCH_KNOWN_(L, C_, M_) do { if (slots) LAUNCH_KNOWN__(L, C_, M_, true); else LAUNCH_KNOWN__(L, C_, M_, false); } while (0)
#define LAUNCH_KNOWN(L) do { if (cls1) { if (msb) LAUNCH_KNOWN_(L, 1, true); else LAUNCH_KNOWN_(L, 1, false); } \
		else { if (msb) LAUNCH_KNOWN_(L, 0, true); else LAUNCH_KNOWN_(L, 0, false); } } while (0)
		switch (max_ac_errors) {
		case 0: LAUNCH_KNOWN(0); break;
		case 1: LAUNCH_KNOWN(1); break;
		case 2: LAUNCH_KNOWN(2); break;
		case 3: LAUNCH_KNOWN(3); break;
		case 4: LAUNCH_KNOWN(4); break;
		default: LAUNCH_KNOWN(-1); break;
		}
#undef LAUNCH_KNOWN
#undef LAUNCH_KNOWN_
#undef LAUNCH_KNOWN__
#ifdef SCAN_PROFILE
		rc = scan_profile_print("known-LAP profile (% of wave time; cumulative over launches):", 5);
		if (rc)
			return rc;
#endif
	}
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

// ---- symbol <-> packed conversion ---------------------------------------------------------

// 16 symbols (bit 0 of 16 bytes) -> 16 bits
__device__ __forceinline__ uint32_t gather16(uint4 v)
{
	auto nib = [](uint32_t x) {
		x &= 0x01010101u;
		return (x | (x >> 7) | (x >> 14) | (x >> 21)) & 0xfu;
	};
	return nib(v.x) | (nib(v.y) << 4) | (nib(v.z) << 8) | (nib(v.w) << 12);
}

__global__ __launch_bounds__(256) void pack_kernel(const uint8_t *sym, uint64_t n_sym, uint64_t *words, uint64_t n_words)
{
	// each lane converts 16 symbols; 4 adjacent lanes make one word
	uint64_t chunk = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	uint64_t n_chunks = n_words * 4;
	for (; chunk < ((n_chunks + 63) & ~63ULL); chunk += stride) {
		uint64_t s0 = chunk * 16;
		uint32_t bits = 0;
		if (s0 + 16 <= n_sym && (((uintptr_t)(sym + s0)) & 15) == 0) {
			bits = gather16(*reinterpret_cast<const uint4 *>(sym + s0));
		} else if (s0 < n_sym) {
			for (uint32_t i = 0; i < 16 && s0 + i < n_sym; i++)
				bits |= (uint32_t)(sym[s0 + i] & 1) << i;
		}
		uint32_t q = threadIdx.x & 3;
		uint64_t part = (uint64_t)bits << (16 * q);
		part |= __shfl_xor(part, 1);
		part |= __shfl_xor(part, 2);
		if (q == 0 && chunk < n_chunks)
			words[chunk >> 2] = part;
	}
}

__global__ __launch_bounds__(256) void unpack_kernel(const uint64_t *words, uint64_t n_sym, uint8_t *sym)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
	for (; i * 8 < n_sym; i += stride) {              // 8 symbols per lane
		uint32_t byte = (uint32_t)(words[i >> 3] >> (8 * (i & 7))) & 0xff;
		uint64_t out = 0;
#pragma unroll
		for (int b = 0; b < 8; b++)
			out |= (uint64_t)((byte >> b) & 1) << (8 * b);
		if (i * 8 + 8 <= n_sym && (((uintptr_t)(sym + i * 8)) & 7) == 0) {
			*reinterpret_cast<uint64_t *>(sym + i * 8) = out;
		} else {
			for (uint32_t b = 0; b < 8 && i * 8 + b < n_sym; b++)
				sym[i * 8 + b] = (uint8_t)(out >> (8 * b));
		}
	}
}

// MSB-first packed bytes (8 symbols per byte, first received symbol in bit 7 -- the order a
// radio front end typically delivers) -> the library's LSB-first words: reverse the bits of
// every byte in place.  brev64 reverses everything, the byte swap puts the bytes back.
__global__ __launch_bounds__(256) void bitrev_bytes_kernel(uint64_t *words, uint64_t n_words)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
	for (; i < n_words; i += step)
		words[i] = __builtin_bswap64(__brevll(words[i]));
}

extern "C" int btbbx_pack_device(const uint8_t *d_symbols, uint64_t n_symbols, uint64_t *d_words, void *hip_stream)
{
	if (n_symbols == 0)
		return BTBBX_OK;
	uint64_t n_words = (n_symbols + 63) / 64;
	uint64_t threads = n_words * 4;
	uint64_t blocks = (threads + 255) / 256;
	if (blocks > 65536) blocks = 65536;
	hipLaunchKernelGGL(pack_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)hip_stream,
			   d_symbols, n_symbols, d_words, n_words);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

extern "C" int btbbx_msb_to_lsb_device(uint64_t *d_words, uint64_t n_words, void *hip_stream)
{
	if (n_words == 0)
		return BTBBX_OK;
	uint64_t blocks = (n_words + 255) / 256;
	if (blocks > 65536) blocks = 65536;
	hipLaunchKernelGGL(bitrev_bytes_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)hip_stream, d_words, n_words);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

extern "C" int btbbx_unpack_device(const uint64_t *d_words, uint64_t n_symbols, uint8_t *d_symbols, void *hip_stream)
{
	if (n_symbols == 0)
		return BTBBX_OK;
	uint64_t threads = (n_symbols + 7) / 8;
	uint64_t blocks = (threads + 255) / 256;
	if (blocks > 65536) blocks = 65536;
	hipLaunchKernelGGL(unpack_kernel, dim3((uint32_t)blocks), dim3(256), 0, (hipStream_t)hip_stream,
			   d_words, n_symbols, d_symbols);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}
