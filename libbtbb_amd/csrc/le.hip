// le.hip -- Bluetooth LE 1M uncoded PHY: access-address search, dewhitening, CRC-24 and the fields
// lell_allocate_and_decode derives (lib/src/bluetooth_le_packet.c:282-312), over whole captures.
//
// Air format (Core v5.x Vol 6 Part B): preamble (8 alternating bits, the first equal to AA bit 0), access address
// (32 bits), PDU = 16-bit header + L octets (L = header octet 1, all 8 bits), CRC-24.  Every octet LSB first, so
// stream bit offset + i is bit i of the 40-bit pattern preamble | AA << 8.  Header, payload and CRC are whitened
// (3.2: x^7 + x^4 + 1, position 0 = 1, positions 1..6 = channel index MSB first); the CRC (3.1.1:
// x^24 + x^10 + x^9 + x^6 + x^4 + x^3 + x + 1, preset with CRCInit) covers the 2 + L PDU octets and is sent from
// register position 23 down to 0.  Both registers run here in their reflected software form: whitening state bit j
// = position 6 - j, CRC state bit j = position 23 - j; tests/_le.py shifts the spec's positions literally.
#include "tile_scan.h"
#include "le_record.h"
#include <algorithm>
#include <stddef.h>

#define LE_THREADS 256
#define LE_WORDS 2                               // consecutive stream words per lane and tile (tile = 512 words)
#define LE_TILE_WORDS (LE_THREADS * LE_WORDS)
#define LE_RING 128                              // per-wave hit ring (entries)

struct LeScanArgs {
	const uint64_t *words;
	uint64_t n_words;
	uint64_t pitch_words;
	uint64_t search_bits;
	uint32_t tiles_per_stream;
	uint32_t full_tiles;         // leading tiles of a stream whose words, halo word and offsets are all in range
	uint32_t n_streams;
	uint32_t pat_lo;             // window bits 0..31 = preamble | AA << 8
	uint32_t pat_hi;             // window bits 32..39 = AA >> 24
	int max_err;
	btbbx_hit *hits;
	uint32_t hit_cap;
	uint32_t *hit_count;
};

// One workgroup of 256 lanes works on a tile of 512 words of one stream at a time; a lane owns two consecutive words
// (four dwords D[0..3]) and reads the next word as its halo (D[4..5]): chain c = the 32 offsets starting at dword c,
// whose 40-bit windows lie in D[c .. c + 2].  Window bit j of chain c's offsets is alignbit(D[c + 1], D[c], j) and window
// bit 32 + j is alignbit(D[c + 2], D[c + 1], j) -- the lower planes of chain c + 1 --, so the filter's sixteen planes of
// the four chains take 5 x 7 funnel shifts (the shift by zero is the dword itself).  Survivors get the exact check
// popcount((window ^ pattern) & mask40) <= limit; hits are ranked with a ballot and mbcnt into a per-wave ring and leave it
// 64 at a time, with one counter atomic per 64 hits.
template <int PAT, int LIMIT>
__global__ __launch_bounds__(LE_THREADS) void le_scan_kernel(LeScanArgs a)
{
	__shared__ uint4 ring_mem[LE_THREADS / 64][LE_RING];
	const uint32_t tid = threadIdx.x, lane = tid & 63;
	uint32_t pat_lo = a.pat_lo, pat_hi = a.pat_hi;
	asm volatile("" : "+v"(pat_lo), "+v"(pat_hi));     // (VGPR copies: a VALU op with an SGPR source issues at half rate)
	uint32_t flip[16];
#pragma unroll
	for (int k = 0; k < 16; k++) {
		flip[k] = (((k < 8 ? pat_lo : pat_hi) >> (k & 7)) & 1) ? 0xffffffffu : 0u;
		if (PAT < 0)
			asm volatile("" : "+v"(flip[k]));
	}
	const uint32_t tiles_per_stream = a.tiles_per_stream;
	uint32_t stream = 0, t = blockIdx.x;
	while (t >= tiles_per_stream && stream < a.n_streams) {
		t -= tiles_per_stream;
		stream++;
	}
	const uint32_t lw = tid * LE_WORDS;
	uint64_t nw[LE_WORDS + 1];
	// Hits wait in a per-wave LDS ring and leave 64 at a time: one counter atomic per 64 hits (a single counter word saturates
	// near 88 M atomics/s, which one atomic per wave and pass ran into at one packet per 4096 bits: 0.46 Tbit/s)
	uint4 *ring = ring_mem[tid >> 6];
	uint32_t q_head = 0, q_tail = 0;                // wave-uniform, free running
	auto flush = [&](uint32_t n) {                  // the n <= 64 oldest entries -> the global hit list
		uint32_t base = 0;
		if (lane == 0)
			base = atomicAdd(a.hit_count, n);
		base = __builtin_amdgcn_readfirstlane(base);
		if (lane < n && base + lane < a.hit_cap)
			reinterpret_cast<uint4 *>(a.hits)[base + lane] = ring[(q_head + lane) & (LE_RING - 1)];
		q_head += n;
	};
	auto stage = [&](bool hit, uint32_t s, uint64_t offset, uint32_t aa_rx, uint32_t nerr) {
		const uint64_t mask = __ballot(hit);
		if (!mask)
			return;
		if (q_tail - q_head + 64 > LE_RING)
			flush(64);
		if (hit) {
			const uint32_t slot = q_tail + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
			uint4 rec;
			rec.x = (uint32_t)offset;
			rec.y = (uint32_t)(offset >> 32);
			rec.z = aa_rx;
			rec.w = nerr | (s << 16);
			ring[slot & (LE_RING - 1)] = rec;
		}
		q_tail += (uint32_t)__popcll(mask);
	};
	auto fetch = [&](uint32_t ft, uint32_t fstream) { fetch_run<LE_TILE_WORDS>(a, ft, fstream, lw * 8u, nw); };
	fetch(t, stream);                                   // (not waited for in front of the loop as in scan_known_lap_kernel: DESIGN 3.8)
	constexpr int NCH = 2 * LE_WORDS;
	while (stream < a.n_streams) {
		const uint64_t word0 = (uint64_t)t * LE_TILE_WORDS + lw;
		uint32_t D[NCH + 2], m[NCH];
#pragma unroll
		for (int u = 0; u <= LE_WORDS; u++) {
			D[2 * u] = (uint32_t)nw[u];
			D[2 * u + 1] = (uint32_t)(nw[u] >> 32);
		}
		const bool ragged = t >= a.full_tiles;
		const uint32_t this_stream = stream;
		t += gridDim.x;
		while (t >= tiles_per_stream && stream < a.n_streams) {
			t -= tiles_per_stream;
			stream++;
		}
		fetch(t, stream);                               // the next tile's words are loaded while this one is worked on
		{
			uint32_t P[2][8];
			P[0][0] = D[0];
#pragma unroll
			for (int j = 1; j < 8; j++)
				P[0][j] = alignbit(D[1], D[0], j);
#pragma unroll
			for (int c = 0; c < NCH; c++) {
				uint32_t *up = P[(c + 1) & 1];
				up[0] = D[c + 1];
#pragma unroll
				for (int j = 1; j < 8; j++)
					up[j] = alignbit(D[c + 2], D[c + 1], j);
				uint32_t r[16];
#pragma unroll
				for (int j = 0; j < 8; j++) {
					r[j] = P[c & 1][j];
					r[8 + j] = up[j];
				}
				m[c] = le_filter16<PAT, LIMIT>(r, flip);
			}
		}
		if (ragged) {
			asm volatile("" ::: "memory");
#pragma unroll
			for (int c = 0; c < NCH; c++) {
				const uint64_t first_off = word0 * 64 + 32u * c;
				m[c] &= first_off >= a.search_bits ? 0u
					: (a.search_bits - first_off >= 32 ? 0xffffffffu : ((1u << (uint32_t)(a.search_bits - first_off)) - 1u));
			}
		}
		// survivors: one offset of every chain per pass, passes until no lane of the wave has one left
		for (;;) {
			uint32_t any = 0;
#pragma unroll
			for (int c = 0; c < NCH; c++)
				any |= m[c];
			if (!__ballot(any != 0))
				break;
#pragma unroll
			for (int c = 0; c < NCH; c++) {
				if (!__ballot(m[c] != 0))
					continue;
				const uint32_t p = (uint32_t)__builtin_ctz(m[c] | 0x80000000u);
				const uint32_t lo = alignbit(D[c + 1], D[c], p), hi = alignbit(D[c + 2], D[c + 1], p);
				const uint32_t e = (uint32_t)__popc(lo ^ pat_lo) + (uint32_t)__popc((hi ^ pat_hi) & 0xffu);
				const bool hit = m[c] != 0 && e <= (uint32_t)LIMIT;
				m[c] &= m[c] - 1;
				stage(hit, this_stream, word0 * 64 + 32u * c + p, (lo >> 8) | (hi << 24), e);
			}
		}
		while (q_tail - q_head >= 64)
			flush(64);
	}
	if (q_tail != q_head)
		flush(q_tail - q_head);
}

// ---- stage 2: dewhitening, CRC-24, the lell fields ----------------------------------------------------------------

// (le_record.h, included above: the channel mapping, the access-address rules, the two tables' entries and le_record, which the
// coded-PHY decoder of le_coded.h calls as well)

// one thread per hit (hits are rare next to the offsets scanned).  LDS: the byte-wise CRC table of the reflected register
// (state >>= 8 ^ T[(state ^ octet) & 0xff]) and the whitening register advanced eight bits at a time (127-state LFSR:
// the eight output bits and the next state of every state).
__global__ __launch_bounds__(256) void le_decode_kernel(const uint64_t *words, uint64_t n_words, uint64_t pitch_words,
							const btbbx_hit *hits, const uint32_t *d_count, uint32_t cap,
							const uint16_t *phys, uint32_t crc_init_reflected, btbbx_le_pkt *out)
{
	__shared__ uint32_t crc_tab[256];
	__shared__ uint16_t wh_tab[128];                    // low byte: eight whitening bits; high byte: the next state
	const uint32_t tid = threadIdx.x;
	crc_tab[tid] = le_crc_tab_entry(tid);
	if (tid < 128)
		wh_tab[tid] = le_wh_tab_entry(tid);
	__syncthreads();
	const uint32_t n = min(*d_count, cap);
	const uint32_t i = blockIdx.x * 256u + tid;
	if (i >= n)
		return;
	const btbbx_hit h = hits[i];
	const uint64_t *w = words + (uint64_t)h.stream * pitch_words;
	auto octet = [&](uint64_t bit) -> uint32_t {       // eight stream bits from `bit`, zeros past the stream's end
		const uint64_t wi = bit >> 6;
		const uint32_t sh = (uint32_t)(bit & 63);
		const uint64_t lo = wi < n_words ? w[wi] : 0;
		const uint64_t hi = sh > 56 && wi + 1 < n_words ? w[wi + 1] : 0;
		return (uint32_t)(((lo >> sh) | (sh ? hi << (64 - sh) : 0)) & 0xffu);
	};
	const uint64_t pdu_bit = h.offset + 40;
	le_record([&](uint32_t k) { return octet(pdu_bit + 8ull * k); },
		  [&](uint32_t pdu) { return pdu_bit + 8ull * (pdu + 3) > n_words * 64; },
		  -1, crc_tab, wh_tab, phys[h.stream], crc_init_reflected, h.lap, h, out[i]);
}

// ---- host side ----------------------------------------------------------------------------------------------------

static_assert(sizeof(btbbx_le_pkt) == 104, "btbbx_le_pkt: 104 bytes (libbtbb_amd LE_PKT_DTYPE)");
static_assert(offsetof(btbbx_le_pkt, stream) == 8 && offsetof(btbbx_le_pkt, aa_errors) == 10 && offsetof(btbbx_le_pkt, crc_ok) == 11,
	      "btbbx_le_pkt layout");
static_assert(offsetof(btbbx_le_pkt, crc_rx) == 12 && offsetof(btbbx_le_pkt, crc_calc) == 16 && offsetof(btbbx_le_pkt, pdu_bytes) == 20 &&
	      offsetof(btbbx_le_pkt, truncated) == 22 && offsetof(btbbx_le_pkt, channel_idx) == 23, "btbbx_le_pkt layout");
static_assert(offsetof(btbbx_le_pkt, access_address_offenses) == 31 && offsetof(btbbx_le_pkt, access_address) == 32 &&
	      offsetof(btbbx_le_pkt, bytes) == 36, "btbbx_le_pkt layout");

static int le_check_args(const char *who, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, uint64_t search_bits,
			 int max_errors)
{
	if (max_errors < 0 || max_errors > BTBBX_LE_MAX_ERRORS) {
		set_error("%s: max_errors must be 0..%d", who, BTBBX_LE_MAX_ERRORS);
		return BTBBX_E_ARG;
	}
	return check_scan_args(who, 40, n_words, pitch_words, n_streams, search_bits);
}

static int le_launch_scan(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, uint64_t search_bits,
			  uint32_t aa, int max_errors, btbbx_hit *d_hits, uint32_t hit_cap, uint32_t *d_hit_count, hipStream_t q)
{
	if (search_bits == 0)
		return BTBBX_OK;
	if ((uintptr_t)d_hits & 15) {
		set_error("btbbx_le_scan_device: the hit buffer must be 16-byte aligned");
		return BTBBX_E_ARG;
	}
	LeScanArgs a;
	a.words = d_words;
	a.n_words = n_words;
	a.pitch_words = n_streams > 1 ? pitch_words : n_words;
	a.search_bits = search_bits;
	a.n_streams = n_streams;
	a.pat_lo = ((aa & 1u) ? 0x55u : 0xaau) | (aa << 8);
	a.pat_hi = aa >> 24;
	a.max_err = max_errors;
	a.hits = d_hits;
	a.hit_cap = hit_cap;
	a.hit_count = d_hit_count;
	TileGrid g;
	const int rc = tile_grid("btbbx_le_scan_device", search_bits, n_words, n_streams, LE_TILE_WORDS, ctx().num_cus, &g);
	if (rc)
		return rc;
	a.full_tiles = g.full_tiles;
	a.tiles_per_stream = (uint32_t)g.tiles_per_stream;
	const bool adv = aa == BTBBX_LE_ADV_AA;
	// the advertising AA's sixteen filter bits (preamble 0xaa, AA octet 0x8e) folded into the adders; any other AA: XORs
	constexpr int ADV_PAT = 0xaa | (0x8e << 8);
#define LE_LAUNCH(P, L) hipLaunchKernelGGL((le_scan_kernel<P, L>), dim3(g.grid), dim3(LE_THREADS), 0, q, a)
#define LE_LAUNCH_L(L) do { if (adv) LE_LAUNCH(ADV_PAT, L); else LE_LAUNCH(-1, L); } while (0)
	switch (max_errors) {
	case 0: LE_LAUNCH_L(0); break;
	case 1: LE_LAUNCH_L(1); break;
	case 2: LE_LAUNCH_L(2); break;
	case 3: LE_LAUNCH_L(3); break;
	default: LE_LAUNCH_L(4); break;
	}
#undef LE_LAUNCH_L
#undef LE_LAUNCH
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

extern "C" int btbbx_le_scan_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				    uint64_t search_bits, uint32_t aa, int max_errors,
				    btbbx_hit *d_hits, uint32_t hit_cap, uint32_t *d_hit_count, void *hip_stream)
{
	int rc = le_check_args("btbbx_le_scan_device", n_words, pitch_words, n_streams, search_bits, max_errors);
	if (rc)
		return rc;
	if (!d_words || !d_hit_count || (!d_hits && hit_cap)) {
		set_error("btbbx_le_scan_device: null pointer");
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	return le_launch_scan(d_words, n_words, pitch_words, n_streams, search_bits, aa, max_errors, d_hits, hit_cap, d_hit_count,
			      (hipStream_t)hip_stream);
}

extern "C" int btbbx_le_decode_hits_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
					   const btbbx_hit *d_hits, const uint32_t *d_count, uint32_t cap,
					   const uint16_t *d_phys_channel, uint32_t crc_init,
					   btbbx_le_pkt *d_out, void *hip_stream)
{
	if (cap && (!d_words || !d_hits || !d_count || !d_phys_channel || !d_out)) {
		set_error("btbbx_le_decode_hits_device: null pointer");
		return BTBBX_E_ARG;
	}
	int rc = ctx_require();
	if (rc)
		return rc;
	if (cap == 0)
		return BTBBX_OK;
	hipLaunchKernelGGL(le_decode_kernel, dim3((cap + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, d_words, n_words, pitch_words,
			   d_hits, d_count, cap, d_phys_channel, le_reverse24(crc_init & 0xffffffu), d_out);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

extern "C" int64_t btbbx_le_scan_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				      uint64_t search_bits, const uint16_t *phys_channel, uint32_t aa, uint32_t crc_init,
				      int max_errors, btbbx_le_pkt *pkts, uint64_t cap)
{
	int rc = le_check_args("btbbx_le_scan_host", n_words, pitch_words, n_streams, search_bits, max_errors);
	if (rc)
		return rc;
	if (!words || !phys_channel || (!pkts && cap)) {
		set_error("btbbx_le_scan_host: null pointer");
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	if (n_streams == 1)
		pitch_words = n_words;
	CallScope scope;
	hipStream_t q = scope_stream();
	// the capture (+ one word of slack) and the channel list in one block of the call's device scratch
	const uint64_t cap_words = (uint64_t)(n_streams - 1) * pitch_words + n_words;
	const size_t words_bytes = ((size_t)(cap_words + 1) * 8 + 255) & ~(size_t)255;
	char *dblock = (char *)scope_device(words_bytes + 2 * (size_t)n_streams);
	if (!dblock)
		return BTBBX_E_NOMEM;
	const uint64_t *d_words = (const uint64_t *)dblock;
	uint16_t *d_phys = (uint16_t *)(dblock + words_bytes);
	HIP_TRY(hipMemcpyAsync(dblock, words, (size_t)cap_words * 8, hipMemcpyHostToDevice, q));
	HIP_TRY(hipMemcpyAsync(d_phys, phys_channel, 2 * (size_t)n_streams, hipMemcpyHostToDevice, q));
	// first guess: what the caller can take, but no more than one hit per 1024 offsets + slack; repeated with room for
	// every match when more were found (the records kept by a full buffer are whichever waves came first)
	uint64_t guess = search_bits / 1024 * n_streams + 4096;
	if (guess > cap)
		guess = cap;
	uint32_t dev_cap = guess > 0xfffffff0ull ? 0xfffffff0u : (uint32_t)guess;
	uint32_t count = 0;
	char *block = nullptr;
	size_t rec_bytes = 0, order_bytes = 0;
	for (int pass = 0; pass < 2; pass++) {
		rec_bytes = ((size_t)dev_cap * sizeof(btbbx_hit) + 255) & ~(size_t)255;
		order_bytes = dev_cap >= 2 ? (btbbx_order_hits_scratch_bytes(dev_cap) + 255) & ~(size_t)255 : 0;
		const size_t pkt_bytes = (size_t)dev_cap * sizeof(btbbx_le_pkt);
		block = (char *)scope_hits(256 + rec_bytes + order_bytes + pkt_bytes);
		if (!block)
			return BTBBX_E_NOMEM;
		uint32_t *d_count = (uint32_t *)block;
		HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(uint32_t), q));
		rc = le_launch_scan(d_words, n_words, pitch_words, n_streams, search_bits, aa, max_errors, (btbbx_hit *)(block + 256), dev_cap,
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
		if (have >= 2) {
			rc = btbbx_order_hits_device(d_hits, d_count, dev_cap, block + 256 + rec_bytes, order_bytes, q);
			if (rc)
				return rc;
		}
		const uint32_t n = (uint32_t)std::min<uint64_t>(have, cap);
		rc = btbbx_le_decode_hits_device(d_words, n_words, pitch_words, d_hits, d_count, n, d_phys, crc_init, d_pkts, q);
		if (rc)
			return rc;
		HIP_TRY(hipMemcpyAsync(pkts, d_pkts, (size_t)n * sizeof(btbbx_le_pkt), hipMemcpyDeviceToHost, q));
		HIP_TRY(hipStreamSynchronize(q));
	}
	return (int64_t)count;
}

#include "le_discover.h"
#include "le_track.h"
#include "le_csa2.h"
#include "le_follow.h"
#include "le_span.h"
#include "le_data.h"
#include "le_crypt.h"
#include "le_keyed.h"
#include "le_pair.h"
#include "le_resolve.h"
#include "le_host.h"
