// le_discover.h -- promiscuous LE connection discovery (included by le.hip, behind its kernels): the access address and the
// CRCInit of every data-channel connection of a capture, neither of them known beforehand.
//
// A candidate is an offset whose eight preamble bits alternate and agree with the AA bit behind them, whose AA
// has no data-channel offense, whose dewhitened header has LLID != 0, no RFU bit and a length <= max_len, and whose packet
// ends inside the stream.  Its CRCInit is what the CRC register must have been preset with for the received CRC to come out:
// the register run backwards from the received CRC through the PDU, last octet first.
//
//   1. le_disc_scan_kernel    the tile frame of le_scan_kernel; the filter is the preamble rule and the three RFU bits, the survivors' cheap header
//      test runs in the lane, and what passes waits in the per-wave ring.  The ring is drained 64 entries at a time, one
//      entry per lane: offense count and backward CRC, a ballot, one counter atomic for the wave, 24-byte records
//   2. le_disc_key_kernel .. le_disc_copy_kernel   grouping: two stable LSD radix sorts (radix_sort.h: by (stream, offset), then
//      by (AA, CRCInit)), boundary flags and their prefix sums, one record per group of min_count or more, the candidate list
//      rewritten in sorted order with every candidate's connection index
//
// Nothing here synchronises or reads back but the host wrapper: the counts stay in device memory.
#pragma once
#include "radix_sort.h"
#include "wave_scan.h"
#include "le_slots.h"

#define LD_RING      128                   // per-wave ring of header-tested survivors (entries)
#define LD_GRP_TILE  2048u                 // records (or groups) a workgroup flags per launch (8 rounds of 256)
#define LD_WAVES     (LE_THREADS / 64)
#define LD_NO_CONN   0xffffffffu

static_assert(sizeof(btbbx_le_cand) == 24 && offsetof(btbbx_le_cand, access_address) == 8 && offsetof(btbbx_le_cand, crc_init) == 12 &&
	      offsetof(btbbx_le_cand, stream) == 16 && offsetof(btbbx_le_cand, header0) == 18 && offsetof(btbbx_le_cand, length) == 19 &&
	      offsetof(btbbx_le_cand, conn) == 20, "btbbx_le_cand layout (libbtbb_amd.LE_CAND_DTYPE)");
static_assert(sizeof(btbbx_le_conn) == 32 && offsetof(btbbx_le_conn, n_packets) == 8 && offsetof(btbbx_le_conn, n_empty) == 12 &&
	      offsetof(btbbx_le_conn, channel_mask) == 16 && offsetof(btbbx_le_conn, first) == 24,
	      "btbbx_le_conn layout (libbtbb_amd.LE_CONN_DTYPE)");

struct LeDiscArgs {
	const uint64_t *words;
	uint64_t n_words;
	uint64_t pitch_words;
	uint64_t search_bits;
	uint32_t tiles_per_stream;
	uint32_t full_tiles;
	uint32_t n_streams;
	uint32_t max_len;
	const uint16_t *phys;
	btbbx_le_cand *cands;
	uint32_t cand_cap;
	uint32_t *cand_count;
};

// ---- 1. the scan ------------------------------------------------------------------------------------------------------

// Frame, fetch and chains as le_scan_kernel.  With X = D ^ (D >> 1) over the lane's run, bit o + j of X says that stream bits
// o + j and o + j + 1 differ: the preamble rule (bits o .. o + 7 alternate, bit o + 8 equals bit o) is X bits o .. o + 7 all
// set, so a chain's mask is the AND of eight planes of X -- five XORs and 5 + 4 x 7 funnel shifts per tile and lane, no adder.
// Three more planes, window bits 45 .. 47 XORed with the stream's whitening bits, are the header's RFU bits: folded into the mask
// they leave 1/2048 of the offsets to the survivor pass instead of 1/256 (measured: 3.14 -> 1.68 ms per 4 GiB).
// LDS: the ring, the byte-wise INVERSE of the reflected CRC table (the feedback enters bit 23, so the top byte of
// T[i] names i: crc_inv[T[i] >> 16] = T[i] << 8 | i, and the state before an octet d is (s << 8 ^ crc_inv[s >> 16]) ^ d), and
// the whitening sequence by phase (127 bits long: wh_seq[p] = its eight bits from phase p, wh_phase[state] = the phase at
// which the register holds `state`), so octet k of a packet is dewhitened without walking there.
__global__ __launch_bounds__(LE_THREADS) void le_disc_scan_kernel(LeDiscArgs a)
{
	__shared__ uint4 ring_mem[LD_WAVES][LD_RING];
	__shared__ uint32_t crc_inv[256];
	__shared__ uint8_t wh_seq[128], wh_phase[128];
	const uint32_t tid = threadIdx.x, lane = tid & 63;
	{
		uint32_t s = tid;
		for (int k = 0; k < 8; k++)
			s = (s >> 1) ^ ((s & 1u) ? 0xda6000u : 0u);
		crc_inv[s >> 16] = (s << 8) | tid;
		if (tid < 127) {
			uint32_t w = 0x40u, o = 0;
			for (uint32_t k = 0; k < tid; k++) {
				if (w & 1u)
					w ^= 0x88u;
				w >>= 1;
			}
			wh_phase[w] = (uint8_t)tid;
			for (int k = 0; k < 8; k++) {
				o |= (w & 1u) << k;
				if (w & 1u)
					w ^= 0x88u;
				w >>= 1;
			}
			wh_seq[tid] = (uint8_t)o;
		} else if (tid == 127) {
			wh_seq[127] = 0;
			wh_phase[0] = 0;
		}
	}
	__syncthreads();
	const uint32_t tiles_per_stream = a.tiles_per_stream;
	const uint64_t total_bits = a.n_words * 64;
	uint32_t stream = 0, t = blockIdx.x;
	while (t >= tiles_per_stream && stream < a.n_streams) {
		t -= tiles_per_stream;
		stream++;
	}
	const uint32_t lw = tid * LE_WORDS;
	uint64_t nw[LE_WORDS + 1];
	uint4 *ring = ring_mem[tid >> 6];
	uint32_t q_head = 0, q_tail = 0;                // wave-uniform, free running
	// the n <= 64 oldest entries, one per lane: rules 3 and the CRCInit; what is left goes to the list with one counter atomic
	auto flush = [&](uint32_t n) {
		bool keep = false;
		uint4 e = make_uint4(0, 0, 0, 0);
		uint32_t init = 0, ch = 0;
		if (lane < n) {
			e = ring[(q_head + lane) & (LD_RING - 1)];
			keep = le_data_offenses(e.z) == 0;
		}
		if (keep) {
			const uint32_t s = e.w >> 16, h0 = e.w & 0xffu, h1 = (e.w >> 8) & 0xffu;
			// (rule 5 has passed: every octet read here lies inside the stream, so the byte behind it is read only when the octet reaches into it)
			const uint8_t *w = reinterpret_cast<const uint8_t *>(a.words + (uint64_t)s * a.pitch_words);
			auto octet = [&](uint64_t bit) -> uint32_t {   // eight stream bits from `bit`
				const uint8_t *b = w + (bit >> 3);
				const uint32_t sh = (uint32_t)bit & 7u;
				const uint32_t v = b[0] | (sh ? (uint32_t)b[1] << 8 : 0u);
				return (v >> sh) & 0xffu;
			};
			ch = le_channel_index(a.phys[s]);
			const uint32_t pdu = 2 + h1;
			const uint64_t pdu_bit = (((uint64_t)e.y << 32) | e.x) + 40;
			uint32_t ph = (wh_phase[(ch & 0x3fu) | 0x40u] + 8u * (pdu + 2)) % 127u;     // phase of the last CRC octet
			auto back = [&]() {
				const uint32_t v = wh_seq[ph];
				ph = ph >= 8 ? ph - 8 : ph + 119;
				return v;
			};
			uint32_t st = 0;                                // the register behind the PDU = the received CRC, first bit in bit 0
			for (int k = 2; k >= 0; k--)
				st = (st << 8) | (octet(pdu_bit + 8ull * (pdu + k)) ^ back());
			for (uint32_t k = pdu; k-- > 2;) {
				const uint32_t d = octet(pdu_bit + 8ull * k) ^ back();
				st = ((st << 8) ^ crc_inv[st >> 16]) ^ d;
			}
			st = ((st << 8) ^ crc_inv[st >> 16]) ^ h1;
			st = ((st << 8) ^ crc_inv[st >> 16]) ^ h0;
			init = __builtin_bitreverse32(st) >> 8;         // reflected register -> CRCInit as the spec writes it
		}
		q_head += n;
		const uint64_t mask = __ballot(keep);
		if (!mask)
			return;
		uint32_t base = 0;
		if (lane == 0)
			base = atomicAdd(a.cand_count, (uint32_t)__popcll(mask));
		base = __builtin_amdgcn_readfirstlane(base);
		const uint32_t slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
		if (keep && slot < a.cand_cap) {
			uint2 *out = reinterpret_cast<uint2 *>(a.cands + slot);
			out[0] = make_uint2(e.x, e.y);
			out[1] = make_uint2(e.z, init);
			out[2] = make_uint2(e.w >> 16 | (e.w << 16), ch); // stream, header0, length; conn = the channel index until grouping
		}
	};
	auto stage = [&](bool hit, uint32_t s, uint64_t offset, uint32_t aa_rx, uint32_t hdr) {
		const uint64_t mask = __ballot(hit);
		if (!mask)
			return;
		if (q_tail - q_head + 64 > LD_RING)
			flush(64);
		if (hit) {
			const uint32_t slot = q_tail + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
			uint4 rec;
			rec.x = (uint32_t)offset;
			rec.y = (uint32_t)(offset >> 32);
			rec.z = aa_rx;
			rec.w = hdr | (s << 16);
			ring[slot & (LD_RING - 1)] = rec;
		}
		q_tail += (uint32_t)__popcll(mask);
	};
	auto fetch = [&](uint32_t ft, uint32_t fstream) { fetch_run<LE_TILE_WORDS>(a, ft, fstream, lw * 8u, nw); };
	fetch(t, stream);
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
		// the stream's channel: its index, and the sixteen whitening bits that lie on a header (wave-uniform)
		const uint32_t ch = le_channel_index(a.phys[this_stream]);
		const uint32_t ph0 = wh_phase[(ch & 0x3fu) | 0x40u], ph1 = ph0 + 8 >= 127 ? ph0 + 8 - 127 : ph0 + 8;
		const uint32_t wh16 = (uint32_t)wh_seq[ph0] | ((uint32_t)wh_seq[ph1] << 8);
		{
			uint32_t rfu[3];
#pragma unroll
			for (int k = 0; k < 3; k++) {
				rfu[k] = ((wh16 >> (5 + k)) & 1u) ? 0xffffffffu : 0u;
				asm volatile("" : "+v"(rfu[k]));            // (VGPR copies: a VALU op with an SGPR source issues at half rate)
			}
			uint32_t X[NCH + 1];
#pragma unroll
			for (int k = 0; k <= NCH; k++)
				X[k] = D[k] ^ alignbit(D[k + 1], D[k], 1);
#pragma unroll
			for (int c = 0; c < NCH; c++) {
				uint32_t p[8];
				p[0] = X[c];
#pragma unroll
				for (int j = 1; j < 8; j++)
					p[j] = alignbit(X[c + 1], X[c], j);
				const uint32_t t0 = BITOP3(p[0], p[1], p[2], 0x80), t1 = BITOP3(p[3], p[4], p[5], 0x80);
				m[c] = BITOP3(p[6], p[7], t0, 0x80) & t1;
				// the three RFU bits of h0 (window bits 45 .. 47) against the stream's whitening bits: all three equal
				const uint32_t r5 = alignbit(D[c + 2], D[c + 1], 13) ^ rfu[0], r6 = alignbit(D[c + 2], D[c + 1], 14) ^ rfu[1];
				const uint32_t r7 = alignbit(D[c + 2], D[c + 1], 15) ^ rfu[2];
				m[c] &= ~BITOP3(r5, r6, r7, 0xfe);
			}
		}
		if (ch >= 37) {                                 // an advertising channel (or no channel at all): no candidates
#pragma unroll
			for (int c = 0; c < NCH; c++)
				m[c] = 0;
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
				const uint32_t hdr = ((hi >> 8) & 0xffffu) ^ wh16;         // dewhitened h0 | h1 << 8
				const uint64_t offset = word0 * 64 + 32u * c + p;
				const bool hit = m[c] != 0 && (hdr & 3u) != 0 && (hdr & 0xe0u) == 0 && (hdr >> 8) <= a.max_len &&
						 offset + 80 + 8 * (hdr >> 8) <= total_bits;
				m[c] &= m[c] - 1;
				stage(hit, this_stream, offset, (lo >> 8) | (hi << 24), hdr);
			}
		}
	}
	while (q_tail != q_head)
		flush(q_tail - q_head < 64 ? q_tail - q_head : 64);
}

static int le_disc_launch_scan(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, uint64_t search_bits,
			       const uint16_t *d_phys, uint32_t max_len, btbbx_le_cand *d_cands, uint32_t cand_cap, uint32_t *d_count,
			       hipStream_t q)
{
	if (search_bits == 0)
		return BTBBX_OK;
	LeDiscArgs a;
	a.words = d_words;
	a.n_words = n_words;
	a.pitch_words = n_streams > 1 ? pitch_words : n_words;
	a.search_bits = search_bits;
	a.n_streams = n_streams;
	a.max_len = max_len;
	a.phys = d_phys;
	a.cands = d_cands;
	a.cand_cap = cand_cap;
	a.cand_count = d_count;
	TileGrid g;
	const int rc = tile_grid("btbbx_le_discover_scan_device", search_bits, n_words, n_streams, LE_TILE_WORDS, ctx().num_cus, &g);
	if (rc)
		return rc;
	a.full_tiles = g.full_tiles;
	a.tiles_per_stream = (uint32_t)g.tiles_per_stream;
	hipLaunchKernelGGL(le_disc_scan_kernel, dim3(g.grid), dim3(LE_THREADS), 0, q, a);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

static int le_disc_check_args(const char *who, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, uint64_t search_bits,
			      uint32_t max_len)
{
	if (max_len > 255) {
		set_error("%s: max_len must be 0..255", who);
		return BTBBX_E_ARG;
	}
	return check_scan_args(who, 40, n_words, pitch_words, n_streams, search_bits);
}

extern "C" int btbbx_le_discover_scan_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
					     uint64_t search_bits, const uint16_t *d_phys_channel, uint32_t max_len,
					     btbbx_le_cand *d_cands, uint32_t cand_cap, uint32_t *d_cand_count, void *hip_stream)
{
	const char *who = "btbbx_le_discover_scan_device";
	int rc = le_disc_check_args(who, n_words, pitch_words, n_streams, search_bits, max_len);
	if (rc)
		return rc;
	if (!d_words || !d_phys_channel || !d_cand_count || (!d_cands && cand_cap)) {
		set_error("%s: null pointer", who);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_cands & 7) || ((uintptr_t)d_cand_count & 3) || ((uintptr_t)d_words & 7) || ((uintptr_t)d_phys_channel & 1)) {
		set_error("%s: misaligned pointer (words and candidates 8 bytes, the counter 4)", who);
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	return le_disc_launch_scan(d_words, n_words, pitch_words, n_streams, search_bits, d_phys_channel, max_len, d_cands, cand_cap,
				   d_cand_count, (hipStream_t)hip_stream);
}

// ---- 2. grouping ------------------------------------------------------------------------------------------------------

struct LeDiscLayout {
	size_t params, keys[2], vals[2], hist, tot, tiles, qtiles, gstart, gid, cidx, sorted, total;
	uint32_t sort_blocks, grp_tiles;
};

static size_t ld_up(size_t x) { return (x + 255) & ~(size_t)255; }

static LeDiscLayout le_disc_layout(uint32_t cap)
{
	LeDiscLayout L;
	const size_t c = cap ? cap : 1;
	L.sort_blocks = radix_sort_blocks(c);
	L.grp_tiles = (uint32_t)((c + LD_GRP_TILE - 1) / LD_GRP_TILE);
	size_t at = 0;
	auto take = [&](size_t bytes) { const size_t here = at; at += ld_up(bytes); return here; };
	L.params = take(256);
	L.keys[0] = take(c * 8);
	L.keys[1] = take(c * 8);
	L.vals[0] = take(c * 4);
	L.vals[1] = take(c * 4);
	L.hist = take((size_t)L.sort_blocks * 256 * 4);
	L.tot = take(256 * 4);
	L.tiles = take(((size_t)L.grp_tiles + 1) * 4);
	L.qtiles = take(((size_t)L.grp_tiles + 1) * 4);
	L.gstart = take((c + 1) * 4);
	L.gid = take(c * 4);
	L.cidx = take(c * 4);
	L.sorted = take(c * sizeof(btbbx_le_cand));
	L.total = at;
	return L;
}

// (LdCand and ld_load: le_slots.h, which the coded tracking's unit includes as well)

__device__ __forceinline__ void ld_store(btbbx_le_cand *c, uint32_t i, const LdCand &r)
{
	uint2 *p = reinterpret_cast<uint2 *>(c + i);
	p[0] = r.a;
	p[1] = r.b;
	p[2] = r.c;
}

// params[0] = candidates to work on; first sort key = stream << 48 | offset, with the candidate's index
__global__ __launch_bounds__(LE_THREADS) void le_disc_key_kernel(const btbbx_le_cand *cands, const uint32_t *d_count, uint32_t cap,
								  uint32_t *params, uint64_t *keys, uint32_t *vals)
{
	const uint32_t have = *d_count, n = have < cap ? have : cap;
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x;
	if (i == 0)
		params[0] = n;
	if (i >= n)
		return;
	const LdCand r = ld_load(cands, i);
	keys[i] = ((uint64_t)(r.c.x & 0xffffu) << 48) | ((((uint64_t)r.a.y << 32) | r.a.x) & 0xffffffffffffULL);
	vals[i] = i;
}

// second sort key, of the list in (stream, offset) order: AA << 24 | CRCInit
__global__ __launch_bounds__(LE_THREADS) void le_disc_rekey_kernel(const btbbx_le_cand *cands, const uint32_t *params, const uint32_t *vals,
								    uint64_t *keys)
{
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x;
	if (i >= params[0])
		return;
	const uint2 b = reinterpret_cast<const uint2 *>(cands + vals[i])[1];
	keys[i] = ((uint64_t)b.x << 24) | (b.y & 0xffffffu);
}

__device__ __forceinline__ bool ld_first_of_group(const uint64_t *keys, uint32_t i, uint32_t n)
{
	return i < n && (i == 0 || keys[i] != keys[i - 1]);
}

// groups that begin in every tile of LD_GRP_TILE candidates
__global__ __launch_bounds__(LE_THREADS) void le_disc_mark_kernel(const uint64_t *keys, const uint32_t *params, uint32_t *tiles)
{
	__shared__ uint32_t count;
	const uint32_t tid = threadIdx.x, n = params[0];
	if (tid == 0)
		count = 0;
	__syncthreads();
	uint32_t mine = 0;
	for (uint32_t k = 0; k < LD_GRP_TILE / LE_THREADS; k++)
		mine += ld_first_of_group(keys, blockIdx.x * LD_GRP_TILE + k * LE_THREADS + tid, n) ? 1u : 0u;
	if (mine)
		atomicAdd(&count, mine);
	__syncthreads();
	if (tid == 0)
		tiles[blockIdx.x] = count;
}

// one workgroup: tile counts -> exclusive prefix sums.  Groups (conn_count null): their number goes to params[1] and, as the end
// of the last group, gstart[groups] = n.  Connections: their number goes to params[2] and *conn_count
__global__ __launch_bounds__(LE_THREADS) void le_disc_prefix_kernel(uint32_t *tiles, uint32_t n_tiles, uint32_t *params, uint32_t *gstart,
								     uint32_t *conn_count)
{
	__shared__ uint32_t lds[LD_WAVES];
	uint32_t carry = 0;
	for (uint32_t base = 0; base < n_tiles; base += LE_THREADS) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t v = i < n_tiles ? tiles[i] : 0;
		uint32_t sum;
		const uint32_t ex = block_exclusive_scan<LD_WAVES>(v, lds, sum);
		if (i < n_tiles)
			tiles[i] = carry + ex;
		carry += sum;
	}
	if (threadIdx.x == 0) {
		if (conn_count) {
			params[2] = carry;
			*conn_count = carry;
		} else {
			params[1] = carry;
			gstart[carry] = params[0];
		}
	}
}

// gstart[g] = first candidate of group g, gid[i] = group of candidate i
__global__ __launch_bounds__(LE_THREADS) void le_disc_starts_kernel(const uint64_t *keys, const uint32_t *params, const uint32_t *tiles,
								     uint32_t *gstart, uint32_t *gid)
{
	__shared__ uint32_t lds[LD_WAVES];
	const uint32_t tid = threadIdx.x, n = params[0];
	uint32_t carry = tiles[blockIdx.x];
	for (uint32_t k = 0; k < LD_GRP_TILE / LE_THREADS; k++) {
		const uint32_t i = blockIdx.x * LD_GRP_TILE + k * LE_THREADS + tid;
		const bool first = ld_first_of_group(keys, i, n);
		uint32_t sum;
		const uint32_t ex = block_exclusive_scan<LD_WAVES>(first ? 1u : 0u, lds, sum);
		const uint32_t g = carry + ex + (first ? 1u : 0u) - 1u;            // (i < n: some candidate at or before i is a first one)
		carry += sum;
		if (i < n) {
			gid[i] = g;
			if (first)
				gstart[g] = i;
		}
	}
}

__device__ __forceinline__ bool ld_qualifies(const uint32_t *gstart, uint32_t g, uint32_t n_groups, uint32_t min_count)
{
	return g < n_groups && gstart[g + 1] - gstart[g] >= min_count;
}

// groups of min_count or more in every tile of LD_GRP_TILE groups
__global__ __launch_bounds__(LE_THREADS) void le_disc_qmark_kernel(const uint32_t *gstart, const uint32_t *params, uint32_t min_count,
								    uint32_t *qtiles)
{
	__shared__ uint32_t count;
	const uint32_t tid = threadIdx.x, n_groups = params[1];
	if (tid == 0)
		count = 0;
	__syncthreads();
	uint32_t mine = 0;
	for (uint32_t k = 0; k < LD_GRP_TILE / LE_THREADS; k++)
		mine += ld_qualifies(gstart, blockIdx.x * LD_GRP_TILE + k * LE_THREADS + tid, n_groups, min_count) ? 1u : 0u;
	if (mine)
		atomicAdd(&count, mine);
	__syncthreads();
	if (tid == 0)
		qtiles[blockIdx.x] = count;
}

// cidx[g] = connection index of group g (LD_NO_CONN: too small); the records of the first conn_cap connections, with empty tallies
__global__ __launch_bounds__(LE_THREADS) void le_disc_emit_kernel(const uint64_t *keys, const uint32_t *gstart, const uint32_t *params,
								   uint32_t min_count, const uint32_t *qtiles, uint32_t *cidx,
								   btbbx_le_conn *conns, uint32_t conn_cap)
{
	__shared__ uint32_t lds[LD_WAVES];
	const uint32_t tid = threadIdx.x, n_groups = params[1];
	uint32_t carry = qtiles[blockIdx.x];
	for (uint32_t k = 0; k < LD_GRP_TILE / LE_THREADS; k++) {
		const uint32_t g = blockIdx.x * LD_GRP_TILE + k * LE_THREADS + tid;
		const bool q = ld_qualifies(gstart, g, n_groups, min_count);
		uint32_t sum;
		const uint32_t ci = carry + block_exclusive_scan<LD_WAVES>(q ? 1u : 0u, lds, sum);
		carry += sum;
		if (g >= n_groups)
			continue;
		cidx[g] = q ? ci : LD_NO_CONN;
		if (q && ci < conn_cap) {
			const uint32_t first = gstart[g];
			const uint64_t key = keys[first];
			btbbx_le_conn r;
			r.access_address = (uint32_t)(key >> 24);
			r.crc_init = (uint32_t)key & 0xffffffu;
			r.n_packets = gstart[g + 1] - first;
			r.n_empty = 0;
			r.channel_mask = 0;
			r.first = first;
			conns[ci] = r;
		}
	}
}

// the list in sorted order with every candidate's connection index (in `sorted`; le_disc_copy_kernel moves it back), and every
// candidate's channel and empty PDU tallied into its connection: a wave whose candidates all belong to one connection (the waves
// of a large one) sends one atomic of each kind
__global__ __launch_bounds__(LE_THREADS) void le_disc_rewrite_kernel(const btbbx_le_cand *cands, const uint32_t *vals, const uint32_t *gid,
								      const uint32_t *cidx, const uint32_t *params, btbbx_le_conn *conns,
								      uint32_t conn_cap, btbbx_le_cand *sorted)
{
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0], lane = threadIdx.x & 63;
	uint32_t ci = LD_NO_CONN, lo = 0, hi = 0;
	bool empty = false;
	if (i < n) {
		LdCand r = ld_load(cands, vals[i]);
		const uint32_t ch = r.c.y & 63u;                 // the scan left the channel index where the connection index goes
		ci = cidx[gid[i]];
		r.c.y = ci;
		ld_store(sorted, i, r);
		lo = ch < 32 ? 1u << ch : 0u;
		hi = ch < 32 ? 0u : 1u << (ch - 32);
		empty = (r.c.x >> 24) == 0;
	}
	const bool tally = ci < conn_cap;                    // (LD_NO_CONN is below no cap)
	const uint32_t c0 = __shfl(ci, 0, 64);
	if (__ballot(tally && ci == c0) == ~0ULL) {
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
			lo |= __shfl_xor(lo, d, 64);
			hi |= __shfl_xor(hi, d, 64);
		}
		const uint32_t n_empty = (uint32_t)__popcll(__ballot(empty));
		if (lane == 0) {
			atomicOr((unsigned long long *)&conns[c0].channel_mask, ((unsigned long long)hi << 32) | lo);
			if (n_empty)
				atomicAdd(&conns[c0].n_empty, n_empty);
		}
	} else if (tally) {
		atomicOr((unsigned long long *)&conns[ci].channel_mask, ((unsigned long long)hi << 32) | lo);
		if (empty)
			atomicAdd(&conns[ci].n_empty, 1u);
	}
}

__global__ __launch_bounds__(LE_THREADS) void le_disc_copy_kernel(const btbbx_le_cand *sorted, const uint32_t *params, btbbx_le_cand *cands)
{
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x;
	if (i < params[0])
		ld_store(cands, i, ld_load(sorted, i));
}

extern "C" size_t btbbx_le_discover_scratch_bytes(uint32_t cand_cap)
{
	return le_disc_layout(cand_cap).total;
}

// the radix sort's buffers where a stage's layout L has them in its scratch s; params[0] holds the list's length
template <class Layout> static RadixBufs le_radix_bufs(char *s, const Layout &L, const uint32_t *params, uint32_t cap)
{
	return {{(uint64_t *)(s + L.keys[0]), (uint64_t *)(s + L.keys[1])}, {(uint32_t *)(s + L.vals[0]), (uint32_t *)(s + L.vals[1])},
		(uint32_t *)(s + L.hist), (uint32_t *)(s + L.tot), params, cap};
}

// a stable sort by the n_bytes low bytes of the keys, least significant first, from side cur; returns the side the list ends in
static int le_sort_bytes(const RadixBufs &b, int n_bytes, int cur, hipStream_t q)
{
	RadixPass passes[8];
	for (int p = 0; p < 8; p++)
		passes[p] = {0, 8u * p};
	return radix_sort_passes(b, nullptr, passes, n_bytes, cur, q);
}

static int le_disc_launch_group(btbbx_le_cand *d_cands, const uint32_t *d_count, uint32_t cap, uint32_t min_count, btbbx_le_conn *d_conns,
				uint32_t conn_cap, uint32_t *d_conn_count, void *d_scratch, hipStream_t q)
{
	const LeDiscLayout L = le_disc_layout(cap);
	char *s = (char *)d_scratch;
	uint32_t *params = (uint32_t *)(s + L.params), *tiles = (uint32_t *)(s + L.tiles), *qtiles = (uint32_t *)(s + L.qtiles);
	uint32_t *gstart = (uint32_t *)(s + L.gstart), *gid = (uint32_t *)(s + L.gid), *cidx = (uint32_t *)(s + L.cidx);
	btbbx_le_cand *sorted = (btbbx_le_cand *)(s + L.sorted);
	const RadixBufs b = le_radix_bufs(s, L, params, cap);
	const dim3 per_cand((cap + LE_THREADS - 1) / LE_THREADS), per_tile(L.grp_tiles), wg(LE_THREADS);
	hipLaunchKernelGGL(le_disc_key_kernel, per_cand, wg, 0, q, d_cands, d_count, cap, params, b.keys[0], b.vals[0]);
	// least significant first: the 48 offset bits and the stream number, then -- rekeyed -- CRCInit and the AA
	int cur = le_sort_bytes(b, 8, 0, q);
	hipLaunchKernelGGL(le_disc_rekey_kernel, per_cand, wg, 0, q, d_cands, params, b.vals[cur], b.keys[cur]);
	cur = le_sort_bytes(b, 7, cur, q);
	const uint64_t *keys = b.keys[cur];
	hipLaunchKernelGGL(le_disc_mark_kernel, per_tile, wg, 0, q, keys, params, tiles);
	hipLaunchKernelGGL(le_disc_prefix_kernel, dim3(1), wg, 0, q, tiles, L.grp_tiles, params, gstart, (uint32_t *)nullptr);
	hipLaunchKernelGGL(le_disc_starts_kernel, per_tile, wg, 0, q, keys, params, tiles, gstart, gid);
	hipLaunchKernelGGL(le_disc_qmark_kernel, per_tile, wg, 0, q, gstart, params, min_count, qtiles);
	hipLaunchKernelGGL(le_disc_prefix_kernel, dim3(1), wg, 0, q, qtiles, L.grp_tiles, params, gstart, d_conn_count);
	hipLaunchKernelGGL(le_disc_emit_kernel, per_tile, wg, 0, q, keys, gstart, params, min_count, qtiles, cidx, d_conns, conn_cap);
	hipLaunchKernelGGL(le_disc_rewrite_kernel, per_cand, wg, 0, q, d_cands, b.vals[cur], gid, cidx, params, d_conns, conn_cap, sorted);
	hipLaunchKernelGGL(le_disc_copy_kernel, per_cand, wg, 0, q, sorted, params, d_cands);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

extern "C" int btbbx_le_discover_group_device(btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap, uint32_t min_count,
					      btbbx_le_conn *d_conns, uint32_t conn_cap, uint32_t *d_conn_count,
					      void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
	const char *who = "btbbx_le_discover_group_device";
	const LeDiscLayout L = le_disc_layout(cand_cap);
	if (!d_conn_count || (cand_cap && (!d_cands || !d_cand_count || !d_scratch || scratch_bytes < L.total)) ||
	    (cand_cap && conn_cap && !d_conns)) {
		set_error("%s: null pointer, or scratch of %zu bytes needed and %zu given", who, L.total, scratch_bytes);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_scratch & 15) || ((uintptr_t)d_cands & 7) || ((uintptr_t)d_conns & 7) || ((uintptr_t)d_cand_count & 3) ||
	    ((uintptr_t)d_conn_count & 3)) {
		set_error("%s: misaligned pointer (scratch 16 bytes, candidates and connections 8, the counters 4)", who);
		return BTBBX_E_ARG;
	}
	int rc = ctx_require();
	if (rc)
		return rc;
	hipStream_t q = (hipStream_t)hip_stream;
	if (!cand_cap) {
		HIP_TRY(hipMemsetAsync(d_conn_count, 0, sizeof(uint32_t), q));
		return BTBBX_OK;
	}
	return le_disc_launch_group(d_cands, d_cand_count, cand_cap, min_count, d_conns, conn_cap, d_conn_count, d_scratch, q);
}
