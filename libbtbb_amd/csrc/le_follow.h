// le_follow.h -- LE following from CONNECT_IND (included by le.hip, behind le_csa2.h): the seed stage joins every connection the
// discovery stored with the CONNECT_IND that opened it; the follow stage gives every event its absolute connEventCounter, reads
// the LL control PDUs out of the streams, puts every channel map update in force at its instant, stops at a parameter update and
// checks every packet's channel against the prediction of the map in force.  The contract is in include/btbbx.h
// (btbbx_le_seed_device, btbbx_le_epoch_device), the reasoning in DESIGN 3.8.4.  All arithmetic is integer arithmetic.
//
// The tracking's records say where a member stands: pkts[i].rank is its place among its connection's members in time order and
// pkts[i].event its event, and the members of g are the candidates [first, first + n_packets).  So position first + rank of a
// SLOT table and position first + event of an EVENT table belong to one member and one event of g, with no sums in front:
//
//   0. le_seed_join_kernel      one wave per connection over the advertising records: rules 1-4 of the seed stage
//   1. le_epoch_init_kernel     N and K, the tables emptied, the per-connection tallies zeroed
//   2. le_epoch_slot_kernel     one lane per candidate: its slot; a control PDU's payload (12 octets at most) read from its stream
//      and dewhitened; the rank of the first LL_START_ENC_REQ by an atomic minimum
//   3. le_epoch_open_kernel     one lane per slot: the member that opens its event stores the anchor and the channel
//   4. le_epoch_step_kernel     one lane per event: c_f for the first counted event, k_e for those behind it, 0 elsewhere; then ONE
//      64-bit prefix sum over the table (le_track_prefix64_kernel, le_track_count_kernel): an event's counter is its sum less the
//      sum in front of its connection (modulo 2^64, so the sums of other connections may wrap)
//   5. le_epoch_stop_kernel     one lane per candidate: a valid parameter update lowers its connection's stop; TERMINATE
//   6. le_epoch_mark_kernel, le_epoch_list_kernel   the valid map updates that are not ignored, compacted in (connection, rank) order
//      (le_track_prefix_kernel between the two), sorted stably by I and then by the connection (radix_sort.h), gathered
//   7. le_epoch_predict_kernel  one lane per event: a binary search of its connection's updates: the map in force and the epoch;
//      both algorithms' predictions; the tallies, one atomic per connection and wave
//   8. le_epoch_verdict_kernel  one lane per connection: the algorithm, the record
//   9. le_epoch_pkt_kernel      one lane per candidate: the per-packet record
//
// No kernel keeps per-connection state in an array of fixed size, and the count of launches depends on conn_cap only through
// the radix passes over its bytes.  The kernels are extern "C", as in le_csa2.h.  Nothing here synchronises or reads back; the
// host wrapper is le_host.h's.  What the span stage (le_span.h) does in the same way is written here once, for both: lf_mark_tile and
// lf_list_tile, the sort of the update list, lf_predict, lf_tallies, lf_verdict, lf_pdu_kind, lf_pkt_event, and kernels 1-3, the
// rekey and the gather kernel, which the span stage launches as they are.
#pragma once
#include "le_csa2.h"

#define LF_NONE     0xffffffffu
#define LF_NO_STOP  0xffffffffffffffffULL
#define LF_CONTROL  1u                      // ctl.x bit 0: LLID 3 and length >= 1; bits 8..15 the opcode, 16..23 the length
#define LF_IS_PARAM (1u << 30)              // ctl.x: a valid parameter update in a counted event
#define LF_IS_MAP   (1u << 31)              // ctl.x: a valid map update that is not ignored

static_assert(sizeof(btbbx_le_seed) == 56 && offsetof(btbbx_le_seed, map) == 8 && offsetof(btbbx_le_seed, access_address) == 16 &&
	      offsetof(btbbx_le_seed, crc_init) == 20 && offsetof(btbbx_le_seed, request) == 24 && offsetof(btbbx_le_seed, interval) == 28 &&
	      offsetof(btbbx_le_seed, win_offset) == 30 && offsetof(btbbx_le_seed, latency) == 32 && offsetof(btbbx_le_seed, timeout) == 34 &&
	      offsetof(btbbx_le_seed, win_size) == 36 && offsetof(btbbx_le_seed, hop) == 37 && offsetof(btbbx_le_seed, sca) == 38 &&
	      offsetof(btbbx_le_seed, chsel) == 39 && offsetof(btbbx_le_seed, init_a) == 40 && offsetof(btbbx_le_seed, adv_a) == 46 &&
	      offsetof(btbbx_le_seed, tx_add) == 52 && offsetof(btbbx_le_seed, rx_add) == 53 && offsetof(btbbx_le_seed, flags) == 54 &&
	      offsetof(btbbx_le_seed, reserved) == 55, "btbbx_le_seed layout (libbtbb_amd.LE_SEED_DTYPE)");
static_assert(sizeof(btbbx_le_follow) == 48 && offsetof(btbbx_le_follow, counter_first) == 8 && offsetof(btbbx_le_follow, stop) == 12 &&
	      offsetof(btbbx_le_follow, n_before) == 16 && offsetof(btbbx_le_follow, n_on) == 20 && offsetof(btbbx_le_follow, n_off) == 24 &&
	      offsetof(btbbx_le_follow, n_beyond) == 28 && offsetof(btbbx_le_follow, n_control) == 32 &&
	      offsetof(btbbx_le_follow, n_map_updates) == 36 && offsetof(btbbx_le_follow, algorithm) == 40 &&
	      offsetof(btbbx_le_follow, flags) == 41 && offsetof(btbbx_le_follow, reserved) == 42,
	      "btbbx_le_follow layout (libbtbb_amd.LE_FOLLOW_DTYPE)");
static_assert(sizeof(btbbx_le_follow_pkt) == 12 && offsetof(btbbx_le_follow_pkt, epoch) == 4 && offsetof(btbbx_le_follow_pkt, kind) == 6 &&
	      offsetof(btbbx_le_follow_pkt, opcode) == 7 && offsetof(btbbx_le_follow_pkt, expected) == 8 &&
	      offsetof(btbbx_le_follow_pkt, on_hop) == 9 && offsetof(btbbx_le_follow_pkt, state) == 10 &&
	      offsetof(btbbx_le_follow_pkt, reserved) == 11, "btbbx_le_follow_pkt layout (libbtbb_amd.LE_FOLLOW_PKT_DTYPE)");

// what the passes gather per connection (scratch; set by le_epoch_init_kernel)
struct LfConn {
	unsigned long long stop;               // the smallest I of a valid parameter update
	uint32_t enc_rank;                     // rank of the first LL_START_ENC_REQ
	uint32_t on1, on2, n_pred;             // events on #1's / #2's prediction; events predicted
	uint32_t n_before, n_beyond, n_control, n_map;
	uint32_t last_pred;                    // 1 + the last predicted event
	uint32_t flags;                        // BTBBX_LE_FOLLOW_TERMINATED
	uint32_t pad[4];
};
static_assert(sizeof(LfConn) == 64, "LfConn");

// params[0] = candidates worked on (N), [1] = connections stored (K), [2] = N (the length le_track_count_kernel scans);
// uparams[0] = [2] = the updates listed (U)
struct LfLayout {
	size_t params, uparams, slot, econn, anchor, step, tiles64, ctl, evres, work, utiles, keys[2], vals[2], hist, tot, u_i, u_map, u_conn,
		s_i, s_map, total;
	uint32_t tiles_n;
};

static LfLayout le_follow_layout(uint32_t cand_cap, uint32_t conn_cap)
{
	LfLayout L;
	const size_t c = cand_cap ? cand_cap : 1, k = conn_cap ? conn_cap : 1;
	L.tiles_n = (uint32_t)((c + LT_TILE - 1) / LT_TILE);
	size_t at = 0;
	auto take = [&](size_t bytes) { const size_t here = at; at += ld_up(bytes); return here; };
	L.params = take(256);
	L.uparams = take(256);
	L.slot = take(c * 4);
	L.econn = take(c * 4);
	L.anchor = take(c * 8);
	L.step = take(c * 8);
	L.tiles64 = take(((size_t)L.tiles_n + 1) * 8);
	L.ctl = take(c * 16);
	L.evres = take(c * 16);
	L.work = take(k * sizeof(LfConn));
	L.utiles = take(((size_t)L.tiles_n + 1) * 4);
	L.keys[0] = take(c * 8);
	L.keys[1] = take(c * 8);
	L.vals[0] = take(c * 4);
	L.vals[1] = take(c * 4);
	L.hist = take((size_t)radix_sort_blocks(c) * 256 * 4);
	L.tot = take(256 * 4);
	L.u_i = take(c * 8);
	L.u_map = take(c * 8);
	L.u_conn = take(c * 4);
	L.s_i = take(c * 8);
	L.s_map = take(c * 8);
	L.total = at;
	return L;
}

// ---- 0. the seed stage ----------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t lf_le16(const uint8_t *b) { return b[0] | ((uint32_t)b[1] << 8); }

// rules 1 and 2 for one advertising record: a valid request; its AA, CRCInit and sort key offset << 16 | stream
__device__ __forceinline__ bool lf_request(const btbbx_le_pkt *r, uint32_t &aa, uint32_t &crc_init, unsigned long long &key)
{
	if (r->crc_ok != 1 || r->truncated != 0 || r->is_data != 0 || r->adv_type != 5 || r->length != 34)
		return false;
	const uint8_t *b = r->bytes;
	const uint32_t hop = b[39] & 0x1fu, interval = lf_le16(b + 28), win_size = b[25], win_offset = lf_le16(b + 26);
	const unsigned long long map = ((unsigned long long)b[34] | ((unsigned long long)b[35] << 8) | ((unsigned long long)b[36] << 16) |
					((unsigned long long)b[37] << 24) | ((unsigned long long)b[38] << 32)) & LC_MAP37;
	if (hop < 5 || hop > 16 || interval < 6 || interval > 3200 || __popcll(map) < 2 || win_size < 1 ||
	    win_size > (interval - 1 < 8 ? interval - 1 : 8u) || win_offset > interval)
		return false;
	aa = b[18] | ((uint32_t)b[19] << 8) | ((uint32_t)b[20] << 16) | ((uint32_t)b[21] << 24);
	crc_init = b[22] | ((uint32_t)b[23] << 8) | ((uint32_t)b[24] << 16);
	key = ((r->offset & LT_OFF_MASK) << 16) | r->stream;
	return true;
}

// one wave per connection: rule 3 over the M advertising records, sixty-four at a time; lane 0 writes the record
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_seed_join_kernel(const btbbx_le_pkt *adv, const uint32_t *d_adv_count, uint32_t adv_cap,
									     const btbbx_le_conn *conns, const uint32_t *d_conn_count, uint32_t conn_cap,
									     const btbbx_le_track *tracks, uint32_t unit_bits, btbbx_le_seed *seeds)
{
	const uint32_t lane = threadIdx.x & 63, g = blockIdx.x * LT_WAVES + (threadIdx.x >> 6);
	const uint32_t kh = *d_conn_count, k = kh < conn_cap ? kh : conn_cap, mh = *d_adv_count, m = mh < adv_cap ? mh : adv_cap;
	if (g >= k)
		return;
	const uint32_t my_aa = conns[g].access_address, my_init = conns[g].crc_init;
	const unsigned long long first_anchor = tracks[g].first_anchor;
	unsigned long long best = 0;                       // key + 1 of the best request so far, 0: none
	uint32_t best_j = 0;
	for (uint32_t j = lane; j < m; j += 64) {
		uint32_t aa, init;
		unsigned long long key;
		if (!lf_request(adv + j, aa, init, key) || aa != my_aa || init != my_init)
			continue;
		if (adv[j].offset + 352 > first_anchor)
			continue;
		if (key + 1 >= best) {                          // (j ascends: among equal keys the last one stays)
			best = key + 1;
			best_j = j;
		}
	}
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) {
		const unsigned long long o = lt_shfl_xor64(best, d);
		const uint32_t oj = __shfl_xor(best_j, d);
		if (o > best || (o == best && oj > best_j)) {
			best = o;
			best_j = oj;
		}
	}
	if (lane)
		return;
	uint2 *out = reinterpret_cast<uint2 *>(seeds + g);
	if (!best) {
#pragma unroll
		for (int w = 0; w < 7; w++)
			out[w] = make_uint2(0, 0);
		return;
	}
	const btbbx_le_pkt *r = adv + best_j;
	const uint8_t *b = r->bytes;
	btbbx_le_seed s;
	const uint32_t win_offset = lf_le16(b + 26);
	s.t0 = r->offset + 352 + (unsigned long long)unit_bits * (1u + win_offset);
	s.map = ((unsigned long long)b[34] | ((unsigned long long)b[35] << 8) | ((unsigned long long)b[36] << 16) |
		 ((unsigned long long)b[37] << 24) | ((unsigned long long)b[38] << 32)) & LC_MAP37;
	s.access_address = my_aa;
	s.crc_init = my_init;
	s.request = best_j;
	s.interval = (uint16_t)lf_le16(b + 28);
	s.win_offset = (uint16_t)win_offset;
	s.latency = (uint16_t)lf_le16(b + 30);
	s.timeout = (uint16_t)lf_le16(b + 32);
	s.win_size = b[25];
	s.hop = b[39] & 0x1fu;
	s.sca = b[39] >> 5;
	s.chsel = (b[4] >> 5) & 1u;
	for (int i = 0; i < 6; i++) {
		s.init_a[i] = b[6 + i];
		s.adv_a[i] = b[12 + i];
	}
	s.tx_add = (b[4] >> 6) & 1u;
	s.rx_add = (b[4] >> 7) & 1u;
	s.flags = BTBBX_LE_SEED_SEEDED;
	s.reserved = 0;
	seeds[g] = s;
}

extern "C" int btbbx_le_seed_device(const btbbx_le_pkt *d_adv, const uint32_t *d_adv_count, uint32_t adv_cap,
				    const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
				    const btbbx_le_track *d_tracks, uint32_t unit_bits, btbbx_le_seed *d_seeds, void *hip_stream)
{
	const char *who = "btbbx_le_seed_device";
	if (!d_adv_count || (!d_adv && adv_cap) || !d_conns || !d_conn_count || !d_tracks || !d_seeds || unit_bits < 2) {
		set_error("%s: null pointer, or unit_bits < 2", who);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_adv & 7) || ((uintptr_t)d_conns & 7) || ((uintptr_t)d_tracks & 7) || ((uintptr_t)d_seeds & 7) ||
	    ((uintptr_t)d_adv_count & 3) || ((uintptr_t)d_conn_count & 3)) {
		set_error("%s: misaligned pointer (records 8 bytes, the counters 4)", who);
		return BTBBX_E_ARG;
	}
	const int rc = ctx_require();
	if (rc)
		return rc;
	if (!conn_cap)
		return BTBBX_OK;
	hipLaunchKernelGGL(le_seed_join_kernel, dim3((conn_cap + LT_WAVES - 1) / LT_WAVES), dim3(LE_THREADS), 0, (hipStream_t)hip_stream, d_adv,
			   d_adv_count, adv_cap, d_conns, d_conn_count, conn_cap, d_tracks, unit_bits, d_seeds);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

// ---- the follow stage: shared pieces --------------------------------------------------------------------------------------

// MEMBERS: candidate i's connection g, its tracking record p and its connection's first list index, which is where g's slots
// and events begin.  A member whose slot or event would lie beyond the list (a list that breaks the grouping's promise) is none
__device__ __forceinline__ bool lf_member(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts, const btbbx_le_conn *conns, uint32_t i,
					  uint32_t n, uint32_t k, uint32_t &g, uint4 &p, uint32_t &first)
{
	g = reinterpret_cast<const uint2 *>(cands + i)[2].y;
	p = reinterpret_cast<const uint4 *>(pkts)[i];
	if (g >= k || p.x == LF_NONE)
		return false;
	const uint2 f = reinterpret_cast<const uint2 *>(conns + g)[3];
	if (f.y || f.x >= n)
		return false;
	first = f.x;
	return p.x < n - first && p.y < n - first;
}

__device__ __forceinline__ bool lf_seeded(const btbbx_le_seed *seeds, uint32_t g) { return seeds[g].flags & BTBBX_LE_SEED_SEEDED; }

// the counter of the event at table position q of a connection whose table begins at first
__device__ __forceinline__ unsigned long long lf_counter(const unsigned long long *step, uint32_t first, uint32_t q)
{
	return step[q] - (first ? step[first - 1] : 0ULL);
}

// eight whitening bits, the register advanced (the reflected register of le_decode_kernel)
__device__ __forceinline__ uint32_t lf_whiten8(uint32_t &ws)
{
	uint32_t o = 0;
#pragma unroll
	for (int b = 0; b < 8; b++) {
		o |= (ws & 1u) << b;
		if (ws & 1u)
			ws ^= 0x88u;
		ws >>= 1;
	}
	return o;
}

// rule 3's update test: delta = (instant - c) mod 2^16 < 32767; I = c + delta
__device__ __forceinline__ bool lf_instant(uint32_t instant, unsigned long long c, unsigned long long &at)
{
	const uint32_t delta = (instant - (uint32_t)c) & 0xffffu;
	at = c + delta;
	return delta < 32767u;
}

// ---- 1. init ----------------------------------------------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_epoch_init_kernel(const uint32_t *d_cand_count, uint32_t cand_cap,
									      const uint32_t *d_conn_count, uint32_t conn_cap, uint32_t *params,
									      uint32_t *uparams, uint32_t *slot, uint32_t *econn, LfConn *work)
{
	const uint32_t nh = *d_cand_count, kh = *d_conn_count;
	const uint32_t n = nh < cand_cap ? nh : cand_cap, k = kh < conn_cap ? kh : conn_cap;
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x;     // (the grid covers the larger of the two caps)
	if (i == 0) {
		params[0] = n;
		params[1] = k;
		params[2] = n;
		uparams[0] = uparams[2] = 0;
	}
	if (i < n) {
		slot[i] = LF_NONE;
		econn[i] = LF_NONE;
	}
	if (i < k) {
		uint4 *w = reinterpret_cast<uint4 *>(work + i);
		w[0] = make_uint4(0xffffffffu, 0xffffffffu, LF_NONE, 0);   // stop, enc_rank, on1
		w[1] = w[2] = w[3] = make_uint4(0, 0, 0, 0);
	}
}

// ---- 2. slots and control PDUs ----------------------------------------------------------------------------------------------

// (le_keyed.h has this kernel's keyed form, le_keyed_slot_kernel, and this payload reader as lk_octets: a change here is made there too)
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_epoch_slot_kernel(const uint64_t *words, uint64_t n_words, uint64_t pitch_words,
									      uint32_t n_streams, const btbbx_le_cand *cands,
									      const btbbx_le_track_pkt *pkts, const btbbx_le_conn *conns,
									      const uint32_t *params, uint32_t *slot, uint4 *ctl, LfConn *work)
{
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0], k = params[1];
	if (i >= n)
		return;
	uint32_t g, first;
	uint4 p, info = make_uint4(0, 0, 0, 0);
	if (lf_member(cands, pkts, conns, i, n, k, g, p, first)) {
		slot[first + p.x] = i;
		const LdCand c = ld_load(cands, i);
		const uint32_t stream = c.c.x & 0xffffu, h0 = (c.c.x >> 16) & 0xffu, len = c.c.x >> 24;
		if ((h0 & 3u) == 3u && len >= 1 && stream < n_streams) {
			const uint64_t *w = words + (uint64_t)stream * pitch_words;
			const uint64_t bit0 = ((((uint64_t)c.a.y << 32) | c.a.x) & LT_OFF_MASK) + 56;
			uint32_t ws = (p.w & 0x3fu) | 0x40u;
			lf_whiten8(ws);
			lf_whiten8(ws);                                 // (behind the two header octets)
			const uint32_t take = len < 12 ? len : 12;
			unsigned long long lo8 = 0;                     // payload octets 0..7
			uint32_t hi4 = 0;                               // and 8..11
			for (uint32_t j = 0; j < take; j++) {
				const uint64_t bit = bit0 + 8ull * j, wi = bit >> 6;
				const uint32_t sh = (uint32_t)(bit & 63);
				const uint64_t lo = wi < n_words ? w[wi] : 0;
				const uint64_t hi = sh > 56 && wi + 1 < n_words ? w[wi + 1] : 0;
				const uint32_t v = ((uint32_t)(((lo >> sh) | (sh ? hi << (64 - sh) : 0)) & 0xffu)) ^ lf_whiten8(ws);
				if (j < 8)
					lo8 |= (unsigned long long)v << (8 * j);
				else
					hi4 |= v << (8 * (j - 8));
			}
			const uint32_t opcode = (uint32_t)lo8 & 0xffu;
			info.x = LF_CONTROL | (opcode << 8) | (len << 16);
			if (opcode == 1 && len == 8) {                  // LL_CHANNEL_MAP_IND: ChM, Instant
				const unsigned long long map = (lo8 >> 8) & LC_MAP37;
				info.y = (uint32_t)(lo8 >> 48);
				info.z = (uint32_t)map;
				info.w = (uint32_t)(map >> 32);
			} else if (opcode == 0 && len == 12) {          // LL_CONNECTION_UPDATE_IND: ..., Instant
				info.y = hi4 >> 16;
			}
			atomicAdd(&work[g].n_control, 1u);
			if (opcode == 5 && len == 1)                    // LL_START_ENC_REQ
				atomicMin(&work[g].enc_rank, p.x);
		}
	}
	ctl[i] = info;
}

// ---- 3. events --------------------------------------------------------------------------------------------------------------

// the member in front of which its connection's time order changes the event stores anchor | channel << 56 and the connection
// (le_keyed.h has this kernel's keyed form, le_keyed_open_kernel: a change here is made there too)
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_epoch_open_kernel(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts,
									      const btbbx_le_conn *conns, const uint32_t *params,
									      const uint32_t *slot, uint64_t *anchor, uint32_t *econn)
{
	const uint32_t q = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0], k = params[1];
	if (q >= n)
		return;
	const uint32_t i = slot[q];
	if (i == LF_NONE)
		return;
	uint32_t g, first;
	uint4 p;
	if (!lf_member(cands, pkts, conns, i, n, k, g, p, first))
		return;
	bool open = q == first;
	if (!open) {
		const uint32_t before = slot[q - 1];
		open = before == LF_NONE || reinterpret_cast<const uint4 *>(pkts)[before].y != p.y;
	}
	if (!open)
		return;
	const uint2 a = reinterpret_cast<const uint2 *>(cands + i)[0];
	anchor[first + p.y] = ((((uint64_t)a.y << 32) | a.x) & LT_OFF_MASK) | ((uint64_t)(p.w & 0xffu) << 56);
	econn[first + p.y] = g;
}

// ---- 4. counters ------------------------------------------------------------------------------------------------------------

// rules 1 and 2: step[q] = c_f at the first event that is not BEFORE, k_e at those behind it, 0 at every other position
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_epoch_step_kernel(const uint64_t *anchor, const uint32_t *econn,
									      const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
									      const uint32_t *params, uint32_t unit_bits, uint32_t jitter_bits,
									      unsigned long long *step, unsigned long long *tiles64)
{
	__shared__ unsigned long long total;
	const uint32_t tid = threadIdx.x, n = params[0];
	if (tid == 0)
		total = 0;
	__syncthreads();
	unsigned long long mine = 0;
	for (uint32_t r = 0; r < LT_TILE / LE_THREADS; r++) {
		const uint32_t q = blockIdx.x * LT_TILE + r * LE_THREADS + tid;
		if (q >= n)
			break;
		const uint32_t g = econn[q];
		unsigned long long kk = 0;
		if (g != LF_NONE && lf_seeded(seeds, g)) {
			const unsigned long long t0 = seeds[g].t0, per = (unsigned long long)seeds[g].interval * unit_bits;
			const unsigned long long a = anchor[q] & LT_OFF_MASK;
			if (per && a + jitter_bits >= t0) {
				const uint32_t first = (uint32_t)conns[g].first;
				const unsigned long long prev = q > first && econn[q - 1] == g ? anchor[q - 1] & LT_OFF_MASK : 0;
				if (q > first && econn[q - 1] == g && prev + jitter_bits >= t0)
					kk = (a - prev + per / 2) / per;
				else
					kk = (a + jitter_bits - t0) / per;
			}
		}
		step[q] = kk;
		mine += kk;
	}
	if (mine)
		atomicAdd(&total, mine);
	__syncthreads();
	if (tid == 0)
		tiles64[blockIdx.x] = total;
}

// ---- 5. stop ----------------------------------------------------------------------------------------------------------------

// what rule 3 needs of a member of a SEEDED connection: whether its event is counted, and the event's counter
__device__ __forceinline__ bool lf_counted(const uint64_t *anchor, const unsigned long long *step, const btbbx_le_seed *seeds, uint32_t g,
					   uint32_t first, uint32_t event, uint32_t jitter_bits, unsigned long long &c)
{
	c = lf_counter(step, first, first + event);
	return (anchor[first + event] & LT_OFF_MASK) + jitter_bits >= seeds[g].t0;
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_epoch_stop_kernel(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts,
									      const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
									      const uint32_t *params, const uint64_t *anchor,
									      const unsigned long long *step, uint32_t jitter_bits, uint4 *ctl, LfConn *work)
{
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0], k = params[1];
	if (i >= n)
		return;
	const uint32_t x = ctl[i].x;
	if (!(x & LF_CONTROL))
		return;
	uint32_t g, first;
	uint4 p;
	if (!lf_member(cands, pkts, conns, i, n, k, g, p, first) || !lf_seeded(seeds, g) || p.x > work[g].enc_rank)
		return;
	const uint32_t opcode = (x >> 8) & 0xffu, len = (x >> 16) & 0xffu;
	if (opcode == 2 && len == 2)
		atomicOr(&work[g].flags, (uint32_t)BTBBX_LE_FOLLOW_TERMINATED);
	if (opcode != 0 || len != 12)
		return;
	unsigned long long c, at;
	if (lf_counted(anchor, step, seeds, g, first, p.y, jitter_bits, c) && lf_instant(ctl[i].y, c, at)) {
		atomicMin(&work[g].stop, at);
		ctl[i].x = x | LF_IS_PARAM;
	}
}

// ---- 6. the update list -----------------------------------------------------------------------------------------------------

// slot q holds a valid map update that is not ignored: its absolute instant
__device__ __forceinline__ bool lf_map_update(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts, const btbbx_le_conn *conns,
					      const btbbx_le_seed *seeds, const uint32_t *slot, const uint4 *ctl, const LfConn *work,
					      const uint64_t *anchor, const unsigned long long *step, uint32_t jitter_bits, uint32_t q, uint32_t n,
					      uint32_t k, uint32_t &i, uint32_t &g, unsigned long long &at)
{
	i = slot[q];
	if (i == LF_NONE)
		return false;
	const uint4 info = ctl[i];
	if ((info.x & 0xffffffu) != (LF_CONTROL | (1u << 8) | (8u << 16)))
		return false;
	uint32_t first;
	uint4 p;
	if (!lf_member(cands, pkts, conns, i, n, k, g, p, first) || !lf_seeded(seeds, g) || p.x > work[g].enc_rank)
		return false;
	unsigned long long c;
	if (!lf_counted(anchor, step, seeds, g, first, p.y, jitter_bits, c) || c >= work[g].stop)
		return false;
	return lf_instant(info.y, c, at) && __popc(info.z) + __popc(info.w) >= 2;
}

// The mark pass and the list pass of an update list, for this stage and for the span stage (le_span.h).  is_update(q, i, g, at, param)
// says whether slot q holds an update that is listed -- candidate i of connection g, in force at `at` -- and may set `param` for
// a slot whose candidate on_param(i, g) is to see.  The mark pass counts a tile's updates into utiles (32 or 64 bits wide, by the
// prefix sum that follows)
template <class Tile, class Pred> __device__ __forceinline__ void lf_mark_tile(uint32_t n, Tile *utiles, Pred is_update)
{
	__shared__ uint32_t count;
	const uint32_t tid = threadIdx.x;
	if (tid == 0)
		count = 0;
	__syncthreads();
	uint32_t mine = 0;
	for (uint32_t r = 0; r < LT_TILE / LE_THREADS; r++) {
		const uint32_t q = blockIdx.x * LT_TILE + r * LE_THREADS + tid;
		if (q >= n)
			break;
		uint32_t i, g;
		unsigned long long at;
		bool param;
		mine += is_update(q, i, g, at, param) ? 1u : 0u;
	}
	if (mine)
		atomicAdd(&count, mine);
	__syncthreads();
	if (tid == 0)
		utiles[blockIdx.x] = count;
}

// the updates in slot order, which is (connection, rank) order: update u gets the sort key I and its own index as the value.
// The list's length is uparams[0]: TOTAL_IN_PARAMS: le_track_prefix_kernel left it in uparams[2]; else the last tile's carry is it
template <bool TOTAL_IN_PARAMS, class Tile, class Pred, class OnParam>
__device__ __forceinline__ void lf_list_tile(uint32_t n, const Tile *utiles, uint32_t *uparams, uint4 *ctl, LfConn *work, uint64_t *keys,
					     uint32_t *vals, uint64_t *u_i, uint64_t *u_map, uint32_t *u_conn, Pred is_update, OnParam on_param)
{
	__shared__ uint32_t lds[LT_WAVES];
	const uint32_t tid = threadIdx.x;
	if (TOTAL_IN_PARAMS && blockIdx.x == 0 && tid == 0)
		uparams[0] = uparams[2];
	uint32_t carry = (uint32_t)utiles[blockIdx.x];
	for (uint32_t r = 0; r < LT_TILE / LE_THREADS; r++) {
		if (blockIdx.x * LT_TILE + r * LE_THREADS >= n)
			break;                                          // (uniform over the workgroup)
		const uint32_t q = blockIdx.x * LT_TILE + r * LE_THREADS + tid;
		uint32_t i = LF_NONE, g = LF_NONE;
		unsigned long long at = 0;
		bool param = false;
		const bool is = q < n && is_update(q, i, g, at, param);
		uint32_t sum;
		const uint32_t ex = block_exclusive_scan<LT_WAVES>(is ? 1u : 0u, lds, sum);
		if (is) {
			const uint32_t u = carry + ex;
			const uint4 info = ctl[i];
			keys[u] = at;
			vals[u] = u;
			u_i[u] = at;
			u_map[u] = ((uint64_t)info.w << 32) | info.z;
			u_conn[u] = g;
			ctl[i].x = info.x | LF_IS_MAP;
			atomicAdd(&work[g].n_map, 1u);
		}
		if (param)
			on_param(i, g);
		carry += sum;
	}
	if (!TOTAL_IN_PARAMS && blockIdx.x == gridDim.x - 1 && tid == 0)
		uparams[0] = uparams[2] = carry;
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_epoch_mark_kernel(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts,
									      const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
									      const uint32_t *params, const uint32_t *slot, const uint4 *ctl,
									      const LfConn *work, const uint64_t *anchor, const unsigned long long *step,
									      uint32_t jitter_bits, uint32_t *utiles)
{
	const uint32_t n = params[0], k = params[1];
	lf_mark_tile(n, utiles, [=](uint32_t q, uint32_t &i, uint32_t &g, unsigned long long &at, bool &) __attribute__((always_inline)) {
		return lf_map_update(cands, pkts, conns, seeds, slot, ctl, work, anchor, step, jitter_bits, q, n, k, i, g, at);
	});
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_epoch_list_kernel(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts,
									      const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
									      const uint32_t *params, const uint32_t *slot, uint4 *ctl, LfConn *work,
									      const uint64_t *anchor, const unsigned long long *step, uint32_t jitter_bits,
									      const uint32_t *utiles, uint32_t *uparams, uint64_t *keys, uint32_t *vals,
									      uint64_t *u_i, uint64_t *u_map, uint32_t *u_conn)
{
	const uint32_t n = params[0], k = params[1];
	lf_list_tile<true>(n, utiles, uparams, ctl, work, keys, vals, u_i, u_map, u_conn,
			   [=](uint32_t q, uint32_t &i, uint32_t &g, unsigned long long &at, bool &) __attribute__((always_inline)) {
				   return lf_map_update(cands, pkts, conns, seeds, slot, ctl, work, anchor, step, jitter_bits, q, n, k, i, g, at);
			   },
			   [](uint32_t, uint32_t) {});
}

// between the two sorts: the key becomes the connection
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_epoch_rekey_kernel(const uint32_t *uparams, const uint32_t *vals, const uint32_t *u_conn,
									       uint64_t *keys)
{
	const uint32_t j = blockIdx.x * LE_THREADS + threadIdx.x;
	if (j < uparams[0])
		keys[j] = u_conn[vals[j]];
}

// behind them: the list in (connection, I, rank) order; the connection stays in keys
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_epoch_gather_kernel(const uint32_t *uparams, const uint32_t *vals, const uint64_t *u_i,
										const uint64_t *u_map, uint64_t *s_i, uint64_t *s_map)
{
	const uint32_t j = blockIdx.x * LE_THREADS + threadIdx.x;
	if (j < uparams[0]) {
		s_i[j] = u_i[vals[j]];
		s_map[j] = u_map[vals[j]];
	}
}

// ---- 7. prediction ----------------------------------------------------------------------------------------------------------

// the first entry of the sorted list whose connection is not below g
__device__ __forceinline__ uint32_t lf_lower(const uint64_t *s_conn, uint32_t u, uint32_t g)
{
	uint32_t lo = 0, hi = u;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if ((uint32_t)s_conn[mid] < g)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}

// the first entry behind those of g with I <= c
__device__ __forceinline__ uint32_t lf_upper(const uint64_t *s_conn, const uint64_t *s_i, uint32_t u, uint32_t g, unsigned long long c)
{
	uint32_t lo = 0, hi = u;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2, cg = (uint32_t)s_conn[mid];
		if (cg < g || (cg == g && s_i[mid] <= c))
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}

// the lanes that hold `flag` counted over a run of lanes (one connection's events within the wave); the run's first lane adds them
__device__ __forceinline__ void lf_tally(bool head, uint64_t run, bool flag, uint32_t *of_mine)
{
	const uint64_t mask = __ballot(flag);
	if (!mask)
		return;
	const uint32_t count = (uint32_t)__popcll(mask & run);
	if (head && count)
		atomicAdd(of_mine, count);
}

// rules 4-6 for a counted event of connection g with counter c on channel ch: the updates in force and, unless the event lies
// beyond *stop, the channel either algorithm expects (0xff: none) and whether the event is on it.  Returns whether the event is
// predicted, that is, not BEYOND.  ev, on1 and on2 come in with the values of an event that is not; u = uparams[0].
// (Pointers, not values: what is read behind the search is not kept in registers over it)
struct LfEvent {
	uint32_t epoch, exp1, exp2;
};

__device__ __forceinline__ bool lf_predict(const btbbx_le_seed *s, const btbbx_le_conn *conn, uint32_t g, unsigned long long c,
					   const unsigned long long *stop, uint32_t ch, const uint64_t *s_conn, const uint64_t *s_i,
					   const uint64_t *s_map, uint32_t u, LfEvent &ev, bool &on1, bool &on2)
{
	const uint32_t lo = lf_lower(s_conn, u, g), hi = lf_upper(s_conn, s_i, u, g, c);
	ev.epoch = hi - lo;
	bool pred = false;
	if (c < *stop) {
		const unsigned long long map = (ev.epoch ? s_map[hi - 1] : s->map) & LC_MAP37;
		const uint32_t n_used = (uint32_t)__popcll(map);
		if (n_used) {
			const uint32_t un = (s->hop * (uint32_t)((c + 1) % 37ull)) % 37u;
			ev.exp1 = (map >> un) & 1 ? un : lt_nth_bit(map, un % n_used);
			uint32_t unmapped;
			ev.exp2 = lc_expected(lc_prn((uint32_t)c & 0xffffu, lc_channel_id(conn->access_address)), map, n_used, BTBBX_LE_CSA2_REMAP,
					      unmapped);
		}
		pred = true;
		on1 = ev.exp1 == ch;
		on2 = ev.exp2 == ch;
	}
	return pred;
}

// The tallies of one event per lane.  A connection's events stand side by side in the table, so within the wave they are a run
// of lanes that begins where the connection changes (a lane without a live event belongs to the run in front of it and holds no
// flag): one atomic per tally, run and wave, whether the wave lies within one connection or over thirty small ones.  gap / n_gap:
// the span stage's extra tally.  The last predicted event: only a lane whose neighbour does not continue its connection's run of
// predicted events asks
__device__ __forceinline__ void lf_tallies(uint32_t g, bool live, uint32_t lane, uint32_t e, bool before, bool gap, bool beyond, bool pred,
					   bool on1, bool on2, LfConn *work, uint32_t *n_gap)
{
	const uint32_t pg = __shfl_up(g, 1);
	const bool head = live && (lane == 0 || pg != g);
	const uint64_t heads = __ballot(head), upto = lane == 63 ? ~0ULL : (2ULL << lane) - 1;
	uint64_t run = 0;
	if (head) {
		const uint64_t behind = heads & ~upto;
		run = (behind ? (1ULL << __builtin_ctzll(behind)) - 1 : ~0ULL) & ~(upto >> 1);
	}
	LfConn *w = work + (live ? g : 0);
	lf_tally(head, run, before, &w->n_before);
	lf_tally(head, run, gap, n_gap);
	lf_tally(head, run, beyond, &w->n_beyond);
	lf_tally(head, run, pred, &w->n_pred);
	lf_tally(head, run, on1, &w->on1);
	lf_tally(head, run, on2, &w->on2);
	const uint32_t ng = __shfl_down(g, 1), np = __shfl_down(pred ? 1u : 0u, 1);
	if (pred && (lane == 63 || ng != g || !np))
		atomicMax(&work[g].last_pred, e + 1);
}

// the event at table position q; evres[q] = expected #1 | expected #2 << 8 | state << 16, epoch, counter, 0
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_epoch_predict_kernel(const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
										 const uint32_t *params, const uint32_t *uparams, const uint64_t *anchor,
										 const uint32_t *econn, const unsigned long long *step,
										 const uint64_t *s_conn, const uint64_t *s_i, const uint64_t *s_map,
										 uint32_t jitter_bits, uint4 *evres, LfConn *work)
{
	const uint32_t q = blockIdx.x * LE_THREADS + threadIdx.x, lane = threadIdx.x & 63, n = params[0];
	uint32_t g = LF_NONE;
	if (q < n)
		g = econn[q];
	const bool live = g != LF_NONE && lf_seeded(seeds, g);
	bool before = false, pred = false, beyond = false, on1 = false, on2 = false;
	uint32_t e = 0;
	if (live) {
		LfEvent ev = {0, 0xff, 0xff};
		const btbbx_le_seed s = seeds[g];
		const uint32_t first = (uint32_t)conns[g].first;
		const uint64_t a = anchor[q];
		e = q - first;
		uint32_t counter = 0, state = BTBBX_LE_STATE_BEFORE;
		before = (a & LT_OFF_MASK) + jitter_bits < s.t0;
		if (!before) {
			const unsigned long long c = lf_counter(step, first, q);
			pred = lf_predict(&s, conns + g, g, c, &work[g].stop, (uint32_t)(a >> 56), s_conn, s_i, s_map, uparams[0], ev, on1, on2);
			counter = (uint32_t)c;
			beyond = !pred;
			state = beyond ? BTBBX_LE_STATE_BEYOND : BTBBX_LE_STATE_COUNTED;
		}
		evres[q] = make_uint4(ev.exp1 | (ev.exp2 << 8) | (state << 16), ev.epoch, counter, 0);
	}
	// (no GAP in this stage: lf_tally leaves before it touches its pointer when no lane of the wave holds the flag)
	lf_tallies(g, live, lane, e, before, false, beyond, pred, on1, on2, work, nullptr);
}

// ---- 8. verdict -------------------------------------------------------------------------------------------------------------

// what a SEEDED connection's tallies w say: the algorithm and its events on the hop, the first counted event's counter, the map in
// force at the last predicted event, and SEEDED | COUNTED with the flags the passes gathered.  f = word 3 of the
// connection's record (first, as 64 bits)
struct LfVerdict {
	unsigned long long map;
	uint32_t algorithm, n_on, c_first, flags;
};

__device__ __forceinline__ LfVerdict lf_verdict(const LfConn &w, const btbbx_le_seed &s, uint2 f, uint32_t g, uint32_t n, const uint32_t *uparams,
						const unsigned long long *step, const uint64_t *s_conn, const uint64_t *s_map,
						const uint4 *evres)
{
	LfVerdict v;
	const bool counted = w.n_pred + w.n_beyond != 0;
	v.algorithm = s.chsel && w.on2 >= w.on1 ? 2u : 1u;
	v.n_on = v.algorithm == 2 ? w.on2 : w.on1;
	v.c_first = 0;
	v.map = s.map;
	if (counted && !f.y && f.x < n && w.n_before < n - f.x) {
		v.c_first = (uint32_t)lf_counter(step, f.x, f.x + w.n_before);
		if (w.last_pred) {
			const uint32_t epoch = evres[f.x + w.last_pred - 1].y;
			if (epoch)
				v.map = s_map[lf_lower(s_conn, uparams[0], g) + epoch - 1] & LC_MAP37;
		}
	}
	v.flags = BTBBX_LE_FOLLOW_SEEDED | (counted ? BTBBX_LE_FOLLOW_COUNTED : 0u) | w.flags;
	return v;
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_epoch_verdict_kernel(const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
										 const uint32_t *params, const uint32_t *uparams,
										 const unsigned long long *step, const uint64_t *s_conn,
										 const uint64_t *s_map, const uint4 *evres, const LfConn *work,
										 btbbx_le_follow *follows)
{
	const uint32_t g = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0];
	if (g >= params[1])
		return;
	uint2 *out = reinterpret_cast<uint2 *>(follows + g);
	if (!lf_seeded(seeds, g)) {
#pragma unroll
		for (int w = 0; w < 6; w++)
			out[w] = make_uint2(0, 0);
		return;
	}
	const LfConn w = work[g];
	const LfVerdict v = lf_verdict(w, seeds[g], reinterpret_cast<const uint2 *>(conns + g)[3], g, n, uparams, step, s_conn, s_map, evres);
	uint32_t flags = v.flags;
	if (w.stop != LF_NO_STOP)
		flags |= BTBBX_LE_FOLLOW_STOPPED;
	if (w.enc_rank != LF_NONE)
		flags |= BTBBX_LE_FOLLOW_ENCRYPTED;
	out[0] = make_uint2((uint32_t)v.map, (uint32_t)(v.map >> 32));
	out[1] = make_uint2(v.c_first, (uint32_t)w.stop);
	out[2] = make_uint2(w.n_before, v.n_on);
	out[3] = make_uint2(w.n_pred - v.n_on, w.n_beyond);
	out[4] = make_uint2(w.n_control, w.n_map);
	out[5] = make_uint2(v.algorithm | (flags << 8), 0);
}

// ---- 9. packets -------------------------------------------------------------------------------------------------------------

// the kind of the PDU whose control word is x, of the member with this rank; op: the opcode, 0xff where none can be read
__device__ __forceinline__ uint32_t lf_pdu_kind(uint32_t x, uint32_t rank, uint32_t enc_rank, uint32_t &op)
{
	const uint32_t opcode = (x >> 8) & 0xffu, len = (x >> 16) & 0xffu;
	uint32_t kind = BTBBX_LE_PDU_DATA;
	op = 0xff;
	if (x & LF_CONTROL) {
		if (rank > enc_rank) {
			kind = BTBBX_LE_PDU_OPAQUE;
		} else {
			op = opcode;
			kind = BTBBX_LE_PDU_CONTROL;
			if (opcode == 5 && len == 1)
				kind = BTBBX_LE_PDU_ENC_START;
			else if (opcode == 2 && len == 2)
				kind = BTBBX_LE_PDU_TERMINATE;
			else if (x & LF_IS_MAP)
				kind = BTBBX_LE_PDU_MAP_UPDATE;
			else if (x & LF_IS_PARAM)
				kind = BTBBX_LE_PDU_PARAM_UPDATE;
		}
	}
	return kind;
}

// what a member on channel ch of a SEEDED connection reads from its event's evres word; *algorithm: the connection's verdict
struct LfPktEvent {
	uint32_t state, epoch, counter, span, expected, on;
};

__device__ __forceinline__ void lf_pkt_event(uint4 ev, const uint8_t *algorithm, uint32_t ch, LfPktEvent &e)
{
	e.state = (ev.x >> 16) & 0xffu;
	e.epoch = ev.y < 0xffffu ? ev.y : 0xffffu;
	e.counter = ev.z;
	e.span = ev.w;
	if (e.state == BTBBX_LE_STATE_COUNTED) {
		e.expected = *algorithm == 2 ? (ev.x >> 8) & 0xffu : ev.x & 0xffu;
		e.on = e.expected == ch ? 1u : 0u;
	}
}

// (le_keyed.h has this kernel's keyed form, le_keyed_pkt_epoch_kernel: a change here is made there too)
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_epoch_pkt_kernel(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts,
									     const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
									     const uint32_t *params, const uint4 *ctl, const uint4 *evres,
									     const LfConn *work, const btbbx_le_follow *follows,
									     btbbx_le_follow_pkt *out)
{
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0], k = params[1];
	if (i >= n)
		return;
	uint32_t g, first, w0 = 0xffffffffu, w1 = 0xffffffffu, w2 = 0xffffffffu;
	uint4 p;
	if (lf_member(cands, pkts, conns, i, n, k, g, p, first)) {
		uint32_t op;
		const uint32_t kind = lf_pdu_kind(ctl[i].x, p.x, work[g].enc_rank, op);
		LfPktEvent e = {0, 0, 0, 0, 0xff, 0};
		if (lf_seeded(seeds, g))
			lf_pkt_event(evres[first + p.y], &follows[g].algorithm, p.w & 0xffu, e);
		w0 = e.counter;
		w1 = e.epoch | (kind << 16) | (op << 24);
		w2 = e.expected | (e.on << 8) | (e.state << 16);
	}
	uint32_t *o = reinterpret_cast<uint32_t *>(out + i);
	o[0] = w0;
	o[1] = w1;
	o[2] = w2;
}

// ---- host side ------------------------------------------------------------------------------------------------------------

extern "C" size_t btbbx_le_epoch_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap)
{
	return le_follow_layout(cand_cap, conn_cap).total;
}

// the arrays of a run in its scratch, for this stage and for the span stage, whose own arrays stand behind them
struct LfBufs {
	uint32_t *params, *uparams, *slot, *econn, *utiles, *u_conn;
	uint64_t *anchor, *u_i, *u_map, *s_i, *s_map;
	unsigned long long *step, *tiles64;
	uint4 *ctl, *evres;
	LfConn *work;
	RadixBufs b;
	uint32_t tiles_n;
};

static LfBufs le_follow_bufs(void *d_scratch, uint32_t cap, uint32_t conn_cap)
{
	const LfLayout L = le_follow_layout(cap, conn_cap);
	char *s = (char *)d_scratch;
	LfBufs B;
	B.params = (uint32_t *)(s + L.params);
	B.uparams = (uint32_t *)(s + L.uparams);
	B.slot = (uint32_t *)(s + L.slot);
	B.econn = (uint32_t *)(s + L.econn);
	B.utiles = (uint32_t *)(s + L.utiles);
	B.u_conn = (uint32_t *)(s + L.u_conn);
	B.anchor = (uint64_t *)(s + L.anchor);
	B.u_i = (uint64_t *)(s + L.u_i);
	B.u_map = (uint64_t *)(s + L.u_map);
	B.s_i = (uint64_t *)(s + L.s_i);
	B.s_map = (uint64_t *)(s + L.s_map);
	B.step = (unsigned long long *)(s + L.step);
	B.tiles64 = (unsigned long long *)(s + L.tiles64);
	B.ctl = (uint4 *)(s + L.ctl);
	B.evres = (uint4 *)(s + L.evres);
	B.work = (LfConn *)(s + L.work);
	B.b = le_radix_bufs(s, L, B.uparams, cap);
	B.tiles_n = L.tiles_n;
	return B;
}

// How a run reads its control PDUs: the kernels that read a payload or say a PDU's kind.  This one reads them in the clear, with
// the kernels above.  le_keyed.h has the one that reads behind LL_START_ENC_REQ: the same number of launches, other kernels
struct LfReadClear {
	void tables(const LfBufs &B, const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, const btbbx_le_cand *d_cands,
		    const btbbx_le_track_pkt *d_pkts, const btbbx_le_conn *d_conns, dim3 per_cand, hipStream_t q) const
	{
		const dim3 wg(LE_THREADS);
		hipLaunchKernelGGL(le_epoch_slot_kernel, per_cand, wg, 0, q, d_words, n_words, pitch_words, n_streams, d_cands, d_pkts, d_conns, B.params,
				   B.slot, B.ctl, B.work);
		hipLaunchKernelGGL(le_epoch_open_kernel, per_cand, wg, 0, q, d_cands, d_pkts, d_conns, B.params, B.slot, B.anchor, B.econn);
	}
	void follow_pkts(const LfBufs &B, const btbbx_le_cand *d_cands, const btbbx_le_track_pkt *d_pkts, const btbbx_le_conn *d_conns,
			 const btbbx_le_seed *d_seeds, btbbx_le_follow *d_follows, btbbx_le_follow_pkt *d_fpkts, dim3 per_cand, hipStream_t q) const
	{
		hipLaunchKernelGGL(le_epoch_pkt_kernel, per_cand, dim3(LE_THREADS), 0, q, d_cands, d_pkts, d_conns, d_seeds, B.params, B.ctl, B.evres,
				   B.work, d_follows, d_fpkts);
	}
};

// kernels 1-3: the tables every later pass of this stage and of the span stage reads
template <class Read>
static void le_follow_open(const LfBufs &B, const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			   const btbbx_le_cand *d_cands, const uint32_t *d_count, uint32_t cap, const btbbx_le_conn *d_conns,
			   const uint32_t *d_conn_count, uint32_t conn_cap, const btbbx_le_track_pkt *d_pkts, hipStream_t q, const Read &read)
{
	const dim3 per_cand((cap + LE_THREADS - 1) / LE_THREADS), wg(LE_THREADS);
	const uint32_t init_grid = (uint32_t)(((uint64_t)std::max(cap, conn_cap) + LE_THREADS - 1) / LE_THREADS);
	hipLaunchKernelGGL(le_epoch_init_kernel, dim3(init_grid), wg, 0, q, d_count, cap, d_conn_count, conn_cap, B.params, B.uparams, B.slot, B.econn,
			   B.work);
	read.tables(B, d_words, n_words, pitch_words, n_streams, d_cands, d_pkts, d_conns, per_cand, q);
}

// the update list a list kernel left in side 0 of the sort's buffers, sorted stably by I -- least significant first: the 48 bits an
// absolute instant can have -- and then, rekeyed, by the connection index; gathered into s_i / s_map.  Returns s_conn
static const uint64_t *le_follow_sort_updates(const LfBufs &B, uint32_t cap, uint32_t conn_cap, hipStream_t q)
{
	const dim3 per_cand((cap + LE_THREADS - 1) / LE_THREADS), wg(LE_THREADS);
	int cur = le_sort_bytes(B.b, 6, 0, q);
	hipLaunchKernelGGL(le_epoch_rekey_kernel, per_cand, wg, 0, q, B.uparams, B.b.vals[cur], B.u_conn, B.b.keys[cur]);
	cur = le_sort_bytes(B.b, le_conn_passes(conn_cap), cur, q);
	hipLaunchKernelGGL(le_epoch_gather_kernel, per_cand, wg, 0, q, B.uparams, B.b.vals[cur], B.u_i, B.u_map, B.s_i, B.s_map);
	return B.b.keys[cur];
}

// the launches of one run: 12 of this stage's kernels, 3 of the tracking's scans, and 3 per radix pass (6 over I, 1 to 4 over conn_cap)
// (`read` chooses three of them: the slot, open and packet kernels, or le_keyed.h's in their places)
template <class Read = LfReadClear>
static int le_follow_launch(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, const btbbx_le_cand *d_cands,
			    const uint32_t *d_count, uint32_t cap, const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
			    const btbbx_le_track_pkt *d_pkts, const btbbx_le_seed *d_seeds, uint32_t unit_bits, uint32_t jitter_bits,
			    btbbx_le_follow *d_follows, btbbx_le_follow_pkt *d_fpkts, void *d_scratch, hipStream_t q, const Read &read = Read())
{
	const LfBufs B = le_follow_bufs(d_scratch, cap, conn_cap);
	const dim3 per_cand((cap + LE_THREADS - 1) / LE_THREADS), per_tile(B.tiles_n), wg(LE_THREADS);
	le_follow_open(B, d_words, n_words, pitch_words, n_streams, d_cands, d_count, cap, d_conns, d_conn_count, conn_cap, d_pkts, q, read);
	hipLaunchKernelGGL(le_epoch_step_kernel, per_tile, wg, 0, q, B.anchor, B.econn, d_conns, d_seeds, B.params, unit_bits, jitter_bits, B.step,
			   B.tiles64);
	hipLaunchKernelGGL(le_track_prefix64_kernel, dim3(1), wg, 0, q, B.tiles64, B.tiles_n);
	hipLaunchKernelGGL(le_track_count_kernel, per_tile, wg, 0, q, B.params, B.tiles64, B.step);
	hipLaunchKernelGGL(le_epoch_stop_kernel, per_cand, wg, 0, q, d_cands, d_pkts, d_conns, d_seeds, B.params, B.anchor, B.step, jitter_bits, B.ctl,
			   B.work);
	hipLaunchKernelGGL(le_epoch_mark_kernel, per_tile, wg, 0, q, d_cands, d_pkts, d_conns, d_seeds, B.params, B.slot, B.ctl, B.work, B.anchor,
			   B.step, jitter_bits, B.utiles);
	hipLaunchKernelGGL(le_track_prefix_kernel, dim3(1), wg, 0, q, B.utiles, B.tiles_n, B.uparams);
	hipLaunchKernelGGL(le_epoch_list_kernel, per_tile, wg, 0, q, d_cands, d_pkts, d_conns, d_seeds, B.params, B.slot, B.ctl, B.work, B.anchor,
			   B.step, jitter_bits, B.utiles, B.uparams, B.b.keys[0], B.b.vals[0], B.u_i, B.u_map, B.u_conn);
	const uint64_t *s_conn = le_follow_sort_updates(B, cap, conn_cap, q);
	hipLaunchKernelGGL(le_epoch_predict_kernel, per_cand, wg, 0, q, d_conns, d_seeds, B.params, B.uparams, B.anchor, B.econn, B.step, s_conn, B.s_i,
			   B.s_map, jitter_bits, B.evres, B.work);
	hipLaunchKernelGGL(le_epoch_verdict_kernel, dim3((conn_cap + LE_THREADS - 1) / LE_THREADS), wg, 0, q, d_conns, d_seeds, B.params, B.uparams,
			   B.step, s_conn, B.s_map, B.evres, B.work, d_follows);
	read.follow_pkts(B, d_cands, d_pkts, d_conns, d_seeds, d_follows, d_fpkts, per_cand, q);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

// the shape of the streams every _device entry that reads them refuses: this stage's and those of the span, data and decryption stages
static int le_check_streams(const char *who, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams)
{
	if (n_streams == 0) {
		set_error("%s: n_streams must be >= 1", who);
		return BTBBX_E_ARG;
	}
	if (n_words == 0 || (n_streams > 1 && pitch_words < n_words) || n_words > (1ull << 42)) {
		set_error("%s: n_words must be 1 .. 2^42 and pitch_words >= n_words", who);
		return BTBBX_E_ARG;
	}
	return BTBBX_OK;
}

extern "C" int btbbx_le_epoch_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				      const uint16_t *d_phys_channel,
				      const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
				      const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
				      const btbbx_le_track *d_tracks, const btbbx_le_track_pkt *d_pkts, const btbbx_le_seed *d_seeds,
				      uint32_t unit_bits, uint32_t jitter_bits,
				      btbbx_le_follow *d_follows, btbbx_le_follow_pkt *d_follow_pkts,
				      void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
	const char *who = "btbbx_le_epoch_device";
	int rc = le_track_check_args(who, n_streams, unit_bits, jitter_bits);
	if (!rc)
		rc = le_check_streams(who, n_words, pitch_words, n_streams);
	if (rc)
		return rc;
	const LfLayout L = le_follow_layout(cand_cap, conn_cap);
	if (!d_words || !d_phys_channel || !d_cands || !d_cand_count || !d_conns || !d_conn_count || !d_tracks || !d_pkts || !d_seeds ||
	    !d_follows || !d_follow_pkts || !d_scratch || scratch_bytes < L.total) {
		set_error("%s: null pointer, or scratch of %zu bytes needed and %zu given", who, L.total, scratch_bytes);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_words & 7) || ((uintptr_t)d_cands & 7) || ((uintptr_t)d_conns & 7) || ((uintptr_t)d_tracks & 7) ||
	    ((uintptr_t)d_pkts & 7) || ((uintptr_t)d_seeds & 7) || ((uintptr_t)d_follows & 7) || ((uintptr_t)d_follow_pkts & 3) ||
	    ((uintptr_t)d_scratch & 15) || ((uintptr_t)d_cand_count & 3) || ((uintptr_t)d_conn_count & 3) || ((uintptr_t)d_phys_channel & 1)) {
		set_error("%s: misaligned pointer (scratch 16 bytes, words and records 8, the packet records and counters 4, the channels 2)", who);
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	if (!cand_cap || !conn_cap)
		return BTBBX_OK;
	return le_follow_launch(d_words, n_words, pitch_words, n_streams, d_cands, d_cand_count, cand_cap, d_conns, d_conn_count, conn_cap, d_pkts,
				d_seeds, unit_bits, jitter_bits, d_follows, d_follow_pkts, d_scratch, (hipStream_t)hip_stream);
}
