// le_track.h -- LE connection tracking (included by le.hip, behind le_discover.h): for every connection the discovery stored, its
// events in time order, the connection interval, the event counter of every event, the hop increment, and for every packet
// whether it lies where channel selection algorithm #1 puts it.  The contract is in include/btbbx.h (btbbx_le_track_device), the
// reasoning in DESIGN 3.8.2.  All arithmetic is integer arithmetic.
//
//   1. le_track_init_kernel .. le_track_rekey_kernel   time order: a slot array of candidate indices sorted stably (radix_sort.h) by
//      offset << 16 | stream, then by the connection index (non-members last)
//   2. le_track_flag_kernel .. le_track_event_kernel   a flag where a slot opens an event, the flags' prefix sums: every slot's event, the
//      compact event list (anchor, channel, connection), every connection's first slot, first event and channel map
//   3. le_track_interval_kernel   q_e of every consecutive event pair; the gcd of a connection's fitting pairs by a segmented scan over
//      the lanes and one compare-and-swap per wave and connection (gcd is associative and commutative: any order gives the same)
//   4. le_track_step_kernel .. le_track_count_kernel   k_e of every pair and ONE 64-bit prefix sum over all events; an event's counter is
//      its sum less that of its connection's first event (modulo 2^64, so the sums of other connections may wrap)
//   5. le_track_score_kernel   for a fixed increment h an event votes for u = (v - h n_e) mod 37, v in V(C_e): 12 x 37 counters per
//      connection.  A tile of events that belongs to one connection votes into LDS and sends 37 sums, so a connection of any size
//      is spread over as many workgroups as it has tiles, twelve times
//   6. le_track_verdict_kernel   one wave per connection: argmax with the tie rule, the runner-up, the record
//   7. le_track_pkt_kernel   the per-packet records, and the events off the hop tallied with one atomic per wave where it can be
//
// Nothing here synchronises or reads back but the host wrapper.
#pragma once
#include "radix_sort.h"
#include "wave_scan.h"
#include "le_slots.h"
#include <string.h>

static_assert(LT_THREADS == LE_THREADS, "a slot pass's workgroup");
#define LT_TILE        2048u               // slots (or events) a workgroup scans per launch (8 rounds of 256)
static_assert(LT_TILE % LT_THREADS == 0, "whole rounds");
// (LT_INFO_EVENT and lt_member_of: le_slots.h)
#define LT_SCORE_TILE  1024u               // events a workgroup of the scoring pass votes for (4 rounds of 256)
#define LT_PAIRS       444u                // 12 hop increments x 37 first unmapped channels
#define LT_WAVES       (LE_THREADS / 64)
#define LT_OFF_MASK    0xffffffffffffULL   // the 48 offset bits the sort keys carry
#define LT_NO_CONN     0xffffffffu

static_assert(sizeof(btbbx_le_track) == 48 && offsetof(btbbx_le_track, map_mask) == 8 && offsetof(btbbx_le_track, n_events) == 16 &&
	      offsetof(btbbx_le_track, n_fit) == 20 && offsetof(btbbx_le_track, interval) == 24 && offsetof(btbbx_le_track, n_on_hop) == 28 &&
	      offsetof(btbbx_le_track, n_off_hop) == 32 && offsetof(btbbx_le_track, n_second) == 36 &&
	      offsetof(btbbx_le_track, hop_increment) == 40 && offsetof(btbbx_le_track, first_unmapped) == 41 &&
	      offsetof(btbbx_le_track, n_used) == 42 && offsetof(btbbx_le_track, flags) == 43 && offsetof(btbbx_le_track, reserved) == 44,
	      "btbbx_le_track layout (libbtbb_amd.LE_TRACK_DTYPE)");
static_assert(sizeof(btbbx_le_track_pkt) == 16 && offsetof(btbbx_le_track_pkt, event) == 4 && offsetof(btbbx_le_track_pkt, counter) == 8 &&
	      offsetof(btbbx_le_track_pkt, channel) == 12 && offsetof(btbbx_le_track_pkt, unmapped) == 13 &&
	      offsetof(btbbx_le_track_pkt, expected) == 14 && offsetof(btbbx_le_track_pkt, on_hop) == 15,
	      "btbbx_le_track_pkt layout (libbtbb_amd.LE_TRACK_PKT_DTYPE)");

// what the passes gather per connection (scratch; zeroed by le_track_init_kernel)
struct LtConn {
	unsigned long long gcd;                // of q_e over the fitting pairs so far (0: none)
	unsigned long long map;                // bit c: some event on data channel index c
	uint32_t slot0, ev0, ev1, n_fit;       // first slot; first event and the one behind the last; fitting pairs
};
static_assert(sizeof(LtConn) == 32, "LtConn");

// params[0] = candidates worked on (N), [1] = connections stored (K), [2] = events
struct LtLayout {
	size_t params, keys[2], vals[2], hist, tot, info, evidx, tiles, ekey, econn, step, tiles64, work, score, total;
	uint32_t tiles_n, score_tiles;
};

static LtLayout le_track_layout(uint32_t cand_cap, uint32_t conn_cap)
{
	LtLayout L;
	const size_t c = cand_cap ? cand_cap : 1, k = conn_cap ? conn_cap : 1;
	L.tiles_n = (uint32_t)((c + LT_TILE - 1) / LT_TILE);
	L.score_tiles = (uint32_t)((c + LT_SCORE_TILE - 1) / LT_SCORE_TILE);
	size_t at = 0;
	auto take = [&](size_t bytes) { const size_t here = at; at += ld_up(bytes); return here; };
	L.params = take(256);
	L.keys[0] = take(c * 8);
	L.keys[1] = take(c * 8);
	L.vals[0] = take(c * 4);
	L.vals[1] = take(c * 4);
	L.hist = take((size_t)radix_sort_blocks(c) * 256 * 4);
	L.tot = take(256 * 4);
	L.info = take(c * 4);
	L.evidx = take(c * 4);
	L.tiles = take(((size_t)L.tiles_n + 1) * 4);
	L.ekey = take(c * 8);
	L.econn = take(c * 4);
	L.step = take(c * 8);
	L.tiles64 = take(((size_t)L.tiles_n + 1) * 8);
	L.work = take(k * sizeof(LtConn));
	L.score = take(k * LT_PAIRS * 4);
	L.total = at;
	return L;
}

__device__ __forceinline__ unsigned long long lt_gcd(unsigned long long a, unsigned long long b)
{
	while (b) {
		const unsigned long long t = ((a | b) >> 32) ? a % b : (unsigned long long)((uint32_t)a % (uint32_t)b);
		a = b;
		b = t;
	}
	return a;
}

// the interval a connection's gathered gcd stands for, as the record stores it
__device__ __forceinline__ uint32_t lt_interval(unsigned long long gcd, uint32_t n_fit)
{
	return !n_fit ? 0u : ((gcd >> 32) ? 0xffffffffu : (uint32_t)gcd);
}

__device__ __forceinline__ bool lt_timed(uint32_t interval) { return interval >= 6 && interval <= 3200; }

// index of the k-th set bit of mask (k < popcount)
__device__ __forceinline__ uint32_t lt_nth_bit(unsigned long long mask, uint32_t k)
{
	for (uint32_t i = 0; i < k; i++)
		mask &= mask - 1;
	return (uint32_t)__builtin_ctzll(mask);
}

__device__ __forceinline__ unsigned long long lt_shfl_up64(unsigned long long v, int d)
{
	const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
	return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ unsigned long long lt_shfl_xor64(unsigned long long v, int d)
{
	const uint32_t lo = __shfl_xor((uint32_t)v, d), hi = __shfl_xor((uint32_t)(v >> 32), d);
	return ((unsigned long long)hi << 32) | lo;
}

// exclusive 64-bit prefix sum over the threads of a workgroup (block_exclusive_scan of wave_scan.h, 64 bits wide); ends with a barrier
__device__ __forceinline__ unsigned long long lt_block_scan64(unsigned long long v, unsigned long long *lds, unsigned long long &total)
{
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	unsigned long long inc = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned long long up = lt_shfl_up64(inc, d);
		if (lane >= (uint32_t)d)
			inc += up;
	}
	if (lane == 63)
		lds[wave] = inc;
	__syncthreads();
	unsigned long long before = 0, sum = 0;
	for (uint32_t w = 0; w < LT_WAVES; w++) {
		const unsigned long long t = lds[w];
		if (w < wave)
			before += t;
		sum += t;
	}
	total = sum;
	__syncthreads();
	return before + inc - v;
}

// ---- 1. time order ----------------------------------------------------------------------------------------------------

// the gathered figures and the score counters of the K connections that will be written
__global__ __launch_bounds__(LE_THREADS) void le_track_init_kernel(const uint32_t *d_conn_count, uint32_t conn_cap, LtConn *work, uint32_t *score)
{
	const uint32_t have = *d_conn_count, k = have < conn_cap ? have : conn_cap;
	const size_t n = (size_t)k * LT_PAIRS, stride = (size_t)gridDim.x * LE_THREADS;
	for (size_t i = (size_t)blockIdx.x * LE_THREADS + threadIdx.x; i < n; i += stride) {
		score[i] = 0;
		if (i < k) {
			LtConn w;
			w.gcd = w.map = 0;
			w.slot0 = w.ev0 = w.ev1 = w.n_fit = 0;
			work[i] = w;
		}
	}
}

// first sort key: offset << 16 | stream, with the candidate's index
__global__ __launch_bounds__(LE_THREADS) void le_track_key_kernel(const btbbx_le_cand *cands, const uint32_t *d_count, uint32_t cap,
								  const uint32_t *d_conn_count, uint32_t conn_cap, uint32_t *params,
								  uint64_t *keys, uint32_t *vals)
{
	const uint32_t have = *d_count, n = have < cap ? have : cap;
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x;
	if (i == 0) {
		const uint32_t kh = *d_conn_count;
		params[0] = n;
		params[1] = kh < conn_cap ? kh : conn_cap;
		params[2] = 0;
	}
	if (i >= n)
		return;
	const LdCand r = ld_load(cands, i);
	keys[i] = (((((uint64_t)r.a.y << 32) | r.a.x) & LT_OFF_MASK) << 16) | (r.c.x & 0xffffu);
	vals[i] = i;
}

// second sort key, of the slots in (offset, stream) order: the connection index, K for a candidate that is no member
__global__ __launch_bounds__(LE_THREADS) void le_track_rekey_kernel(const btbbx_le_cand *cands, const uint32_t *params, const uint32_t *vals,
								    const uint16_t *phys, uint32_t n_streams, uint64_t *keys)
{
	const uint32_t j = blockIdx.x * LE_THREADS + threadIdx.x;
	if (j >= params[0])
		return;
	uint32_t ch;
	keys[j] = lt_member_of(reinterpret_cast<const uint2 *>(cands + vals[j])[2], phys, n_streams, params[1], ch);
}

// ---- 2. events --------------------------------------------------------------------------------------------------------

// rule 3 for every slot against the slot in front of it; events that begin in every tile of LT_TILE slots
__global__ __launch_bounds__(LE_THREADS) void le_track_flag_kernel(const btbbx_le_cand *cands, const uint64_t *keys, const uint32_t *vals,
								   const uint32_t *params, const uint16_t *phys, uint32_t n_streams, uint32_t ifs_bits,
								   uint32_t *info, uint32_t *tiles)
{
	__shared__ uint32_t count;
	const uint32_t tid = threadIdx.x, n = params[0], k = params[1];
	if (tid == 0)
		count = 0;
	__syncthreads();
	uint32_t mine = 0;
	for (uint32_t r = 0; r < LT_TILE / LE_THREADS; r++) {
		const uint32_t j = blockIdx.x * LT_TILE + r * LE_THREADS + tid;
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
				const LdCand p = ld_load(cands, vals[j - 1]);
				lt_member_of(p.c, phys, n_streams, k, chp);
				const uint64_t off = ((uint64_t)me.a.y << 32) | me.a.x, end = (((uint64_t)p.a.y << 32) | p.a.x) + 80 + 8 * (p.c.x >> 24);
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

// one workgroup: tile counts -> exclusive prefix sums; their sum, the number of events, goes to params[2]
__global__ __launch_bounds__(LE_THREADS) void le_track_prefix_kernel(uint32_t *tiles, uint32_t n_tiles, uint32_t *params)
{
	__shared__ uint32_t lds[LT_WAVES];
	uint32_t carry = 0;
	for (uint32_t base = 0; base < n_tiles; base += LE_THREADS) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t v = i < n_tiles ? tiles[i] : 0;
		uint32_t sum;
		const uint32_t ex = block_exclusive_scan<LT_WAVES>(v, lds, sum);
		if (i < n_tiles)
			tiles[i] = carry + ex;
		carry += sum;
	}
	if (threadIdx.x == 0)
		params[2] = carry;
}

// evidx[j] = event of slot j; the event list: ekey[e] = anchor | channel << 56, econn[e] = connection; every connection's first slot,
// its events [ev0, ev1) and channel map
__global__ __launch_bounds__(LE_THREADS) void le_track_event_kernel(const btbbx_le_cand *cands, const uint64_t *keys, const uint32_t *vals,
								    const uint32_t *params, const uint32_t *info, const uint32_t *tiles,
								    uint32_t *evidx, uint64_t *ekey, uint32_t *econn, LtConn *work)
{
	__shared__ uint32_t lds[LT_WAVES];
	const uint32_t tid = threadIdx.x, lane = tid & 63, n = params[0], k = params[1];
	uint32_t carry = tiles[blockIdx.x];
	for (uint32_t r = 0; r < LT_TILE / LE_THREADS; r++) {
		if (blockIdx.x * LT_TILE + r * LE_THREADS >= n)
			break;                                          // (uniform over the workgroup)
		const uint32_t j = blockIdx.x * LT_TILE + r * LE_THREADS + tid;
		uint32_t c = LT_NO_CONN, v = 0;
		if (j < n) {
			c = (uint32_t)keys[j];
			v = info[j];
		}
		const bool member = c < k, open = member && (v & LT_INFO_EVENT);
		uint32_t sum;
		const uint32_t ex = block_exclusive_scan<LT_WAVES>(open ? 1u : 0u, lds, sum);
		const uint32_t e = carry + ex + (open ? 1u : 0u) - 1u;      // (a member: its connection's first slot, at or before it, opens an event)
		carry += sum;
		unsigned long long bit = 0;
		if (member) {
			evidx[j] = e;
			if (open) {
				const uint2 a = reinterpret_cast<const uint2 *>(cands + vals[j])[0];
				ekey[e] = ((((uint64_t)a.y << 32) | a.x) & LT_OFF_MASK) | ((uint64_t)(v & 0xffu) << 56);
				econn[e] = c;
				bit = 1ULL << (v & 0x3fu);
			}
			if (j == 0 || (uint32_t)keys[j - 1] != c) {
				work[c].slot0 = j;
				work[c].ev0 = e;
			}
			if (j + 1 == n || (uint32_t)keys[j + 1] != c)
				work[c].ev1 = e + 1;
		}
		// the map: a wave whose slots all belong to one connection (the waves of a large one) sends one atomic
		const uint32_t c0 = __shfl(c, 0, 64);
		if (__ballot(member && c == c0) == ~0ULL) {
#pragma unroll
			for (int d = 32; d >= 1; d >>= 1)
				bit |= lt_shfl_xor64(bit, d);
			if (lane == 0 && bit)
				atomicOr(&work[c0].map, bit);
		} else if (bit) {
			atomicOr(&work[c].map, bit);
		}
	}
}

// ---- 3. interval ------------------------------------------------------------------------------------------------------

// rule 4: one lane per event pair (e, e + 1) of one connection.  An inclusive scan over the lanes that stops at connection
// boundaries leaves every connection's gcd and fit count of this wave in its last lane, which folds them into the connection
__global__ __launch_bounds__(LE_THREADS) void le_track_interval_kernel(const uint64_t *ekey, const uint32_t *econn, const uint32_t *params,
								       uint32_t unit_bits, uint32_t jitter_bits, LtConn *work)
{
	const uint32_t e = blockIdx.x * LE_THREADS + threadIdx.x, lane = threadIdx.x & 63, n_ev = params[2];
	uint32_t c = LT_NO_CONN, fits = 0;
	unsigned long long g = 0;
	if (e < n_ev) {
		c = econn[e];
		if (e + 1 < n_ev && econn[e + 1] == c) {
			const uint64_t d = (ekey[e + 1] & LT_OFF_MASK) - (ekey[e] & LT_OFF_MASK);
			const uint64_t q = (d + unit_bits / 2) / unit_bits, m = q * unit_bits;
			if (q >= 1 && (d >= m ? d - m : m - d) <= jitter_bits) {
				g = q;
				fits = 1;
			}
		}
	}
	if (!__ballot(fits != 0))
		return;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned long long ug = lt_shfl_up64(g, d);
		const uint32_t uf = __shfl_up(fits, d), uc = __shfl_up(c, d);
		if (lane >= (uint32_t)d && uc == c) {               // (sorted by connection: lane - d in it means all lanes between are)
			if (ug)
				g = g ? lt_gcd(g, ug) : ug;
			fits += uf;
		}
	}
	const uint32_t next = __shfl_down(c, 1);
	if (fits && (lane == 63 || next != c)) {
		atomicAdd(&work[c].n_fit, fits);
		unsigned long long seen = __hip_atomic_load(&work[c].gcd, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		for (;;) {
			const unsigned long long want = seen ? lt_gcd(seen, g) : g;
			if (want == seen)
				break;
			const unsigned long long was = atomicCAS(&work[c].gcd, seen, want);
			if (was == seen)
				break;
			seen = was;
		}
	}
}

// ---- 4. counters ------------------------------------------------------------------------------------------------------

// rule 5: step[e] = k of the pair (e - 1, e) of a TIMED connection, 0 for a connection's first event; their sum per tile
__global__ __launch_bounds__(LE_THREADS) void le_track_step_kernel(const uint64_t *ekey, const uint32_t *econn, const uint32_t *params,
								   uint32_t unit_bits, const LtConn *work, unsigned long long *step,
								   unsigned long long *tiles64)
{
	__shared__ unsigned long long total;
	const uint32_t tid = threadIdx.x, n_ev = params[2];
	if (tid == 0)
		total = 0;
	__syncthreads();
	unsigned long long mine = 0;
	for (uint32_t r = 0; r < LT_TILE / LE_THREADS; r++) {
		const uint32_t e = blockIdx.x * LT_TILE + r * LE_THREADS + tid;
		if (e >= n_ev)
			break;
		const uint32_t c = econn[e];
		unsigned long long kk = 0;
		if (e > 0 && econn[e - 1] == c) {
			const uint32_t iv = lt_interval(work[c].gcd, work[c].n_fit);
			if (lt_timed(iv)) {
				const uint64_t p = (uint64_t)iv * unit_bits, d = (ekey[e] & LT_OFF_MASK) - (ekey[e - 1] & LT_OFF_MASK);
				kk = (d + p / 2) / p;
			}
		}
		step[e] = kk;
		mine += kk;
	}
	if (mine)
		atomicAdd(&total, mine);
	__syncthreads();
	if (tid == 0)
		tiles64[blockIdx.x] = total;
}

// one workgroup: tile sums -> exclusive prefix sums
__global__ __launch_bounds__(LE_THREADS) void le_track_prefix64_kernel(unsigned long long *tiles64, uint32_t n_tiles)
{
	__shared__ unsigned long long lds[LT_WAVES];
	unsigned long long carry = 0;
	for (uint32_t base = 0; base < n_tiles; base += LE_THREADS) {
		const uint32_t i = base + threadIdx.x;
		const unsigned long long v = i < n_tiles ? tiles64[i] : 0;
		unsigned long long sum;
		const unsigned long long ex = lt_block_scan64(v, lds, sum);
		if (i < n_tiles)
			tiles64[i] = carry + ex;
		carry += sum;
	}
}

// step[e] = the sum of all steps up to and including e's
__global__ __launch_bounds__(LE_THREADS) void le_track_count_kernel(const uint32_t *params, const unsigned long long *tiles64,
								    unsigned long long *step)
{
	__shared__ unsigned long long lds[LT_WAVES];
	const uint32_t tid = threadIdx.x, n_ev = params[2];
	unsigned long long carry = tiles64[blockIdx.x];
	for (uint32_t r = 0; r < LT_TILE / LE_THREADS; r++) {
		if (blockIdx.x * LT_TILE + r * LE_THREADS >= n_ev)
			break;                                          // (uniform over the workgroup)
		const uint32_t e = blockIdx.x * LT_TILE + r * LE_THREADS + tid;
		const unsigned long long v = e < n_ev ? step[e] : 0;
		unsigned long long sum;
		const unsigned long long ex = lt_block_scan64(v, lds, sum);
		if (e < n_ev)
			step[e] = carry + ex + v;
		carry += sum;
	}
}

// ---- 5. scoring -------------------------------------------------------------------------------------------------------

// rule 6, blockIdx.y = h - 5: event e of a TIMED connection votes for u = (v - h n_e) mod 37 for each v in V(C_e) -- C_e itself and,
// with REMAP, the unused v whose remapping index v mod n_used is C_e's position among the used channels.  A tile within one
// connection: 37 LDS counters, 37 atomics; a tile over several (small) connections: its votes go to their counters directly
__global__ __launch_bounds__(LE_THREADS) void le_track_score_kernel(const uint64_t *ekey, const uint32_t *econn, const unsigned long long *step,
								    const uint32_t *params, const LtConn *work, uint32_t flags, uint32_t *score)
{
	__shared__ uint32_t bins[37];
	const uint32_t tid = threadIdx.x, n_ev = params[2], base = blockIdx.x * LT_SCORE_TILE, h = 5 + blockIdx.y;
	if (base >= n_ev)
		return;
	const uint32_t last = base + LT_SCORE_TILE <= n_ev ? base + LT_SCORE_TILE - 1 : n_ev - 1;
	const uint32_t c_first = econn[base];
	const bool one = c_first == econn[last];
	if (tid < 37)
		bins[tid] = 0;
	__syncthreads();
	for (uint32_t r = 0; r < LT_SCORE_TILE / LE_THREADS; r++) {
		const uint32_t e = base + r * LE_THREADS + tid;
		if (e > last)
			break;
		const uint32_t c = econn[e];
		const LtConn w = work[c];
		if (!lt_timed(lt_interval(w.gcd, w.n_fit)))
			continue;
		const uint32_t ch = (uint32_t)(ekey[e] >> 56), hn = h * (uint32_t)((step[e] - step[w.ev0]) % 37ull);
		uint32_t *mine = score + (size_t)c * LT_PAIRS + (h - 5) * 37;
		auto vote = [&](uint32_t v) {
			const uint32_t u = (v + 16 * 37 - hn) % 37;                 // (h n <= 16 x 36 < 16 x 37)
			if (one)
				atomicAdd(&bins[u], 1u);
			else
				atomicAdd(&mine[u], 1u);
		};
		vote(ch);
		if (flags & BTBBX_LE_TRACK_REMAP) {
			const uint32_t n_used = (uint32_t)__popcll(w.map);
			for (uint32_t v = (uint32_t)__popcll(w.map & ((1ULL << ch) - 1)); v < 37; v += n_used)
				if (!((w.map >> v) & 1))
					vote(v);
		}
	}
	__syncthreads();
	if (one && tid < 37 && bins[tid])
		atomicAdd(&score[(size_t)c_first * LT_PAIRS + (h - 5) * 37 + tid], bins[tid]);
}

// ---- 6. verdict -------------------------------------------------------------------------------------------------------

// one wave per connection: the pair with the largest score, ties to the smallest h, then the smallest u (the smallest counter
// index); the largest score of any other pair; the record, every byte of it
__global__ __launch_bounds__(LE_THREADS) void le_track_verdict_kernel(const LtConn *work, const uint32_t *score, const uint64_t *ekey,
								      const uint32_t *params, btbbx_le_track *tracks)
{
	const uint32_t lane = threadIdx.x & 63, g = blockIdx.x * LT_WAVES + (threadIdx.x >> 6);
	if (g >= params[1])
		return;
	const LtConn w = work[g];
	const uint32_t n_events = w.ev1 - w.ev0, iv = lt_interval(w.gcd, w.n_fit);
	const bool timed = n_events && lt_timed(iv);
	uint32_t best = 0, best_at = 0, second = 0;
	if (timed) {
		const uint32_t *s = score + (size_t)g * LT_PAIRS;
		unsigned long long top = 0;
		for (uint32_t i = lane; i < LT_PAIRS; i += 64) {
			const unsigned long long key = ((unsigned long long)s[i] << 32) | (0xffffu - i);
			top = key > top ? key : top;
		}
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
			const unsigned long long o = lt_shfl_xor64(top, d);
			top = o > top ? o : top;
		}
		best = (uint32_t)(top >> 32);
		best_at = 0xffffu - ((uint32_t)top & 0xffffu);
		for (uint32_t i = lane; i < LT_PAIRS; i += 64)
			if (i != best_at)
				second = s[i] > second ? s[i] : second;
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) {
			const uint32_t o = __shfl_xor(second, d);
			second = o > second ? o : second;
		}
	}
	if (lane)
		return;
	btbbx_le_track t;
	t.first_anchor = n_events ? ekey[w.ev0] & LT_OFF_MASK : 0;
	t.map_mask = w.map;
	t.n_events = n_events;
	t.n_fit = w.n_fit;
	t.interval = iv;
	t.n_on_hop = best;
	t.n_off_hop = 0;                                        // (le_track_pkt_kernel tallies it)
	t.n_second = second;
	t.hop_increment = timed ? (uint8_t)(5 + best_at / 37) : 0;
	t.first_unmapped = timed ? (uint8_t)(best_at % 37) : 0;
	t.n_used = (uint8_t)__popcll(w.map);
	t.flags = timed ? (uint8_t)(BTBBX_LE_TRACK_TIMED | (best > second ? BTBBX_LE_TRACK_HOPPING : 0u)) : 0;
	t.reserved = 0;
	tracks[g] = t;
}

// ---- 7. packets -------------------------------------------------------------------------------------------------------

// rule 7: one lane per slot writes the record of the slot's candidate; a slot that opens an event off the hop counts in n_off_hop,
// one atomic for a wave whose slots all belong to one connection
__global__ __launch_bounds__(LE_THREADS) void le_track_pkt_kernel(const uint64_t *keys, const uint32_t *vals, const uint32_t *info,
								  const uint32_t *evidx, const unsigned long long *step, const uint32_t *params,
								  const LtConn *work, uint32_t flags, btbbx_le_track *tracks, btbbx_le_track_pkt *pkts)
{
	const uint32_t j = blockIdx.x * LE_THREADS + threadIdx.x, lane = threadIdx.x & 63, n = params[0], k = params[1];
	uint32_t c = LT_NO_CONN;
	bool off_hop = false;
	if (j < n) {
		c = (uint32_t)keys[j];
		uint4 out = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
		if (c < k) {
			const LtConn w = work[c];
			const uint32_t word = reinterpret_cast<const uint32_t *>(tracks + c)[10];    // hop_increment, first_unmapped, n_used, flags
			const uint32_t v = info[j], ch = v & 0xffu, e = evidx[j];
			uint32_t counter = 0, unmapped = 0xff, expected = 0xff, on = 0;
			if ((word >> 24) & BTBBX_LE_TRACK_TIMED) {
				const unsigned long long cnt = step[e] - step[w.ev0];
				counter = (uint32_t)cnt;
				unmapped = ((word >> 8 & 0xffu) + (word & 0xffu) * (uint32_t)(cnt % 37ull)) % 37;
				if ((w.map >> unmapped) & 1)
					expected = unmapped;
				else if (flags & BTBBX_LE_TRACK_REMAP)
					expected = lt_nth_bit(w.map, unmapped % (word >> 16 & 0xffu));
				on = expected == ch ? 1u : 0u;
				off_hop = (v & LT_INFO_EVENT) && expected != 0xff && !on;
			}
			out = make_uint4(j - w.slot0, e - w.ev0, counter, ch | (unmapped << 8) | (expected << 16) | (on << 24));
		}
		reinterpret_cast<uint4 *>(pkts)[vals[j]] = out;
	}
	const uint64_t off_mask = __ballot(off_hop);
	if (!off_mask)
		return;
	const uint32_t c0 = __shfl(c, 0, 64);
	if (__ballot(c == c0) == ~0ULL) {
		if (lane == 0)
			atomicAdd(&tracks[c0].n_off_hop, (uint32_t)__popcll(off_mask));
	} else if (off_hop) {
		atomicAdd(&tracks[c].n_off_hop, 1u);
	}
}

// ---- host side ----------------------------------------------------------------------------------------------------------

extern "C" size_t btbbx_le_track_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap)
{
	return le_track_layout(cand_cap, conn_cap).total;
}

static int le_track_check_args(const char *who, uint32_t n_streams, uint32_t unit_bits, uint32_t jitter_bits)
{
	if (n_streams == 0 || unit_bits < 2 || jitter_bits >= unit_bits / 2) {
		set_error("%s: n_streams must be >= 1, unit_bits >= 2 and jitter_bits < unit_bits / 2", who);
		return BTBBX_E_ARG;
	}
	return BTBBX_OK;
}

// the bytes of a connection index, whose largest value is conn_cap: the radix passes a sort by the connection takes
static int le_conn_passes(uint32_t conn_cap)
{
	int passes = 1;
	while (passes < 4 && (conn_cap >> (8 * passes)))
		passes++;
	return passes;
}

// the launches of one tracking run: 24 + 3 per eight bits of conn_cap for the two sorts, 13 of its own.  stand_in (null: the
// flag pass above) enqueues the flag pass in its place, as the coded tracking does, whose rule 3 reads a duration per candidate
static int le_track_launch(const btbbx_le_cand *d_cands, const uint32_t *d_count, uint32_t cap, const uint32_t *d_conn_count, uint32_t conn_cap,
			   const uint16_t *d_phys, uint32_t n_streams, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
			   btbbx_le_track *d_tracks, btbbx_le_track_pkt *d_pkts, void *d_scratch, hipStream_t q,
			   const LtFlagStandIn *stand_in = nullptr)
{
	const LtLayout L = le_track_layout(cap, conn_cap);
	char *s = (char *)d_scratch;
	uint32_t *params = (uint32_t *)(s + L.params), *info = (uint32_t *)(s + L.info), *evidx = (uint32_t *)(s + L.evidx);
	uint32_t *tiles = (uint32_t *)(s + L.tiles), *econn = (uint32_t *)(s + L.econn), *score = (uint32_t *)(s + L.score);
	uint64_t *ekey = (uint64_t *)(s + L.ekey);
	unsigned long long *step = (unsigned long long *)(s + L.step), *tiles64 = (unsigned long long *)(s + L.tiles64);
	LtConn *work = (LtConn *)(s + L.work);
	const RadixBufs b = le_radix_bufs(s, L, params, cap);
	const dim3 per_cand((cap + LE_THREADS - 1) / LE_THREADS), per_tile(L.tiles_n), wg(LE_THREADS);
	const size_t init_items = ((size_t)conn_cap * LT_PAIRS + LE_THREADS - 1) / LE_THREADS;
	hipLaunchKernelGGL(le_track_init_kernel, dim3((uint32_t)std::min<size_t>(init_items, 4096)), wg, 0, q, d_conn_count, conn_cap, work, score);
	hipLaunchKernelGGL(le_track_key_kernel, per_cand, wg, 0, q, d_cands, d_count, cap, d_conn_count, conn_cap, params, b.keys[0], b.vals[0]);
	// least significant first: the stream number and the 48 offset bits, then -- rekeyed -- the connection index, whose largest value is conn_cap
	int cur = le_sort_bytes(b, 8, 0, q);
	hipLaunchKernelGGL(le_track_rekey_kernel, per_cand, wg, 0, q, d_cands, params, b.vals[cur], d_phys, n_streams, b.keys[cur]);
	cur = le_sort_bytes(b, le_conn_passes(conn_cap), cur, q);
	const uint64_t *keys = b.keys[cur];
	const uint32_t *vals = b.vals[cur];
	if (stand_in) {
		const LtFlagPass pass = {d_cands, keys, vals, params, d_phys, n_streams, ifs_bits, info, tiles, L.tiles_n, LT_TILE, q};
		stand_in->enqueue(pass, stand_in->user);
	} else {
		hipLaunchKernelGGL(le_track_flag_kernel, per_tile, wg, 0, q, d_cands, keys, vals, params, d_phys, n_streams, ifs_bits, info, tiles);
	}
	hipLaunchKernelGGL(le_track_prefix_kernel, dim3(1), wg, 0, q, tiles, L.tiles_n, params);
	hipLaunchKernelGGL(le_track_event_kernel, per_tile, wg, 0, q, d_cands, keys, vals, params, info, tiles, evidx, ekey, econn, work);
	hipLaunchKernelGGL(le_track_interval_kernel, per_cand, wg, 0, q, ekey, econn, params, unit_bits, jitter_bits, work);
	hipLaunchKernelGGL(le_track_step_kernel, per_tile, wg, 0, q, ekey, econn, params, unit_bits, work, step, tiles64);
	hipLaunchKernelGGL(le_track_prefix64_kernel, dim3(1), wg, 0, q, tiles64, L.tiles_n);
	hipLaunchKernelGGL(le_track_count_kernel, per_tile, wg, 0, q, params, tiles64, step);
	hipLaunchKernelGGL(le_track_score_kernel, dim3(L.score_tiles, 12), wg, 0, q, ekey, econn, step, params, work, flags, score);
	hipLaunchKernelGGL(le_track_verdict_kernel, dim3((conn_cap + LT_WAVES - 1) / LT_WAVES), wg, 0, q, work, score, ekey, params, d_tracks);
	hipLaunchKernelGGL(le_track_pkt_kernel, per_cand, wg, 0, q, keys, vals, info, evidx, step, params, work, flags, d_tracks, d_pkts);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

// btbbx_le_track_device's checks and launches under the name `who`, with a stand-in for the flag pass or none.  Not exported:
// the coded tracking's unit (le_ctrack.h) reaches le_track_launch through it
int le_track_run(const char *who, const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
		 const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
		 const uint16_t *d_phys_channel, uint32_t n_streams,
		 uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
		 btbbx_le_track *d_tracks, btbbx_le_track_pkt *d_pkts,
		 void *d_scratch, size_t scratch_bytes, void *hip_stream, const LtFlagStandIn *stand_in)
{
	int rc = le_track_check_args(who, n_streams, unit_bits, jitter_bits);
	if (rc)
		return rc;
	const LtLayout L = le_track_layout(cand_cap, conn_cap);
	if (!d_cands || !d_cand_count || !d_conns || !d_conn_count || !d_phys_channel || !d_tracks || !d_pkts || !d_scratch ||
	    scratch_bytes < L.total) {
		set_error("%s: null pointer, or scratch of %zu bytes needed and %zu given", who, L.total, scratch_bytes);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_cands & 7) || ((uintptr_t)d_conns & 7) || ((uintptr_t)d_tracks & 7) || ((uintptr_t)d_pkts & 7) ||
	    ((uintptr_t)d_scratch & 7) || ((uintptr_t)d_cand_count & 3) || ((uintptr_t)d_conn_count & 3) || ((uintptr_t)d_phys_channel & 1)) {
		set_error("%s: misaligned pointer (records and scratch 8 bytes, the counters 4, the channels 2)", who);
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	if (!cand_cap || !conn_cap)
		return BTBBX_OK;
	return le_track_launch(d_cands, d_cand_count, cand_cap, d_conn_count, conn_cap, d_phys_channel, n_streams, unit_bits, ifs_bits,
			       jitter_bits, flags, d_tracks, d_pkts, d_scratch, (hipStream_t)hip_stream, stand_in);
}

extern "C" int btbbx_le_track_device(const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
				     const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
				     const uint16_t *d_phys_channel, uint32_t n_streams,
				     uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
				     btbbx_le_track *d_tracks, btbbx_le_track_pkt *d_pkts,
				     void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
	return le_track_run("btbbx_le_track_device", d_cands, d_cand_count, cand_cap, d_conns, d_conn_count, conn_cap, d_phys_channel, n_streams,
			    unit_bits, ifs_bits, jitter_bits, flags, d_tracks, d_pkts, d_scratch, scratch_bytes, hip_stream, nullptr);
}
