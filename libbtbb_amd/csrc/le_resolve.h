// le_resolve.h -- LE address resolution (included by le.hip, behind le_pair.h): the distinct device addresses of a capture's
// advertising records, the identity resolving keys (IRKs) the peers distribute in their SMP messages next to the caller's own, every
// resolvable private address tried against every key, and per connection which address and which key its two ends have.  The
// contract is in include/btbbx.h (btbbx_le_resolve_device), the reasoning in DESIGN 3.8.10.  All arithmetic is integer arithmetic.
// AES is le_aes.h's (lx_te_entry, lx_expand, lx_load_rk, lx_aes), the sort radix_sort.h's.
//
//   1. le_resolve_init_kernel      rule 2: a key per slot; the per-address words and per-connection tables cleared; the round table; A, K, W
//   2. le_resolve_find_kernel      rule 4: one lane per message, the first Identity messages of a (connection, role) by atomicMin
//   3. le_resolve_table_kernel     rule 4: the table slots by a prefix over (connection, role), the IRK records, the count
//   4. le_resolve_expand_kernel    one lane per table slot: its schedule, 44 words, into scratch; which slots are tried
//   5. seven radix passes          rule 3: the slots by their 49-bit keys (21 launches)
//   6. le_resolve_mark_, _prefix_, _rank_kernel   rule 3: a head where a key differs from the one before, the heads' prefix sums: ranks
//   7. le_resolve_tally_kernel     rule 6: one lane per sorted slot, a segmented reduction over the wave, one atomic per wave and address
//   8. le_resolve_trial_kernel     rule 5: a fixed grid over (table slot, tile of addresses): the schedule uniform, one block per lane
//   9. le_resolve_addr_kernel      rules 6 and 7: the address records; the keys' tallies, reduced per wave and key
//  10. le_resolve_peer_kernel      rule 8
//
// 32 launches, whatever the counts and caps.  Nothing here synchronises or reads back but the host wrappers.
#pragma once
#include "le_aes.h"
#include "radix_sort.h"
#include "wave_scan.h"

#define LR_NONE       0xffffffffu
#define LR_MAX_IRKS   BTBBX_LE_RESOLVE_MAX_IRKS
#define LR_TILE       1024u                // sorted slots a workgroup marks and ranks (4 rounds of 256)
#define LR_PER        4u                   // addresses a lane tries under one schedule
#define LR_ITEM       (LE_THREADS * LR_PER) // addresses of one trial item
#define LR_WGS_PER_CU 8u                   // workgroups of the trial kernel per compute unit, at most
#define LR_KEY_BITS   49u                  // t << 48 | the address; a slot without an address: all ones, which sorts behind

static_assert(sizeof(btbbx_le_addr) == 40 && offsetof(btbbx_le_addr, last_offset) == 8 && offsetof(btbbx_le_addr, n_slots) == 16 &&
	      offsetof(btbbx_le_addr, first_rec) == 20 && offsetof(btbbx_le_addr, addr) == 24 && offsetof(btbbx_le_addr, random) == 30 &&
	      offsetof(btbbx_le_addr, kind) == 31 && offsetof(btbbx_le_addr, irk) == 32 && offsetof(btbbx_le_addr, roles) == 34 &&
	      offsetof(btbbx_le_addr, channels) == 35 && offsetof(btbbx_le_addr, reserved) == 36,
	      "btbbx_le_addr layout (libbtbb_amd.LE_ADDR_DTYPE)");
static_assert(sizeof(btbbx_le_irk) == 40 && offsetof(btbbx_le_irk, id_addr) == 16 && offsetof(btbbx_le_irk, id_random) == 22 &&
	      offsetof(btbbx_le_irk, flags) == 23 && offsetof(btbbx_le_irk, conn) == 24 && offsetof(btbbx_le_irk, n_addrs) == 28 &&
	      offsetof(btbbx_le_irk, n_slots) == 32 && offsetof(btbbx_le_irk, role) == 36 && offsetof(btbbx_le_irk, reserved) == 37,
	      "btbbx_le_irk layout (libbtbb_amd.LE_IRK_DTYPE)");
static_assert(sizeof(btbbx_le_peer) == 16 && offsetof(btbbx_le_peer, adv_addr) == 4 && offsetof(btbbx_le_peer, init_irk) == 8 &&
	      offsetof(btbbx_le_peer, adv_irk) == 10 && offsetof(btbbx_le_peer, irk) == 12, "btbbx_le_peer layout (libbtbb_amd.LE_PEER_DTYPE)");

struct LrArgs {
	const btbbx_le_pkt *adv;
	const uint32_t *d_adv_count, *d_conn_count, *d_msg_count;
	const btbbx_le_seed *seeds;
	const btbbx_le_msg *msgs;
	const uint8_t *bytes, *given;
	uint64_t byte_cap;
	uint32_t adv_cap, conn_cap, msg_cap, n_given, addr_cap, irk_cap, n_tiles;
	uint32_t *slot_addr, *addr_count, *irk_count;
	btbbx_le_addr *addrs;
	btbbx_le_irk *irks;
	btbbx_le_peer *peers;
	// scratch.  keys0 / vals0: the sort's side 0, which init fills; keys / vals: the side the sorted list ends in.  Per address (rank):
	// start (the first sorted position; start[N]: the end), akey (the key), match (the smallest matching table slot), amin / amax
	// (the offsets), aor (roles | channels << 8).  Per (connection, role): hk / ha (the first Identity Information / Identity
	// Address Information message), hslot (the table slot).  Per table slot: sched (44 words), live (is it tried).
	// counts[0]: A, [1]: K, [2]: W, [3]: N, [4]: T, the table slots in use
	uint64_t *keys0;
	const uint64_t *keys;
	uint32_t *vals0;
	const uint32_t *vals;
	uint32_t *te, *params, *counts, *tiles, *start, *match, *aor, *hk, *ha, *hslot, *sched, *live;
	unsigned long long *akey, *amin, *amax;
};

struct LrLayout {
	size_t te, params, counts, keys[2], vals[2], hist, tot, tiles, start, akey, match, amin, amax, aor, hk, ha, hslot, sched, live, total;
	uint32_t n_tiles;
};

static LrLayout le_resolve_layout(uint32_t adv_cap, uint32_t conn_cap, uint32_t irk_cap)
{
	LrLayout L;
	const size_t s = adv_cap ? 2 * (size_t)adv_cap : 1, k = conn_cap ? 2 * (size_t)conn_cap : 1, t = irk_cap ? irk_cap : 1;
	L.n_tiles = (uint32_t)((s + LR_TILE - 1) / LR_TILE);
	size_t at = 0;
	auto take = [&](size_t bytes) { const size_t here = at; at += ld_up(bytes); return here; };
	L.te = take(256 * 4);
	L.params = take(256);
	L.counts = take(256);
	L.keys[0] = take(s * 8);
	L.keys[1] = take(s * 8);
	L.vals[0] = take(s * 4);
	L.vals[1] = take(s * 4);
	L.hist = take((size_t)radix_sort_blocks(s) * 256 * 4);
	L.tot = take(256 * 4);
	L.tiles = take(((size_t)L.n_tiles + 1) * 4);
	L.start = take((s + 1) * 4);
	L.akey = take(s * 8);
	L.match = take(s * 4);
	L.amin = take(s * 8);
	L.amax = take(s * 8);
	L.aor = take(s * 4);
	L.hk = take(k * 4);
	L.ha = take(k * 4);
	L.hslot = take(k * 4);
	L.sched = take(t * LX_RK * 4);
	L.live = take(t * 4);
	L.total = at;
	return L;
}

// ---- 1. rule 2: the slots -------------------------------------------------------------------------------------------------------------

// six octets from p, least significant first
__device__ __forceinline__ unsigned long long lr_octets6(const uint8_t *p)
{
	unsigned long long v = 0;
#pragma unroll
	for (int j = 0; j < 6; j++)
		v |= (unsigned long long)p[j] << (8 * j);
	return v;
}

// slot `which` of record p: its key and its role; false: the slot holds no address
__device__ __forceinline__ bool lr_slot(const btbbx_le_pkt &p, uint32_t which, unsigned long long &key, uint32_t &role)
{
	if (!p.crc_ok || p.is_data || p.channel_idx < 37)
		return false;
	const uint32_t ty = p.adv_type, len = p.length;
	uint32_t t;
	if (ty == 0 || ty == 2 || ty == 4 || ty == 6) {
		if (which || len < 6)
			return false;
		role = BTBBX_LE_ADDR_ADVERTISER;
		t = p.adv_tx_add;
	} else if (ty == 1 || ty == 3 || ty == 5) {
		if (len < 12)
			return false;
		if (!which) {
			role = ty == 1 ? BTBBX_LE_ADDR_ADVERTISER : (ty == 3 ? BTBBX_LE_ADDR_SCANNER : BTBBX_LE_ADDR_INITIATOR);
			t = p.adv_tx_add;
		} else {
			role = ty == 1 ? BTBBX_LE_ADDR_TARGET : BTBBX_LE_ADDR_ADVERTISER;
			t = p.adv_rx_add;
		}
	} else {
		return false;
	}
	key = lr_octets6(p.bytes + 6 + 6 * which) | ((unsigned long long)(t ? 1u : 0u) << 48);
	return true;
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_resolve_init_kernel(LrArgs a)
{
	const uint32_t ah = a.adv_cap ? *a.d_adv_count : 0u, kh = a.conn_cap ? *a.d_conn_count : 0u, wh = a.msg_cap ? *a.d_msg_count : 0u;
	const uint32_t n = ah < a.adv_cap ? ah : a.adv_cap, k = kh < a.conn_cap ? kh : a.conn_cap, w = wh < a.msg_cap ? wh : a.msg_cap;
	const uint64_t i = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	if (i == 0) {
		a.params[0] = 2 * n;
		a.counts[0] = n;
		a.counts[1] = k;
		a.counts[2] = w;
		a.counts[3] = 0;
		a.counts[4] = 0;
	}
	if (blockIdx.x == 0)
		a.te[threadIdx.x] = lx_te_entry(threadIdx.x);
	if (i < 2 * (uint64_t)a.adv_cap) {
		a.slot_addr[i] = LR_NONE;
		if (i < 2 * (uint64_t)n) {
			unsigned long long key = ~0ull;
			uint32_t role;
			if (!lr_slot(a.adv[i >> 1], (uint32_t)i & 1u, key, role))
				key = ~0ull;
			a.keys0[i] = key;
			a.vals0[i] = (uint32_t)i;
			a.match[i] = LR_NONE;
			a.amin[i] = ~0ull;
			a.amax[i] = 0;
			a.aor[i] = 0;
		}
	}
	if (i < 2 * (uint64_t)k) {
		a.hk[i] = LR_NONE;
		a.ha[i] = LR_NONE;
		a.hslot[i] = 0xffffu;
	}
}

// ---- 2. rule 4: the harvest, the table ---------------------------------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_resolve_find_kernel(LrArgs a)
{
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t k = a.counts[1], w = a.counts[2], m = (uint32_t)at;
	if (at >= w)
		return;
	const btbbx_le_msg &r = a.msgs[m];
	const uint32_t need = BTBBX_LE_MSG_COMPLETE | BTBBX_LE_MSG_STORED, len = r.l2cap_len, role = r.role, g = r.conn;
	if (g >= k || r.byte_offset > a.byte_cap || r.bytes > a.byte_cap - r.byte_offset || r.bytes < 4u + len)
		return;
	if ((r.flags & need) != need || r.cid != 0x0006u || len < 1 || role > 1)
		return;
	const uint32_t code = a.bytes[r.byte_offset + 4];
	if (code == 0x08u && len == 17)
		atomicMin(a.hk + 2 * (size_t)g + role, m);
	else if (code == 0x09u && len == 8)
		atomicMin(a.ha + 2 * (size_t)g + role, m);
}

// an IRK record as its ten words
__device__ __forceinline__ void lr_put_irk(btbbx_le_irk *o, const uint32_t (&key)[4], unsigned long long id, uint32_t id_random, uint32_t flags,
					   uint32_t conn, uint32_t role)
{
	if (!(key[0] | key[1] | key[2] | key[3]))
		flags |= BTBBX_LE_IRK_NULLKEY;
	uint32_t *p = reinterpret_cast<uint32_t *>(o);
	p[0] = key[0];
	p[1] = key[1];
	p[2] = key[2];
	p[3] = key[3];
	p[4] = (uint32_t)id;
	p[5] = (uint32_t)(id >> 32) | (id_random << 16) | (flags << 24);
	p[6] = conn;
	p[7] = 0;
	p[8] = 0;
	p[9] = role;
}

// one workgroup walks the (connection, role) pairs 256 at a time: a pair's slot is n_given + the number of pairs with a key in front
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_resolve_table_kernel(LrArgs a)
{
	__shared__ uint32_t wave_sum[LE_THREADS / 64];
	const uint32_t k2 = 2 * a.counts[1], lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t base = a.n_given;
	for (uint64_t g0 = 0; g0 < k2; g0 += LE_THREADS) {
		const uint64_t g = g0 + threadIdx.x;
		const uint32_t m = g < k2 ? a.hk[g] : LR_NONE;
		const bool has = m != LR_NONE;
		const unsigned long long mask = __ballot(has);
		if (lane == 0)
			wave_sum[wave] = (uint32_t)__popcll(mask);
		__syncthreads();
		uint32_t front = 0, total = 0;
#pragma unroll
		for (uint32_t v = 0; v < LE_THREADS / 64; v++) {
			front += v < wave ? wave_sum[v] : 0u;
			total += wave_sum[v];
		}
		if (has) {
			const uint32_t slot = base + front + (uint32_t)__popcll(mask & ((1ull << lane) - 1));
			if (slot < a.irk_cap) {
				const uint8_t *v = a.bytes + a.msgs[m].byte_offset + 4;
				uint32_t key[4];
#pragma unroll
				for (int wd = 0; wd < 4; wd++)              // key[j] = v[16 - j]
					key[wd] = v[16 - 4 * wd] | ((uint32_t)v[15 - 4 * wd] << 8) | ((uint32_t)v[14 - 4 * wd] << 16) |
						  ((uint32_t)v[13 - 4 * wd] << 24);
				const uint32_t ma = a.ha[g];
				unsigned long long id = 0;
				uint32_t id_random = 0, flags = BTBBX_LE_IRK_HARVESTED;
				if (ma != LR_NONE) {
					const uint8_t *u = a.bytes + a.msgs[ma].byte_offset + 4;
					id_random = u[1] & 1u;
					id = lr_octets6(u + 2);
					flags |= BTBBX_LE_IRK_HAS_ADDR;
				}
				lr_put_irk(a.irks + slot, key, id, id_random, flags, (uint32_t)(g >> 1), (uint32_t)g & 1u);
				a.hslot[g] = slot;
			}
		}
		base += total;
		__syncthreads();
	}
	const uint32_t used = base < a.irk_cap ? base : a.irk_cap;
	if (threadIdx.x == 0) {
		*a.irk_count = base;
		a.counts[4] = used;
	}
	for (uint32_t j = threadIdx.x; j < a.irk_cap; j += LE_THREADS) {
		if (j < a.n_given) {
			const uint8_t *v = a.given + 16 * (size_t)j;
			uint32_t key[4];
#pragma unroll
			for (int wd = 0; wd < 4; wd++)
				key[wd] = v[4 * wd] | ((uint32_t)v[4 * wd + 1] << 8) | ((uint32_t)v[4 * wd + 2] << 16) | ((uint32_t)v[4 * wd + 3] << 24);
			lr_put_irk(a.irks + j, key, 0, 0, BTBBX_LE_IRK_GIVEN, LR_NONE, 0);
		} else if (j >= used) {
			uint32_t *p = reinterpret_cast<uint32_t *>(a.irks + j);
#pragma unroll
			for (int wd = 0; wd < 10; wd++)
				p[wd] = wd == 6 ? LR_NONE : 0u;
		}
	}
}

// one lane per table slot: the schedule of a slot that is tried
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_resolve_expand_kernel(LrArgs a)
{
	__shared__ uint32_t te[256];
	te[threadIdx.x] = a.te[threadIdx.x];
	__syncthreads();
	const uint32_t slot = blockIdx.x * LE_THREADS + threadIdx.x;
	if (slot >= a.irk_cap)
		return;
	const uint32_t *p = reinterpret_cast<const uint32_t *>(a.irks + slot);
	const bool tried = slot < a.counts[4] && !((p[5] >> 24) & BTBBX_LE_IRK_NULLKEY);
	a.live[slot] = tried ? 1u : 0u;
	if (!tried)
		return;
	uint32_t rk[LX_RK];
	rk[0] = p[0];
	rk[1] = p[1];
	rk[2] = p[2];
	rk[3] = p[3];
	lx_expand(te, rk);
	uint4 *o = reinterpret_cast<uint4 *>(a.sched + (size_t)LX_RK * slot);
#pragma unroll
	for (int j = 0; j < (int)LX_RK / 4; j++)
		o[j] = make_uint4(rk[4 * j], rk[4 * j + 1], rk[4 * j + 2], rk[4 * j + 3]);
}

// ---- 3. rule 3: the distinct list ---------------------------------------------------------------------------------------------------------

// does sorted position i open an address?  (a slot without an address has a key of all ones)
__device__ __forceinline__ bool lr_head(const uint64_t *keys, uint64_t i, uint32_t n)
{
	if (i >= n)
		return false;
	const uint64_t key = keys[i];
	return (key >> LR_KEY_BITS) == 0 && (i == 0 || keys[i - 1] != key);
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_resolve_mark_kernel(LrArgs a)
{
	__shared__ uint32_t lds[LE_THREADS / 64];
	const uint32_t n = a.params[0];
	uint32_t mine = 0;
	for (uint32_t r = 0; r < LR_TILE / LE_THREADS; r++)
		mine += lr_head(a.keys, (uint64_t)blockIdx.x * LR_TILE + r * LE_THREADS + threadIdx.x, n) ? 1u : 0u;
	uint32_t total;
	(void)block_exclusive_scan<LE_THREADS / 64>(mine, lds, total);
	if (threadIdx.x == 0)
		a.tiles[blockIdx.x] = total;
}

// one workgroup: the tiles' counts become exclusive prefix sums, their sum is N
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_resolve_prefix_kernel(LrArgs a)
{
	__shared__ uint32_t lds[LE_THREADS / 64];
	uint32_t carry = 0;
	for (uint32_t base = 0; base < a.n_tiles; base += LE_THREADS) {
		const uint32_t i = base + threadIdx.x;
		const uint32_t v = i < a.n_tiles ? a.tiles[i] : 0u;
		uint32_t sum;
		const uint32_t ex = block_exclusive_scan<LE_THREADS / 64>(v, lds, sum);
		if (i < a.n_tiles)
			a.tiles[i] = carry + ex;
		carry += sum;
	}
	if (threadIdx.x == 0) {
		a.counts[3] = carry;
		*a.addr_count = carry;
	}
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_resolve_rank_kernel(LrArgs a)
{
	__shared__ uint32_t lds[LE_THREADS / 64];
	const uint32_t n = a.params[0];
	uint32_t base = a.tiles[blockIdx.x];
	for (uint32_t r = 0; r < LR_TILE / LE_THREADS; r++) {
		const uint64_t i = (uint64_t)blockIdx.x * LR_TILE + r * LE_THREADS + threadIdx.x;
		const uint32_t h = lr_head(a.keys, i, n) ? 1u : 0u;
		uint32_t total;
		const uint32_t ex = block_exclusive_scan<LE_THREADS / 64>(h, lds, total);
		if (i < n) {
			const uint64_t key = a.keys[i];
			if ((key >> LR_KEY_BITS) == 0) {
				const uint32_t rank = base + ex + h - 1u;
				a.slot_addr[a.vals[i]] = rank;
				if (h) {
					a.start[rank] = (uint32_t)i;
					a.akey[rank] = key;
				}
				if (i + 1 == n || (a.keys[i + 1] >> LR_KEY_BITS) != 0)
					a.start[rank + 1] = (uint32_t)i + 1u;
			}
		}
		base += total;
	}
}

// ---- 4. rule 6: the tallies of an address ------------------------------------------------------------------------------------------------

// One lane per sorted slot.  The slots of an address are consecutive, so a segmented scan over the lanes leaves an address's part of
// the wave in the last of its lanes, which alone goes to memory: an advertiser that fills thousands of slots costs one atomic per wave
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_resolve_tally_kernel(LrArgs a)
{
	const uint64_t i = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t n = a.params[0], lane = threadIdx.x & 63u;
	uint32_t rank = LR_NONE, bits = 0;
	unsigned long long lo = ~0ull, hi = 0;
	if (i < n && (a.keys[i] >> LR_KEY_BITS) == 0) {
		const uint32_t s = a.vals[i];
		const btbbx_le_pkt &p = a.adv[s >> 1];
		unsigned long long key;
		uint32_t role = 0;
		(void)lr_slot(p, s & 1u, key, role);
		rank = a.slot_addr[s];
		lo = hi = p.offset;
		bits = role | (0x100u << ((p.channel_idx - 37u) & 7u));
	}
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t r_up = __shfl_up(rank, d), b_up = __shfl_up(bits, d);
		const unsigned long long lo_up = __shfl_up(lo, d), hi_up = __shfl_up(hi, d);
		if (lane >= (uint32_t)d && r_up == rank) {
			bits |= b_up;
			lo = lo_up < lo ? lo_up : lo;
			hi = hi_up > hi ? hi_up : hi;
		}
	}
	const uint32_t r_next = __shfl_down(rank, 1);
	if (rank != LR_NONE && (lane == 63 || r_next != rank)) {
		atomicMin(a.amin + rank, lo);
		atomicMax(a.amax + rank, hi);
		atomicOr(a.aor + rank, bits);
	}
}

// ---- 5. rule 5: the trials -------------------------------------------------------------------------------------------------------------------

// A fixed grid strides over the items t = slot * per + tile of the device's counts, 64 bits wide; per = the tiles of LR_ITEM consecutive
// addresses.  An item's schedule depends on the item alone, so it is uniform over the workgroup; a lane takes LR_PER addresses, one
// block and one compare each.  Of the output only the last word is looked at
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_resolve_trial_kernel(LrArgs a)
{
	__shared__ uint32_t te[256];
	te[threadIdx.x] = a.te[threadIdx.x];
	__syncthreads();
	const uint32_t n = a.counts[3], used = a.counts[4];
	const uint32_t per = (uint32_t)(((uint64_t)n + LR_ITEM - 1) / LR_ITEM);
	const uint64_t all = (uint64_t)used * per;
	for (uint64_t t = blockIdx.x; t < all; t += gridDim.x) {
		const uint32_t slot = (uint32_t)(t / per), tile = (uint32_t)(t % per);
		if (!a.live[slot])
			continue;
		uint32_t rk[LX_RK];
		lx_load_rk(a.sched + (size_t)LX_RK * slot, rk);
#pragma unroll
		for (uint32_t j = 0; j < LR_PER; j++) {
			const uint64_t r = (uint64_t)tile * LR_ITEM + j * LE_THREADS + threadIdx.x;
			if (r >= n)
				continue;
			const unsigned long long key = a.akey[r];
			if ((key >> 46) != 5u)                          // t == 1 and a[5] >> 6 == 1: RESOLVABLE
				continue;
			LxBlock b;
			b.w[0] = b.w[1] = b.w[2] = 0;
			b.w[3] = lx_bswap((uint32_t)(key >> 24) & 0xffffffu);           // block[13..15] = a[5], a[4], a[3]
			const LxBlock o = lx_aes(te, rk, b);
			if ((o.w[3] & 0xffffff00u) == lx_bswap((uint32_t)key & 0xffffffu))   // o[13..15] == a[2], a[1], a[0]
				atomicMin(a.match + r, slot);
		}
	}
}

// ---- 6. rules 6 to 8: the records ----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ uint32_t lr_wave_sum(uint32_t v)
{
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1)
		v += __shfl_xor(v, d);
	return v;
}

// One lane per address.  A key's tallies: the lanes of a wave that resolved to the same slot are summed first, one pair of atomics per
// wave and slot (most addresses resolve to none and a neighbourhood to few)
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_resolve_addr_kernel(LrArgs a)
{
	const uint64_t r = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t n = a.counts[3], lane = threadIdx.x & 63u;
	const bool have = r < n;
	uint32_t irk = LR_NONE, n_slots = 0;
	if (have) {
		const uint32_t first = a.start[r];
		irk = a.match[r];
		n_slots = a.start[r + 1] - first;
		if (r < a.addr_cap) {
			const unsigned long long key = a.akey[r], lo = a.amin[r], hi = a.amax[r];
			const uint32_t bits = a.aor[r], random = (uint32_t)(key >> 48) & 1u;
			const uint32_t kind = random ? 1u + ((uint32_t)(key >> 46) & 3u) : 0u;
			uint2 *o = reinterpret_cast<uint2 *>(a.addrs + r);
			o[0] = make_uint2((uint32_t)lo, (uint32_t)(lo >> 32));
			o[1] = make_uint2((uint32_t)hi, (uint32_t)(hi >> 32));
			o[2] = make_uint2(n_slots, a.vals[first] >> 1);
			o[3] = make_uint2((uint32_t)key, ((uint32_t)(key >> 32) & 0xffffu) | (random << 16) | (kind << 24));
			o[4] = make_uint2((irk & 0xffffu) | ((bits & 0xffu) << 16) | (((bits >> 8) & 0xffu) << 24), 0u);
		}
	}
	bool pending = irk != LR_NONE;
	for (;;) {
		const unsigned long long waiting = __ballot(pending);
		if (!waiting)
			break;
		// (readlane, not __shfl: a second caller of __shfl in this translation unit changes how the compiler inlines it into
		// le_track_event_kernel and with that the register figure DESIGN 3.8.2 states for that kernel)
		const uint32_t leader = (uint32_t)__builtin_ctzll(waiting);
		const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane((int)irk, (int)__builtin_amdgcn_readfirstlane((int)leader));
		const bool mine = pending && irk == slot;
		const uint32_t addrs = (uint32_t)__popcll(__ballot(mine)), slots = lr_wave_sum(mine ? n_slots : 0u);
		if (lane == leader) {
			atomicAdd(&a.irks[slot].n_addrs, addrs);
			atomicAdd(&a.irks[slot].n_slots, slots);
		}
		pending = pending && !mine;
	}
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_resolve_peer_kernel(LrArgs a)
{
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t n = a.counts[0], k = a.counts[1], g = (uint32_t)at;
	if (at >= k)
		return;
	const btbbx_le_seed &sd = a.seeds[g];
	uint32_t init_addr = LR_NONE, adv_addr = LR_NONE, init_irk = 0xffffu, adv_irk = 0xffffu;
	if ((sd.flags & BTBBX_LE_SEED_SEEDED) && sd.request < n) {
		init_addr = a.slot_addr[2 * (size_t)sd.request];
		adv_addr = a.slot_addr[2 * (size_t)sd.request + 1];
		if (init_addr != LR_NONE)
			init_irk = a.match[init_addr] & 0xffffu;
		if (adv_addr != LR_NONE)
			adv_irk = a.match[adv_addr] & 0xffffu;
	}
	uint32_t *o = reinterpret_cast<uint32_t *>(a.peers + g);
	o[0] = init_addr;
	o[1] = adv_addr;
	o[2] = init_irk | (adv_irk << 16);
	o[3] = (a.hslot[2 * (size_t)g] & 0xffffu) | ((a.hslot[2 * (size_t)g + 1] & 0xffffu) << 16);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------

extern "C" size_t btbbx_le_resolve_scratch_bytes(uint32_t adv_cap, uint32_t conn_cap, uint32_t irk_cap)
{
	return le_resolve_layout(adv_cap, conn_cap, irk_cap).total;
}

// the 32 launches of one run
static int le_resolve_launch(const btbbx_le_pkt *d_adv, const uint32_t *d_adv_count, uint32_t adv_cap, const uint32_t *d_conn_count,
			     uint32_t conn_cap, const btbbx_le_seed *d_seeds, const btbbx_le_msg *d_msgs, const uint32_t *d_msg_count,
			     uint32_t msg_cap, const uint8_t *d_bytes, uint64_t byte_cap, const uint8_t *d_given, uint32_t n_given,
			     uint32_t *d_slot_addr, btbbx_le_addr *d_addrs, uint32_t addr_cap, uint32_t *d_addr_count, btbbx_le_irk *d_irks,
			     uint32_t irk_cap, uint32_t *d_irk_count, btbbx_le_peer *d_peers, void *d_scratch, hipStream_t q)
{
	const LrLayout L = le_resolve_layout(adv_cap, conn_cap, irk_cap);
	char *s = (char *)d_scratch;
	const size_t slots = 2 * (size_t)adv_cap;
	LrArgs a;
	a.adv = d_adv;
	a.d_adv_count = d_adv_count;
	a.d_conn_count = d_conn_count;
	a.d_msg_count = d_msg_count;
	a.seeds = d_seeds;
	a.msgs = d_msgs;
	a.bytes = d_bytes;
	a.given = d_given;
	a.byte_cap = byte_cap;
	a.adv_cap = adv_cap;
	a.conn_cap = conn_cap;
	a.msg_cap = msg_cap;
	a.n_given = n_given;
	a.addr_cap = addr_cap;
	a.irk_cap = irk_cap;
	a.n_tiles = L.n_tiles;
	a.slot_addr = d_slot_addr;
	a.addr_count = d_addr_count;
	a.irk_count = d_irk_count;
	a.addrs = d_addrs;
	a.irks = d_irks;
	a.peers = d_peers;
	a.te = (uint32_t *)(s + L.te);
	a.params = (uint32_t *)(s + L.params);
	a.counts = (uint32_t *)(s + L.counts);
	a.tiles = (uint32_t *)(s + L.tiles);
	a.start = (uint32_t *)(s + L.start);
	a.akey = (unsigned long long *)(s + L.akey);
	a.match = (uint32_t *)(s + L.match);
	a.amin = (unsigned long long *)(s + L.amin);
	a.amax = (unsigned long long *)(s + L.amax);
	a.aor = (uint32_t *)(s + L.aor);
	a.hk = (uint32_t *)(s + L.hk);
	a.ha = (uint32_t *)(s + L.ha);
	a.hslot = (uint32_t *)(s + L.hslot);
	a.sched = (uint32_t *)(s + L.sched);
	a.live = (uint32_t *)(s + L.live);
	const RadixBufs b = le_radix_bufs(s, L, a.params, (uint32_t)std::max<size_t>(slots, 1));
	a.keys0 = b.keys[0];
	a.vals0 = b.vals[0];
	a.keys = b.keys[1];                                     // (seven passes from side 0 end in side 1)
	a.vals = b.vals[1];
	const auto blocks = [](uint64_t items) { return (uint32_t)std::max<uint64_t>((items + LE_THREADS - 1) / LE_THREADS, 1); };
	const dim3 per_slot(blocks(slots)), per_msg(blocks(msg_cap)), per_conn(blocks(conn_cap)), per_key(blocks(irk_cap)), per_tile(L.n_tiles);
	const dim3 init(blocks(std::max<uint64_t>(slots, 2 * (uint64_t)conn_cap))), wg(LE_THREADS), one(1);
	// the trials: every (slot, tile) the caps allow, but no more workgroups than stay resident
	const uint64_t items = (uint64_t)std::max(irk_cap, 1u) * ((std::max<size_t>(slots, 1) + LR_ITEM - 1) / LR_ITEM);
	const dim3 trial((uint32_t)std::min<uint64_t>(items, (uint64_t)ctx().num_cus * LR_WGS_PER_CU));
	hipLaunchKernelGGL(le_resolve_init_kernel, init, wg, 0, q, a);
	hipLaunchKernelGGL(le_resolve_find_kernel, per_msg, wg, 0, q, a);
	hipLaunchKernelGGL(le_resolve_table_kernel, one, wg, 0, q, a);
	hipLaunchKernelGGL(le_resolve_expand_kernel, per_key, wg, 0, q, a);
	const int cur = le_sort_bytes(b, 7, 0, q);               // 49 bits
	if (cur != 1) {
		set_error("btbbx_le_resolve_device: the sort ended in side %d", cur);
		return BTBBX_E_ARG;
	}
	hipLaunchKernelGGL(le_resolve_mark_kernel, per_tile, wg, 0, q, a);
	hipLaunchKernelGGL(le_resolve_prefix_kernel, one, wg, 0, q, a);
	hipLaunchKernelGGL(le_resolve_rank_kernel, per_tile, wg, 0, q, a);
	hipLaunchKernelGGL(le_resolve_tally_kernel, per_slot, wg, 0, q, a);
	hipLaunchKernelGGL(le_resolve_trial_kernel, trial, wg, 0, q, a);
	hipLaunchKernelGGL(le_resolve_addr_kernel, per_slot, wg, 0, q, a);
	hipLaunchKernelGGL(le_resolve_peer_kernel, per_conn, wg, 0, q, a);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

static int le_resolve_check_limits(const char *who, uint64_t adv_cap, uint32_t n_given, uint32_t irk_cap)
{
	if (irk_cap > LR_MAX_IRKS || n_given > irk_cap || adv_cap > 0x7fffffffull) {
		set_error("%s: irk_cap must be 0..%u, n_given <= irk_cap and adv_cap < 2^31", who, LR_MAX_IRKS);
		return BTBBX_E_ARG;
	}
	return BTBBX_OK;
}

extern "C" int btbbx_le_resolve_device(const btbbx_le_pkt *d_adv, const uint32_t *d_adv_count, uint32_t adv_cap, const uint32_t *d_conn_count,
				       uint32_t conn_cap, const btbbx_le_seed *d_seeds, const btbbx_le_msg *d_msgs,
				       const uint32_t *d_msg_count, uint32_t msg_cap, const uint8_t *d_bytes, uint64_t byte_cap,
				       const uint8_t *d_given, uint32_t n_given, uint32_t *d_slot_addr, btbbx_le_addr *d_addrs,
				       uint32_t addr_cap, uint32_t *d_addr_count, btbbx_le_irk *d_irks, uint32_t irk_cap, uint32_t *d_irk_count,
				       btbbx_le_peer *d_peers, void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
	const char *who = "btbbx_le_resolve_device";
	int rc = le_resolve_check_limits(who, adv_cap, n_given, irk_cap);
	if (rc)
		return rc;
	const LrLayout L = le_resolve_layout(adv_cap, conn_cap, irk_cap);
	if (((!d_adv || !d_adv_count || !d_slot_addr) && adv_cap) || ((!d_conn_count || !d_seeds || !d_peers) && conn_cap) ||
	    ((!d_msgs || !d_msg_count) && msg_cap) || (!d_bytes && byte_cap) || (!d_given && n_given) || (!d_addrs && addr_cap) || !d_addr_count ||
	    (!d_irks && irk_cap) || !d_irk_count || !d_scratch || scratch_bytes < L.total) {
		set_error("%s: null pointer, or scratch of %zu bytes needed and %zu given", who, L.total, scratch_bytes);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_adv & 7) || ((uintptr_t)d_seeds & 7) || ((uintptr_t)d_msgs & 7) || ((uintptr_t)d_addrs & 7) || ((uintptr_t)d_irks & 7) ||
	    ((uintptr_t)d_peers & 7) || ((uintptr_t)d_slot_addr & 3) || ((uintptr_t)d_adv_count & 3) || ((uintptr_t)d_conn_count & 3) ||
	    ((uintptr_t)d_msg_count & 3) || ((uintptr_t)d_addr_count & 3) || ((uintptr_t)d_irk_count & 3) || ((uintptr_t)d_scratch & 15)) {
		set_error("%s: misaligned pointer (scratch 16 bytes; the records 8; the slot map and the counters 4)", who);
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	return le_resolve_launch(d_adv, d_adv_count, adv_cap, d_conn_count, conn_cap, d_seeds, d_msgs, d_msg_count, msg_cap, d_bytes, byte_cap,
				 d_given, n_given, d_slot_addr, d_addrs, addr_cap, d_addr_count, d_irks, irk_cap, d_irk_count, d_peers, d_scratch,
				 (hipStream_t)hip_stream);
}
