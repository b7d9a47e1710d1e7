// le_pair.h -- LE legacy pairing key recovery (included by le.hip, behind le_crypt.h): behind the data stage or the decryption stage,
// for every connection the SMP exchange among its L2CAP messages, the temporary key (TK) of a legacy pairing by trying every value
// below tk_limit against the Confirm values, the short-term key (STK) under it, as a key table the decryption stage takes as it is,
// and the long-term keys the peers distribute.  The contract is in include/btbbx.h (btbbx_le_pair_device), the reasoning in DESIGN
// 3.8.8.  All arithmetic is integer arithmetic.  AES is le_aes.h's (lx_te_entry, lx_expand, lx_aes); of le_crypt.h only LX_MAX_KEYS,
// the size of the key table the decryption stage takes.
//
//   1. le_pair_init_kernel                           the per-connection tables cleared; AES's round table; K and W
//   2. le_pair_find_kernel                           rules 1, 2 and 8: one lane per message, its class; PREQ and the LTKs by atomicMin
//   3. le_pair_prsp_, _mconf_, _sconf_, _mrand_, _srand_kernel   rule 2: each the first of its class above the one before
//   4. le_pair_method_kernel                         rules 3 and 4: method, key size, the checks as AES blocks, the job list
//   5. le_pair_search_kernel                         rule 5: one lane per (job, tk), a fixed grid over the device's count
//   6. le_pair_finish_kernel                         rule 6: the STK, cut to the key size
//   7. le_pair_slots_kernel                          rule 7: the key slots by a prefix over the connections, the table, its count
//   8. le_pair_record_kernel                         rules 8 and 9: the records
//
// 12 launches, whatever the counts and caps.  Nothing here synchronises or reads back but the host wrapper.
#pragma once
#include "le_aes.h"
#include "le_crypt.h"

#define LP_NONE       0xffffffffu
#define LP_MAX_TK     1000000u
#define LP_WGS_PER_CU 8u                   // workgroups of the search kernel per compute unit, at most
// a message's class: 1..6 the procedure messages in rule 2's order, 7 + role a distributed LTK
#define LP_PREQ  1u
#define LP_LTK   7u
// info[4 * g]: method | flags << 8 | keys << 16 | key_size << 24; + 1: the search's result; + 2: the key slot; + 3: the checks (bit per role)

static_assert(sizeof(btbbx_le_pair) == 88 && offsetof(btbbx_le_pair, ltk) == 16 && offsetof(btbbx_le_pair, preq) == 48 &&
	      offsetof(btbbx_le_pair, prsp) == 52 && offsetof(btbbx_le_pair, mconf) == 56 && offsetof(btbbx_le_pair, sconf) == 60 &&
	      offsetof(btbbx_le_pair, mrand) == 64 && offsetof(btbbx_le_pair, srand) == 68 && offsetof(btbbx_le_pair, tk) == 72 &&
	      offsetof(btbbx_le_pair, method) == 76 && offsetof(btbbx_le_pair, flags) == 77 && offsetof(btbbx_le_pair, keys) == 78 &&
	      offsetof(btbbx_le_pair, key_size) == 79 && offsetof(btbbx_le_pair, key) == 80 && offsetof(btbbx_le_pair, reserved) == 81,
	      "btbbx_le_pair layout (libbtbb_amd.LE_PAIR_DTYPE)");

struct LpArgs {
	const uint32_t *d_conn_count, *d_msg_count;
	const btbbx_le_seed *seeds;
	const btbbx_le_msg *msgs;
	const uint8_t *bytes;
	uint64_t byte_cap;
	uint32_t conn_cap, msg_cap, tk_limit, key_cap;
	uint32_t per;                          // tk_limit rounded up to whole workgroups: item t is (job t / per, tk t % per)
	btbbx_le_pair *pairs;
	uint8_t *keys;
	uint32_t *key_count;
	// scratch: per connection proc (the six procedure messages, the two LTK messages), info, blk (b, then r ^ a and conf per check,
	// as AES blocks), stk; the ARMED connections; counts[0]: how many of them, [1]: K, [2]: W
	uint32_t *te, *proc, *info, *blk, *stk, *jobs, *counts;
};

struct LpLayout {
	size_t te, proc, info, blk, stk, jobs, counts, total;
};

static LpLayout le_pair_layout(uint32_t conn_cap)
{
	LpLayout L;
	const size_t k = conn_cap ? conn_cap : 1;
	size_t at = 0;
	auto take = [&](size_t bytes) { const size_t here = at; at += ld_up(bytes); return here; };
	L.te = take(256 * 4);
	L.proc = take(k * 32);
	L.info = take(k * 16);
	L.blk = take(k * 80);
	L.stk = take(k * 16);
	L.jobs = take(k * 4);
	L.counts = take(256);
	L.total = at;
	return L;
}

// ---- 1. tables -------------------------------------------------------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_pair_init_kernel(LpArgs a)
{
	const uint32_t kh = *a.d_conn_count, wh = *a.d_msg_count;
	const uint32_t k = kh < a.conn_cap ? kh : a.conn_cap, w = wh < a.msg_cap ? wh : a.msg_cap;
	const uint64_t i = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	if (i == 0) {
		a.counts[0] = 0;
		a.counts[1] = k;
		a.counts[2] = w;
	}
	if (i < k) {
		uint4 *p = reinterpret_cast<uint4 *>(a.proc + i * 8);
		p[0] = p[1] = make_uint4(LP_NONE, LP_NONE, LP_NONE, LP_NONE);
		reinterpret_cast<uint4 *>(a.info)[i] = make_uint4(0, LP_NONE, 0xffu, 0);
		reinterpret_cast<uint4 *>(a.stk)[i] = make_uint4(0, 0, 0, 0);
	}
	if (blockIdx.x == 0)
		a.te[threadIdx.x] = lx_te_entry(threadIdx.x);
}

// ---- 2. rules 1 and 2: a message's class, the procedure ------------------------------------------------------------------------------------

// the class of record m and its connection; 0: skipped (the guards), no SMP message, or none of the table's
__device__ __forceinline__ uint32_t lp_class(const LpArgs &a, uint32_t m, uint32_t k, uint32_t &g)
{
	const btbbx_le_msg &r = a.msgs[m];
	const uint32_t need = BTBBX_LE_MSG_COMPLETE | BTBBX_LE_MSG_STORED, len = r.l2cap_len, role = r.role;
	g = r.conn;
	if (g >= k || r.byte_offset > a.byte_cap || r.bytes > a.byte_cap - r.byte_offset || r.bytes < 4u + len)
		return 0;
	if ((r.flags & need) != need || r.cid != 0x0006u || len < 1 || role > 1)
		return 0;
	const uint32_t code = a.bytes[r.byte_offset + 4];
	if (len == 7)
		return code == 1 + role ? LP_PREQ + role : 0u;
	if (len != 17)
		return 0;
	return code == 3 ? 3u + role : (code == 4 ? 5u + role : (code == 6 ? LP_LTK + role : 0u));
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_pair_find_kernel(LpArgs a)
{
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t k = a.counts[1], w = a.counts[2], m = (uint32_t)at;
	if (at >= w)
		return;
	uint32_t g;
	const uint32_t cls = lp_class(a, m, k, g);
	if (cls == LP_PREQ || cls >= LP_LTK)
		atomicMin(a.proc + 8 * (size_t)g + cls - 1, m);
}

// WHICH = 2 .. 6: the first message of that class above the one the table names
template <uint32_t WHICH> __device__ __forceinline__ void lp_next(const LpArgs &a)
{
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t k = a.counts[1], w = a.counts[2], m = (uint32_t)at;
	if (at >= w)
		return;
	uint32_t g;
	if (lp_class(a, m, k, g) != WHICH)
		return;
	const uint32_t *p = a.proc + 8 * (size_t)g;
	uint32_t before = p[WHICH - 2];
	if (WHICH == 5 && before == LP_NONE)                    // MRAND: above SCONF if there is one, else above MCONF
		before = p[2];
	if (before != LP_NONE && m > before)
		atomicMin(a.proc + 8 * (size_t)g + WHICH - 1, m);
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_pair_prsp_kernel(LpArgs a) { lp_next<2>(a); }
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_pair_mconf_kernel(LpArgs a) { lp_next<3>(a); }
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_pair_sconf_kernel(LpArgs a) { lp_next<4>(a); }
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_pair_mrand_kernel(LpArgs a) { lp_next<5>(a); }
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_pair_srand_kernel(LpArgs a) { lp_next<6>(a); }

// ---- 3. rules 3 and 4: method, checks ----------------------------------------------------------------------------------------------------

// N <= 8 octets from p, least significant first
template <int N> __device__ __forceinline__ unsigned long long lp_octets(const uint8_t *p)
{
	unsigned long long v = 0;
#pragma unroll
	for (int j = 0; j < N; j++)
		v |= (unsigned long long)p[j] << (8 * j);
	return v;
}

// octet k of message m
__device__ __forceinline__ const uint8_t *lp_at(const LpArgs &a, uint32_t m, uint32_t k) { return a.bytes + a.msgs[m].byte_offset + 4 + k; }

// the AES block of the array x[0..15] = lo | hi << 64: block[j] = x[15 - j]
__device__ __forceinline__ uint4 lp_block(unsigned long long lo, unsigned long long hi)
{
	return make_uint4(lx_bswap((uint32_t)(hi >> 32)), lx_bswap((uint32_t)hi), lx_bswap((uint32_t)(lo >> 32)), lx_bswap((uint32_t)lo));
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_pair_method_kernel(LpArgs a)
{
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t k = a.counts[1], g = (uint32_t)at;
	if (at >= k)
		return;
	const uint4 p0 = reinterpret_cast<const uint4 *>(a.proc + 8 * (size_t)g)[0], p1 = reinterpret_cast<const uint4 *>(a.proc + 8 * (size_t)g)[1];
	const uint32_t preq = p0.x, prsp = p0.y, mconf = p0.z, sconf = p0.w, mrand = p1.x, srand = p1.y;
	uint32_t flags = (preq != LP_NONE ? BTBBX_LE_PAIR_PREQ : 0u) | (prsp != LP_NONE ? BTBBX_LE_PAIR_PRSP : 0u) |
			 (mconf != LP_NONE ? BTBBX_LE_PAIR_MCONF : 0u) | (sconf != LP_NONE ? BTBBX_LE_PAIR_SCONF : 0u) |
			 (mrand != LP_NONE ? BTBBX_LE_PAIR_MRAND : 0u) | (srand != LP_NONE ? BTBBX_LE_PAIR_SRAND : 0u);
	uint32_t method = BTBBX_LE_PAIR_NONE, ks = 0, checks = 0;
	unsigned long long q7 = 0, s7 = 0;                      // preq[0..6], pres[0..6]
	if (preq != LP_NONE && prsp != LP_NONE) {
		q7 = lp_octets<7>(lp_at(a, preq, 0));
		s7 = lp_octets<7>(lp_at(a, prsp, 0));
		const uint32_t kq = (uint32_t)(q7 >> 32) & 0xffu, kr = (uint32_t)(s7 >> 32) & 0xffu;
		ks = kq < kr ? kq : kr;
		if (ks < 7 || ks > 16)
			method = BTBBX_LE_PAIR_INVALID;
		else if ((q7 >> 24) & (s7 >> 24) & 8u)
			method = BTBBX_LE_PAIR_SECURE;
		else if (((q7 >> 16) & 0xffu) == 1 && ((s7 >> 16) & 0xffu) == 1)
			method = BTBBX_LE_PAIR_OOB;
		else
			method = BTBBX_LE_PAIR_LEGACY;
	}
	if (mconf != LP_NONE && mrand != LP_NONE)
		checks |= 1u;
	if (sconf != LP_NONE && srand != LP_NONE)
		checks |= 2u;
	const btbbx_le_seed &sd = a.seeds[g];
	const bool armed = method == BTBBX_LE_PAIR_LEGACY && (sd.flags & BTBBX_LE_SEED_SEEDED) && checks && a.tk_limit >= 1;
	if (armed) {
		flags |= BTBBX_LE_PAIR_ARMED;
		const unsigned long long iat = sd.tx_add & 1u, rat = sd.rx_add & 1u;
		const unsigned long long adv = lp_octets<6>(sd.adv_a), init = lp_octets<6>(sd.init_a);
		const unsigned long long a_lo = iat | (rat << 8) | (q7 << 16), a_hi = (q7 >> 48) | (s7 << 8);
		uint4 *o = reinterpret_cast<uint4 *>(a.blk + 20 * (size_t)g);
		o[0] = lp_block(adv | (init << 48), init >> 16);
		for (uint32_t c = 0; c < 2; c++) {
			if (!(checks & (1u << c)))
				continue;
			const uint32_t rnd = c ? srand : mrand, conf = c ? sconf : mconf;
			o[1 + 2 * c] = lp_block(lp_octets<8>(lp_at(a, rnd, 1)) ^ a_lo, lp_octets<8>(lp_at(a, rnd, 9)) ^ a_hi);
			o[2 + 2 * c] = lp_block(lp_octets<8>(lp_at(a, conf, 1)), lp_octets<8>(lp_at(a, conf, 9)));
		}
		a.jobs[atomicAdd(a.counts, 1u)] = g;
	}
	uint32_t *info = a.info + 4 * (size_t)g;
	info[0] = method | (flags << 8) | (ks << 24);
	info[3] = checks;
}

// ---- 4. rule 5: the search -----------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ LxBlock lp_from(const uint4 v)
{
	LxBlock b;
	b.w[0] = v.x;
	b.w[1] = v.y;
	b.w[2] = v.z;
	b.w[3] = v.w;
	return b;
}

// does the check (ra, b, conf) hold under the schedule rk?  AES(AES(r ^ a) ^ b) == conf, all as blocks
__device__ __forceinline__ bool lp_holds(const uint32_t *te, const uint32_t (&rk)[LX_RK], const uint4 ra, const uint4 b, const uint4 conf)
{
	LxBlock x = lx_aes(te, rk, lp_from(ra));
	x.w[0] ^= b.x;
	x.w[1] ^= b.y;
	x.w[2] ^= b.z;
	x.w[3] ^= b.w;
	x = lx_aes(te, rk, x);
	return x.w[0] == conf.x && x.w[1] == conf.y && x.w[2] == conf.z && x.w[3] == conf.w;
}

// key octets 0..11 zero, 12..15 = BE32(tk), as lx_expand's little-endian words
__device__ __forceinline__ void lp_schedule(const uint32_t *te, uint32_t tk, uint32_t (&rk)[LX_RK])
{
	rk[0] = rk[1] = rk[2] = 0;
	rk[3] = lx_bswap(tk);
	lx_expand(te, rk);
}

// A fixed grid strides over the items t = job * per + tk of the device's count, 64 bits wide.  per is a multiple of the workgroup's
// size, so a workgroup's lanes take consecutive tk of ONE job and the job's blocks are uniform
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_pair_search_kernel(LpArgs a)
{
	__shared__ uint32_t te[256];
	te[threadIdx.x] = a.te[threadIdx.x];
	__syncthreads();
	const uint64_t all = (uint64_t)a.counts[0] * a.per;
	for (uint64_t t0 = (uint64_t)blockIdx.x * LE_THREADS; t0 < all; t0 += (uint64_t)gridDim.x * LE_THREADS) {
		const uint32_t g = a.jobs[t0 / a.per], tk = (uint32_t)(t0 % a.per) + threadIdx.x;
		uint32_t *result = a.info + 4 * (size_t)g + 1;
		if (tk >= a.tk_limit || tk >= __atomic_load_n(result, __ATOMIC_RELAXED))   // (a larger tk than one that holds cannot win)
			continue;
		const uint4 *blk = reinterpret_cast<const uint4 *>(a.blk + 20 * (size_t)g);
		const uint32_t checks = a.info[4 * (size_t)g + 3];      // 1 or 3: SCONF stands above MCONF and SRAND above MRAND (rule 2)
		uint32_t rk[LX_RK];
		lp_schedule(te, tk, rk);
		bool ok = lp_holds(te, rk, blk[1], blk[0], blk[2]);
		if (ok && checks == 3u)                                 // the peripheral's, only after the central's held
			ok = lp_holds(te, rk, blk[3], blk[0], blk[4]);
		if (ok)
			atomicMin(result, tk);
	}
}

// ---- 5. rule 6: the STK ----------------------------------------------------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_pair_finish_kernel(LpArgs a)
{
	__shared__ uint32_t te[256];
	te[threadIdx.x] = a.te[threadIdx.x];
	__syncthreads();
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t k = a.counts[1], g = (uint32_t)at;
	if (at >= k)
		return;
	uint32_t *info = a.info + 4 * (size_t)g;
	const uint32_t tk = info[1];
	if (tk == LP_NONE)
		return;
	uint32_t x = info[0] | (BTBBX_LE_PAIR_CRACKED << 8);
	const uint32_t mrand = a.proc[8 * (size_t)g + 4], srand = a.proc[8 * (size_t)g + 5], ks = x >> 24;
	if (mrand != LP_NONE && srand != LP_NONE) {
		uint32_t rk[LX_RK];
		lp_schedule(te, tk, rk);
		const LxBlock o = lx_aes(te, rk, lp_from(lp_block(lp_octets<8>(lp_at(a, mrand, 1)), lp_octets<8>(lp_at(a, srand, 1)))));
		const uint32_t zero = 16u - ks;                         // output octets 0 .. 15 - ks
		uint32_t v[4];
#pragma unroll
		for (uint32_t w = 0; w < 4; w++)
			v[w] = zero >= 4 * w + 4 ? 0u : (zero <= 4 * w ? o.w[w] : o.w[w] & (0xffffffffu << (8 * (zero - 4 * w))));
		reinterpret_cast<uint4 *>(a.stk)[g] = make_uint4(v[0], v[1], v[2], v[3]);
		x |= BTBBX_LE_PAIR_KEY_STK << 16;
	}
	info[0] = x;
}

// ---- 6. rule 7: the key table ------------------------------------------------------------------------------------------------------------------

// one workgroup walks the connections 256 at a time: a connection's slot is the number of connections with an STK in front of it
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_pair_slots_kernel(LpArgs a)
{
	__shared__ uint32_t wave_sum[LE_THREADS / 64];
	const uint32_t k = a.counts[1], lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	uint32_t base = 0;
	for (uint64_t g0 = 0; g0 < k; g0 += LE_THREADS) {
		const uint64_t g = g0 + threadIdx.x;
		const bool has = g < k && ((a.info[4 * g] >> 16) & BTBBX_LE_PAIR_KEY_STK);
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
			if (slot < a.key_cap) {
				const uint4 v = reinterpret_cast<const uint4 *>(a.stk)[g];
				const uint32_t w[4] = {v.x, v.y, v.z, v.w};
				uint8_t *o = a.keys + 16 * (size_t)slot;
#pragma unroll
				for (int j = 0; j < 16; j++)
					o[j] = (uint8_t)(w[j >> 2] >> (8 * (j & 3)));
				a.info[4 * g + 2] = slot;
			}
		}
		base += total;
		__syncthreads();
	}
	if (threadIdx.x == 0)
		*a.key_count = base;
	for (uint32_t j = 16 * (base < a.key_cap ? base : a.key_cap) + threadIdx.x; j < 16 * a.key_cap; j += LE_THREADS)
		a.keys[j] = 0;
}

// ---- 7. rules 8 and 9: the records -------------------------------------------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_pair_record_kernel(LpArgs a)
{
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t k = a.counts[1], g = (uint32_t)at;
	if (at >= k)
		return;
	const uint4 p0 = reinterpret_cast<const uint4 *>(a.proc + 8 * (size_t)g)[0], p1 = reinterpret_cast<const uint4 *>(a.proc + 8 * (size_t)g)[1];
	const uint4 info = reinterpret_cast<const uint4 *>(a.info)[g], stk = reinterpret_cast<const uint4 *>(a.stk)[g];
	uint4 ltk[2];
	uint32_t keys = 0;
#pragma unroll
	for (uint32_t r = 0; r < 2; r++) {                      // ltk[role][j] = v[16 - j]
		const uint32_t m = r ? p1.w : p1.z;
		ltk[r] = make_uint4(0, 0, 0, 0);
		if (m != LP_NONE) {
			ltk[r] = lp_block(lp_octets<8>(lp_at(a, m, 1)), lp_octets<8>(lp_at(a, m, 9)));
			keys |= BTBBX_LE_PAIR_KEY_LTK_CENTRAL << r;
		}
	}
	uint2 *o = reinterpret_cast<uint2 *>(a.pairs + g);
	o[0] = make_uint2(stk.x, stk.y);
	o[1] = make_uint2(stk.z, stk.w);
	o[2] = make_uint2(ltk[0].x, ltk[0].y);
	o[3] = make_uint2(ltk[0].z, ltk[0].w);
	o[4] = make_uint2(ltk[1].x, ltk[1].y);
	o[5] = make_uint2(ltk[1].z, ltk[1].w);
	o[6] = make_uint2(p0.x, p0.y);
	o[7] = make_uint2(p0.z, p0.w);
	o[8] = make_uint2(p1.x, p1.y);
	o[9] = make_uint2(info.y, info.x | (keys << 16));
	o[10] = make_uint2(info.z & 0xffu, 0u);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------

extern "C" size_t btbbx_le_pair_scratch_bytes(uint32_t conn_cap) { return le_pair_layout(conn_cap).total; }

// the 12 launches of one run
static int le_pair_launch(const uint32_t *d_conn_count, uint32_t conn_cap, const btbbx_le_seed *d_seeds, const btbbx_le_msg *d_msgs,
			  const uint32_t *d_msg_count, uint32_t msg_cap, const uint8_t *d_bytes, uint64_t byte_cap, uint32_t tk_limit,
			  btbbx_le_pair *d_pairs, uint8_t *d_keys, uint32_t key_cap, uint32_t *d_key_count, void *d_scratch, hipStream_t q)
{
	const LpLayout L = le_pair_layout(conn_cap);
	char *s = (char *)d_scratch;
	LpArgs a;
	a.d_conn_count = d_conn_count;
	a.d_msg_count = d_msg_count;
	a.seeds = d_seeds;
	a.msgs = d_msgs;
	a.bytes = d_bytes;
	a.byte_cap = byte_cap;
	a.conn_cap = conn_cap;
	a.msg_cap = msg_cap;
	a.tk_limit = tk_limit;
	a.key_cap = key_cap;
	a.per = (tk_limit + LE_THREADS - 1) / LE_THREADS * LE_THREADS;
	a.pairs = d_pairs;
	a.keys = d_keys;
	a.key_count = d_key_count;
	a.te = (uint32_t *)(s + L.te);
	a.proc = (uint32_t *)(s + L.proc);
	a.info = (uint32_t *)(s + L.info);
	a.blk = (uint32_t *)(s + L.blk);
	a.stk = (uint32_t *)(s + L.stk);
	a.jobs = (uint32_t *)(s + L.jobs);
	a.counts = (uint32_t *)(s + L.counts);
	const auto blocks = [](uint64_t items) { return (uint32_t)std::max<uint64_t>((items + LE_THREADS - 1) / LE_THREADS, 1); };
	const dim3 per_conn(blocks(conn_cap)), per_msg(blocks(msg_cap)), wg(LE_THREADS), one(1);
	// the search: every (connection, tk) the caps allow, but no more workgroups than stay resident
	const dim3 search((uint32_t)std::min<uint64_t>(blocks((uint64_t)conn_cap * a.per), (uint64_t)ctx().num_cus * LP_WGS_PER_CU));
	hipLaunchKernelGGL(le_pair_init_kernel, per_conn, wg, 0, q, a);
	hipLaunchKernelGGL(le_pair_find_kernel, per_msg, wg, 0, q, a);
	hipLaunchKernelGGL(le_pair_prsp_kernel, per_msg, wg, 0, q, a);
	hipLaunchKernelGGL(le_pair_mconf_kernel, per_msg, wg, 0, q, a);
	hipLaunchKernelGGL(le_pair_sconf_kernel, per_msg, wg, 0, q, a);
	hipLaunchKernelGGL(le_pair_mrand_kernel, per_msg, wg, 0, q, a);
	hipLaunchKernelGGL(le_pair_srand_kernel, per_msg, wg, 0, q, a);
	hipLaunchKernelGGL(le_pair_method_kernel, per_conn, wg, 0, q, a);
	hipLaunchKernelGGL(le_pair_search_kernel, search, wg, 0, q, a);
	hipLaunchKernelGGL(le_pair_finish_kernel, per_conn, wg, 0, q, a);
	hipLaunchKernelGGL(le_pair_slots_kernel, one, wg, 0, q, a);
	hipLaunchKernelGGL(le_pair_record_kernel, per_conn, wg, 0, q, a);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

static int le_pair_check_limits(const char *who, uint32_t tk_limit, uint32_t key_cap)
{
	if (tk_limit > LP_MAX_TK || key_cap > LX_MAX_KEYS) {
		set_error("%s: tk_limit must be 0..%u and key_cap 0..%u", who, LP_MAX_TK, LX_MAX_KEYS);
		return BTBBX_E_ARG;
	}
	return BTBBX_OK;
}

extern "C" int btbbx_le_pair_device(const uint32_t *d_conn_count, uint32_t conn_cap, const btbbx_le_seed *d_seeds, const btbbx_le_msg *d_msgs,
				    const uint32_t *d_msg_count, uint32_t msg_cap, const uint8_t *d_bytes, uint64_t byte_cap, uint32_t tk_limit,
				    btbbx_le_pair *d_pairs, uint8_t *d_keys, uint32_t key_cap, uint32_t *d_key_count, void *d_scratch,
				    size_t scratch_bytes, void *hip_stream)
{
	const char *who = "btbbx_le_pair_device";
	int rc = le_pair_check_limits(who, tk_limit, key_cap);
	if (rc)
		return rc;
	const LpLayout L = le_pair_layout(conn_cap);
	if (!d_conn_count || !d_seeds || (!d_msgs && msg_cap) || !d_msg_count || (!d_bytes && byte_cap) || !d_pairs || (!d_keys && key_cap) ||
	    !d_key_count || !d_scratch || scratch_bytes < L.total) {
		set_error("%s: null pointer, or scratch of %zu bytes needed and %zu given", who, L.total, scratch_bytes);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_seeds & 7) || ((uintptr_t)d_msgs & 7) || ((uintptr_t)d_pairs & 7) || ((uintptr_t)d_conn_count & 3) ||
	    ((uintptr_t)d_msg_count & 3) || ((uintptr_t)d_key_count & 3) || ((uintptr_t)d_scratch & 15)) {
		set_error("%s: misaligned pointer (scratch 16 bytes; the records 8; the counters 4)", who);
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	hipStream_t q = (hipStream_t)hip_stream;
	if (!conn_cap) {
		HIP_TRY(hipMemsetAsync(d_key_count, 0, sizeof(uint32_t), q));
		if (key_cap)
			HIP_TRY(hipMemsetAsync(d_keys, 0, 16 * (size_t)key_cap, q));
		return BTBBX_OK;
	}
	return le_pair_launch(d_conn_count, conn_cap, d_seeds, d_msgs, d_msg_count, msg_cap, d_bytes, byte_cap, tk_limit, d_pairs, d_keys, key_cap,
			      d_key_count, d_scratch, q);
}
