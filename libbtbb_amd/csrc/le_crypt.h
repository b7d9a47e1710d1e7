// le_crypt.h -- LE decryption (included by le.hip, behind le_data.h): behind the data stage, for every connection whose LL_ENC_REQ,
// LL_ENC_RSP and LL_START_ENC_REQ are in the capture the session key under one of the caller's long-term keys, for every encrypted
// packet its packet counter, and the L2CAP messages once more, over plaintext.  The contract is in include/btbbx.h
// (btbbx_le_crypt_device), the reasoning in DESIGN 3.8.7.  All arithmetic is integer arithmetic.
//
// The slot table is the data stage's (slot first + rank holds the member of that rank) and is built again from the same input, so
// the stage reads nothing of the data stage's scratch.  The scans run on le_data.h's frame (ldt_tile, ldt_prefix, ldt_block_scan):
//
//   1. le_crypt_init_kernel, le_data_slot_kernel     the slot table; the whitening table; AES's round table, from the field's definition
//   2. le_crypt_find_kernel, _rsp_, _begin_          rule 2: a slot's packed state, the procedure PDUs; REQ, RSP above it, START above that
//   3. le_crypt_sched_kernel                         rule 3: per (connection, key) the session key and its schedule
//   4. le_crypt_ord_*    (sum, prefix, apply)        rule 4: a member's state, its ordinal per (connection, role), the four probes
//   5. le_crypt_probe_kernel, le_crypt_key_kernel    rule 6: one lane per (probe, key), the skews in turn; the connection's key
//   6. le_crypt_first_kernel, le_crypt_retry_kernel  rule 7: skew 0 for every member; (member, skew >= 1) for those still unverified
//   7. le_crypt_effect_kernel                        rule 8: the effective length and kind, a VERIFIED member's first four octets
//   8. le_data_msg_*, le_data_close_kernel, le_crypt_number_*     the data stage's rules 5 and 6 over the effective members: its own
//                                                     kernels where the rule reads nothing of this stage's, launched with the frame's part of the arguments
//   9. le_crypt_pkt_kernel, le_crypt_conn_kernel     the records
//  10. le_crypt_plain_kernel                         one lane per 16 octets of a fragment: keystream, plaintext to its place in d_bytes
//
// 24 launches, whatever the counts, caps, keys and window.  Nothing here synchronises or reads back but the host wrapper.
#pragma once
#include "le_data.h"
#include "le_aes.h"

#define LX_NONE      0xffffffffu
#define LX_MAX_KEYS  64u
#define LX_MAX_SKEW  32u
#define LX_GRID      (1u << 20)            // workgroups of a grid-stride launch, at most
// base[q]: sinfo's fields (length | (header0 & 0x1f) << 8 | role << 14 | kind << 17 | phase << 24) and the procedure class << 21
#define LX_CLASS(x)  (((x) >> 21) & 3u)    // 1 ENC_REQ, 2 ENC_RSP, 3 START_ENC_REQ
// cst[q]: state | skew << 8 | opcode << 16; until le_crypt_effect_kernel the state alone, LX_ENCRYPTED for a member that will be tried
#define LX_ENCRYPTED 5u

static_assert(sizeof(btbbx_le_crypt) == 56 && offsetof(btbbx_le_crypt, iv) == 16 && offsetof(btbbx_le_crypt, req) == 24 &&
	      offsetof(btbbx_le_crypt, rsp) == 28 && offsetof(btbbx_le_crypt, start) == 32 && offsetof(btbbx_le_crypt, n_encrypted) == 36 &&
	      offsetof(btbbx_le_crypt, n_verified) == 40 && offsetof(btbbx_le_crypt, n_failed) == 44 && offsetof(btbbx_le_crypt, n_skipped) == 48 &&
	      offsetof(btbbx_le_crypt, key) == 52 && offsetof(btbbx_le_crypt, max_skew) == 53 && offsetof(btbbx_le_crypt, flags) == 54 &&
	      offsetof(btbbx_le_crypt, reserved) == 55, "btbbx_le_crypt layout (libbtbb_amd.LE_CRYPT_DTYPE)");
static_assert(sizeof(btbbx_le_crypt_pkt) == 16 && offsetof(btbbx_le_crypt_pkt, ordinal) == 4 && offsetof(btbbx_le_crypt_pkt, state) == 8 &&
	      offsetof(btbbx_le_crypt_pkt, skew) == 9 && offsetof(btbbx_le_crypt_pkt, opcode) == 10 && offsetof(btbbx_le_crypt_pkt, counter_hi) == 11 &&
	      offsetof(btbbx_le_crypt_pkt, reserved) == 12, "btbbx_le_crypt_pkt layout (libbtbb_amd.LE_CRYPT_PKT_DTYPE)");

// what every kernel of the stage is launched with: the frame's arguments over this stage's own arrays (sinfo: the EFFECTIVE members;
// dpkts: the records under them) and what the frame does not know
struct LxArgs : LdtArgs {
	const btbbx_le_data_pkt *in_dpkts;     // the data stage's
	const uint8_t *keys;
	uint32_t n_keys, window;
	// scratch: per slot; per connection (proc: the slots of REQ, RSP, START; probe: four slots; ctal: encrypted, verified, failed,
	// skipped, max skew, a member; civ: IVm, IVs); per (connection, key) the score and the schedule; counts[0]: the members to try again
	uint32_t *te, *base, *ord, *cst, *skew, *hdr4, *retry, *proc, *probe, *ctal, *ckey, *civ, *score, *sched, *counts;
	btbbx_le_crypt *crypt;
	btbbx_le_crypt_pkt *cpkts;
};

struct LxLayout {
	LdtLayout frame;
	size_t te, base, ord, cst, skew, hdr4, retry, proc, probe, ctal, ckey, civ, score, sched, counts, total;
};

static LxLayout le_crypt_layout(uint32_t cand_cap, uint32_t conn_cap, uint32_t n_keys)
{
	LxLayout L;
	L.frame = le_data_layout(cand_cap, conn_cap);
	const size_t c = cand_cap ? cand_cap : 1, k = conn_cap ? conn_cap : 1, nk = n_keys ? n_keys : 1;
	size_t at = L.frame.total;
	auto take = [&](size_t bytes) { const size_t here = at; at += ld_up(bytes); return here; };
	L.te = take(256 * 4);
	L.base = take(c * 4);
	L.ord = take(c * 4);
	L.cst = take(c * 4);
	L.skew = take(c * 4);
	L.hdr4 = take(c * 4);
	L.retry = take(c * 4);
	L.proc = take(k * 16);
	L.probe = take(k * 16);
	L.ctal = take(k * 32);
	L.ckey = take(k * 4);
	L.civ = take(k * 8);
	L.score = take(k * nk * 4);
	L.sched = take(k * nk * LX_RK * 4);
	L.counts = take(256);
	L.total = at;
	return L;
}

__device__ __forceinline__ const LxArgs &lx_args(const LdtArgs &a) { return static_cast<const LxArgs &>(a); }

// the tables of a workgroup: te and the data stage's whitening table.  Every thread of the workgroup calls it, before any return
__device__ __forceinline__ void lx_tables(const LxArgs &a, uint32_t *te, unsigned long long *wt)
{
	te[threadIdx.x] = a.te[threadIdx.x];
	if (threadIdx.x < 127)
		wt[threadIdx.x] = a.wtab[threadIdx.x];
	__syncthreads();
}

// ---- rule 5: a trial (a member's payload is read by the data stage's ldt_where and ldt_octets) --------------------------------------

// A_i (flags 0x01) or B0 (flags 0x49) of rule 5: flags | nonce | BE16(last)
__device__ __forceinline__ LxBlock lx_nonce_block(uint32_t flags, unsigned long long c, uint32_t dir, uint32_t ivm, uint32_t ivs, uint32_t last)
{
	LxBlock b;
	const uint32_t c32 = (uint32_t)c, n4 = ((uint32_t)(c >> 32) & 0x7fu) | (dir << 7);
	b.w[0] = flags | (c32 << 8);
	b.w[1] = (c32 >> 24) | (n4 << 8) | (ivm << 16);
	b.w[2] = (ivm >> 16) | (ivs << 16);
	b.w[3] = (ivs >> 16) | ((last >> 8) << 16) | ((last & 0xffu) << 24);
	return b;
}

// Rule 5: does the member in slot q (L >= 5) verify under the schedule rk with counter c?
__device__ __forceinline__ bool lx_trial(const LxArgs &a, const uint32_t *te, const unsigned long long *wt, const uint32_t (&rk)[LX_RK], uint32_t q,
					 uint32_t x, uint32_t g, unsigned long long c)
{
	const LdtWhere p = ldt_where(a, q, x);
	const uint32_t m = (x & 0xffu) - 4u, dir = LDT_ROLE(x) == BTBBX_LE_ROLE_CENTRAL ? 1u : 0u;
	const uint32_t ivm = a.civ[2 * (size_t)g], ivs = a.civ[2 * (size_t)g + 1];
	const LxBlock s0 = lx_aes(te, rk, lx_nonce_block(0x01u, c, dir, ivm, ivs, 0));
	LxBlock xb = lx_aes(te, rk, lx_nonce_block(0x49u, c, dir, ivm, ivs, m));
	xb.w[0] ^= 0x0100u | ((p.h0 & 0xe3u) << 16);
	xb = lx_aes(te, rk, xb);
#pragma unroll 1
	for (uint32_t k = 0; k < m; k += 16) {
		const LxBlock s = lx_aes(te, rk, lx_nonce_block(0x01u, c, dir, ivm, ivs, k / 16 + 1));
		unsigned long long lo = ldt_octets(a, p, wt, k) ^ (((unsigned long long)s.w[1] << 32) | s.w[0]);
		unsigned long long hi = ldt_octets(a, p, wt, k + 8) ^ (((unsigned long long)s.w[3] << 32) | s.w[2]);
		const uint32_t rem = m - k;                             // the last block is padded with zeros
		if (rem < 8)
			lo &= (1ull << (8 * rem)) - 1;
		if (rem <= 8)
			hi = 0;
		else if (rem < 16)
			hi &= (1ull << (8 * (rem - 8))) - 1;
		xb.w[0] ^= (uint32_t)lo;
		xb.w[1] ^= (uint32_t)(lo >> 32);
		xb.w[2] ^= (uint32_t)hi;
		xb.w[3] ^= (uint32_t)(hi >> 32);
		xb = lx_aes(te, rk, xb);
	}
	return (xb.w[0] ^ s0.w[0]) == (uint32_t)ldt_octets(a, p, wt, m);
}

// ---- 1. slots, tables ------------------------------------------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_init_kernel(LxArgs a)
{
	const uint64_t i = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	ldt_init_frame(a, i, [=] {
		uint4 *t = reinterpret_cast<uint4 *>(a.ctal + i * 8);
		t[0] = t[1] = make_uint4(0, 0, 0, 0);
		reinterpret_cast<uint4 *>(a.proc)[i] = reinterpret_cast<uint4 *>(a.probe)[i] = make_uint4(LX_NONE, LX_NONE, LX_NONE, LX_NONE);
		a.ckey[i] = 0xffu;
		a.civ[2 * i] = a.civ[2 * i + 1] = 0;
		for (uint32_t j = 0; j < a.n_keys; j++)
			a.score[i * a.n_keys + j] = 0;
	});
	if (i == 0)
		a.counts[0] = 0;
	if (blockIdx.x == 0) {
		a.te[threadIdx.x] = lx_te_entry(threadIdx.x);
		if (threadIdx.x < 127)
			ldt_init_whitening(a, threadIdx.x);
	}
}

// ---- 2. rules 1 and 2: COUNTING members, the procedure PDUs ----------------------------------------------------------------------------

__device__ __forceinline__ bool lx_counting(uint32_t x)
{
	return LDT_ROLE(x) < 2 && LDT_KIND(x) != BTBBX_LE_DATA_RETRANSMIT && LDT_KIND(x) != BTBBX_LE_DATA_UNKNOWN;
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_find_kernel(LxArgs a)
{
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t n = a.params[0], q = (uint32_t)at;
	if (at >= n)
		return;
	const uint32_t i = a.slot[q];
	if (i == LX_NONE) {
		a.sg[q] = LX_NONE;
		a.base[q] = 3u << 14;
		return;
	}
	const uint2 c = reinterpret_cast<const uint2 *>(a.cands + i)[2];            // stream | header0 << 16 | length << 24, conn
	const uint32_t ch = reinterpret_cast<const uint4 *>(a.pkts)[i].w & 0x3fu;
	const uint32_t tail = reinterpret_cast<const uint32_t *>(a.in_dpkts + i)[2];   // role | kind << 8 | bits << 16
	const uint32_t role = (tail & 0xffu) < 2 ? tail & 0xffu : 2u, kind = role < 2 ? (tail >> 8) & 7u : (uint32_t)BTBBX_LE_DATA_UNKNOWN;
	const uint32_t len = c.x >> 24, llid = (c.x >> 16) & 3u;
	uint32_t x = len | (((c.x >> 16) & 0x1fu) << 8) | (role << 14) | (kind << 17) | (a.wphase[0x40u | ch] << 24);
	if (lx_counting(x) && llid == 3 && len >= 1) {
		const LdtWhere p = ldt_where(a, q, x);
		const uint32_t op = (uint32_t)ldt_octets(a, p, a.wtab, 0) & 0xffu;
		uint32_t cls = 0;
		if (role == BTBBX_LE_ROLE_CENTRAL && len == 23 && op == 0x03u)
			cls = 1;
		else if (role == BTBBX_LE_ROLE_PERIPHERAL && len == 13 && op == 0x04u)
			cls = 2;
		else if (role == BTBBX_LE_ROLE_PERIPHERAL && len == 1 && op == 0x05u)
			cls = 3;
		x |= cls << 21;
		if (cls == 1)
			atomicMin(a.proc + 4 * (size_t)c.y, q);
	}
	a.sg[q] = c.y;
	a.base[q] = x;
	a.ctal[8 * (size_t)c.y + 5] = 1;                        // the connection has a member
}

// WHICH = 2: the ENC_RSP of the smallest rank above REQ's; 3: the START of the smallest rank above RSP's
template <uint32_t WHICH> __device__ __forceinline__ void lx_next(const LxArgs &a)
{
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t n = a.params[0], q = (uint32_t)at;
	if (at >= n)
		return;
	const uint32_t g = a.sg[q];
	if (g == LX_NONE || LX_CLASS(a.base[q]) != WHICH)
		return;
	const uint32_t before = a.proc[4 * (size_t)g + WHICH - 2];
	if (before != LX_NONE && q > before)
		atomicMin(a.proc + 4 * (size_t)g + WHICH - 1, q);
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_rsp_kernel(LxArgs a) { lx_next<2>(a); }
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_begin_kernel(LxArgs a) { lx_next<3>(a); }

__device__ __forceinline__ bool lx_armed(const LxArgs &a, uint32_t g) { return a.proc[4 * (size_t)g + 2] != LX_NONE; }

// ---- 3. rule 3: the session keys -----------------------------------------------------------------------------------------------------

// one lane per (ARMED connection, key): SK = AES(key, the reversed SKD); its schedule
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_sched_kernel(LxArgs a)
{
	__shared__ uint32_t te[256];
	__shared__ unsigned long long wt[128];
	lx_tables(a, te, wt);
	const uint64_t all = (uint64_t)a.params[1] * a.n_keys;
	for (uint64_t t = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x; t < all; t += (uint64_t)gridDim.x * LE_THREADS) {
		const uint32_t g = (uint32_t)(t / a.n_keys), kk = (uint32_t)(t % a.n_keys);
		if (!lx_armed(a, g))
			continue;
		const uint32_t q_req = a.proc[4 * (size_t)g], q_rsp = a.proc[4 * (size_t)g + 1];
		const LdtWhere req = ldt_where(a, q_req, a.base[q_req]), rsp = ldt_where(a, q_rsp, a.base[q_rsp]);
		const unsigned long long skdm = ldt_octets(a, req, wt, 11), skds = ldt_octets(a, rsp, wt, 1);
		uint32_t rk[LX_RK];
#pragma unroll
		for (int w = 0; w < 4; w++) {
			const uint8_t *b = a.keys + 16 * (size_t)kk + 4 * w;
			rk[w] = b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
		}
		lx_expand(te, rk);
		LxBlock in;                                             // block[j] = skd[15 - j]
		in.w[0] = lx_bswap((uint32_t)(skds >> 32));
		in.w[1] = lx_bswap((uint32_t)skds);
		in.w[2] = lx_bswap((uint32_t)(skdm >> 32));
		in.w[3] = lx_bswap((uint32_t)skdm);
		const LxBlock sk = lx_aes(te, rk, in);
#pragma unroll
		for (int w = 0; w < 4; w++)
			rk[w] = sk.w[w];
		lx_expand(te, rk);
		uint4 *o = reinterpret_cast<uint4 *>(a.sched + (size_t)t * LX_RK);
#pragma unroll
		for (int j = 0; j < (int)LX_RK / 4; j++)
			o[j] = make_uint4(rk[4 * j], rk[4 * j + 1], rk[4 * j + 2], rk[4 * j + 3]);
		if (kk == 0) {
			a.civ[2 * (size_t)g] = (uint32_t)ldt_octets(a, req, wt, 19);
			a.civ[2 * (size_t)g + 1] = (uint32_t)ldt_octets(a, rsp, wt, 9);
		}
	}
}

// ---- 4. rule 4: the members' states, the ordinals, the probes -------------------------------------------------------------------------------

// state: w0 bit 0 = a connection begins (what lies in front is cut off); w1 + r = the ENCRYPTED members of role r
struct LxOrd {
	static constexpr int NW = 3;
	typedef LdtState<NW> S;
	static __device__ __forceinline__ S combine(const S &x, const S &y)
	{
		if (y.w[0] & 1u)
			return y;
		S r;
		r.w[0] = x.w[0] | y.w[0];
		r.w[1] = x.w[1] + y.w[1];
		r.w[2] = x.w[2] + y.w[2];
		return r;
	}
	static __device__ __forceinline__ S value(const LdtArgs &d, uint32_t q, uint32_t n, LdtSlot &sl)
	{
		const LxArgs &a = lx_args(d);
		S v = ldt_zero<NW>();
		sl.g = a.sg[q];
		sl.x = a.base[q];
		const bool first = sl.g == LX_NONE || ldt_first(a.sg, q, sl.g);
		uint32_t st = BTBBX_LE_CRYPT_CLEAR;
		if (sl.g != LX_NONE && lx_armed(a, sl.g) && q > a.proc[4 * (size_t)sl.g + 2]) {
			const uint32_t len = sl.x & 0xffu, llid = (sl.x >> 8) & 3u;
			if (!lx_counting(sl.x))
				st = len ? BTBBX_LE_CRYPT_SKIPPED : BTBBX_LE_CRYPT_CLEAR;
			else if (llid && len)
				st = len >= 5 ? LX_ENCRYPTED : BTBBX_LE_CRYPT_SHORT;
		}
		sl.y = (first ? 1u : 0u) | (st << 1);
		v.w[0] = first ? 1u : 0u;
		if (st == LX_ENCRYPTED) {
			v.w[1] = LDT_ROLE(sl.x) ? 0u : 1u;
			v.w[2] = LDT_ROLE(sl.x) ? 1u : 0u;
		}
		return v;
	}
	static __device__ __forceinline__ void emit(const LdtArgs &d, uint32_t q, uint32_t n, bool live, const LdtSlot &sl, const S &ex, const S &in)
	{
		const LxArgs &a = lx_args(d);
		if (!live)
			return;
		const uint32_t st = sl.y >> 1;
		uint32_t ord = 0;
		if (st == LX_ENCRYPTED) {
			const uint32_t e0 = (sl.y & 1u) ? 0u : ex.w[1], e1 = (sl.y & 1u) ? 0u : ex.w[2];
			ord = LDT_ROLE(sl.x) ? e1 : e0;
			if (e0 + e1 < 4)                                // one of the connection's first four: a probe
				a.probe[4 * (size_t)sl.g + e0 + e1] = q;
		}
		a.ord[q] = ord;
		a.cst[q] = st;
		a.skew[q] = 0xffu;
	}
};

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_ord_sum_kernel(LxArgs a) { ldt_tile<LxOrd, false>(a); }
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_ord_prefix_kernel(LxArgs a) { ldt_prefix<LxOrd>(a); }
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_ord_kernel(LxArgs a) { ldt_tile<LxOrd, true>(a); }

// ---- 5. rule 6: the connection's key -------------------------------------------------------------------------------------------------

// one lane per (connection, probe, key): the skews in turn until one verifies
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_probe_kernel(LxArgs a)
{
	__shared__ uint32_t te[256];
	__shared__ unsigned long long wt[128];
	lx_tables(a, te, wt);
	const uint64_t all = (uint64_t)a.params[1] * 4 * a.n_keys;
	for (uint64_t t = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x; t < all; t += (uint64_t)gridDim.x * LE_THREADS) {
		const uint32_t g = (uint32_t)(t / (4 * a.n_keys)), rest = (uint32_t)(t % (4 * a.n_keys)), kk = rest % a.n_keys;
		const uint32_t q = a.probe[4 * (size_t)g + rest / a.n_keys];
		if (q == LX_NONE)
			continue;
		uint32_t rk[LX_RK];
		lx_load_rk(a.sched + ((size_t)g * a.n_keys + kk) * LX_RK, rk);
		const uint32_t x = a.base[q], ord = a.ord[q];
#pragma unroll 1
		for (uint32_t d = 0; d < a.window; d++)
			if (lx_trial(a, te, wt, rk, q, x, g, (unsigned long long)ord + d)) {
				atomicAdd(a.score + (size_t)g * a.n_keys + kk, 1u);
				break;
			}
	}
}

// the smallest key of the largest score, if that is >= 1
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_key_kernel(LxArgs a)
{
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	if (at >= a.params[1])
		return;
	uint32_t best = 0, key = 0xffu;
	for (uint32_t kk = 0; kk < a.n_keys; kk++) {
		const uint32_t s = a.score[at * a.n_keys + kk];
		if (s > best) {
			best = s;
			key = kk;
		}
	}
	a.ckey[at] = key;
}

// ---- 6. rule 7: the skews ---------------------------------------------------------------------------------------------------------------

// skew 0 for every ENCRYPTED member of a KEYED connection; who fails is listed for le_crypt_retry_kernel
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_first_kernel(LxArgs a)
{
	__shared__ uint32_t te[256];
	__shared__ unsigned long long wt[128];
	lx_tables(a, te, wt);
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t n = a.params[0], q = (uint32_t)at;
	if (at >= n || a.cst[q] != LX_ENCRYPTED)
		return;
	const uint32_t g = a.sg[q], key = a.ckey[g];
	if (key == 0xffu)
		return;
	uint32_t rk[LX_RK];
	lx_load_rk(a.sched + ((size_t)g * a.n_keys + key) * LX_RK, rk);
	if (lx_trial(a, te, wt, rk, q, a.base[q], g, a.ord[q]))
		a.skew[q] = 0;
	else if (a.window > 1)
		a.retry[atomicAdd(a.counts, 1u)] = q;
}

// one lane per (listed member, skew 1 .. window - 1): a fixed grid that strides over what the device counted; the smallest wins
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_retry_kernel(LxArgs a)
{
	__shared__ uint32_t te[256];
	__shared__ unsigned long long wt[128];
	lx_tables(a, te, wt);
	const uint32_t per = a.window - 1;
	const uint64_t all = (uint64_t)a.counts[0] * per;
	for (uint64_t t = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x; t < all; t += (uint64_t)gridDim.x * LE_THREADS) {
		const uint32_t q = a.retry[t / per], d = 1 + (uint32_t)(t % per), g = a.sg[q];
		uint32_t rk[LX_RK];
		lx_load_rk(a.sched + ((size_t)g * a.n_keys + a.ckey[g]) * LX_RK, rk);
		if (lx_trial(a, te, wt, rk, q, a.base[q], g, (unsigned long long)a.ord[q] + d))
			atomicMin(a.skew + q, d);
	}
}

// ---- 7. rule 8: the effective members ------------------------------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_effect_kernel(LxArgs a)
{
	__shared__ uint32_t te[256];
	__shared__ unsigned long long wt[128];
	lx_tables(a, te, wt);
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t n = a.params[0], q = (uint32_t)at;
	if (at >= n)
		return;
	const uint32_t g = a.sg[q];
	uint32_t x = a.base[q] & ~(3u << 21);
	if (g == LX_NONE) {
		a.sinfo[q] = x;
		return;
	}
	uint32_t st = a.cst[q], skew = 0, opcode = 0xffu, *t = a.ctal + 8 * (size_t)g;
	if (st == LX_ENCRYPTED) {
		skew = a.skew[q];
		st = skew != 0xffu ? BTBBX_LE_CRYPT_VERIFIED : BTBBX_LE_CRYPT_FAILED;
		atomicAdd(t + 0, 1u);
		atomicAdd(t + (st == BTBBX_LE_CRYPT_VERIFIED ? 1 : 2), 1u);
	}
	if (st == BTBBX_LE_CRYPT_VERIFIED) {
		const uint32_t llid = (x >> 8) & 3u, len = (x & 0xffu) - 4u, role = LDT_ROLE(x);
		const uint32_t kind = llid == 2 ? BTBBX_LE_DATA_START : (llid == 1 ? BTBBX_LE_DATA_CONTINUATION : BTBBX_LE_DATA_CONTROL);
		uint32_t rk[LX_RK];
		lx_load_rk(a.sched + ((size_t)g * a.n_keys + a.ckey[g]) * LX_RK, rk);
		const LxBlock s = lx_aes(te, rk, lx_nonce_block(0x01u, (unsigned long long)a.ord[q] + skew, role == BTBBX_LE_ROLE_CENTRAL ? 1u : 0u,
								 a.civ[2 * (size_t)g], a.civ[2 * (size_t)g + 1], 1));
		const uint32_t plain = (uint32_t)ldt_octets(a, ldt_where(a, q, x), wt, 0) ^ s.w[0];
		a.hdr4[q] = plain;
		if (llid == 3)
			opcode = plain & 0xffu;
		x = (x & ~(0xffu | (7u << 17))) | len | (kind << 17);
		atomicMax(t + 4, skew);
	} else if (st != BTBBX_LE_CRYPT_CLEAR) {
		x = (x & ~(7u << 17)) | (BTBBX_LE_DATA_IGNORED << 17);
		if (st == BTBBX_LE_CRYPT_SKIPPED)
			atomicAdd(t + 3, 1u);
	}
	a.sinfo[q] = x;
	a.cst[q] = st | (skew << 8) | (opcode << 16);
}

// ---- 8. the data stage's rules 5 and 6 over the effective members -------------------------------------------------------------------

// (LdtMsg and le_data_close_kernel read sg and sinfo and nothing of the streams: over this stage's sinfo they are rule 8 as it stands,
// and le_crypt_launch launches the data stage's kernels)

// LdtNumber without the data records' tallies; the L2CAP header of a VERIFIED START is its stashed plaintext
struct LxNumber {
	static constexpr int NW = 3;
	typedef LdtState<NW> S;
	static __device__ __forceinline__ S combine(const S &x, const S &y) { return LdtNumber::combine(x, y); }
	static __device__ __forceinline__ S value(const LdtArgs &a, uint32_t q, uint32_t n, LdtSlot &sl) { return LdtNumber::value(a, q, n, sl); }
	static __device__ __forceinline__ void emit(const LdtArgs &d, uint32_t q, uint32_t n, bool live, const LdtSlot &sl, const S &ex, const S &in)
	{
		const LxArgs &a = lx_args(d);
		if (!live)
			return;
		a.gdst[q] = ~0ULL;                                      // (le_crypt_pkt_kernel sets it for a stored message's fragment)
		if (sl.g == LX_NONE || LDT_KIND(sl.x) != BTBBX_LE_DATA_START || LDT_ROLE(sl.x) >= 2)
			return;
		ldt_start(a, q, sl, ex, (a.cst[q] & 0xffu) == BTBBX_LE_CRYPT_VERIFIED ? a.hdr4 + q : nullptr);
	}
};

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_number_sum_kernel(LxArgs a) { ldt_tile<LxNumber, false>(a); }
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_number_kernel(LxArgs a) { ldt_tile<LxNumber, true>(a); }

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_number_prefix_kernel(LxArgs a) { ldt_totals(a); }

// ---- 9. rule 9: the records ----------------------------------------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_pkt_kernel(LxArgs a)
{
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t n = a.params[0], k = a.params[1], i = (uint32_t)at;
	if (at >= n)
		return;
	uint32_t g, first;
	uint4 p, rec = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
	const bool member = lf_member(a.cands, a.pkts, a.conns, i, n, k, g, p, first);
	const uint32_t q = first + p.x;
	ldt_pkt(a, i, member, q);
	if (member) {
		const uint32_t cs = a.cst[q], st = cs & 0xffu;
		const bool tried = st == BTBBX_LE_CRYPT_VERIFIED || st == BTBBX_LE_CRYPT_FAILED;
		const unsigned long long c = tried ? (unsigned long long)a.ord[q] + (st == BTBBX_LE_CRYPT_VERIFIED ? (cs >> 8) & 0xffu : 0u) : 0ull;
		rec = make_uint4((uint32_t)c, tried ? a.ord[q] : 0u, (cs & 0xffffffu) | (((uint32_t)(c >> 32) & 0x7fu) << 24), 0u);
	}
	reinterpret_cast<uint4 *>(a.cpkts)[i] = rec;
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_conn_kernel(LxArgs a)
{
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t k = a.params[1], g = (uint32_t)at;
	if (at >= k)
		return;
	uint2 *o = reinterpret_cast<uint2 *>(a.crypt + g);
	if (!a.ctal[(size_t)g * 8 + 5]) {                       // no member
#pragma unroll
		for (int w = 0; w < 7; w++)
			o[w] = make_uint2(0, 0);
		return;
	}
	const uint4 pr = reinterpret_cast<const uint4 *>(a.proc)[g];
	const uint4 t0 = reinterpret_cast<const uint4 *>(a.ctal + (size_t)g * 8)[0];
	const uint32_t max_skew = a.ctal[(size_t)g * 8 + 4], key = a.ckey[g];
	const bool armed = pr.z != LX_NONE;
	uint32_t flags = (pr.x != LX_NONE ? BTBBX_LE_CRYPT_REQ : 0u) | (pr.y != LX_NONE ? BTBBX_LE_CRYPT_RSP : 0u) |
			 (armed ? BTBBX_LE_CRYPT_START | BTBBX_LE_CRYPT_ARMED : 0u) | (key != 0xffu ? BTBBX_LE_CRYPT_KEYED : 0u);
	uint4 sk = make_uint4(0, 0, 0, 0);
	if (key != 0xffu)
		sk = reinterpret_cast<const uint4 *>(a.sched + ((size_t)g * a.n_keys + key) * LX_RK)[0];
	o[0] = make_uint2(sk.x, sk.y);
	o[1] = make_uint2(sk.z, sk.w);
	o[2] = make_uint2(a.civ[2 * (size_t)g], a.civ[2 * (size_t)g + 1]);
	o[3] = make_uint2(pr.x != LX_NONE ? a.slot[pr.x] : LX_NONE, pr.y != LX_NONE ? a.slot[pr.y] : LX_NONE);
	o[4] = make_uint2(armed ? a.slot[pr.z] : LX_NONE, t0.x);
	o[5] = make_uint2(t0.y, t0.z);
	o[6] = make_uint2(t0.w, key | (max_skew << 8) | (flags << 16));
}

// ---- 10. the octets -------------------------------------------------------------------------------------------------------------------

// 16 lanes per slot, one per 16 octets of a stored message's fragment: the dewhitened octets, under the keystream block of a VERIFIED
// member, to their place in d_bytes -- in 8-byte words where the place is aligned, octet by octet where it is not
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_crypt_plain_kernel(LxArgs a)
{
	__shared__ uint32_t te[256];
	__shared__ unsigned long long wt[128];
	lx_tables(a, te, wt);
	const uint64_t at = (uint64_t)blockIdx.x * (LE_THREADS / 16) + threadIdx.x / 16;
	const uint32_t n = a.params[0], q = (uint32_t)at, k = 16 * (threadIdx.x % 16);
	if (at >= n)
		return;
	const unsigned long long dst = a.gdst[q];
	if (dst == ~0ULL)
		return;
	const uint32_t x = a.sinfo[q], len = x & 0xffu, cs = a.cst[q], g = a.sg[q];
	if (k >= len)
		return;
	const LdtWhere p = ldt_where(a, q, x);
	unsigned long long lo = ldt_octets(a, p, wt, k), hi = ldt_octets(a, p, wt, k + 8);
	if ((cs & 0xffu) == BTBBX_LE_CRYPT_VERIFIED) {
		uint32_t rk[LX_RK];
		lx_load_rk(a.sched + ((size_t)g * a.n_keys + a.ckey[g]) * LX_RK, rk);
		const LxBlock s = lx_aes(te, rk, lx_nonce_block(0x01u, (unsigned long long)a.ord[q] + ((cs >> 8) & 0xffu),
								 LDT_ROLE(x) == BTBBX_LE_ROLE_CENTRAL ? 1u : 0u, a.civ[2 * (size_t)g],
								 a.civ[2 * (size_t)g + 1], k / 16 + 1));
		lo ^= ((unsigned long long)s.w[1] << 32) | s.w[0];
		hi ^= ((unsigned long long)s.w[3] << 32) | s.w[2];
	}
	uint8_t *out = a.bytes + dst + k;
	const uint32_t take = len - k < 16 ? len - k : 16u;
	if (take == 16 && !((dst + k) & 7)) {
		reinterpret_cast<unsigned long long *>(out)[0] = lo;
		reinterpret_cast<unsigned long long *>(out)[1] = hi;
	} else {
		for (uint32_t j = 0; j < take; j++)
			out[j] = (uint8_t)((j < 8 ? lo : hi) >> (8 * (j & 7)));
	}
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------

extern "C" size_t btbbx_le_crypt_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap, uint32_t n_keys)
{
	return le_crypt_layout(cand_cap, conn_cap, n_keys).total;
}

// the 24 launches of one run
static int le_crypt_launch(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, const btbbx_le_cand *d_cands,
			   const uint32_t *d_count, uint32_t cap, const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
			   const btbbx_le_track_pkt *d_pkts, const btbbx_le_data_pkt *d_data_pkts, const uint8_t *d_keys, uint32_t n_keys,
			   uint32_t window, btbbx_le_crypt *d_crypt, btbbx_le_crypt_pkt *d_crypt_pkts, btbbx_le_data_pkt *d_plain_pkts,
			   btbbx_le_msg *d_msgs, uint32_t msg_cap, uint32_t *d_msg_count, uint8_t *d_bytes, uint64_t byte_cap, uint64_t *d_byte_count,
			   void *d_scratch, hipStream_t q)
{
	const LxLayout C = le_crypt_layout(cap, conn_cap, n_keys);
	const LdtLayout &L = C.frame;
	char *s = (char *)d_scratch;
	LxArgs a;
	// (the data records are the data stage's; dpkts: the records over plaintext)
	static_cast<LdtArgs &>(a) = le_data_args(L, d_words, n_words, pitch_words, n_streams, d_cands, d_count, cap, d_conns, d_conn_count, conn_cap, d_pkts,
						  nullptr, d_plain_pkts, d_msgs, msg_cap, d_msg_count, d_bytes, byte_cap, d_byte_count, d_scratch);
	a.in_dpkts = d_data_pkts;
	a.keys = d_keys;
	a.n_keys = n_keys;
	a.window = window;
	a.te = (uint32_t *)(s + C.te);
	a.base = (uint32_t *)(s + C.base);
	a.ord = (uint32_t *)(s + C.ord);
	a.cst = (uint32_t *)(s + C.cst);
	a.skew = (uint32_t *)(s + C.skew);
	a.hdr4 = (uint32_t *)(s + C.hdr4);
	a.retry = (uint32_t *)(s + C.retry);
	a.proc = (uint32_t *)(s + C.proc);
	a.probe = (uint32_t *)(s + C.probe);
	a.ctal = (uint32_t *)(s + C.ctal);
	a.ckey = (uint32_t *)(s + C.ckey);
	a.civ = (uint32_t *)(s + C.civ);
	a.score = (uint32_t *)(s + C.score);
	a.sched = (uint32_t *)(s + C.sched);
	a.counts = (uint32_t *)(s + C.counts);
	a.crypt = d_crypt;
	a.cpkts = d_crypt_pkts;
	const auto blocks = [](uint64_t items, uint32_t per) { return (uint32_t)std::min<uint64_t>((items + per - 1) / per, LX_GRID); };
	const dim3 per_cand((uint32_t)(((uint64_t)cap + LE_THREADS - 1) / LE_THREADS)), per_tile(L.tiles_n), wg(LE_THREADS), one(1);
	const dim3 per_conn((uint32_t)(((uint64_t)conn_cap + LE_THREADS - 1) / LE_THREADS));
	const dim3 per_16((uint32_t)(((uint64_t)cap + LE_THREADS / 16 - 1) / (LE_THREADS / 16)));
	const dim3 init_grid((uint32_t)(((uint64_t)std::max(cap, conn_cap) + LE_THREADS - 1) / LE_THREADS));
	const dim3 per_key(blocks((uint64_t)conn_cap * n_keys, LE_THREADS)), per_probe(blocks((uint64_t)conn_cap * 4 * n_keys, LE_THREADS));
	const dim3 per_retry(blocks((uint64_t)cap * (window - 1) + 1, LE_THREADS));
	const LdtArgs &frame = a;                               // what the data stage's kernels take
	hipLaunchKernelGGL(le_crypt_init_kernel, init_grid, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_slot_kernel, per_cand, wg, 0, q, frame);
	hipLaunchKernelGGL(le_crypt_find_kernel, per_cand, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_rsp_kernel, per_cand, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_begin_kernel, per_cand, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_sched_kernel, per_key, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_ord_sum_kernel, per_tile, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_ord_prefix_kernel, one, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_ord_kernel, per_tile, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_probe_kernel, per_probe, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_key_kernel, per_conn, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_first_kernel, per_cand, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_retry_kernel, per_retry, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_effect_kernel, per_cand, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_msg_sum_kernel, per_tile, wg, 0, q, frame);
	hipLaunchKernelGGL(le_data_msg_prefix_kernel, one, wg, 0, q, frame);
	hipLaunchKernelGGL(le_data_msg_kernel, per_tile, wg, 0, q, frame);
	hipLaunchKernelGGL(le_data_close_kernel, per_cand, wg, 0, q, frame);
	hipLaunchKernelGGL(le_crypt_number_sum_kernel, per_tile, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_number_prefix_kernel, one, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_number_kernel, per_tile, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_pkt_kernel, per_cand, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_conn_kernel, per_conn, wg, 0, q, a);
	hipLaunchKernelGGL(le_crypt_plain_kernel, per_16, wg, 0, q, a);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

static int le_crypt_check_keys(const char *who, uint32_t n_keys, uint32_t window)
{
	if (n_keys < 1 || n_keys > LX_MAX_KEYS || window < 1 || window > LX_MAX_SKEW) {
		set_error("%s: n_keys must be 1..%u and window 1..%u", who, LX_MAX_KEYS, LX_MAX_SKEW);
		return BTBBX_E_ARG;
	}
	return BTBBX_OK;
}

extern "C" int btbbx_le_crypt_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				     const uint16_t *d_phys_channel,
				     const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
				     const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
				     const btbbx_le_track *d_tracks, const btbbx_le_track_pkt *d_pkts, const btbbx_le_data_pkt *d_data_pkts,
				     const uint8_t *d_keys, uint32_t n_keys, uint32_t window,
				     btbbx_le_crypt *d_crypt, btbbx_le_crypt_pkt *d_crypt_pkts, btbbx_le_data_pkt *d_plain_pkts,
				     btbbx_le_msg *d_msgs, uint32_t msg_cap, uint32_t *d_msg_count, uint8_t *d_bytes, uint64_t byte_cap,
				     uint64_t *d_byte_count, void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
	const char *who = "btbbx_le_crypt_device";
	int rc = le_check_streams(who, n_words, pitch_words, n_streams);
	if (!rc)
		rc = le_crypt_check_keys(who, n_keys, window);
	if (rc)
		return rc;
	const LxLayout L = le_crypt_layout(cand_cap, conn_cap, n_keys);
	if (!d_words || !d_phys_channel || !d_cands || !d_cand_count || !d_conns || !d_conn_count || !d_tracks || !d_pkts || !d_data_pkts ||
	    !d_keys || !d_crypt || !d_crypt_pkts || !d_plain_pkts || (!d_msgs && msg_cap) || !d_msg_count || (!d_bytes && byte_cap) ||
	    !d_byte_count || !d_scratch || scratch_bytes < L.total) {
		set_error("%s: null pointer, or scratch of %zu bytes needed and %zu given", who, L.total, scratch_bytes);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_words & 7) || ((uintptr_t)d_cands & 7) || ((uintptr_t)d_conns & 7) || ((uintptr_t)d_tracks & 7) ||
	    ((uintptr_t)d_pkts & 7) || ((uintptr_t)d_crypt & 7) || ((uintptr_t)d_crypt_pkts & 15) || ((uintptr_t)d_msgs & 7) ||
	    ((uintptr_t)d_bytes & 7) || ((uintptr_t)d_byte_count & 7) || ((uintptr_t)d_data_pkts & 3) || ((uintptr_t)d_plain_pkts & 3) ||
	    ((uintptr_t)d_scratch & 15) || ((uintptr_t)d_cand_count & 3) || ((uintptr_t)d_conn_count & 3) || ((uintptr_t)d_msg_count & 3) ||
	    ((uintptr_t)d_phys_channel & 1)) {
		set_error("%s: misaligned pointer (scratch and the 16-byte records 16 bytes; words, records, the byte buffer and its count 8; the "
			  "12-byte records and the counters 4; the channels 2)", who);
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	hipStream_t q = (hipStream_t)hip_stream;
	if (!cand_cap || !conn_cap) {
		HIP_TRY(hipMemsetAsync(d_msg_count, 0, sizeof(uint32_t), q));
		HIP_TRY(hipMemsetAsync(d_byte_count, 0, sizeof(uint64_t), q));
		return BTBBX_OK;
	}
	return le_crypt_launch(d_words, n_words, pitch_words, n_streams, d_cands, d_cand_count, cand_cap, d_conns, d_conn_count, conn_cap, d_pkts,
			       d_data_pkts, d_keys, n_keys, window, d_crypt, d_crypt_pkts, d_plain_pkts, d_msgs, msg_cap, d_msg_count, d_bytes, byte_cap,
			       d_byte_count, d_scratch, q);
}
