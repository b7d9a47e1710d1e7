// le_data.h -- LE data extraction (included by le.hip, behind le_span.h): behind the tracking, for every packet of every stored connection
// the role of its sender, its SN / NESN / MD bits and whether it is new or a retransmission; for every direction of every connection
// the L2CAP messages reassembled from their fragments, their dewhitened octets packed into one buffer.  The contract is in
// include/btbbx.h (btbbx_le_data_device), the reasoning in DESIGN 3.8.6.  All arithmetic is integer arithmetic.
//
// Time order is a permutation: slot first + rank of the list holds the member of that rank, so a connection's members lie next to each
// other, connections in list order.  Rules 2 to 6 are four scans over the slots, each in three launches (the sums of the tiles of
// LT_TILE slots, one workgroup that turns them into exclusive prefixes, the tiles again with their carry), so a connection may
// cross any number of waves, workgroups and tiles:
//
//   1. le_data_init_kernel, le_data_slot_kernel      the slot table; the whitening sequence, 64 bits from each of its 127 phases
//   2. le_data_open_*    (sum, prefix, apply)        the latest slot that opens an event and whether that event is HEAD: the role
//   3. le_data_prev_*                                 per connection the last SN of either role: NEW / RETRANSMIT, the kind
//   4. le_data_msg_*                                  per connection and role the latest START; per role the running octets and
//                                                     fragments: a fragment's message and position, ORPHAN
//   5. le_data_close_kernel                           a START closes the message of the START of its role in front of it, a connection's
//                                                     last slot the two that are open: octets and fragments of every message
//   6. le_data_number_*                               M and byte_offset of every START (32 and 64 bits); the message records, the tallies
//   7. le_data_pkt_kernel, le_data_conn_kernel        the per-candidate and per-connection records
//   8. le_data_gather_kernel                          eight lanes per fragment: the payload, dewhitened, to its place in d_bytes
//
// 18 launches, whatever the counts and caps.  Nothing here synchronises or reads back but the host wrapper.
#pragma once
#include "le_span.h"

#define LDT_NONE     0xffffffffu
#define LDT_FRAG     8u                    // lanes of the gather per fragment
// sinfo[q], the slot's packed state: length | (header0 & 0x1f) << 8 | role << 14 | new << 16 | kind << 17 | stored << 20 | phase << 24 (the whitening
// sequence's phase at the packet's first PDU bit: wphase of the channel's register value)
#define LDT_ROLE(x)  (((x) >> 14) & 3u)    // 3: an empty slot
#define LDT_KIND(x)  (((x) >> 17) & 7u)
#define LDT_STORED   (1u << 20)

static_assert(sizeof(btbbx_le_data_pkt) == 12 && offsetof(btbbx_le_data_pkt, pos) == 4 && offsetof(btbbx_le_data_pkt, role) == 8 &&
	      offsetof(btbbx_le_data_pkt, kind) == 9 && offsetof(btbbx_le_data_pkt, bits) == 10 && offsetof(btbbx_le_data_pkt, reserved) == 11,
	      "btbbx_le_data_pkt layout (libbtbb_amd.LE_DATA_PKT_DTYPE)");
static_assert(sizeof(btbbx_le_data) == 48 && offsetof(btbbx_le_data, first_msg) == 8 && offsetof(btbbx_le_data, n_msgs) == 12 &&
	      offsetof(btbbx_le_data, n_complete) == 16 && offsetof(btbbx_le_data, n_central) == 20 && offsetof(btbbx_le_data, n_peripheral) == 24 &&
	      offsetof(btbbx_le_data, n_unknown) == 28 && offsetof(btbbx_le_data, n_retransmit) == 32 && offsetof(btbbx_le_data, n_orphan) == 36 &&
	      offsetof(btbbx_le_data, n_control) == 40 && offsetof(btbbx_le_data, n_empty) == 44, "btbbx_le_data layout (libbtbb_amd.LE_DATA_DTYPE)");
static_assert(sizeof(btbbx_le_msg) == 32 && offsetof(btbbx_le_msg, conn) == 8 && offsetof(btbbx_le_msg, start) == 12 &&
	      offsetof(btbbx_le_msg, n_fragments) == 16 && offsetof(btbbx_le_msg, bytes) == 20 && offsetof(btbbx_le_msg, l2cap_len) == 24 &&
	      offsetof(btbbx_le_msg, cid) == 26 && offsetof(btbbx_le_msg, role) == 28 && offsetof(btbbx_le_msg, flags) == 29 &&
	      offsetof(btbbx_le_msg, reserved) == 30, "btbbx_le_msg layout (libbtbb_amd.LE_MSG_DTYPE)");

// what every kernel of the stage is launched with
struct LdtArgs {
	const uint64_t *words;
	uint64_t n_words, pitch_words;
	const btbbx_le_cand *cands;
	const btbbx_le_track_pkt *pkts;
	const btbbx_le_conn *conns;
	const uint32_t *d_cand_count, *d_conn_count;
	uint32_t n_streams, cand_cap, conn_cap, n_tiles, msg_cap;
	// scratch: params[0] = N, [1] = K; per slot; per tile (the scan in hand); per connection; the whitening table
	uint32_t *params, *slot, *sg, *sinfo, *sx, *cx, *ps, *mbytes, *mfrag, *msgno, *tiles, *cend, *cnum, *tally, *wphase;
	unsigned long long *boff, *gdst, *wtab;
	btbbx_le_data *data;
	btbbx_le_data_pkt *dpkts;
	btbbx_le_msg *msgs;
	uint32_t *msg_count;
	uint8_t *bytes;
	uint64_t byte_cap;
	unsigned long long *byte_count;
};

struct LdtLayout {
	size_t params, slot, sg, sinfo, sx, cx, ps, mbytes, mfrag, msgno, boff, gdst, tiles, cend, cnum, tally, wtab, wphase, total;
	uint32_t tiles_n;
};

static LdtLayout le_data_layout(uint32_t cand_cap, uint32_t conn_cap)
{
	LdtLayout L;
	const size_t c = cand_cap ? cand_cap : 1, k = conn_cap ? conn_cap : 1;
	L.tiles_n = (uint32_t)((c + LT_TILE - 1) / LT_TILE);
	size_t at = 0;
	auto take = [&](size_t bytes) { const size_t here = at; at += ld_up(bytes); return here; };
	L.params = take(256);
	L.slot = take(c * 4);
	L.sg = take(c * 4);
	L.sinfo = take(c * 4);
	L.sx = take(c * 4);
	L.cx = take(c * 4);
	L.ps = take(c * 4);
	L.mbytes = take(c * 4);
	L.mfrag = take(c * 4);
	L.msgno = take(c * 4);
	L.boff = take(c * 8);
	L.gdst = take(c * 8);
	L.tiles = take(((size_t)L.tiles_n + 1) * 8 * 4);
	L.cend = take(k * 32);
	L.cnum = take(k * 32);
	L.tally = take(k * 32);
	L.wtab = take(128 * 8);
	L.wphase = take(128 * 4);
	L.total = at;
	return L;
}

// ---- the scans' frame ------------------------------------------------------------------------------------------------------------

template <int N> struct LdtState { uint32_t w[N]; };

template <int N> __device__ __forceinline__ LdtState<N> ldt_zero()
{
	LdtState<N> s;
#pragma unroll
	for (int j = 0; j < N; j++)
		s.w[j] = 0;
	return s;
}

template <int N> __device__ __forceinline__ LdtState<N> ldt_shfl_up(const LdtState<N> &v, int d)
{
	LdtState<N> s;
#pragma unroll
	for (int j = 0; j < N; j++)
		s.w[j] = __shfl_up(v.w[j], d);
	return s;
}

// what a slot's value() loaded and its emit() needs again
struct LdtSlot { uint32_t g, x, y; };

// Inclusive and exclusive scan of v over the workgroup's threads under St::combine(earlier, later), whose identity is the zero state;
// carry: the state in front of the workgroup's first thread on entry, behind its last on return.  Ends with a barrier.
template <class St> __device__ __forceinline__ void ldt_block_scan(const LdtState<St::NW> &v, uint32_t (*lds)[St::NW], LdtState<St::NW> &carry,
								     LdtState<St::NW> &ex, LdtState<St::NW> &in)
{
	typedef LdtState<St::NW> S;
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	S inc = v;
#pragma unroll
	for (int d = 1; d < 64; d <<= 1) {
		const S up = ldt_shfl_up<St::NW>(inc, d);
		if (lane >= (uint32_t)d)
			inc = St::combine(up, inc);
	}
	if (lane == 63) {
#pragma unroll
		for (int j = 0; j < St::NW; j++)
			lds[wave][j] = inc.w[j];
	}
	__syncthreads();
	S before = carry;
#pragma unroll 1
	for (uint32_t w = 0; w < LT_WAVES; w++) {
		S t;
#pragma unroll
		for (int j = 0; j < St::NW; j++)
			t.w[j] = lds[w][j];
		if (w == wave)
			before = carry;
		carry = St::combine(carry, t);
	}
	const S up = ldt_shfl_up<St::NW>(inc, 1);
	ex = lane ? St::combine(before, up) : before;
	in = St::combine(before, inc);
	__syncthreads();
}

// one tile of LT_TILE slots: its sum (APPLY false: tiles[blockIdx.x]) or, with its carry, every slot's emit()
template <class St, bool APPLY> __device__ __forceinline__ void ldt_tile(const LdtArgs &a)
{
	typedef LdtState<St::NW> S;
	__shared__ uint32_t lds[LT_WAVES][St::NW];
	const uint32_t tid = threadIdx.x, n = a.params[0];
	S carry = ldt_zero<St::NW>();
	if (APPLY) {
#pragma unroll
		for (int j = 0; j < St::NW; j++)
			carry.w[j] = a.tiles[(size_t)blockIdx.x * 8 + j];
	}
	for (uint32_t r = 0; r < LT_TILE / LE_THREADS; r++) {
		const uint64_t at = (uint64_t)blockIdx.x * LT_TILE + r * LE_THREADS;
		if (at >= n)
			break;                                          // (uniform over the workgroup)
		const uint32_t q = (uint32_t)at + tid;
		const bool live = at + tid < n;
		LdtSlot sl;
		sl.g = LDT_NONE;
		sl.x = sl.y = 0;
		S v = ldt_zero<St::NW>(), ex, in;
		if (live)
			v = St::value(a, q, n, sl);
		ldt_block_scan<St>(v, lds, carry, ex, in);
		if (APPLY)
			St::emit(a, q, n, live, sl, ex, in);
	}
	if (!APPLY && tid == 0) {
#pragma unroll
		for (int j = 0; j < St::NW; j++)
			a.tiles[(size_t)blockIdx.x * 8 + j] = carry.w[j];
	}
}

// one workgroup: the tiles' sums -> their exclusive prefixes; returns the sum of all
template <class St> __device__ __forceinline__ LdtState<St::NW> ldt_prefix(const LdtArgs &a)
{
	typedef LdtState<St::NW> S;
	__shared__ uint32_t lds[LT_WAVES][St::NW];
	S carry = ldt_zero<St::NW>();
	for (uint32_t base = 0; base < a.n_tiles; base += LE_THREADS) {
		const uint32_t i = base + threadIdx.x;
		S v = ldt_zero<St::NW>(), ex, in;
		if (i < a.n_tiles) {
#pragma unroll
			for (int j = 0; j < St::NW; j++)
				v.w[j] = a.tiles[(size_t)i * 8 + j];
		}
		ldt_block_scan<St>(v, lds, carry, ex, in);
		if (i < a.n_tiles) {
#pragma unroll
			for (int j = 0; j < St::NW; j++)
				a.tiles[(size_t)i * 8 + j] = ex.w[j];
		}
	}
	return carry;
}

// slot q is the first (last) of its connection g: the slot in front of (behind) it holds none or another's
__device__ __forceinline__ bool ldt_first(const uint32_t *sg, uint32_t q, uint32_t g) { return q == 0 || sg[q - 1] != g; }
__device__ __forceinline__ bool ldt_last(const uint32_t *sg, uint32_t q, uint32_t n, uint32_t g) { return q + 1 >= n || sg[q + 1] != g; }

// 64 stream bits from `bit`, zeros beyond the stream's end
__device__ __forceinline__ unsigned long long ldt_read64(const uint64_t *w, uint64_t n_words, uint64_t bit)
{
	const uint64_t wi = bit >> 6;
	const uint32_t sh = (uint32_t)(bit & 63);
	const uint64_t lo = wi < n_words ? w[wi] : 0;
	const uint64_t hi = sh && wi + 1 < n_words ? w[wi + 1] : 0;
	return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}

// where the payload of the member in slot q begins, and the whitening phase there (x: the slot's sinfo)
struct LdtWhere {
	const uint64_t *w;
	uint64_t bit0;
	uint32_t phase, h0;
	bool in_range;
};

__device__ __forceinline__ LdtWhere ldt_where(const LdtArgs &a, uint32_t q, uint32_t x)
{
	LdtWhere p;
	const uint32_t i = a.slot[q];
	const uint2 where = reinterpret_cast<const uint2 *>(a.cands + i)[0];
	const uint32_t c = reinterpret_cast<const uint2 *>(a.cands + i)[2].x, stream = c & 0xffffu;
	p.in_range = stream < a.n_streams;
	p.w = a.words + (p.in_range ? (uint64_t)stream * a.pitch_words : 0);
	p.bit0 = ((((uint64_t)where.y << 32) | where.x) & LT_OFF_MASK) + 56;
	p.phase = (x >> 24) + 16u;
	p.h0 = (c >> 16) & 0xffu;
	return p;
}

// payload octets k .. k + 7, dewhitened; zeros beyond the stream's end
__device__ __forceinline__ unsigned long long ldt_octets(const LdtArgs &a, const LdtWhere &p, const unsigned long long *wt, uint32_t k)
{
	const unsigned long long v = p.in_range ? ldt_read64(p.w, a.n_words, p.bit0 + 8ull * k) : 0;
	return v ^ wt[(p.phase + 8u * k) % 127u];
}

// ---- 1. slots, the whitening table --------------------------------------------------------------------------------------------

// params, the empty slots and cend, cleared: the part of an init kernel every stage on this frame needs.  i: the thread's index in the
// grid, which covers the larger of the two caps; own(): what the stage itself clears of connection i
template <class Own> __device__ __forceinline__ void ldt_init_frame(const LdtArgs &a, uint64_t i, Own own)
{
	const uint32_t nh = *a.d_cand_count, kh = *a.d_conn_count;
	const uint32_t n = nh < a.cand_cap ? nh : a.cand_cap, k = kh < a.conn_cap ? kh : a.conn_cap;
	if (i == 0) {
		a.params[0] = n;
		a.params[1] = k;
		a.wphase[0] = 0;
	}
	if (i < n)
		a.slot[i] = LDT_NONE;
	if (i < k) {
		own();
		uint4 *c = reinterpret_cast<uint4 *>(a.cend + i * 8);
		c[0] = c[1] = make_uint4(0, 0, 0, 0);
	}
}

// wtab[t] = the 64 whitening bits behind t steps of the register from 0x40 (the reflected register of le_decode_kernel, period 127);
// wphase[s] = the t at which the register holds s.  For the threads t < 127 of one workgroup
__device__ __forceinline__ void ldt_init_whitening(const LdtArgs &a, uint32_t t)
{
	uint32_t s = 0x40u;
	for (uint32_t j = 0; j < t; j++) {
		if (s & 1u)
			s ^= 0x88u;
		s >>= 1;
	}
	a.wphase[s] = t;
	unsigned long long o = 0;
	for (uint32_t j = 0; j < 64; j++) {
		o |= (unsigned long long)(s & 1u) << j;
		if (s & 1u)
			s ^= 0x88u;
		s >>= 1;
	}
	a.wtab[t] = o;
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_init_kernel(LdtArgs a)
{
	const uint64_t i = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	ldt_init_frame(a, i, [=] {
		uint4 *m = reinterpret_cast<uint4 *>(a.cnum + i * 8), *t = reinterpret_cast<uint4 *>(a.tally + i * 8);
		m[0] = m[1] = t[0] = t[1] = make_uint4(0, 0, 0, 0);
	});
	if (blockIdx.x == 0 && threadIdx.x < 127)
		ldt_init_whitening(a, threadIdx.x);
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_slot_kernel(LdtArgs a)
{
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t n = a.params[0], k = a.params[1];
	if (at >= n)
		return;
	const uint32_t i = (uint32_t)at;
	uint32_t g, first;
	uint4 p;
	if (lf_member(a.cands, a.pkts, a.conns, i, n, k, g, p, first))
		a.slot[first + p.x] = i;
}

// ---- 2. rules 2 and 3: the event a slot lies in, HEAD, the role ----------------------------------------------------------------------

// state: w0 = 1 | head << 1 where a slot opens an event, w1 = that slot; the later one wins
struct LdtOpen {
	static constexpr int NW = 2;
	typedef LdtState<NW> S;
	static __device__ __forceinline__ S combine(const S &x, const S &y) { return (y.w[0] & 1u) ? y : x; }
	static __device__ __forceinline__ S value(const LdtArgs &a, uint32_t q, uint32_t n, LdtSlot &sl)
	{
		S v = ldt_zero<NW>();
		const uint32_t i = a.slot[q];
		sl.x = 3u << 14;
		if (i == LDT_NONE)
			return v;
		const uint2 c = reinterpret_cast<const uint2 *>(a.cands + i)[2];    // stream | header0 << 16 | length << 24, conn
		const uint4 p = reinterpret_cast<const uint4 *>(a.pkts)[i];
		bool same = false;
		uint32_t pe = 0, pc = 0;
		if (q > 0) {
			const uint32_t ip = a.slot[q - 1];
			if (ip != LDT_NONE && reinterpret_cast<const uint2 *>(a.cands + ip)[2].y == c.y) {
				const uint4 pp = reinterpret_cast<const uint4 *>(a.pkts)[ip];
				same = true;
				pe = pp.y;
				pc = pp.z;
			}
		}
		const bool opens = !same || pe != p.y, head = opens && (!same || p.y == 0 || p.z != pc);
		sl.g = c.y;
		sl.x = (c.x >> 24) | (((c.x >> 16) & 0x1fu) << 8) | (a.wphase[0x40u | (p.w & 0x3fu)] << 24);
		if (opens) {
			v.w[0] = 1u | (head ? 2u : 0u);
			v.w[1] = q;
		}
		return v;
	}
	static __device__ __forceinline__ void emit(const LdtArgs &a, uint32_t q, uint32_t n, bool live, const LdtSlot &sl, const S &ex, const S &in)
	{
		if (!live)
			return;
		uint32_t x = sl.x;
		if (sl.g != LDT_NONE)
			x |= ((in.w[0] & 2u) ? (q - in.w[1]) & 1u : 2u) << 14;
		a.sg[q] = sl.g;
		a.sinfo[q] = x;
	}
};

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_open_sum_kernel(LdtArgs a) { ldt_tile<LdtOpen, false>(a); }
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_open_prefix_kernel(LdtArgs a) { ldt_prefix<LdtOpen>(a); }
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_open_kernel(LdtArgs a) { ldt_tile<LdtOpen, true>(a); }

// ---- 3. rule 4: NEW / RETRANSMIT, the kind ---------------------------------------------------------------------------------------

// state: bit 0 = a connection begins (what lies in front is cut off); role r: bit 1 + 2r = a member seen, bit 2 + 2r = its SN
struct LdtPrev {
	static constexpr int NW = 1;
	typedef LdtState<NW> S;
	static __device__ __forceinline__ S combine(const S &x, const S &y)
	{
		if (y.w[0] & 1u)
			return y;
		S r;
		r.w[0] = (x.w[0] & 1u) | ((y.w[0] & 2u) ? y.w[0] & 6u : x.w[0] & 6u) | ((y.w[0] & 8u) ? y.w[0] & 24u : x.w[0] & 24u);
		return r;
	}
	static __device__ __forceinline__ S value(const LdtArgs &a, uint32_t q, uint32_t n, LdtSlot &sl)
	{
		S v;
		sl.g = a.sg[q];
		sl.x = a.sinfo[q];
		sl.y = sl.g == LDT_NONE || ldt_first(a.sg, q, sl.g) ? 1u : 0u;
		const uint32_t role = LDT_ROLE(sl.x), sn = (sl.x >> 11) & 1u;
		v.w[0] = sl.y | (role < 2 ? (2u | (sn << 2)) << (2 * role) : 0u);
		return v;
	}
	static __device__ __forceinline__ void emit(const LdtArgs &a, uint32_t q, uint32_t n, bool live, const LdtSlot &sl, const S &ex, const S &in)
	{
		if (!live || sl.g == LDT_NONE)
			return;
		const uint32_t role = LDT_ROLE(sl.x), sn = (sl.x >> 11) & 1u, llid = (sl.x >> 8) & 3u, len = sl.x & 0xffu;
		uint32_t kind = BTBBX_LE_DATA_UNKNOWN, fresh = 0;
		if (role < 2) {
			const bool has = !sl.y && ((ex.w[0] >> (1 + 2 * role)) & 1u);
			fresh = !has || ((ex.w[0] >> (2 + 2 * role)) & 1u) != sn ? 1u : 0u;
			if (!fresh)
				kind = BTBBX_LE_DATA_RETRANSMIT;
			else if (llid == 2 && len)
				kind = BTBBX_LE_DATA_START;
			else if (llid == 1)
				kind = len ? BTBBX_LE_DATA_CONTINUATION : BTBBX_LE_DATA_EMPTY;
			else
				kind = llid == 3 ? BTBBX_LE_DATA_CONTROL : BTBBX_LE_DATA_IGNORED;
		}
		a.sinfo[q] = sl.x | (fresh << 16) | (kind << 17);
	}
};

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_prev_sum_kernel(LdtArgs a) { ldt_tile<LdtPrev, false>(a); }
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_prev_prefix_kernel(LdtArgs a) { ldt_prefix<LdtPrev>(a); }
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_prev_kernel(LdtArgs a) { ldt_tile<LdtPrev, true>(a); }

// ---- 4. rule 5: a fragment's message and position --------------------------------------------------------------------------------

// state: w0 bit 0 = a connection begins, bit 1 + r = a START of role r seen; w1 + r = its slot; w3 + r = the octets, w5 + r = the
// number of role r's fragments (sums over the whole table modulo 2^32: only differences within a connection are read)
struct LdtMsg {
	static constexpr int NW = 7;
	typedef LdtState<NW> S;
	static __device__ __forceinline__ S combine(const S &x, const S &y)
	{
		S r;
		const bool cut = y.w[0] & 1u;
		r.w[0] = cut ? y.w[0] : x.w[0] | y.w[0];
		r.w[1] = cut || (y.w[0] & 2u) ? y.w[1] : x.w[1];
		r.w[2] = cut || (y.w[0] & 4u) ? y.w[2] : x.w[2];
#pragma unroll
		for (int j = 3; j < 7; j++)
			r.w[j] = x.w[j] + y.w[j];
		return r;
	}
	static __device__ __forceinline__ S value(const LdtArgs &a, uint32_t q, uint32_t n, LdtSlot &sl)
	{
		S v = ldt_zero<NW>();
		sl.g = a.sg[q];
		sl.x = a.sinfo[q];
		sl.y = sl.g == LDT_NONE || ldt_first(a.sg, q, sl.g) ? 1u : 0u;
		const uint32_t role = LDT_ROLE(sl.x) & 1u, kind = LDT_KIND(sl.x);
		v.w[0] = sl.y;
		if (sl.g != LDT_NONE && kind <= BTBBX_LE_DATA_CONTINUATION) {       // (START 0, CONTINUATION 1: NEW, of role 0 or 1)
			const uint32_t len = sl.x & 0xffu;
			if (kind == BTBBX_LE_DATA_START) {
				v.w[0] |= 2u << role;
				v.w[1] = role ? 0u : q;                 // (no indexing by the role: the state stays in registers)
				v.w[2] = role ? q : 0u;
			}
			v.w[3] = role ? 0u : len;
			v.w[4] = role ? len : 0u;
			v.w[5] = role ? 0u : 1u;
			v.w[6] = role;
		}
		return v;
	}
	static __device__ __forceinline__ void emit(const LdtArgs &a, uint32_t q, uint32_t n, bool live, const LdtSlot &sl, const S &ex, const S &in)
	{
		if (!live || sl.g == LDT_NONE)
			return;
		const uint32_t role = LDT_ROLE(sl.x), kind = LDT_KIND(sl.x), r = role & 1u;
		// (sx, cx and ps of an UNKNOWN member stay unwritten: they are read only of fragments and STARTs, whose role is 0 or 1.
		// mbytes and mfrag of a START are le_data_close_kernel's to write: every START is closed exactly once, by the next START
		// of its role in its connection or by the connection's last slot)
		if (role < 2) {
			uint32_t from = LDT_NONE;
			a.sx[q] = r ? ex.w[4] : ex.w[3];
			a.cx[q] = r ? ex.w[6] : ex.w[5];
			if (kind == BTBBX_LE_DATA_START) {
				if (!sl.y && (ex.w[0] & (2u << r)))
					from = r ? ex.w[2] : ex.w[1];           // the START this one closes
			} else if (kind == BTBBX_LE_DATA_CONTINUATION) {
				if (in.w[0] & (2u << r))
					from = r ? in.w[2] : in.w[1];
				else
					a.sinfo[q] = (sl.x & ~(7u << 17)) | (BTBBX_LE_DATA_ORPHAN << 17);
			}
			a.ps[q] = from;
		}
		if (ldt_last(a.sg, q, n, sl.g)) {
#pragma unroll
			for (int j = 0; j < NW; j++)
				a.cend[(size_t)sl.g * 8 + j] = in.w[j];
		}
	}
};

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_msg_sum_kernel(LdtArgs a) { ldt_tile<LdtMsg, false>(a); }
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_msg_prefix_kernel(LdtArgs a) { ldt_prefix<LdtMsg>(a); }
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_msg_kernel(LdtArgs a) { ldt_tile<LdtMsg, true>(a); }

// ---- 5. the messages' octets and fragments -----------------------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_close_kernel(LdtArgs a)
{
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t n = a.params[0], q = (uint32_t)at;
	if (at >= n)
		return;
	const uint32_t g = a.sg[q];
	if (g == LDT_NONE)
		return;
	const uint32_t x = a.sinfo[q];
	if (LDT_KIND(x) == BTBBX_LE_DATA_START && LDT_ROLE(x) < 2) {
		const uint32_t from = a.ps[q];
		if (from != LDT_NONE) {
			a.mbytes[from] = a.sx[q] - a.sx[from];
			a.mfrag[from] = a.cx[q] - a.cx[from];
		}
	}
	if (ldt_last(a.sg, q, n, g)) {
		const uint32_t *e = a.cend + (size_t)g * 8;
		for (uint32_t r = 0; r < 2; r++)
			if (e[0] & (2u << r)) {
				const uint32_t from = e[1 + r];
				a.mbytes[from] = e[3 + r] - a.sx[from];
				a.mfrag[from] = e[5 + r] - a.cx[from];
			}
	}
}

// ---- 6. rule 6: the messages' numbers and offsets, their records, the tallies ---------------------------------------------------------

// one tally of a wave: a wave whose slots all belong to one connection sends one atomic
__device__ __forceinline__ void ldt_tally(bool mine, bool one, uint32_t lane, uint32_t *at)
{
	const uint64_t mask = __ballot(mine);
	if (!mask)
		return;
	if (one) {
		if (lane == 0)
			atomicAdd(at, (uint32_t)__popcll(mask));
	} else if (mine) {
		atomicAdd(at, 1u);
	}
}

// A START of role 0 or 1 in slot q (sl: what LdtNumber::value loaded, ex: the exclusive prefix): its message's number and offset,
// RUNT / COMPLETE / OVERRUN from the L2CAP header, STORED under the caps, the message record.  plain: the header's four octets
// where the caller has them, else NULL: they are read from the stream.  Returns whether the message is COMPLETE
__device__ __forceinline__ bool ldt_start(const LdtArgs &a, uint32_t q, const LdtSlot &sl, const LdtState<3> &ex, const uint32_t *plain)
{
	const uint32_t m = ex.w[0], bytes = sl.y, len = sl.x & 0xffu, i = a.slot[q];
	const unsigned long long off = ((unsigned long long)ex.w[2] << 32) | ex.w[1];
	uint32_t flags = BTBBX_LE_MSG_RUNT, hdr = 0xffffffffu;
	bool complete = false;
	if (len >= 4) {
		hdr = plain ? *plain : (uint32_t)ldt_octets(a, ldt_where(a, q, sl.x), a.wtab, 0);
		const unsigned long long whole = 4ull + (hdr & 0xffffu);
		complete = bytes == whole;
		flags = complete ? BTBBX_LE_MSG_COMPLETE : (bytes > whole ? BTBBX_LE_MSG_OVERRUN : 0u);
	}
	if (m < a.msg_cap && off + bytes <= a.byte_cap) {
		flags |= BTBBX_LE_MSG_STORED;
		a.sinfo[q] = sl.x | LDT_STORED;
	}
	a.msgno[q] = m;
	a.boff[q] = off;
	if (m < a.msg_cap) {
		uint2 *o = reinterpret_cast<uint2 *>(a.msgs + m);
		o[0] = make_uint2((uint32_t)off, (uint32_t)(off >> 32));
		o[1] = make_uint2(sl.g, i);
		o[2] = make_uint2(a.mfrag[q], bytes);
		o[3] = make_uint2(hdr, LDT_ROLE(sl.x) | (flags << 8));
	}
	return complete;
}

// state: w0 = STARTs, w1 | w2 << 32 = their messages' octets
struct LdtNumber {
	static constexpr int NW = 3;
	typedef LdtState<NW> S;
	static __device__ __forceinline__ S combine(const S &x, const S &y)
	{
		S r;
		const unsigned long long s = (((unsigned long long)x.w[2] << 32) | x.w[1]) + (((unsigned long long)y.w[2] << 32) | y.w[1]);
		r.w[0] = x.w[0] + y.w[0];
		r.w[1] = (uint32_t)s;
		r.w[2] = (uint32_t)(s >> 32);
		return r;
	}
	static __device__ __forceinline__ S value(const LdtArgs &a, uint32_t q, uint32_t n, LdtSlot &sl)
	{
		S v = ldt_zero<NW>();
		sl.g = a.sg[q];
		sl.x = a.sinfo[q];
		if (sl.g != LDT_NONE && LDT_KIND(sl.x) == BTBBX_LE_DATA_START && LDT_ROLE(sl.x) < 2) {
			v.w[0] = 1;
			v.w[1] = sl.y = a.mbytes[q];
		}
		return v;
	}
	static __device__ __forceinline__ void emit(const LdtArgs &a, uint32_t q, uint32_t n, bool live, const LdtSlot &sl, const S &ex, const S &in)
	{
		const uint32_t lane = threadIdx.x & 63, g = sl.g;
		const bool member = live && g != LDT_NONE;
		const uint32_t role = member ? LDT_ROLE(sl.x) : 3u, kind = member ? LDT_KIND(sl.x) : 0xffu;
		bool complete = false;
		if (live)
			a.gdst[q] = ~0ULL;                              // (le_data_pkt_kernel sets it for a stored message's fragment)
		if (member) {
			if (ldt_first(a.sg, q, g))
				reinterpret_cast<uint4 *>(a.cnum + (size_t)g * 8)[0] = make_uint4(1, ex.w[0], ex.w[1], ex.w[2]);
			if (ldt_last(a.sg, q, n, g))
				reinterpret_cast<uint4 *>(a.cnum + (size_t)g * 8)[1] = make_uint4(in.w[0], in.w[1], in.w[2], 0);
		}
		if (member && kind == BTBBX_LE_DATA_START && role < 2)
			complete = ldt_start(a, q, sl, ex, nullptr);
		const uint32_t g0 = __shfl(g, 0, 64);
		const bool one = __ballot(member && g == g0) == ~0ULL;
		uint32_t *t = a.tally + (size_t)(member ? g : 0) * 8;
		ldt_tally(role == 0, one, lane, t + 0);
		ldt_tally(role == 1, one, lane, t + 1);
		ldt_tally(role == 2, one, lane, t + 2);
		ldt_tally(kind == BTBBX_LE_DATA_RETRANSMIT, one, lane, t + 3);
		ldt_tally(kind == BTBBX_LE_DATA_ORPHAN, one, lane, t + 4);
		ldt_tally(kind == BTBBX_LE_DATA_CONTROL, one, lane, t + 5);
		ldt_tally(kind == BTBBX_LE_DATA_EMPTY, one, lane, t + 6);
		ldt_tally(complete, one, lane, t + 7);
	}
};

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_number_sum_kernel(LdtArgs a) { ldt_tile<LdtNumber, false>(a); }
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_number_kernel(LdtArgs a) { ldt_tile<LdtNumber, true>(a); }

// one workgroup: the prefixes of the tiles' sums; the sum of all is the two counts
__device__ __forceinline__ void ldt_totals(const LdtArgs &a)
{
	const LdtState<3> all = ldt_prefix<LdtNumber>(a);
	if (threadIdx.x == 0) {
		*a.msg_count = all.w[0];
		*a.byte_count = ((unsigned long long)all.w[2] << 32) | all.w[1];
	}
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_number_prefix_kernel(LdtArgs a) { ldt_totals(a); }

// ---- 7. rule 7: the records ----------------------------------------------------------------------------------------------------------

// the record of candidate i, which is the member in slot q or no member: its message and its position there, role | kind | bits;
// a.gdst of a stored message's fragment
__device__ __forceinline__ void ldt_pkt(const LdtArgs &a, uint32_t i, bool member, uint32_t q)
{
	uint32_t msg = LDT_NONE, pos = 0, tail = 0xffffffffu;
	if (member) {
		const uint32_t x = a.sinfo[q], kind = LDT_KIND(x);
		if (kind <= BTBBX_LE_DATA_CONTINUATION) {               // a fragment: its message; where its octets go
			const uint32_t from = kind == BTBBX_LE_DATA_START ? q : a.ps[q];
			msg = a.msgno[from];
			pos = a.sx[q] - a.sx[from];
			if (a.sinfo[from] & LDT_STORED)
				a.gdst[q] = a.boff[from] + pos;
		}
		tail = LDT_ROLE(x) | (kind << 8) | ((((x >> 11) & 1u) | (((x >> 10) & 1u) << 1) | (((x >> 12) & 1u) << 2)) << 16);
	} else {
		pos = 0xffffffffu;
	}
	uint32_t *o = reinterpret_cast<uint32_t *>(a.dpkts + i);
	o[0] = msg;
	o[1] = pos;
	o[2] = tail;
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_pkt_kernel(LdtArgs a)
{
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	const uint32_t n = a.params[0], k = a.params[1], i = (uint32_t)at;
	if (at >= n)
		return;
	uint32_t g, first;
	uint4 p;
	const bool member = lf_member(a.cands, a.pkts, a.conns, i, n, k, g, p, first);
	ldt_pkt(a, i, member, first + p.x);
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_conn_kernel(LdtArgs a)
{
	const uint64_t at = (uint64_t)blockIdx.x * LE_THREADS + threadIdx.x;
	if (at >= a.params[1])
		return;
	const uint32_t g = (uint32_t)at;
	const uint4 lo = reinterpret_cast<const uint4 *>(a.cnum + (size_t)g * 8)[0], hi = reinterpret_cast<const uint4 *>(a.cnum + (size_t)g * 8)[1];
	const uint4 t0 = reinterpret_cast<const uint4 *>(a.tally + (size_t)g * 8)[0], t1 = reinterpret_cast<const uint4 *>(a.tally + (size_t)g * 8)[1];
	uint2 *o = reinterpret_cast<uint2 *>(a.data + g);
	if (!lo.x) {                                            // no member
#pragma unroll
		for (int w = 0; w < 6; w++)
			o[w] = make_uint2(0, 0);
		return;
	}
	const unsigned long long bytes = (((unsigned long long)hi.z << 32) | hi.y) - (((unsigned long long)lo.w << 32) | lo.z);
	o[0] = make_uint2((uint32_t)bytes, (uint32_t)(bytes >> 32));
	o[1] = make_uint2(lo.y, hi.x - lo.y);
	o[2] = make_uint2(t1.w, t0.x);
	o[3] = make_uint2(t0.y, t0.z);
	o[4] = make_uint2(t0.w, t1.x);
	o[5] = make_uint2(t1.y, t1.z);
}

// ---- 8. the gather -----------------------------------------------------------------------------------------------------------------

// LDT_FRAG lanes per slot.  A fragment of a stored message goes to d_bytes in the 8-byte words of its DESTINATION: word c of the
// fragment's range covers payload octets 8c - head .. 8c - head + 7 (head = the destination's offset in its first word), which are 64
// stream bits from one funnel shift of two words, XORed with the 64 whitening bits of their position from the table.  A word that lies
// inside the fragment is one 8-byte store; the first and last words, where they hold a neighbour's octets, go out octet by octet
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_data_gather_kernel(LdtArgs a)
{
	__shared__ unsigned long long wt[128];
	const uint32_t tid = threadIdx.x, n = a.params[0];
	if (tid < 127)
		wt[tid] = a.wtab[tid];
	__syncthreads();
	const uint64_t at = (uint64_t)blockIdx.x * (LE_THREADS / LDT_FRAG) + tid / LDT_FRAG;
	if (at >= n)
		return;
	const uint32_t q = (uint32_t)at, sub = tid % LDT_FRAG;
	const unsigned long long dst = a.gdst[q];
	if (dst == ~0ULL)
		return;
	const uint32_t x = a.sinfo[q], len = x & 0xffu;
	const uint32_t i = a.slot[q];
	const uint2 where = reinterpret_cast<const uint2 *>(a.cands + i)[0];
	const uint32_t stream = reinterpret_cast<const uint2 *>(a.cands + i)[2].x & 0xffffu;
	const bool in_range = stream < a.n_streams;
	const uint64_t *w = a.words + (in_range ? (uint64_t)stream * a.pitch_words : 0);
	const uint64_t bit0 = ((((uint64_t)where.y << 32) | where.x) & LT_OFF_MASK) + 56;
	const uint32_t phase = (x >> 24) + 16u + 127u, head = (uint32_t)(dst & 7);
	const uint32_t n_chunks = (head + len + 7) >> 3;
	uint8_t *out = a.bytes + (dst - head);
	for (uint32_t c = sub; c < n_chunks; c += LDT_FRAG) {
		const int k0 = (int)(8 * c) - (int)head;                // the payload octet at the word's first byte
		unsigned long long v = in_range ? ldt_read64(w, a.n_words, bit0 + (int64_t)(8 * k0)) : 0;
		v ^= wt[(uint32_t)((int)phase + 8 * k0) % 127u];
		const uint32_t lo = k0 < 0 ? (uint32_t)-k0 : 0u, hi = len - k0 < 8 ? (uint32_t)(len - k0) : 8u;
		if (lo == 0 && hi == 8) {
			*reinterpret_cast<unsigned long long *>(out + 8 * (size_t)c) = v;
		} else {
			for (uint32_t j = lo; j < hi; j++)
				out[8 * (size_t)c + j] = (uint8_t)(v >> (8 * j));
		}
	}
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------

extern "C" size_t btbbx_le_data_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap)
{
	return le_data_layout(cand_cap, conn_cap).total;
}

// what the kernels are launched with, from a run's parameters and the layout of its scratch
static LdtArgs le_data_args(const LdtLayout &L, const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			    const btbbx_le_cand *d_cands, const uint32_t *d_count, uint32_t cap, const btbbx_le_conn *d_conns,
			    const uint32_t *d_conn_count, uint32_t conn_cap, const btbbx_le_track_pkt *d_pkts, btbbx_le_data *d_data,
			    btbbx_le_data_pkt *d_data_pkts, btbbx_le_msg *d_msgs, uint32_t msg_cap, uint32_t *d_msg_count, uint8_t *d_bytes,
			    uint64_t byte_cap, uint64_t *d_byte_count, void *d_scratch)
{
	char *s = (char *)d_scratch;
	LdtArgs a;
	a.words = d_words;
	a.n_words = n_words;
	a.pitch_words = n_streams > 1 ? pitch_words : n_words;
	a.cands = d_cands;
	a.pkts = d_pkts;
	a.conns = d_conns;
	a.d_cand_count = d_count;
	a.d_conn_count = d_conn_count;
	a.n_streams = n_streams;
	a.cand_cap = cap;
	a.conn_cap = conn_cap;
	a.n_tiles = L.tiles_n;
	a.msg_cap = msg_cap;
	a.params = (uint32_t *)(s + L.params);
	a.slot = (uint32_t *)(s + L.slot);
	a.sg = (uint32_t *)(s + L.sg);
	a.sinfo = (uint32_t *)(s + L.sinfo);
	a.sx = (uint32_t *)(s + L.sx);
	a.cx = (uint32_t *)(s + L.cx);
	a.ps = (uint32_t *)(s + L.ps);
	a.mbytes = (uint32_t *)(s + L.mbytes);
	a.mfrag = (uint32_t *)(s + L.mfrag);
	a.msgno = (uint32_t *)(s + L.msgno);
	a.tiles = (uint32_t *)(s + L.tiles);
	a.cend = (uint32_t *)(s + L.cend);
	a.cnum = (uint32_t *)(s + L.cnum);
	a.tally = (uint32_t *)(s + L.tally);
	a.wphase = (uint32_t *)(s + L.wphase);
	a.boff = (unsigned long long *)(s + L.boff);
	a.gdst = (unsigned long long *)(s + L.gdst);
	a.wtab = (unsigned long long *)(s + L.wtab);
	a.data = d_data;
	a.dpkts = d_data_pkts;
	a.msgs = d_msgs;
	a.msg_count = d_msg_count;
	a.bytes = d_bytes;
	a.byte_cap = byte_cap;
	a.byte_count = (unsigned long long *)d_byte_count;
	return a;
}

// the 18 launches of one run
static int le_data_launch(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, const btbbx_le_cand *d_cands,
			  const uint32_t *d_count, uint32_t cap, const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
			  const btbbx_le_track_pkt *d_pkts, btbbx_le_data *d_data, btbbx_le_data_pkt *d_data_pkts, btbbx_le_msg *d_msgs,
			  uint32_t msg_cap, uint32_t *d_msg_count, uint8_t *d_bytes, uint64_t byte_cap, uint64_t *d_byte_count, void *d_scratch,
			  hipStream_t q)
{
	const LdtLayout L = le_data_layout(cap, conn_cap);
	const LdtArgs a = le_data_args(L, d_words, n_words, pitch_words, n_streams, d_cands, d_count, cap, d_conns, d_conn_count, conn_cap, d_pkts,
				       d_data, d_data_pkts, d_msgs, msg_cap, d_msg_count, d_bytes, byte_cap, d_byte_count, d_scratch);
	const dim3 per_cand((uint32_t)(((uint64_t)cap + LE_THREADS - 1) / LE_THREADS)), per_tile(L.tiles_n), wg(LE_THREADS), one(1);
	const dim3 per_conn((uint32_t)(((uint64_t)conn_cap + LE_THREADS - 1) / LE_THREADS));
	const dim3 per_frag((uint32_t)(((uint64_t)cap + LE_THREADS / LDT_FRAG - 1) / (LE_THREADS / LDT_FRAG)));
	const dim3 init_grid((uint32_t)(((uint64_t)std::max(std::max(cap, conn_cap), 127u) + LE_THREADS - 1) / LE_THREADS));
	hipLaunchKernelGGL(le_data_init_kernel, init_grid, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_slot_kernel, per_cand, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_open_sum_kernel, per_tile, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_open_prefix_kernel, one, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_open_kernel, per_tile, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_prev_sum_kernel, per_tile, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_prev_prefix_kernel, one, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_prev_kernel, per_tile, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_msg_sum_kernel, per_tile, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_msg_prefix_kernel, one, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_msg_kernel, per_tile, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_close_kernel, per_cand, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_number_sum_kernel, per_tile, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_number_prefix_kernel, one, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_number_kernel, per_tile, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_pkt_kernel, per_cand, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_conn_kernel, per_conn, wg, 0, q, a);
	hipLaunchKernelGGL(le_data_gather_kernel, per_frag, wg, 0, q, a);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

extern "C" int btbbx_le_data_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				    const uint16_t *d_phys_channel,
				    const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
				    const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
				    const btbbx_le_track *d_tracks, const btbbx_le_track_pkt *d_pkts,
				    btbbx_le_data *d_data, btbbx_le_data_pkt *d_data_pkts, btbbx_le_msg *d_msgs, uint32_t msg_cap,
				    uint32_t *d_msg_count, uint8_t *d_bytes, uint64_t byte_cap, uint64_t *d_byte_count,
				    void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
	const char *who = "btbbx_le_data_device";
	int rc = le_check_streams(who, n_words, pitch_words, n_streams);
	if (rc)
		return rc;
	const LdtLayout L = le_data_layout(cand_cap, conn_cap);
	if (!d_words || !d_phys_channel || !d_cands || !d_cand_count || !d_conns || !d_conn_count || !d_tracks || !d_pkts || !d_data ||
	    !d_data_pkts || (!d_msgs && msg_cap) || !d_msg_count || (!d_bytes && byte_cap) || !d_byte_count || !d_scratch ||
	    scratch_bytes < L.total) {
		set_error("%s: null pointer, or scratch of %zu bytes needed and %zu given", who, L.total, scratch_bytes);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_words & 7) || ((uintptr_t)d_cands & 7) || ((uintptr_t)d_conns & 7) || ((uintptr_t)d_tracks & 7) ||
	    ((uintptr_t)d_pkts & 7) || ((uintptr_t)d_data & 7) || ((uintptr_t)d_msgs & 7) || ((uintptr_t)d_bytes & 7) ||
	    ((uintptr_t)d_byte_count & 7) || ((uintptr_t)d_data_pkts & 3) || ((uintptr_t)d_scratch & 15) || ((uintptr_t)d_cand_count & 3) ||
	    ((uintptr_t)d_conn_count & 3) || ((uintptr_t)d_msg_count & 3) || ((uintptr_t)d_phys_channel & 1)) {
		set_error("%s: misaligned pointer (scratch 16 bytes; words, records, the byte buffer and its count 8; the 12-byte records and the "
			  "counters 4; the channels 2)", who);
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
	return le_data_launch(d_words, n_words, pitch_words, n_streams, d_cands, d_cand_count, cand_cap, d_conns, d_conn_count, conn_cap, d_pkts,
			      d_data, d_data_pkts, d_msgs, msg_cap, d_msg_count, d_bytes, byte_cap, d_byte_count, d_scratch, q);
}
