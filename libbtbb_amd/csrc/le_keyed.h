// le_keyed.h -- keyed LE following (included by le.hip, behind le_crypt.h): the follow stage of le_follow.h and the span stage of
// le_span.h with the control PDUs behind LL_START_ENC_REQ read as plaintext where the decryption stage VERIFIED them.  The contract
// is in include/btbbx.h (btbbx_le_keyed_epoch_device, btbbx_le_keyed_span_device), the reasoning in DESIGN 3.8.9.
//
// Both stages read a control PDU's payload in two places only: le_epoch_slot_kernel writes the control word ctl[i], and
// le_span_param_kernel reads a parameter update's octets 0..9 again.  Every later pass reads ctl, and only the packet kernels say a
// PDU's kind.  So a keyed run has as many launches as an unkeyed one, with these five kernels in the places of five of its own:
//
//   le_keyed_slot_kernel    le_epoch_slot_kernel, with the ENC_START rank kept where no kernel of either stage looks (LfConn.pad[0],
//                           inverted) and LfConn.enc_rank left at LF_NONE: no later kernel hides a member; two bits per candidate say
//                           which are CONTROL members and which of them rule 1 lets read if their rank allows, so that the
//                           next kernel looks at those alone
//   le_keyed_open_kernel    le_epoch_open_kernel; and one lane per candidate: a CONTROL member above ENC_START gets its control word
//                           again -- from its plaintext when it is READABLE, with opcode 0xff when it is not, so that no later pass
//                           acts on it; the member's mark goes into the word's free bits, a READABLE member's 12 octets to plain[i]
//   le_keyed_param_kernel   le_span_param_kernel, with a READABLE member's octets taken from plain[i]
//   le_keyed_pkt_epoch_kernel, le_keyed_pkt_span_kernel    le_epoch_pkt_kernel and le_span_pkt_kernel, with kind OPAQUE for the
//                           members that stayed unread, kind CONTROL for a READABLE member that reads as opcode 5 and length 1, and
//                           the ENCRYPTED and DECRYPTED flags put into the connection's record
//
// Each keeps its original's rules through the original's own device functions (lf_member, lf_pdu_kind, lf_pkt_event, ...); what is
// written twice is the octet reader (lk_octets) and the frame of each kernel.  A change to one of the five originals is made here
// too; equality (a) of the contract, which the GPU tests hold on both stages' lattices, is what keeps the pairs together.
// Only a workgroup that holds a member that may be READABLE builds AES's round table (1 KiB of LDS, from the field's definition) -- control PDUs
// are a handful per connection.
#pragma once
#include "le_span.h"
#include "le_crypt.h"

#define LK_ABOVE     (1u << 24)            // ctl.x: a CONTROL member above ENC_START (no pass of either stage looks at bits 24..28)
#define LK_READABLE  (1u << 25)            // ctl.x: and read as plaintext; plain[i] holds its octets

struct LkLayout {
	size_t plain, control, maybe, total;   // behind the stage's own layout
};

static LkLayout le_keyed_layout(size_t stage_total, uint32_t cand_cap, uint32_t conn_cap)
{
	LkLayout K;
	const size_t c = cand_cap ? cand_cap : 1;
	(void)conn_cap;
	K.plain = ld_up(stage_total);
	K.control = K.plain + ld_up(c * 16);
	K.maybe = K.control + ld_up((c + 63) / 64 * 8);
	K.total = K.maybe + ld_up((c + 63) / 64 * 8);
	return K;
}

// what the keyed kernels take beside the stage's own arrays
struct LkArgs {
	const uint64_t *words;
	uint64_t n_words, pitch_words;
	uint32_t n_streams;
	const btbbx_le_cand *cands;
	const btbbx_le_track_pkt *pkts;
	const btbbx_le_conn *conns;
	const btbbx_le_seed *seeds;
	const btbbx_le_data_pkt *dpkts;
	const btbbx_le_crypt *crypt;
	const btbbx_le_crypt_pkt *cpkts;
	uint4 *plain;                          // per candidate: a READABLE member's plaintext octets 0..7 and 8..11 (written for those alone)
	unsigned long long *control;           // per 64 candidates (a wave of the slot kernel): bit i & 63 = candidate i is a CONTROL member
	unsigned long long *maybe;             // the same for: and READABLE, if its rank lies above ENC_START's (rule 1 but for the rank)
};

// The ENC_START rank of connection g, LF_NONE without one.  pad[0] holds its complement: le_epoch_init_kernel leaves 0 there, and
// no kernel of the follow or span stage reads the word
__device__ __forceinline__ uint32_t lk_enc_rank(const LfConn *work, uint32_t g)
{
	return ~work[g].pad[0];
}

// follow rule 3's octets: `take` (<= 12) payload octets of the candidate c on a channel whose whitening register starts at ch,
// dewhitened, bits beyond the stream's end as 0 (the reader of le_epoch_slot_kernel and le_span_param_kernel)
__device__ __forceinline__ void lk_octets(const LkArgs &a, const LdCand &c, uint32_t ch, uint32_t take, unsigned long long &lo8, uint32_t &hi4)
{
	const uint64_t *w = a.words + (uint64_t)(c.c.x & 0xffffu) * a.pitch_words;
	const uint64_t bit0 = ((((uint64_t)c.a.y << 32) | c.a.x) & LT_OFF_MASK) + 56;
	uint32_t ws = (ch & 0x3fu) | 0x40u;
	lf_whiten8(ws);
	lf_whiten8(ws);
	lo8 = 0;
	hi4 = 0;
#pragma unroll 1
	for (uint32_t j = 0; j < take; j++) {
		const uint64_t bit = bit0 + 8ull * j, wi = bit >> 6;
		const uint32_t sh = (uint32_t)(bit & 63);
		const uint64_t lo = wi < a.n_words ? w[wi] : 0;
		const uint64_t hi = sh > 56 && wi + 1 < a.n_words ? w[wi + 1] : 0;
		const uint32_t v = ((uint32_t)(((lo >> sh) | (sh ? hi << (64 - sh) : 0)) & 0xffu)) ^ lf_whiten8(ws);
		if (j < 8)
			lo8 |= (unsigned long long)v << (8 * j);
		else
			hi4 |= v << (8 * (j - 8));
	}
}

// follow rule 3's control word of a PDU with these payload octets and this length (the marks of this file not among its bits)
__device__ __forceinline__ uint4 lk_word(unsigned long long lo8, uint32_t hi4, uint32_t len)
{
	const uint32_t opcode = (uint32_t)lo8 & 0xffu;
	uint4 info = make_uint4(LF_CONTROL | (opcode << 8) | (len << 16), 0, 0, 0);
	if (opcode == 1 && len == 8) {                          // LL_CHANNEL_MAP_IND: ChM, Instant
		const unsigned long long map = (lo8 >> 8) & LC_MAP37;
		info.y = (uint32_t)(lo8 >> 48);
		info.z = (uint32_t)map;
		info.w = (uint32_t)(map >> 32);
	} else if (opcode == 0 && len == 12) {                  // LL_CONNECTION_UPDATE_IND: ..., Instant
		info.y = hi4 >> 16;
	}
	return info;
}

// Rule 1 for a CONTROL member i of g, but for its rank: the decryption stage VERIFIED it under the connection's key, it is long
// enough to carry a MIC and its sender is known.  role: the data stage's
__device__ __forceinline__ bool lk_readable(const LkArgs &a, uint32_t i, uint32_t g, uint32_t len, uint32_t &role)
{
	role = reinterpret_cast<const uint32_t *>(a.dpkts)[3 * (size_t)i + 2] & 0xffu;
	const uint32_t cflags = (reinterpret_cast<const uint32_t *>(a.crypt + g)[13] >> 16) & 0xffu;
	const uint32_t state = reinterpret_cast<const uint32_t *>(a.cpkts + i)[2] & 0xffu;
	return (cflags & BTBBX_LE_CRYPT_KEYED) && state == BTBBX_LE_CRYPT_VERIFIED && len >= 5 &&
	       (role == BTBBX_LE_ROLE_CENTRAL || role == BTBBX_LE_ROLE_PERIPHERAL);
}

// ---- in the place of le_epoch_slot_kernel ---------------------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_keyed_slot_kernel(LkArgs a, const uint32_t *params, uint32_t *slot, uint4 *ctl, LfConn *work)
{
	static_assert(LE_THREADS % 64 == 0, "a wave holds 64 candidates in a row");
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0], k = params[1];
	uint32_t g, first;
	uint4 p, info = make_uint4(0, 0, 0, 0);
	bool maybe = false;
	if (i < n && lf_member(a.cands, a.pkts, a.conns, i, n, k, g, p, first)) {
		slot[first + p.x] = i;
		const LdCand c = ld_load(a.cands, i);
		const uint32_t stream = c.c.x & 0xffffu, h0 = (c.c.x >> 16) & 0xffu, len = c.c.x >> 24;
		if ((h0 & 3u) == 3u && len >= 1 && stream < a.n_streams) {
			unsigned long long lo8;
			uint32_t hi4;
			lk_octets(a, c, p.w, len < 12 ? len : 12, lo8, hi4);
			info = lk_word(lo8, hi4, len);
			atomicAdd(&work[g].n_control, 1u);
			if (((info.x >> 8) & 0xffu) == 5 && len == 1)   // LL_START_ENC_REQ: the smallest rank, as the largest complement
				atomicMax(&work[g].pad[0], ~p.x);
			uint32_t role;
			maybe = lk_readable(a, i, g, len, role);
		}
	}
	// (every lane of the wave is here.)  The open kernel asks these words, not 16 bytes of ctl per candidate, whether to look closer
	const unsigned long long control = __ballot(info.x & LF_CONTROL), readable = __ballot(maybe);
	if ((threadIdx.x & 63u) == 0 && (i & ~63u) < n) {
		a.control[i >> 6] = control;
		a.maybe[i >> 6] = readable;
	}
	if (i < n)
		ctl[i] = info;
}

// ---- in the place of le_epoch_open_kernel ---------------------------------------------------------------------------------------

// that kernel's work for the position q of the time order
__device__ __forceinline__ void lk_open(const LkArgs &a, uint32_t q, uint32_t n, uint32_t k, const uint32_t *slot, uint64_t *anchor, uint32_t *econn)
{
	const uint32_t i = slot[q];
	if (i == LF_NONE)
		return;
	uint32_t g, first;
	uint4 p;
	if (!lf_member(a.cands, a.pkts, a.conns, i, n, k, g, p, first))
		return;
	bool open = q == first;
	if (!open) {
		const uint32_t before = slot[q - 1];
		open = before == LF_NONE || reinterpret_cast<const uint4 *>(a.pkts)[before].y != p.y;
	}
	if (!open)
		return;
	const uint2 at = reinterpret_cast<const uint2 *>(a.cands + i)[0];
	anchor[first + p.y] = ((((uint64_t)at.y << 32) | at.x) & LT_OFF_MASK) | ((uint64_t)(p.w & 0xffu) << 56);
	econn[first + p.y] = g;
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_keyed_open_kernel(LkArgs a, const uint32_t *params, const uint32_t *slot, uint64_t *anchor,
									      uint32_t *econn, uint4 *ctl, const LfConn *work)
{
	__shared__ uint32_t te[256];
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0], k = params[1];
	// the round table, where one of the workgroup's candidates may be READABLE (the same answer in every thread: no thread has left)
	bool table = false;
#pragma unroll
	for (uint32_t w = 0; w < LE_THREADS / 64; w++) {
		const uint32_t at = blockIdx.x * (LE_THREADS / 64) + w;
		if ((uint64_t)at * 64 < n)
			table = table || a.maybe[at] != 0;
	}
	if (table) {
		te[threadIdx.x] = lx_te_entry(threadIdx.x);
		__syncthreads();
	}
	if (i >= n)
		return;
	lk_open(a, i, n, k, slot, anchor, econn);
	if (!((a.control[i >> 6] >> (i & 63u)) & 1u))
		return;
	uint32_t g, first;
	uint4 p;
	if (!lf_member(a.cands, a.pkts, a.conns, i, n, k, g, p, first) || p.x <= lk_enc_rank(work, g))
		return;
	const uint32_t len = (ctl[i].x >> 16) & 0xffu;
	const bool readable = (a.maybe[i >> 6] >> (i & 63u)) & 1u;
	uint4 info = make_uint4(LF_CONTROL | (0xffu << 8) | (len << 16) | LK_ABOVE, 0, 0, 0);
	if (readable) {
		// rule 2: S_1 under the connection's session key, the nonce of the decryption stage's rule 5
		const uint32_t *cw = reinterpret_cast<const uint32_t *>(a.crypt + g);
		const uint4 cp = reinterpret_cast<const uint4 *>(a.cpkts)[i];
		const uint32_t role = reinterpret_cast<const uint32_t *>(a.dpkts)[3 * (size_t)i + 2] & 0xffu;
		uint32_t rk[LX_RK];
		rk[0] = cw[0];
		rk[1] = cw[1];
		rk[2] = cw[2];
		rk[3] = cw[3];
		lx_expand(te, rk);
		const unsigned long long c = cp.x | ((unsigned long long)((cp.z >> 24) & 0x7fu) << 32);   // (39 bits: a list from elsewhere)
		const LxBlock s = lx_aes(te, rk, lx_nonce_block(0x01u, c, role == BTBBX_LE_ROLE_CENTRAL ? 1u : 0u, cw[4], cw[5], 1));
		const uint32_t plen = len - 4, take = plen < 12 ? plen : 12;
		unsigned long long lo8;
		uint32_t hi4;
		lk_octets(a, ld_load(a.cands, i), p.w, take, lo8, hi4);
		lo8 ^= ((unsigned long long)s.w[1] << 32) | s.w[0];
		hi4 ^= s.w[2];
		if (take < 8)
			lo8 &= (1ull << (8 * take)) - 1;
		hi4 = take <= 8 ? 0u : (take < 12 ? hi4 & ((1u << (8 * (take - 8))) - 1) : hi4);
		// rule 3: the slot kernel's parsing, with L' in the length's place
		info = lk_word(lo8, hi4, plen);
		info.x |= LK_ABOVE | LK_READABLE;
		a.plain[i] = make_uint4((uint32_t)lo8, (uint32_t)(lo8 >> 32), hi4, 0);
	}
	ctl[i] = info;
}

// ---- in the place of le_span_param_kernel ---------------------------------------------------------------------------------------

// prm[i] and ctl[i].z as that kernel leaves them; a READABLE member's octets are its plaintext's.  (No member is hidden here: one
// above ENC_START that was not read has opcode 0xff)
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_keyed_param_kernel(LkArgs a, const uint32_t *params, uint4 *ctl, uint2 *prm, LfConn *work)
{
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0], k = params[1];
	if (i >= n)
		return;
	const uint32_t x = ctl[i].x;
	if (!(x & LF_CONTROL))
		return;
	uint32_t g, first;
	uint4 p;
	if (!lf_member(a.cands, a.pkts, a.conns, i, n, k, g, p, first) || !lf_seeded(a.seeds, g))
		return;
	const uint32_t opcode = (x >> 8) & 0xffu, len = (x >> 16) & 0xffu;
	if (opcode == 2 && len == 2)
		atomicOr(&work[g].flags, (uint32_t)BTBBX_LE_FOLLOW_TERMINATED);
	if (opcode != 0 || len != 12)
		return;
	unsigned long long lo8;
	uint32_t hi4;
	if (x & LK_READABLE) {
		const uint4 pl = a.plain[i];
		lo8 = ((unsigned long long)pl.y << 32) | pl.x;
		hi4 = pl.z;
	} else {
		const LdCand c = ld_load(a.cands, i);
		if ((c.c.x & 0xffffu) >= a.n_streams)
			return;
		lk_octets(a, c, p.w, 10, lo8, hi4);
	}
	const uint32_t win_size = (uint32_t)(lo8 >> 8) & 0xffu, win_offset = (uint32_t)(lo8 >> 16) & 0xffffu;
	const uint32_t interval = (uint32_t)(lo8 >> 32) & 0xffffu, latency = (uint32_t)(lo8 >> 48) & 0xffffu;
	prm[i] = make_uint2(win_size | (win_offset << 16), interval | (latency << 16));
	ctl[i].z = hi4 & 0xffffu;                               // Timeout
}

// ---- in the places of le_epoch_pkt_kernel and le_span_pkt_kernel ------------------------------------------------------------------

// The kind and opcode of member i (control word x, rank `rank`) of connection g, as rule 3 of the contract has them, where
// lf_pdu_kind sees no ENC_START.  flags: the 32-bit word of g's record that holds its flags, at bit `shift`: a READABLE member of a
// SEEDED connection sets DECRYPTED there and the ENC_START itself ENCRYPTED (the verdict kernel, which sees no start, left them 0;
// no bit of the word that a packet kernel reads changes)
__device__ __forceinline__ uint32_t lk_pdu_kind(uint32_t x, uint32_t rank, uint32_t enc_rank, bool seeded, uint32_t *flags, uint32_t shift, uint32_t &op)
{
	uint32_t kind = lf_pdu_kind(x, rank, LF_NONE, op);
	if (x & LK_ABOVE) {
		if (!(x & LK_READABLE)) {
			kind = BTBBX_LE_PDU_OPAQUE;
			op = 0xff;
		} else {
			if (kind == BTBBX_LE_PDU_ENC_START)
				kind = BTBBX_LE_PDU_CONTROL;
			if (seeded)
				atomicOr(flags, (uint32_t)BTBBX_LE_FOLLOW_DECRYPTED << shift);
		}
	} else if (seeded && rank == enc_rank) {
		atomicOr(flags, (uint32_t)BTBBX_LE_FOLLOW_ENCRYPTED << shift);
	}
	return kind;
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_keyed_pkt_epoch_kernel(LkArgs a, const uint32_t *params, const uint4 *ctl, const uint4 *evres,
										   const LfConn *work, btbbx_le_follow *follows,
										   btbbx_le_follow_pkt *out)
{
	static_assert(offsetof(btbbx_le_follow, flags) == 41 && offsetof(btbbx_le_follow, algorithm) == 40, "the word lk_pdu_kind sets flags in");
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0], k = params[1];
	if (i >= n)
		return;
	uint32_t g, first, w0 = 0xffffffffu, w1 = 0xffffffffu, w2 = 0xffffffffu;
	uint4 p;
	if (lf_member(a.cands, a.pkts, a.conns, i, n, k, g, p, first)) {
		const bool seeded = lf_seeded(a.seeds, g);
		uint32_t op;
		const uint32_t kind = lk_pdu_kind(ctl[i].x, p.x, lk_enc_rank(work, g), seeded, reinterpret_cast<uint32_t *>(follows + g) + 10, 8, op);
		LfPktEvent e = {0, 0, 0, 0, 0xff, 0};
		if (seeded)
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

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_keyed_pkt_span_kernel(LkArgs a, const uint32_t *params, const uint4 *ctl, const uint4 *evres,
										  const LfConn *work, btbbx_le_span *spans, btbbx_le_span_pkt *out)
{
	static_assert(offsetof(btbbx_le_span, flags) == 55 && offsetof(btbbx_le_span, algorithm) == 54, "the word lk_pdu_kind sets flags in");
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0], k = params[1];
	if (i >= n)
		return;
	uint32_t g, first;
	uint4 p, o = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
	if (lf_member(a.cands, a.pkts, a.conns, i, n, k, g, p, first)) {
		const uint32_t x = ctl[i].x;
		const bool seeded = lf_seeded(a.seeds, g);
		uint32_t op, applied = 0;
		const uint32_t kind = lk_pdu_kind(x, p.x, lk_enc_rank(work, g), seeded, reinterpret_cast<uint32_t *>(spans + g) + 13, 24, op);
		LfPktEvent e = {0, 0, 0, 0, 0xff, 0};
		if (seeded) {
			lf_pkt_event(evres[first + p.y], &spans[g].algorithm, p.w & 0xffu, e);
			applied = (x & LS_APPLIED) ? 1u : 0u;
		}
		o = make_uint4(e.counter, e.epoch | (e.span << 16), kind | (op << 8) | (e.expected << 16) | (e.on << 24), e.state | (applied << 8));
	}
	reinterpret_cast<uint4 *>(out)[i] = o;
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------

// the keyed reading of a run's control PDUs, in LfReadClear's and LsReadClear's place: the same launches, with this file's kernels
struct LkRead {
	LkArgs a;

	void tables(const LfBufs &B, const uint64_t *, uint64_t, uint64_t, uint32_t, const btbbx_le_cand *, const btbbx_le_track_pkt *,
		    const btbbx_le_conn *, dim3 per_cand, hipStream_t q) const
	{
		const dim3 wg(LE_THREADS);
		hipLaunchKernelGGL(le_keyed_slot_kernel, per_cand, wg, 0, q, a, B.params, B.slot, B.ctl, B.work);
		hipLaunchKernelGGL(le_keyed_open_kernel, per_cand, wg, 0, q, a, B.params, B.slot, B.anchor, B.econn, B.ctl, B.work);
	}
	void param(const LfBufs &B, const uint64_t *, uint64_t, uint64_t, uint32_t, const btbbx_le_cand *, const btbbx_le_track_pkt *,
		   const btbbx_le_conn *, const btbbx_le_seed *, uint2 *prm, dim3 per_cand, hipStream_t q) const
	{
		hipLaunchKernelGGL(le_keyed_param_kernel, per_cand, dim3(LE_THREADS), 0, q, a, B.params, B.ctl, prm, B.work);
	}
	void follow_pkts(const LfBufs &B, const btbbx_le_cand *, const btbbx_le_track_pkt *, const btbbx_le_conn *, const btbbx_le_seed *,
			 btbbx_le_follow *d_follows, btbbx_le_follow_pkt *d_fpkts, dim3 per_cand, hipStream_t q) const
	{
		hipLaunchKernelGGL(le_keyed_pkt_epoch_kernel, per_cand, dim3(LE_THREADS), 0, q, a, B.params, B.ctl, B.evres, B.work, d_follows, d_fpkts);
	}
	void span_pkts(const LfBufs &B, const btbbx_le_cand *, const btbbx_le_track_pkt *, const btbbx_le_conn *, const btbbx_le_seed *,
		       btbbx_le_span *d_spans, btbbx_le_span_pkt *d_spkts, dim3 per_cand, hipStream_t q) const
	{
		hipLaunchKernelGGL(le_keyed_pkt_span_kernel, per_cand, dim3(LE_THREADS), 0, q, a, B.params, B.ctl, B.evres, B.work, d_spans, d_spkts);
	}
};

// stage_total: the bytes of the stage's own layout, behind which this one's array stands in d_scratch
static LkRead le_keyed_read(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, const btbbx_le_cand *d_cands,
			    uint32_t cap, const btbbx_le_conn *d_conns, uint32_t conn_cap, const btbbx_le_track_pkt *d_pkts, const btbbx_le_seed *d_seeds,
			    const btbbx_le_data_pkt *d_data_pkts, const btbbx_le_crypt *d_crypt, const btbbx_le_crypt_pkt *d_crypt_pkts,
			    size_t stage_total, void *d_scratch)
{
	const LkLayout K = le_keyed_layout(stage_total, cap, conn_cap);
	LkRead r;
	r.a = {d_words, n_words, pitch_words, n_streams, d_cands, d_pkts, d_conns, d_seeds, d_data_pkts, d_crypt, d_crypt_pkts,
	       (uint4 *)((char *)d_scratch + K.plain), (unsigned long long *)((char *)d_scratch + K.control),
	       (unsigned long long *)((char *)d_scratch + K.maybe)};
	return r;
}

extern "C" size_t btbbx_le_keyed_epoch_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap)
{
	return le_keyed_layout(le_follow_layout(cand_cap, conn_cap).total, cand_cap, conn_cap).total;
}

extern "C" size_t btbbx_le_keyed_span_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap, uint32_t max_updates)
{
	const uint32_t m = max_updates > LS_MAX_UPDATES ? LS_MAX_UPDATES : max_updates;
	return le_keyed_layout(le_span_layout(cand_cap, conn_cap, m).total, cand_cap, conn_cap).total;
}

static int le_keyed_launch_epoch(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, const btbbx_le_cand *d_cands,
				 const uint32_t *d_count, uint32_t cap, const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
				 const btbbx_le_track_pkt *d_pkts, const btbbx_le_seed *d_seeds, const btbbx_le_data_pkt *d_data_pkts,
				 const btbbx_le_crypt *d_crypt, const btbbx_le_crypt_pkt *d_crypt_pkts, uint32_t unit_bits, uint32_t jitter_bits,
				 btbbx_le_follow *d_follows, btbbx_le_follow_pkt *d_fpkts, void *d_scratch, hipStream_t q)
{
	return le_follow_launch(d_words, n_words, pitch_words, n_streams, d_cands, d_count, cap, d_conns, d_conn_count, conn_cap, d_pkts, d_seeds,
				unit_bits, jitter_bits, d_follows, d_fpkts, d_scratch, q,
				le_keyed_read(d_words, n_words, pitch_words, n_streams, d_cands, cap, d_conns, conn_cap, d_pkts, d_seeds, d_data_pkts, d_crypt,
					      d_crypt_pkts, le_follow_layout(cap, conn_cap).total, d_scratch));
}

static int le_keyed_launch_span(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, const btbbx_le_cand *d_cands,
				const uint32_t *d_count, uint32_t cap, const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
				const btbbx_le_track_pkt *d_pkts, const btbbx_le_seed *d_seeds, const btbbx_le_data_pkt *d_data_pkts,
				const btbbx_le_crypt *d_crypt, const btbbx_le_crypt_pkt *d_crypt_pkts, uint32_t unit_bits, uint32_t jitter_bits,
				uint32_t max_updates, btbbx_le_span *d_spans, btbbx_le_span_pkt *d_spkts, btbbx_le_span_rec *d_recs, void *d_scratch,
				hipStream_t q)
{
	return le_span_launch(d_words, n_words, pitch_words, n_streams, d_cands, d_count, cap, d_conns, d_conn_count, conn_cap, d_pkts, d_seeds,
			      unit_bits, jitter_bits, max_updates, d_spans, d_spkts, d_recs, d_scratch, q,
			      le_keyed_read(d_words, n_words, pitch_words, n_streams, d_cands, cap, d_conns, conn_cap, d_pkts, d_seeds, d_data_pkts, d_crypt,
					    d_crypt_pkts, le_span_layout(cap, conn_cap, max_updates).total, d_scratch));
}

// the three arrays a keyed entry takes beside the unkeyed one's
static int le_keyed_check_args(const char *who, const btbbx_le_data_pkt *d_data_pkts, const btbbx_le_crypt *d_crypt,
			       const btbbx_le_crypt_pkt *d_crypt_pkts)
{
	if (!d_data_pkts || !d_crypt || !d_crypt_pkts) {
		set_error("%s: null pointer", who);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_crypt & 7) || ((uintptr_t)d_crypt_pkts & 15) || ((uintptr_t)d_data_pkts & 3)) {
		set_error("%s: misaligned pointer (d_crypt 8 bytes, d_crypt_pkts 16, d_data_pkts 4)", who);
		return BTBBX_E_ARG;
	}
	return BTBBX_OK;
}

extern "C" int btbbx_le_keyed_epoch_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
					   const uint16_t *d_phys_channel,
					   const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
					   const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
					   const btbbx_le_track *d_tracks, const btbbx_le_track_pkt *d_pkts, const btbbx_le_seed *d_seeds,
					   const btbbx_le_data_pkt *d_data_pkts, const btbbx_le_crypt *d_crypt, const btbbx_le_crypt_pkt *d_crypt_pkts,
					   uint32_t unit_bits, uint32_t jitter_bits,
					   btbbx_le_follow *d_follows, btbbx_le_follow_pkt *d_follow_pkts,
					   void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
	const char *who = "btbbx_le_keyed_epoch_device";
	int rc = le_track_check_args(who, n_streams, unit_bits, jitter_bits);
	if (!rc)
		rc = le_check_streams(who, n_words, pitch_words, n_streams);
	if (!rc)
		rc = le_keyed_check_args(who, d_data_pkts, d_crypt, d_crypt_pkts);
	if (rc)
		return rc;
	const size_t total = btbbx_le_keyed_epoch_scratch_bytes(cand_cap, conn_cap);
	if (!d_words || !d_phys_channel || !d_cands || !d_cand_count || !d_conns || !d_conn_count || !d_tracks || !d_pkts || !d_seeds ||
	    !d_follows || !d_follow_pkts || !d_scratch || scratch_bytes < total) {
		set_error("%s: null pointer, or scratch of %zu bytes needed and %zu given", who, total, scratch_bytes);
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
	return le_keyed_launch_epoch(d_words, n_words, pitch_words, n_streams, d_cands, d_cand_count, cand_cap, d_conns, d_conn_count, conn_cap, d_pkts,
				     d_seeds, d_data_pkts, d_crypt, d_crypt_pkts, unit_bits, jitter_bits, d_follows, d_follow_pkts, d_scratch,
				     (hipStream_t)hip_stream);
}

extern "C" int btbbx_le_keyed_span_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
					  const uint16_t *d_phys_channel,
					  const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
					  const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
					  const btbbx_le_track *d_tracks, const btbbx_le_track_pkt *d_pkts, const btbbx_le_seed *d_seeds,
					  const btbbx_le_data_pkt *d_data_pkts, const btbbx_le_crypt *d_crypt, const btbbx_le_crypt_pkt *d_crypt_pkts,
					  uint32_t unit_bits, uint32_t jitter_bits, uint32_t max_updates,
					  btbbx_le_span *d_spans, btbbx_le_span_pkt *d_span_pkts, btbbx_le_span_rec *d_span_recs,
					  void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
	const char *who = "btbbx_le_keyed_span_device";
	if (max_updates > LS_MAX_UPDATES) {
		set_error("%s: max_updates must be 0..%u", who, LS_MAX_UPDATES);
		return BTBBX_E_ARG;
	}
	int rc = le_track_check_args(who, n_streams, unit_bits, jitter_bits);
	if (!rc)
		rc = le_check_streams(who, n_words, pitch_words, n_streams);
	if (!rc)
		rc = le_keyed_check_args(who, d_data_pkts, d_crypt, d_crypt_pkts);
	if (rc)
		return rc;
	const size_t total = btbbx_le_keyed_span_scratch_bytes(cand_cap, conn_cap, max_updates);
	if (!d_words || !d_phys_channel || !d_cands || !d_cand_count || !d_conns || !d_conn_count || !d_tracks || !d_pkts || !d_seeds ||
	    !d_spans || !d_span_pkts || !d_span_recs || !d_scratch || scratch_bytes < total) {
		set_error("%s: null pointer, or scratch of %zu bytes needed and %zu given", who, total, scratch_bytes);
		return BTBBX_E_ARG;
	}
	if (((uintptr_t)d_words & 7) || ((uintptr_t)d_cands & 7) || ((uintptr_t)d_conns & 7) || ((uintptr_t)d_tracks & 7) ||
	    ((uintptr_t)d_pkts & 7) || ((uintptr_t)d_seeds & 7) || ((uintptr_t)d_spans & 7) || ((uintptr_t)d_span_pkts & 7) ||
	    ((uintptr_t)d_span_recs & 7) || ((uintptr_t)d_scratch & 15) || ((uintptr_t)d_cand_count & 3) || ((uintptr_t)d_conn_count & 3) ||
	    ((uintptr_t)d_phys_channel & 1)) {
		set_error("%s: misaligned pointer (scratch 16 bytes, words and records 8, the counters 4, the channels 2)", who);
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	if (!cand_cap || !conn_cap)
		return BTBBX_OK;
	return le_keyed_launch_span(d_words, n_words, pitch_words, n_streams, d_cands, d_cand_count, cand_cap, d_conns, d_conn_count, conn_cap, d_pkts,
				    d_seeds, d_data_pkts, d_crypt, d_crypt_pkts, unit_bits, jitter_bits, max_updates, d_spans, d_span_pkts, d_span_recs,
				    d_scratch, (hipStream_t)hip_stream);
}
