// le_span.h -- LE following through connection parameter updates (included by le.hip, behind le_follow.h): the span stage does what
// the follow stage of le_follow.h does and goes on where that one stops -- at the instant of an LL_CONNECTION_UPDATE_IND it finds the
// anchor of the new transmit window on the old grid, restarts the counting there with the new interval and carries counters, map
// updates and the hop check through.  A SPAN is the stretch of events one set of connection parameters times.  The contract is in
// include/btbbx.h (btbbx_le_span_device), the reasoning in DESIGN 3.8.5.  All arithmetic is integer arithmetic.
//
// The tables are the follow stage's (slot, event, anchor, control PDUs: its kernels 1-3 are launched as they are).  Behind them:
//
//   a. le_span_param_kernel     one lane per candidate: the fields of an LL_CONNECTION_UPDATE_IND the slot kernel did not keep; TERMINATE
//   b. le_span_begin_kernel     one lane per connection: span 0 from the seed, its first counted event, the records zeroed
//   c. max_updates + 1 ROUNDS; in round s every connection that is still followed works on its span s:
//        le_span_step_kernel      one lane per event: the steps of span s's events behind start_s, the others' kept; then the 64-bit
//                                 prefix sum over the whole table (le_track_prefix64_kernel, le_track_count_kernel)
//        le_span_instant_kernel   one lane per candidate: a valid parameter update in span s lowers I_s by an atomic minimum
//        le_span_pick_kernel      one lane per candidate: among those with I = I_s in front of it, the largest rank
//        le_span_bound_kernel     one lane per connection: L by a binary search of the counters, rule 5, f_(s+1) by a binary search of
//                                 the anchors -- both rise with the event index --, the span's record; or rule 6
//   d. le_span_mark_kernel, le_span_list_kernel, then the follow stage's sort (its radix passes, rekey and gather kernels)   the map
//      updates, as the follow stage lists them, over the final counters; the list kernel also marks and counts the valid parameter
//      updates
//   e. le_span_predict_kernel, le_span_verdict_kernel, le_span_pkt_kernel   the follow stage's 7-9 (its lf_predict, lf_tallies,
//      lf_verdict, lf_pdu_kind and lf_pkt_event), with the span and GAP
//
// The count of launches is 13 + 6 * (max_updates + 1) + 3 per radix pass: it depends on max_updates, on conn_cap through the radix
// passes over its bytes, and on nothing else.  Every loop of a kernel is bounded by N, by max_updates + 1 or by a constant.
#pragma once
#include "le_follow.h"

#define LS_APPLIED      (1u << 29)          // ctl.x: the parameter update that opened a span
#define LS_MAX_UPDATES  16u

static_assert(sizeof(btbbx_le_span) == 56 && offsetof(btbbx_le_span, counter_first) == 8 && offsetof(btbbx_le_span, stop) == 12 &&
	      offsetof(btbbx_le_span, n_before) == 16 && offsetof(btbbx_le_span, n_on) == 20 && offsetof(btbbx_le_span, n_off) == 24 &&
	      offsetof(btbbx_le_span, n_beyond) == 28 && offsetof(btbbx_le_span, n_gap) == 32 && offsetof(btbbx_le_span, n_control) == 36 &&
	      offsetof(btbbx_le_span, n_map_updates) == 40 && offsetof(btbbx_le_span, n_param_updates) == 44 &&
	      offsetof(btbbx_le_span, n_spans) == 48 && offsetof(btbbx_le_span, interval) == 52 && offsetof(btbbx_le_span, algorithm) == 54 &&
	      offsetof(btbbx_le_span, flags) == 55, "btbbx_le_span layout (libbtbb_amd.LE_SPAN_DTYPE)");
static_assert(sizeof(btbbx_le_span_pkt) == 16 && offsetof(btbbx_le_span_pkt, epoch) == 4 && offsetof(btbbx_le_span_pkt, span) == 6 &&
	      offsetof(btbbx_le_span_pkt, kind) == 8 && offsetof(btbbx_le_span_pkt, opcode) == 9 && offsetof(btbbx_le_span_pkt, expected) == 10 &&
	      offsetof(btbbx_le_span_pkt, on_hop) == 11 && offsetof(btbbx_le_span_pkt, state) == 12 && offsetof(btbbx_le_span_pkt, applied) == 13 &&
	      offsetof(btbbx_le_span_pkt, reserved) == 14, "btbbx_le_span_pkt layout (libbtbb_amd.LE_SPAN_PKT_DTYPE)");
static_assert(sizeof(btbbx_le_span_rec) == 40 && offsetof(btbbx_le_span_rec, base) == 8 && offsetof(btbbx_le_span_rec, first_event) == 12 &&
	      offsetof(btbbx_le_span_rec, n_events) == 16 && offsetof(btbbx_le_span_rec, pdu) == 20 && offsetof(btbbx_le_span_rec, interval) == 24 &&
	      offsetof(btbbx_le_span_rec, win_offset) == 26 && offsetof(btbbx_le_span_rec, latency) == 28 &&
	      offsetof(btbbx_le_span_rec, timeout) == 30 && offsetof(btbbx_le_span_rec, win_size) == 32 && offsetof(btbbx_le_span_rec, flags) == 33 &&
	      offsetof(btbbx_le_span_rec, reserved) == 34, "btbbx_le_span_rec layout (libbtbb_amd.LE_SPAN_REC_DTYPE)");

// the span a connection is in (scratch; set by le_span_begin_kernel, moved on by le_span_bound_kernel)
struct LsConn {
	unsigned long long origin;             // T_s
	unsigned long long base;               // B_s
	unsigned long long instant;            // I_s so far: the smallest I of a valid parameter update in span s
	unsigned long long c_last;             // the counter of L of span s - 1: the sum in front of f_s
	unsigned long long stop;
	uint32_t interval, allow, start, f;    // Int_s, a_s, start_s, f_s (LF_NONE: every event behind start_s is EARLY)
	uint32_t s, live, pick, n_ev;          // the span; still followed; 1 + the largest rank that can apply; the connection's events
	uint32_t flags, n_gap, n_param, pad0;  // STOPPED | CAPPED | REFUSED
	uint32_t pad1, pad2;
};
static_assert(sizeof(LsConn) == 96, "LsConn");

struct LsLayout {
	size_t kk, prm, sc, sstart, total;     // behind the follow stage's layout
};

static LsLayout le_span_layout(uint32_t cand_cap, uint32_t conn_cap, uint32_t max_updates)
{
	LsLayout S;
	const size_t c = cand_cap ? cand_cap : 1, k = conn_cap ? conn_cap : 1;
	size_t at = le_follow_layout(cand_cap, conn_cap).total;
	auto take = [&](size_t bytes) { const size_t here = at; at += ld_up(bytes); return here; };
	S.kk = take(c * 8);
	S.prm = take(c * 8);
	S.sc = take(k * sizeof(LsConn));
	S.sstart = take(k * ((size_t)max_updates + 1) * 4);
	S.total = at;
	return S;
}

// ---- a. the parameter updates' fields ---------------------------------------------------------------------------------------

// prm[i] = WinSize | WinOffset << 16, Interval | Latency << 16; the timeout goes to ctl[i].z, which an opcode-0 PDU leaves free
// (le_keyed.h has this kernel's keyed form, le_keyed_param_kernel: a change here is made there too)
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_span_param_kernel(const uint64_t *words, uint64_t n_words, uint64_t pitch_words,
									      uint32_t n_streams, const btbbx_le_cand *cands,
									      const btbbx_le_track_pkt *pkts, const btbbx_le_conn *conns,
									      const btbbx_le_seed *seeds, const uint32_t *params, uint4 *ctl,
									      uint2 *prm, LfConn *work)
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
	const LdCand c = ld_load(cands, i);
	const uint32_t stream = c.c.x & 0xffffu;               // (< n_streams: the slot kernel parsed it)
	if (stream >= n_streams)
		return;
	const uint64_t *w = words + (uint64_t)stream * pitch_words;
	const uint64_t bit0 = ((((uint64_t)c.a.y << 32) | c.a.x) & LT_OFF_MASK) + 56;
	uint32_t ws = (p.w & 0x3fu) | 0x40u;
	lf_whiten8(ws);
	lf_whiten8(ws);
	unsigned long long lo8 = 0;
	uint32_t hi4 = 0;
#pragma unroll 1
	for (uint32_t j = 0; j < 10; j++) {                     // octets 0..9
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
	const uint32_t win_size = (uint32_t)(lo8 >> 8) & 0xffu, win_offset = (uint32_t)(lo8 >> 16) & 0xffffu;
	const uint32_t interval = (uint32_t)(lo8 >> 32) & 0xffffu, latency = (uint32_t)(lo8 >> 48) & 0xffffu;
	prm[i] = make_uint2(win_size | (win_offset << 16), interval | (latency << 16));
	ctl[i].z = hi4 & 0xffffu;                               // Timeout
}

// ---- b. span 0 ----------------------------------------------------------------------------------------------------------------

// the number of g's events: the positions [first, first + n_ev) of the event table hold g (events are numbered without gaps)
__device__ __forceinline__ uint32_t ls_events(const btbbx_le_conn *conns, const uint32_t *econn, uint32_t g, uint32_t n, uint32_t &first)
{
	const uint2 f = reinterpret_cast<const uint2 *>(conns + g)[3];
	first = f.x;
	if (f.y || f.x >= n)
		return 0;
	const uint32_t np = conns[g].n_packets, room = n - f.x;
	uint32_t lo = 0, hi = np < room ? np : room;            // the first event position that is not g's
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (econn[f.x + mid] == g)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo;
}

// the first event of [from, n_ev) that is not EARLY: A_e + allow >= origin; LF_NONE without one
__device__ __forceinline__ uint32_t ls_first(const uint64_t *anchor, uint32_t first, uint32_t from, uint32_t n_ev, unsigned long long origin,
					     uint32_t allow)
{
	uint32_t lo = from, hi = n_ev;
	while (lo < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if ((anchor[first + mid] & LT_OFF_MASK) + allow < origin)
			lo = mid + 1;
		else
			hi = mid;
	}
	return lo < n_ev ? lo : LF_NONE;
}

__device__ __forceinline__ void ls_rec_zero(btbbx_le_span_rec *r)
{
	uint2 *o = reinterpret_cast<uint2 *>(r);
#pragma unroll
	for (int w = 0; w < 5; w++)
		o[w] = make_uint2(0, 0);
}

// the head of a span's record: everything but first_event and n_events, which the bound kernel of the span's round sets
__device__ __forceinline__ void ls_rec_open(btbbx_le_span_rec *r, unsigned long long origin, uint32_t base, uint32_t pdu, uint32_t interval,
					    uint32_t win_offset, uint32_t latency, uint32_t timeout, uint32_t win_size)
{
	uint2 *o = reinterpret_cast<uint2 *>(r);
	o[0] = make_uint2((uint32_t)origin, (uint32_t)(origin >> 32));
	o[1] = make_uint2(base, LF_NONE);
	o[2] = make_uint2(0, pdu);
	o[3] = make_uint2((interval & 0xffffu) | (win_offset << 16), (latency & 0xffffu) | (timeout << 16));
	o[4] = make_uint2((win_size & 0xffu) | (1u << 8), 0);
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_span_begin_kernel(const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
									      const uint32_t *params, const uint32_t *econn, const uint64_t *anchor,
									      uint32_t jitter_bits, uint32_t max_updates, LsConn *sc, uint32_t *sstart,
									      btbbx_le_span_rec *recs)
{
	const uint32_t g = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0];
	if (g >= params[1])
		return;
	const size_t at = (size_t)g * (max_updates + 1);
	for (uint32_t s = 0; s <= max_updates; s++) {
		ls_rec_zero(recs + at + s);
		sstart[at + s] = LF_NONE;
	}
	LsConn c;
	c.origin = c.base = c.c_last = 0;
	c.instant = c.stop = LF_NO_STOP;
	c.interval = c.allow = c.start = c.s = c.live = c.pick = c.n_ev = c.flags = c.n_gap = c.n_param = c.pad0 = c.pad1 = c.pad2 = 0;
	c.f = LF_NONE;
	if (lf_seeded(seeds, g)) {
		const btbbx_le_seed s = seeds[g];
		uint32_t first;
		c.n_ev = ls_events(conns, econn, g, n, first);
		c.origin = s.t0;
		c.interval = s.interval;
		c.allow = jitter_bits;
		c.live = 1;
		c.f = ls_first(anchor, first, 0, c.n_ev, c.origin, c.allow);
		sstart[at] = 0;
		ls_rec_open(recs + at, s.t0, 0, LF_NONE, s.interval, s.win_offset, s.latency, s.timeout, s.win_size);
	}
	sc[g] = c;
}

// ---- c. the rounds --------------------------------------------------------------------------------------------------------------

// rule 2 for the events of span s behind start_s of the connections still followed; every other event keeps its step
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_span_step_kernel(const uint64_t *anchor, const uint32_t *econn,
									     const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
									     const uint32_t *params, const LsConn *sc, uint32_t unit_bits,
									     unsigned long long *kk, unsigned long long *step,
									     unsigned long long *tiles64)
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
		unsigned long long v = 0;
		if (g != LF_NONE && lf_seeded(seeds, g)) {
			const uint32_t first = (uint32_t)conns[g].first, e = q - first;
			const uint32_t live = sc[g].live, start = sc[g].start, f = sc[g].f;
			if (live && e >= start) {
				const unsigned long long per = (unsigned long long)sc[g].interval * unit_bits;
				const unsigned long long a = anchor[q] & LT_OFF_MASK;
				if (per && e >= f) {                    // (f LF_NONE: no event is)
					if (e > f)
						v = (a - (anchor[q - 1] & LT_OFF_MASK) + per / 2) / per;
					else
						v = sc[g].base + (a + sc[g].allow - sc[g].origin) / per - sc[g].c_last;
				}
				kk[q] = v;
			} else {
				v = kk[q];
			}
		}
		step[q] = v;
		mine += v;
	}
	if (mine)
		atomicAdd(&total, mine);
	__syncthreads();
	if (tid == 0)
		tiles64[blockIdx.x] = total;
}

// candidate i holds a parameter update that span s of its connection reads: its connection, its event's counter, its instant
__device__ __forceinline__ bool ls_param_update(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts, const btbbx_le_conn *conns,
						const btbbx_le_seed *seeds, const uint4 *ctl, const LfConn *work, const LsConn *sc,
						const unsigned long long *step, uint32_t i, uint32_t n, uint32_t k, uint32_t &g, uint32_t &rank,
						unsigned long long &c, unsigned long long &at)
{
	const uint4 info = ctl[i];
	if ((info.x & 0xffffffu) != (LF_CONTROL | (0u << 8) | (12u << 16)))
		return false;
	uint32_t first;
	uint4 p;
	if (!lf_member(cands, pkts, conns, i, n, k, g, p, first) || !lf_seeded(seeds, g) || p.x > work[g].enc_rank)
		return false;
	if (!sc[g].live || p.y < sc[g].f)                       // (f >= start_s; LF_NONE: no event is counted)
		return false;
	rank = p.x;
	c = lf_counter(step, first, first + p.y);
	return lf_instant(info.y, c, at);
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_span_instant_kernel(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts,
										const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
										const uint32_t *params, const uint4 *ctl, const LfConn *work,
										const unsigned long long *step, LsConn *sc)
{
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0], k = params[1];
	if (i >= n)
		return;
	uint32_t g, rank;
	unsigned long long c, at;
	if (ls_param_update(cands, pkts, conns, seeds, ctl, work, sc, step, i, n, k, g, rank, c, at))
		atomicMin(&sc[g].instant, at);
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_span_pick_kernel(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts,
									     const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
									     const uint32_t *params, const uint4 *ctl, const LfConn *work,
									     const unsigned long long *step, LsConn *sc)
{
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0], k = params[1];
	if (i >= n)
		return;
	uint32_t g, rank;
	unsigned long long c, at;
	if (ls_param_update(cands, pkts, conns, seeds, ctl, work, sc, step, i, n, k, g, rank, c, at) && at == sc[g].instant && c < at)
		atomicMax(&sc[g].pick, rank + 1);
}

// rules 4-6 for span s of connection g
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_span_bound_kernel(const btbbx_le_conn *conns, const uint32_t *params,
									      const uint32_t *slot, const uint64_t *anchor,
									      const unsigned long long *step, uint4 *ctl, const uint2 *prm,
									      uint32_t unit_bits, uint32_t jitter_bits, uint32_t max_updates, LsConn *sc,
									      uint32_t *sstart, btbbx_le_span_rec *recs)
{
	const uint32_t g = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0];
	if (g >= params[1] || !sc[g].live)
		return;
	LsConn *mine = sc + g;
	const uint32_t first = (uint32_t)conns[g].first, s = mine->s, f = mine->f, n_ev = mine->n_ev, pick = mine->pick;
	const unsigned long long instant = mine->instant;
	uint32_t *rec = reinterpret_cast<uint32_t *>(recs + (size_t)g * (max_updates + 1) + s);
	uint32_t counted = 0;                                   // the span's events in front of I_s
	if (f != LF_NONE) {
		uint32_t lo = f, hi = n_ev;                         // the first event with c_e >= I_s
		while (lo < hi) {
			const uint32_t mid = lo + (hi - lo) / 2;
			if (lf_counter(step, first, first + mid) < instant)
				lo = mid + 1;
			else
				hi = mid;
		}
		counted = lo - f;
	}
	rec[3] = f;
	rec[4] = counted;
	bool apply = false;
	uint32_t i = LF_NONE;
	uint2 pr = make_uint2(0, 0);
	if (instant != LF_NO_STOP && pick && counted && s < max_updates && first + (pick - 1) < n) {
		i = slot[first + (pick - 1)];
		if (i != LF_NONE) {
			pr = prm[i];
			const uint32_t win_size = pr.x & 0xffu, win_offset = pr.x >> 16, interval = pr.y & 0xffffu;
			apply = interval >= 6 && interval <= 3200 && win_size >= 1 && win_size <= (interval - 1 < 8 ? interval - 1 : 8u) &&
				win_offset <= interval;
		}
	}
	if (!apply) {
		mine->live = 0;
		if (instant != LF_NO_STOP) {
			mine->stop = instant;
			mine->flags = BTBBX_LE_FOLLOW_STOPPED | (s == max_updates ? BTBBX_LE_SPAN_CAPPED : BTBBX_LE_SPAN_REFUSED);
		}
		return;
	}
	const uint32_t last = f + counted - 1;                      // L
	const unsigned long long c_l = lf_counter(step, first, first + last);
	const unsigned long long per = (unsigned long long)mine->interval * unit_bits;
	const uint32_t win_offset = pr.x >> 16, timeout = ctl[i].z & 0xffffu, interval = pr.y & 0xffffu;
	const unsigned long long origin = (anchor[first + last] & LT_OFF_MASK) + (instant - c_l) * per + (unsigned long long)win_offset * unit_bits;
	mine->origin = origin;
	mine->base = instant;
	mine->c_last = c_l;
	mine->interval = interval;
	mine->allow = 2 * jitter_bits;
	mine->start = last + 1;
	mine->f = ls_first(anchor, first, last + 1, n_ev, origin, 2 * jitter_bits);
	mine->s = s + 1;
	mine->instant = LF_NO_STOP;
	mine->pick = 0;
	sstart[(size_t)g * (max_updates + 1) + s + 1] = last + 1;
	ls_rec_open(recs + (size_t)g * (max_updates + 1) + s + 1, origin, (uint32_t)instant, i, interval, win_offset, pr.y >> 16, timeout, pr.x & 0xffu);
	ctl[i].x |= LS_APPLIED;
}

// ---- d. the final counters: states, the update list ----------------------------------------------------------------------------

// the span of event e of g -- the last one that starts at or in front of it -- and whether e is EARLY in it
__device__ __forceinline__ uint32_t ls_span_of(const LsConn *sc, const uint32_t *sstart, const btbbx_le_span_rec *recs, uint32_t g, uint32_t e,
					       uint32_t max_updates, bool &early)
{
	const size_t at = (size_t)g * (max_updates + 1);
	const uint32_t last = sc[g].s;
	uint32_t s = 0;
	for (uint32_t t = 1; t <= max_updates; t++)
		if (t <= last && sstart[at + t] <= e)
			s = t;
	early = e < recs[at + s].first_event;                    // (LF_NONE: every event is)
	return s;
}

// slot q holds a valid map update that is not ignored, or (param) a valid parameter update in a counted event
__device__ __forceinline__ bool ls_update(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts, const btbbx_le_conn *conns,
					  const btbbx_le_seed *seeds, const uint32_t *slot, const uint4 *ctl, const LfConn *work, const LsConn *sc,
					  const uint32_t *sstart, const btbbx_le_span_rec *recs, const unsigned long long *step,
					  uint32_t max_updates, uint32_t q, uint32_t n, uint32_t k, uint32_t &i, uint32_t &g,
					  unsigned long long &at, bool &param)
{
	param = false;
	i = slot[q];
	if (i == LF_NONE)
		return false;
	const uint4 info = ctl[i];
	const uint32_t head = info.x & 0xffffffu;
	const bool is_map = head == (LF_CONTROL | (1u << 8) | (8u << 16)), is_param = head == (LF_CONTROL | (12u << 16));
	if (!is_map && !is_param)
		return false;
	uint32_t first;
	uint4 p;
	if (!lf_member(cands, pkts, conns, i, n, k, g, p, first) || !lf_seeded(seeds, g) || p.x > work[g].enc_rank)
		return false;
	bool early;
	ls_span_of(sc, sstart, recs, g, p.y, max_updates, early);
	if (early)
		return false;
	const unsigned long long c = lf_counter(step, first, first + p.y);
	const bool valid = lf_instant(info.y, c, at);
	if (is_param) {
		param = valid;
		return false;
	}
	return valid && c < sc[g].stop && __popc(info.z) + __popc(info.w) >= 2;
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_span_mark_kernel(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts,
									     const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
									     const uint32_t *params, const uint32_t *slot, const uint4 *ctl,
									     const LfConn *work, const LsConn *sc, const uint32_t *sstart,
									     const btbbx_le_span_rec *recs, const unsigned long long *step,
									     uint32_t max_updates, unsigned long long *utiles)
{
	const uint32_t n = params[0], k = params[1];
	lf_mark_tile(n, utiles, [=](uint32_t q, uint32_t &i, uint32_t &g, unsigned long long &at, bool &param) __attribute__((always_inline)) {
		return ls_update(cands, pkts, conns, seeds, slot, ctl, work, sc, sstart, recs, step, max_updates, q, n, k, i, g, at, param);
	});
}

// as le_epoch_list_kernel; the last tile's carry is the list's length
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_span_list_kernel(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts,
									     const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
									     const uint32_t *params, const uint32_t *slot, uint4 *ctl, LfConn *work,
									     LsConn *sc, const uint32_t *sstart, const btbbx_le_span_rec *recs,
									     const unsigned long long *step, uint32_t max_updates,
									     const unsigned long long *utiles, uint32_t *uparams, uint64_t *keys,
									     uint32_t *vals, uint64_t *u_i, uint64_t *u_map, uint32_t *u_conn)
{
	const uint32_t n = params[0], k = params[1];
	lf_list_tile<false>(n, utiles, uparams, ctl, work, keys, vals, u_i, u_map, u_conn,
			    [=](uint32_t q, uint32_t &i, uint32_t &g, unsigned long long &at, bool &param) __attribute__((always_inline)) {
				    return ls_update(cands, pkts, conns, seeds, slot, ctl, work, sc, sstart, recs, step, max_updates, q, n, k, i, g, at, param);
			    },
			    [=](uint32_t i, uint32_t g) __attribute__((always_inline)) {
				    ctl[i].x |= LF_IS_PARAM;
				    atomicAdd(&sc[g].n_param, 1u);
			    });
}

// ---- e. prediction, verdict, packets ----------------------------------------------------------------------------------------------

// rule 7 for the event at table position q; evres[q] = expected #1 | expected #2 << 8 | state << 16, epoch, counter, span
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_span_predict_kernel(const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
										const uint32_t *params, const uint32_t *uparams, const uint64_t *anchor,
										const uint32_t *econn, const unsigned long long *step,
										const uint64_t *s_conn, const uint64_t *s_i, const uint64_t *s_map,
										const uint32_t *sstart, const btbbx_le_span_rec *recs,
										uint32_t max_updates, uint4 *evres, LfConn *work, LsConn *sc)
{
	const uint32_t q = blockIdx.x * LE_THREADS + threadIdx.x, lane = threadIdx.x & 63, n = params[0];
	uint32_t g = LF_NONE;
	if (q < n)
		g = econn[q];
	const bool live = g != LF_NONE && lf_seeded(seeds, g);
	bool before = false, gap = false, beyond = false, pred = false, on1 = false, on2 = false;
	uint32_t e = 0;
	if (live) {
		LfEvent ev = {0, 0xff, 0xff};
		const uint32_t first = (uint32_t)conns[g].first;
		const uint64_t a = anchor[q];
		e = q - first;
		bool early;
		const uint32_t span = ls_span_of(sc, sstart, recs, g, e, max_updates, early);
		uint32_t counter = 0, state = span ? BTBBX_LE_STATE_GAP : BTBBX_LE_STATE_BEFORE;
		before = early && !span;
		gap = early && span;
		if (!early) {
			const unsigned long long c = lf_counter(step, first, q);
			pred = lf_predict(seeds + g, conns + g, g, c, &sc[g].stop, (uint32_t)(a >> 56), s_conn, s_i, s_map, uparams[0], ev, on1, on2);
			counter = (uint32_t)c;
			beyond = !pred;
			state = beyond ? BTBBX_LE_STATE_BEYOND : BTBBX_LE_STATE_COUNTED;
		}
		evres[q] = make_uint4(ev.exp1 | (ev.exp2 << 8) | (state << 16), ev.epoch, counter, span);
	}
	lf_tallies(g, live, lane, e, before, gap, beyond, pred, on1, on2, work, &sc[live ? g : 0].n_gap);
}

extern "C" __global__ __launch_bounds__(LE_THREADS) void le_span_verdict_kernel(const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
										const uint32_t *params, const uint32_t *uparams,
										const unsigned long long *step, const uint64_t *s_conn,
										const uint64_t *s_map, const uint4 *evres, const LfConn *work,
										const LsConn *sc, btbbx_le_span *spans)
{
	const uint32_t g = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0];
	if (g >= params[1])
		return;
	uint2 *out = reinterpret_cast<uint2 *>(spans + g);
	if (!lf_seeded(seeds, g)) {
#pragma unroll
		for (int w = 0; w < 7; w++)
			out[w] = make_uint2(0, 0);
		return;
	}
	const LfConn w = work[g];
	const LfVerdict v = lf_verdict(w, seeds[g], reinterpret_cast<const uint2 *>(conns + g)[3], g, n, uparams, step, s_conn, s_map, evres);
	uint32_t flags = v.flags | sc[g].flags;
	if (w.enc_rank != LF_NONE)
		flags |= BTBBX_LE_FOLLOW_ENCRYPTED;
	out[0] = make_uint2((uint32_t)v.map, (uint32_t)(v.map >> 32));
	out[1] = make_uint2(v.c_first, (uint32_t)sc[g].stop);
	out[2] = make_uint2(w.n_before, v.n_on);
	out[3] = make_uint2(w.n_pred - v.n_on, w.n_beyond);
	out[4] = make_uint2(sc[g].n_gap, w.n_control);
	out[5] = make_uint2(w.n_map, sc[g].n_param);
	out[6] = make_uint2(sc[g].s + 1, (sc[g].interval & 0xffffu) | (v.algorithm << 16) | (flags << 24));
}

// (le_keyed.h has this kernel's keyed form, le_keyed_pkt_span_kernel: a change here is made there too)
extern "C" __global__ __launch_bounds__(LE_THREADS) void le_span_pkt_kernel(const btbbx_le_cand *cands, const btbbx_le_track_pkt *pkts,
									    const btbbx_le_conn *conns, const btbbx_le_seed *seeds,
									    const uint32_t *params, const uint4 *ctl, const uint4 *evres,
									    const LfConn *work, const btbbx_le_span *spans, btbbx_le_span_pkt *out)
{
	const uint32_t i = blockIdx.x * LE_THREADS + threadIdx.x, n = params[0], k = params[1];
	if (i >= n)
		return;
	uint32_t g, first;
	uint4 p, o = make_uint4(0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
	if (lf_member(cands, pkts, conns, i, n, k, g, p, first)) {
		const uint32_t x = ctl[i].x;
		uint32_t op, applied = 0;
		const uint32_t kind = lf_pdu_kind(x, p.x, work[g].enc_rank, op);
		LfPktEvent e = {0, 0, 0, 0, 0xff, 0};
		if (lf_seeded(seeds, g)) {
			lf_pkt_event(evres[first + p.y], &spans[g].algorithm, p.w & 0xffu, e);
			applied = (x & LS_APPLIED) ? 1u : 0u;
		}
		o = make_uint4(e.counter, e.epoch | (e.span << 16), kind | (op << 8) | (e.expected << 16) | (e.on << 24), e.state | (applied << 8));
	}
	reinterpret_cast<uint4 *>(out)[i] = o;
}

// ---- host side ------------------------------------------------------------------------------------------------------------

extern "C" size_t btbbx_le_span_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap, uint32_t max_updates)
{
	return le_span_layout(cand_cap, conn_cap, max_updates > LS_MAX_UPDATES ? LS_MAX_UPDATES : max_updates).total;
}

// the clear reading of a run's control PDUs (le_follow.h), with the kernel that reads a parameter update's fields and this stage's
// packet kernel
struct LsReadClear : LfReadClear {
	void param(const LfBufs &B, const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, const btbbx_le_cand *d_cands,
		   const btbbx_le_track_pkt *d_pkts, const btbbx_le_conn *d_conns, const btbbx_le_seed *d_seeds, uint2 *prm, dim3 per_cand,
		   hipStream_t q) const
	{
		hipLaunchKernelGGL(le_span_param_kernel, per_cand, dim3(LE_THREADS), 0, q, d_words, n_words, pitch_words, n_streams, d_cands, d_pkts,
				   d_conns, d_seeds, B.params, B.ctl, prm, B.work);
	}
	void span_pkts(const LfBufs &B, const btbbx_le_cand *d_cands, const btbbx_le_track_pkt *d_pkts, const btbbx_le_conn *d_conns,
		       const btbbx_le_seed *d_seeds, btbbx_le_span *d_spans, btbbx_le_span_pkt *d_spkts, dim3 per_cand, hipStream_t q) const
	{
		hipLaunchKernelGGL(le_span_pkt_kernel, per_cand, dim3(LE_THREADS), 0, q, d_cands, d_pkts, d_conns, d_seeds, B.params, B.ctl, B.evres,
				   B.work, d_spans, d_spkts);
	}
};

// the launches of one run: 13 kernels -- 5 of them the follow stage's, 1 the tracking's --, 6 per round, 3 per radix pass (6 over I, 1 to 4
// over conn_cap); `read` chooses four of them: the slot, open, parameter and packet kernels, or le_keyed.h's in their places
template <class Read = LsReadClear>
static int le_span_launch(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, const btbbx_le_cand *d_cands,
			  const uint32_t *d_count, uint32_t cap, const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
			  const btbbx_le_track_pkt *d_pkts, const btbbx_le_seed *d_seeds, uint32_t unit_bits, uint32_t jitter_bits,
			  uint32_t max_updates, btbbx_le_span *d_spans, btbbx_le_span_pkt *d_spkts, btbbx_le_span_rec *d_recs, void *d_scratch,
			  hipStream_t q, const Read &read = Read())
{
	const LfBufs B = le_follow_bufs(d_scratch, cap, conn_cap);
	const LsLayout S = le_span_layout(cap, conn_cap, max_updates);
	char *s = (char *)d_scratch;
	uint32_t *sstart = (uint32_t *)(s + S.sstart);
	unsigned long long *kk = (unsigned long long *)(s + S.kk);
	uint2 *prm = (uint2 *)(s + S.prm);
	LsConn *sc = (LsConn *)(s + S.sc);
	const dim3 per_cand((cap + LE_THREADS - 1) / LE_THREADS), per_tile(B.tiles_n), per_conn((conn_cap + LE_THREADS - 1) / LE_THREADS), wg(LE_THREADS);
	le_follow_open(B, d_words, n_words, pitch_words, n_streams, d_cands, d_count, cap, d_conns, d_conn_count, conn_cap, d_pkts, q, read);
	read.param(B, d_words, n_words, pitch_words, n_streams, d_cands, d_pkts, d_conns, d_seeds, prm, per_cand, q);
	hipLaunchKernelGGL(le_span_begin_kernel, per_conn, wg, 0, q, d_conns, d_seeds, B.params, B.econn, B.anchor, jitter_bits, max_updates, sc,
			   sstart, d_recs);
	for (uint32_t round = 0; round <= max_updates; round++) {
		hipLaunchKernelGGL(le_span_step_kernel, per_tile, wg, 0, q, B.anchor, B.econn, d_conns, d_seeds, B.params, sc, unit_bits, kk, B.step,
				   B.tiles64);
		hipLaunchKernelGGL(le_track_prefix64_kernel, dim3(1), wg, 0, q, B.tiles64, B.tiles_n);
		hipLaunchKernelGGL(le_track_count_kernel, per_tile, wg, 0, q, B.params, B.tiles64, B.step);
		hipLaunchKernelGGL(le_span_instant_kernel, per_cand, wg, 0, q, d_cands, d_pkts, d_conns, d_seeds, B.params, B.ctl, B.work, B.step, sc);
		hipLaunchKernelGGL(le_span_pick_kernel, per_cand, wg, 0, q, d_cands, d_pkts, d_conns, d_seeds, B.params, B.ctl, B.work, B.step, sc);
		hipLaunchKernelGGL(le_span_bound_kernel, per_conn, wg, 0, q, d_conns, B.params, B.slot, B.anchor, B.step, B.ctl, prm, unit_bits,
				   jitter_bits, max_updates, sc, sstart, d_recs);
	}
	// (the tile counts of the update list go through the 64-bit prefix sum, in the step's tile sums, which are free now)
	hipLaunchKernelGGL(le_span_mark_kernel, per_tile, wg, 0, q, d_cands, d_pkts, d_conns, d_seeds, B.params, B.slot, B.ctl, B.work, sc, sstart,
			   d_recs, B.step, max_updates, B.tiles64);
	hipLaunchKernelGGL(le_track_prefix64_kernel, dim3(1), wg, 0, q, B.tiles64, B.tiles_n);
	hipLaunchKernelGGL(le_span_list_kernel, per_tile, wg, 0, q, d_cands, d_pkts, d_conns, d_seeds, B.params, B.slot, B.ctl, B.work, sc, sstart,
			   d_recs, B.step, max_updates, B.tiles64, B.uparams, B.b.keys[0], B.b.vals[0], B.u_i, B.u_map, B.u_conn);
	const uint64_t *s_conn = le_follow_sort_updates(B, cap, conn_cap, q);
	hipLaunchKernelGGL(le_span_predict_kernel, per_cand, wg, 0, q, d_conns, d_seeds, B.params, B.uparams, B.anchor, B.econn, B.step, s_conn, B.s_i,
			   B.s_map, sstart, d_recs, max_updates, B.evres, B.work, sc);
	hipLaunchKernelGGL(le_span_verdict_kernel, per_conn, wg, 0, q, d_conns, d_seeds, B.params, B.uparams, B.step, s_conn, B.s_map, B.evres, B.work,
			   sc, d_spans);
	read.span_pkts(B, d_cands, d_pkts, d_conns, d_seeds, d_spans, d_spkts, per_cand, q);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

extern "C" int btbbx_le_span_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				    const uint16_t *d_phys_channel,
				    const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
				    const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
				    const btbbx_le_track *d_tracks, const btbbx_le_track_pkt *d_pkts, const btbbx_le_seed *d_seeds,
				    uint32_t unit_bits, uint32_t jitter_bits, uint32_t max_updates,
				    btbbx_le_span *d_spans, btbbx_le_span_pkt *d_span_pkts, btbbx_le_span_rec *d_span_recs,
				    void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
	const char *who = "btbbx_le_span_device";
	if (max_updates > LS_MAX_UPDATES) {
		set_error("%s: max_updates must be 0..%u", who, LS_MAX_UPDATES);
		return BTBBX_E_ARG;
	}
	int rc = le_track_check_args(who, n_streams, unit_bits, jitter_bits);
	if (!rc)
		rc = le_check_streams(who, n_words, pitch_words, n_streams);
	if (rc)
		return rc;
	const LsLayout S = le_span_layout(cand_cap, conn_cap, max_updates);
	if (!d_words || !d_phys_channel || !d_cands || !d_cand_count || !d_conns || !d_conn_count || !d_tracks || !d_pkts || !d_seeds ||
	    !d_spans || !d_span_pkts || !d_span_recs || !d_scratch || scratch_bytes < S.total) {
		set_error("%s: null pointer, or scratch of %zu bytes needed and %zu given", who, S.total, scratch_bytes);
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
	return le_span_launch(d_words, n_words, pitch_words, n_streams, d_cands, d_cand_count, cand_cap, d_conns, d_conn_count, conn_cap, d_pkts,
			      d_seeds, unit_bits, jitter_bits, max_updates, d_spans, d_span_pkts, d_span_recs, d_scratch, (hipStream_t)hip_stream);
}
