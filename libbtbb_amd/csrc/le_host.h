// le_host.h -- the host wrappers of the LE stages (included by le.hip, behind le_resolve.h).  Every wrapper runs one chain: the
// capture goes to the device, the discovery scans and groups it, the tracking works on what the discovery stored, the wrapper's own
// stages follow on the same stream and the records are copied out.  The chain is written here once:
//
//   le_disc_host_chain    copy in, scan (twice when the first guess was too small), group; the caller's tail behind the block
//   le_host_check         the argument checks every wrapper behind the discovery makes
//   le_host_begin         the discovery chain with the tracking's part of the tail and the wrapper's own behind it
//   le_host_track         the tracking's launches
//   le_host_finish        the copy-out, or the fill of the per-candidate arrays when no connection was stored
//
// A wrapper calls these in this order, launches its own stages between le_host_track and le_host_finish, and names its own
// outputs (LeHostOut).  Nothing of one call outlives it: what a tail's size depends on is captured by the callable that computes it.
#pragma once
#include "le_resolve.h"

// What the discovery leaves on the device, inside the caller's CallScope: the counters, the sorted candidates, the connection
// records and, behind them, `tail` (tail_bytes(dev_cap, dev_conns) bytes for what a caller runs next on the same stream).
struct LeDiscHostRun {
	uint32_t dev_cap, dev_conns;                   // what the device buffers hold
	uint32_t count, have, n_conns;                 // candidates found, candidates kept (min(count, dev_cap)), connections found
	uint32_t *d_count, *d_conn_count;
	btbbx_le_cand *d_cands;
	btbbx_le_conn *d_conns;
	const uint16_t *d_phys;
	const uint64_t *d_words;                       // the capture as it was copied in
	char *tail;
};

// copy in, scan (again with room for every candidate when the first guess was too small, as btbbx_scan_host does), group; both
// counts read back.  have == 0: nothing was grouped and nothing but count is set
template <class Tail>
static int le_disc_host_chain(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, uint64_t search_bits,
			      const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count, uint64_t conn_cap, Tail tail_bytes,
			      LeDiscHostRun *r)
{
	int rc;
	if (n_streams == 1)
		pitch_words = n_words;
	hipStream_t q = scope_stream();
	const uint64_t cap_words = (uint64_t)(n_streams - 1) * pitch_words + n_words;
	const size_t words_bytes = ((size_t)(cap_words + 1) * 8 + 255) & ~(size_t)255;
	char *dblock = (char *)scope_device(words_bytes + 2 * (size_t)n_streams);
	if (!dblock)
		return BTBBX_E_NOMEM;
	const uint64_t *d_words = (const uint64_t *)dblock;
	uint16_t *d_phys = (uint16_t *)(dblock + words_bytes);
	HIP_TRY(hipMemcpyAsync(dblock, words, (size_t)cap_words * 8, hipMemcpyHostToDevice, q));
	HIP_TRY(hipMemcpyAsync(d_phys, phys_channel, 2 * (size_t)n_streams, hipMemcpyHostToDevice, q));
	// first guess: one candidate per 4096 offsets + slack (noise yields one per 37 000 at max_len 27, one per 4000 at 255)
	uint64_t guess = search_bits / 4096 * n_streams + 4096;
	uint32_t dev_cap = guess > 0xfffffff0ull ? 0xfffffff0u : (uint32_t)guess;
	uint32_t count = 0;
	char *block = nullptr;
	size_t cand_bytes = 0, scratch_bytes = 0, conn_bytes = 0;
	uint32_t dev_conns = 0;
	for (int pass = 0; pass < 2; pass++) {
		cand_bytes = ld_up((size_t)dev_cap * sizeof(btbbx_le_cand));
		scratch_bytes = ld_up(btbbx_le_discover_scratch_bytes(dev_cap));
		dev_conns = (uint32_t)std::min<uint64_t>(conn_cap, dev_cap);
		conn_bytes = ld_up((size_t)dev_conns * sizeof(btbbx_le_conn));
		block = (char *)scope_hits(256 + cand_bytes + scratch_bytes + conn_bytes + tail_bytes(dev_cap, dev_conns));
		if (!block)
			return BTBBX_E_NOMEM;
		HIP_TRY(hipMemsetAsync(block, 0, 2 * sizeof(uint32_t), q));
		rc = le_disc_launch_scan(d_words, n_words, pitch_words, n_streams, search_bits, d_phys, max_len, (btbbx_le_cand *)(block + 256),
					 dev_cap, (uint32_t *)block, q);
		if (rc)
			return rc;
		HIP_TRY(hipMemcpyAsync(&count, block, sizeof(count), hipMemcpyDeviceToHost, q));
		HIP_TRY(hipStreamSynchronize(q));
		if (count <= dev_cap)
			break;
		dev_cap = count;
	}
	r->dev_cap = dev_cap;
	r->dev_conns = dev_conns;
	r->count = count;
	r->have = std::min(count, dev_cap);
	r->n_conns = 0;
	r->d_count = (uint32_t *)block;
	r->d_conn_count = (uint32_t *)block + 1;
	r->d_cands = (btbbx_le_cand *)(block + 256);
	r->d_conns = (btbbx_le_conn *)(block + 256 + cand_bytes + scratch_bytes);
	r->d_phys = d_phys;
	r->d_words = d_words;
	r->tail = block + 256 + cand_bytes + scratch_bytes + conn_bytes;
	if (!r->have)
		return BTBBX_OK;
	rc = le_disc_launch_group(r->d_cands, r->d_count, dev_cap, min_count, r->d_conns, dev_conns, r->d_conn_count, block + 256 + cand_bytes, q);
	if (rc)
		return rc;
	HIP_TRY(hipMemcpyAsync(&r->n_conns, r->d_conn_count, sizeof(uint32_t), hipMemcpyDeviceToHost, q));
	HIP_TRY(hipStreamSynchronize(q));
	return BTBBX_OK;
}

// ---- the frame of the wrappers --------------------------------------------------------------------------------------------------

// what every wrapper behind the discovery takes
struct LeHostArgs {
	const char *who;
	const uint64_t *words;
	uint64_t n_words, pitch_words;
	uint32_t n_streams;
	uint64_t search_bits;
	const uint16_t *phys_channel;
	uint32_t max_len, min_count;
	btbbx_le_conn *conns;
	uint64_t conn_cap;
	btbbx_le_cand *cands;
	uint64_t cand_cap;
	uint64_t *n_cands_out;
	uint32_t unit_bits, ifs_bits, jitter_bits, flags;
	btbbx_le_track *tracks;
	btbbx_le_track_pkt *pkts;
};
// a wrapper's LeHostArgs: its parameters carry the fields' names, so the order is written here alone
#define LE_HOST_ARGS(who)                                                                                                          \
	{who, words, n_words, pitch_words, n_streams, search_bits, phys_channel, max_len, min_count, conns, conn_cap, cands, cand_cap,  \
	 n_cands_out, unit_bits, ifs_bits, jitter_bits, flags, tracks, pkts}

// the tracking's part of the tail, as offsets from LeDiscHostRun::tail
struct LtHostTail {
	size_t scratch, tracks, pkts, total;
};

static LtHostTail le_track_host_layout(uint32_t dev_cap, uint32_t dev_conns)
{
	LtHostTail T;
	T.scratch = 0;
	T.tracks = ld_up(le_track_layout(dev_cap, dev_conns).total);
	T.pkts = T.tracks + ld_up((size_t)dev_conns * sizeof(btbbx_le_track));
	T.total = T.pkts + ld_up((size_t)dev_cap * sizeof(btbbx_le_track_pkt));
	return T;
}

static size_t le_track_host_tail(uint32_t dev_cap, uint32_t dev_conns) { return le_track_host_layout(dev_cap, dev_conns).total; }

struct LeHostRun : LeDiscHostRun {
	hipStream_t q;
	uint64_t nc, nk;                               // the connections and the candidates that are copied out
	btbbx_le_track *d_tracks;
	btbbx_le_track_pkt *d_pkts;
	char *own;                                     // the wrapper's own part of the tail, behind the tracking's
	// le_follow_host_chain's advertising block, for its last stage: the decoded records, their count, what the block holds
	const btbbx_le_pkt *d_adv = nullptr;
	const uint32_t *d_adv_count = nullptr;
	uint32_t adv_cap = 0;
};

// an output of a wrapper beyond conns / tracks / pkts / cands: one record of `size` bytes per connection, or per candidate; a
// per-candidate array is filled with 0xff when no connection was stored (no candidate is a member then).  fixed >= 0: a table of
// that many records whatever was found (the pairing stage's key table and its count), zeros when no connection was stored
struct LeHostOut {
	void *dst;
	const void *src;
	size_t size;
	bool per_cand;
	int64_t fixed = -1;
	size_t count(size_t per_conn, size_t per_candidate) const { return fixed >= 0 ? (size_t)fixed : (per_cand ? per_candidate : per_conn); }
};

// adv_errors: NULL when the wrapper scans no advertising channel; missing: one of the wrapper's own outputs is NULL and must not be
static int le_host_check(const LeHostArgs &a, const int *adv_errors, bool missing)
{
	int rc = le_disc_check_args(a.who, a.n_words, a.pitch_words, a.n_streams, a.search_bits, a.max_len);
	if (!rc && adv_errors)
		rc = le_check_args(a.who, a.n_words, a.pitch_words, a.n_streams, a.search_bits, *adv_errors);
	if (!rc)
		rc = le_track_check_args(a.who, a.n_streams, a.unit_bits, a.jitter_bits);
	if (rc)
		return rc;
	if (!a.words || !a.phys_channel || ((!a.conns || !a.tracks) && a.conn_cap) || (!a.cands && a.cand_cap) || missing) {
		set_error("%s: null pointer", a.who);
		return BTBBX_E_ARG;
	}
	return ctx_require();
}

// inside the wrapper's CallScope.  own_tail(dev_cap, dev_conns): the bytes the wrapper needs behind the tracking's.  r->have == 0:
// the capture held no candidate and the wrapper returns 0
template <class Tail> static int le_host_begin(const LeHostArgs &a, Tail own_tail, LeHostRun *r)
{
	if (a.n_cands_out)
		*a.n_cands_out = 0;
	r->q = scope_stream();
	const int rc = le_disc_host_chain(a.words, a.n_words, a.pitch_words, a.n_streams, a.search_bits, a.phys_channel, a.max_len, a.min_count,
					  a.conn_cap, [&](uint32_t cap, uint32_t conns) { return le_track_host_tail(cap, conns) + own_tail(cap, conns); },
					  r);
	if (rc)
		return rc;
	if (a.n_cands_out)
		*a.n_cands_out = r->count;
	if (!r->have)
		return BTBBX_OK;
	const LtHostTail T = le_track_host_layout(r->dev_cap, r->dev_conns);
	r->nc = std::min<uint64_t>(r->n_conns, r->dev_conns);
	r->nk = std::min<uint64_t>(r->have, a.cand_cap);
	r->d_tracks = (btbbx_le_track *)(r->tail + T.tracks);
	r->d_pkts = (btbbx_le_track_pkt *)(r->tail + T.pkts);
	r->own = r->tail + T.total;
	return BTBBX_OK;
}

static int le_host_track(const LeHostArgs &a, const LeHostRun &r)
{
	return le_track_launch(r.d_cands, r.d_count, r.dev_cap, r.d_conn_count, r.dev_conns, r.d_phys, a.n_streams, a.unit_bits, a.ifs_bits,
			       a.jitter_bits, a.flags, r.d_tracks, r.d_pkts, r.tail, r.q);
}

// rc: what the wrapper's launches gave.  With a connection stored: the records are copied out unless rc is set, the stream is
// synchronised whatever happened, and rc is reported in front of a failed copy.  Returns the wrapper's result
static int64_t le_host_finish(const LeHostArgs &a, const LeHostRun &r, int rc, const LeHostOut *outs, int n_outs)
{
	hipError_t e = hipSuccess;
	auto out = [&](void *dst, const void *src, size_t bytes) {
		if (!rc && e == hipSuccess && dst && bytes)
			e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, r.q);
	};
	if (r.nc) {
		out(a.conns, r.d_conns, (size_t)r.nc * sizeof(btbbx_le_conn));
		out(a.tracks, r.d_tracks, (size_t)r.nc * sizeof(btbbx_le_track));
		out(a.pkts, r.d_pkts, (size_t)r.nk * sizeof(btbbx_le_track_pkt));
		for (int o = 0; o < n_outs; o++)
			out(outs[o].dst, outs[o].src, outs[o].count(r.nc, r.nk) * outs[o].size);
	} else {
		if (a.pkts)
			memset(a.pkts, 0xff, (size_t)r.nk * sizeof(btbbx_le_track_pkt));
		for (int o = 0; o < n_outs; o++)
			if (outs[o].fixed >= 0 && outs[o].dst)
				memset(outs[o].dst, 0, (size_t)outs[o].fixed * outs[o].size);
			else if (outs[o].per_cand && outs[o].dst)
				memset(outs[o].dst, 0xff, (size_t)r.nk * outs[o].size);
	}
	out(a.cands, r.d_cands, (size_t)r.nk * sizeof(btbbx_le_cand));
	const hipError_t e2 = hipStreamSynchronize(r.q);
	if (rc)
		return rc;
	if (e != hipSuccess || e2 != hipSuccess) {
		char what[64];
		snprintf(what, sizeof what, "%s: copy out", a.who);
		return hip_fail(e != hipSuccess ? e : e2, what);
	}
	return (int64_t)r.n_conns;
}

// ---- discovery, tracking, channel selection #2 ----------------------------------------------------------------------------------

extern "C" int64_t btbbx_le_discover_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
					  uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
					  btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
					  uint64_t *n_cands_out)
{
	const char *who = "btbbx_le_discover_host";
	int rc = le_disc_check_args(who, n_words, pitch_words, n_streams, search_bits, max_len);
	if (rc)
		return rc;
	if (!words || !phys_channel || (!conns && conn_cap) || (!cands && cand_cap)) {
		set_error("%s: null pointer", who);
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	if (n_cands_out)
		*n_cands_out = 0;
	CallScope scope;
	hipStream_t q = scope_stream();
	LeDiscHostRun r;
	rc = le_disc_host_chain(words, n_words, pitch_words, n_streams, search_bits, phys_channel, max_len, min_count, conn_cap,
				[](uint32_t, uint32_t) { return (size_t)0; }, &r);
	if (rc)
		return rc;
	if (n_cands_out)
		*n_cands_out = r.count;
	if (!r.have)
		return 0;
	const uint64_t nc = std::min<uint64_t>(r.n_conns, r.dev_conns), nk = std::min<uint64_t>(r.have, cand_cap);
	if (nc)
		HIP_TRY(hipMemcpyAsync(conns, r.d_conns, (size_t)nc * sizeof(btbbx_le_conn), hipMemcpyDeviceToHost, q));
	if (nk)
		HIP_TRY(hipMemcpyAsync(cands, r.d_cands, (size_t)nk * sizeof(btbbx_le_cand), hipMemcpyDeviceToHost, q));
	HIP_TRY(hipStreamSynchronize(q));
	return (int64_t)r.n_conns;
}

extern "C" int64_t btbbx_le_track_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				       uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
				       btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
				       uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
				       btbbx_le_track *tracks, btbbx_le_track_pkt *pkts)
{
	const LeHostArgs a = LE_HOST_ARGS("btbbx_le_track_host");
	int rc = le_host_check(a, nullptr, false);
	if (rc)
		return rc;
	CallScope scope;
	LeHostRun r;
	rc = le_host_begin(a, [](uint32_t, uint32_t) { return (size_t)0; }, &r);
	if (rc || !r.have)
		return rc;
	if (r.nc && (rc = le_host_track(a, r)))
		return rc;
	return le_host_finish(a, r, 0, nullptr, 0);
}

extern "C" int64_t btbbx_le_csa2_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				      uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
				      btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
				      uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
				      btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_csa2 *sel, btbbx_le_csa2_pkt *sel_pkts)
{
	const LeHostArgs a = LE_HOST_ARGS("btbbx_le_csa2_host");
	int rc = le_host_check(a, nullptr, !sel && conn_cap);
	if (rc)
		return rc;
	CallScope scope;
	LeHostRun r;
	// behind the tracking's part: this stage's scratch, its per-connection and its per-candidate records
	const auto scratch = [](uint32_t cap, uint32_t conns) { return ld_up(le_csa2_layout(cap, conns).total); };
	rc = le_host_begin(a, [&](uint32_t cap, uint32_t conns) {
		return scratch(cap, conns) + ld_up((size_t)conns * sizeof(btbbx_le_csa2)) + ld_up((size_t)cap * sizeof(btbbx_le_csa2_pkt)); }, &r);
	if (rc || !r.have)
		return rc;
	btbbx_le_csa2 *d_sel = (btbbx_le_csa2 *)(r.own + scratch(r.dev_cap, r.dev_conns));
	btbbx_le_csa2_pkt *d_sel_pkts = (btbbx_le_csa2_pkt *)((char *)d_sel + ld_up((size_t)r.dev_conns * sizeof(btbbx_le_csa2)));
	if (r.nc && (rc = le_host_track(a, r)))
		return rc;
	if (r.nc && (rc = le_csa2_launch(r.d_cands, r.d_count, r.dev_cap, r.d_conns, r.d_conn_count, r.dev_conns, r.d_tracks, r.d_pkts, flags, d_sel,
					  d_sel_pkts, r.own, r.q)))
		return rc;
	const LeHostOut outs[] = {{sel, d_sel, sizeof(btbbx_le_csa2), false}, {sel_pkts, d_sel_pkts, sizeof(btbbx_le_csa2_pkt), true}};
	return le_host_finish(a, r, 0, outs, 2);
}

// ---- data extraction ------------------------------------------------------------------------------------------------------------

// this stage's part of the tail, as offsets from LeHostRun::own
struct LdtHostTail {
	size_t scratch, data, dpkts, msgs, counts, bytes, total;
	uint32_t msg_cap;
	uint64_t byte_cap;
};

static LdtHostTail le_data_host_layout(uint32_t dev_cap, uint32_t dev_conns, uint64_t msg_cap, uint64_t byte_cap)
{
	LdtHostTail T;
	T.msg_cap = (uint32_t)std::min<uint64_t>(msg_cap, dev_cap);                       // (a message has a START of its own)
	T.byte_cap = std::min<uint64_t>(byte_cap, 255ull * dev_cap);                     // (and a fragment at most 255 octets)
	size_t at = 0;
	auto take = [&](size_t bytes) { const size_t here = at; at += ld_up(bytes); return here; };
	T.scratch = take(le_data_layout(dev_cap, dev_conns).total);
	T.data = take((size_t)dev_conns * sizeof(btbbx_le_data));
	T.dpkts = take((size_t)dev_cap * sizeof(btbbx_le_data_pkt));
	T.msgs = take((size_t)T.msg_cap * sizeof(btbbx_le_msg));
	T.counts = take(256);
	T.bytes = take((size_t)T.byte_cap + 8);
	T.total = at;
	return T;
}

// the first have_msgs message records and the stored prefix of their octets, copied out behind the frame's synchronize: how many
// there are is known only then
static int le_host_messages(btbbx_le_msg *msgs, const btbbx_le_msg *d_msgs, uint64_t have_msgs, uint8_t *bytes, const uint8_t *d_bytes,
			    hipStream_t q)
{
	if (!have_msgs)
		return BTBBX_OK;
	HIP_TRY(hipMemcpyAsync(msgs, d_msgs, (size_t)have_msgs * sizeof(btbbx_le_msg), hipMemcpyDeviceToHost, q));
	HIP_TRY(hipStreamSynchronize(q));
	uint64_t lo = 0, hi = have_msgs;                                // the stored messages are a prefix: the first that is not
	while (lo < hi) {
		const uint64_t mid = lo + (hi - lo) / 2;
		if (msgs[mid].flags & BTBBX_LE_MSG_STORED)
			lo = mid + 1;
		else
			hi = mid;
	}
	const uint64_t stored = lo ? msgs[lo - 1].byte_offset + msgs[lo - 1].bytes : 0;
	if (stored) {
		HIP_TRY(hipMemcpyAsync(bytes, d_bytes, (size_t)stored, hipMemcpyDeviceToHost, q));
		HIP_TRY(hipStreamSynchronize(q));
	}
	return BTBBX_OK;
}

// the data stage over a tail that le_data_host_layout laid out at `base`; its counts stand at base + T.counts, the octets' first
static int le_host_data(const LeHostRun &r, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams, char *base, const LdtHostTail &T)
{
	uint64_t *d_counts = (uint64_t *)(base + T.counts);
	return le_data_launch(r.d_words, n_words, pitch_words, n_streams, r.d_cands, r.d_count, r.dev_cap, r.d_conns, r.d_conn_count, r.dev_conns,
			      r.d_pkts, (btbbx_le_data *)(base + T.data), (btbbx_le_data_pkt *)(base + T.dpkts), (btbbx_le_msg *)(base + T.msgs), T.msg_cap,
			      (uint32_t *)(d_counts + 1), (uint8_t *)(base + T.bytes), T.byte_cap, d_counts, base + T.scratch, r.q);
}

// behind le_host_finish (ret: what it gave): the two counts as they were read back, the messages and their octets
static int64_t le_host_message_outs(int64_t ret, const LeHostRun &r, const uint64_t *counts, uint32_t msg_cap, btbbx_le_msg *msgs,
				    const btbbx_le_msg *d_msgs, uint64_t *n_msgs_out, uint8_t *bytes, const uint8_t *d_bytes, uint64_t *n_bytes_out)
{
	if (ret < 0 || !r.nc)
		return ret;
	const uint64_t n_msgs = (uint32_t)counts[1];
	if (n_msgs_out)
		*n_msgs_out = n_msgs;
	if (n_bytes_out)
		*n_bytes_out = counts[0];
	const int rc = le_host_messages(msgs, d_msgs, std::min<uint64_t>(n_msgs, msg_cap), bytes, d_bytes, r.q);
	return rc ? rc : ret;
}

extern "C" int64_t btbbx_le_data_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				      uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
				      btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
				      uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
				      btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_data *data, btbbx_le_data_pkt *data_pkts,
				      btbbx_le_msg *msgs, uint64_t msg_cap, uint64_t *n_msgs_out, uint8_t *bytes, uint64_t byte_cap,
				      uint64_t *n_bytes_out)
{
	const LeHostArgs a = LE_HOST_ARGS("btbbx_le_data_host");
	int rc = le_host_check(a, nullptr, (!data && conn_cap) || (!msgs && msg_cap) || (!bytes && byte_cap));
	if (rc)
		return rc;
	if (n_msgs_out)
		*n_msgs_out = 0;
	if (n_bytes_out)
		*n_bytes_out = 0;
	CallScope scope;
	LeHostRun r;
	rc = le_host_begin(a, [&](uint32_t cap, uint32_t conns) { return le_data_host_layout(cap, conns, msg_cap, byte_cap).total; }, &r);
	if (rc || !r.have)
		return rc;
	const LdtHostTail T = le_data_host_layout(r.dev_cap, r.dev_conns, msg_cap, byte_cap);
	btbbx_le_msg *d_msgs = (btbbx_le_msg *)(r.own + T.msgs);
	uint64_t *d_counts = (uint64_t *)(r.own + T.counts), counts[2] = {0, 0};
	uint8_t *d_bytes = (uint8_t *)(r.own + T.bytes);
	if (r.nc) {
		if ((rc = le_host_track(a, r)))
			return rc;
		if ((rc = le_host_data(r, n_words, pitch_words, n_streams, r.own, T)))
			return rc;
		HIP_TRY(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, r.q));
	}
	const LeHostOut outs[] = {{data, r.own + T.data, sizeof(btbbx_le_data), false}, {data_pkts, r.own + T.dpkts, sizeof(btbbx_le_data_pkt), true}};
	return le_host_message_outs(le_host_finish(a, r, 0, outs, 2), r, counts, T.msg_cap, msgs, d_msgs, n_msgs_out, bytes, d_bytes, n_bytes_out);
}

// ---- decryption -------------------------------------------------------------------------------------------------------------------

// this stage's part of the tail, behind the data stage's (whose messages and octets are not kept: its caps are 0 here)
struct LxHostTail {
	size_t scratch, crypt, cpkts, ppkts, msgs, counts, bytes, keys, total;
};

// (records: with the stage's own records crypt and cpkts; a wrapper that keeps them among its outputs lays none out here)
static LxHostTail le_crypt_host_layout(uint32_t dev_cap, uint32_t dev_conns, uint32_t n_keys, const LdtHostTail &T, bool records = true)
{
	LxHostTail C;
	size_t at = le_data_host_layout(dev_cap, dev_conns, 0, 0).total;
	auto take = [&](size_t bytes) { const size_t here = at; at += ld_up(bytes); return here; };
	C.scratch = take(le_crypt_layout(dev_cap, dev_conns, n_keys).total);
	C.crypt = take(records ? (size_t)dev_conns * sizeof(btbbx_le_crypt) : 0);
	C.cpkts = take(records ? (size_t)dev_cap * sizeof(btbbx_le_crypt_pkt) : 0);
	C.ppkts = take((size_t)dev_cap * sizeof(btbbx_le_data_pkt));
	C.msgs = take((size_t)T.msg_cap * sizeof(btbbx_le_msg));
	C.counts = take(256);
	C.bytes = take((size_t)T.byte_cap + 8);
	C.keys = take(16 * (size_t)n_keys);
	C.total = at;
	return C;
}

extern "C" int64_t btbbx_le_crypt_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				       uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
				       btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
				       uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
				       btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_data *data, btbbx_le_data_pkt *data_pkts,
				       const uint8_t *keys, uint32_t n_keys, uint32_t window, btbbx_le_crypt *crypt,
				       btbbx_le_crypt_pkt *crypt_pkts, btbbx_le_data_pkt *plain_pkts, btbbx_le_msg *msgs, uint64_t msg_cap,
				       uint64_t *n_msgs_out, uint8_t *bytes, uint64_t byte_cap, uint64_t *n_bytes_out)
{
	const LeHostArgs a = LE_HOST_ARGS("btbbx_le_crypt_host");
	int rc = le_crypt_check_keys(a.who, n_keys, window);
	if (!rc)
		rc = le_host_check(a, nullptr, (!data && conn_cap) || (!crypt && conn_cap) || !keys || (!msgs && msg_cap) || (!bytes && byte_cap));
	if (rc)
		return rc;
	if (n_msgs_out)
		*n_msgs_out = 0;
	if (n_bytes_out)
		*n_bytes_out = 0;
	CallScope scope;
	LeHostRun r;
	const auto caps = [&](uint32_t cap, uint32_t k) { return le_data_host_layout(cap, k, msg_cap, byte_cap); };   // (the caps as the data wrapper cuts them)
	rc = le_host_begin(a, [&](uint32_t cap, uint32_t k) { return le_crypt_host_layout(cap, k, n_keys, caps(cap, k)).total; }, &r);
	if (rc || !r.have)
		return rc;
	const LdtHostTail T = caps(r.dev_cap, r.dev_conns), D = le_data_host_layout(r.dev_cap, r.dev_conns, 0, 0);
	const LxHostTail C = le_crypt_host_layout(r.dev_cap, r.dev_conns, n_keys, T);
	btbbx_le_data_pkt *d_dpkts = (btbbx_le_data_pkt *)(r.own + D.dpkts);
	btbbx_le_msg *d_msgs = (btbbx_le_msg *)(r.own + C.msgs);
	uint64_t *d_counts = (uint64_t *)(r.own + C.counts), counts[2] = {0, 0};
	uint8_t *d_bytes = (uint8_t *)(r.own + C.bytes), *d_keys = (uint8_t *)(r.own + C.keys);
	if (r.nc) {
		HIP_TRY(hipMemcpyAsync(d_keys, keys, 16 * (size_t)n_keys, hipMemcpyHostToDevice, r.q));
		if ((rc = le_host_track(a, r)))
			return rc;
		rc = le_host_data(r, n_words, pitch_words, n_streams, r.own, D);        // (caps 0: its messages and octets are not kept)
		if (!rc)
			rc = le_crypt_launch(r.d_words, n_words, pitch_words, n_streams, r.d_cands, r.d_count, r.dev_cap, r.d_conns, r.d_conn_count,
					     r.dev_conns, r.d_pkts, d_dpkts, d_keys, n_keys, window, (btbbx_le_crypt *)(r.own + C.crypt),
					     (btbbx_le_crypt_pkt *)(r.own + C.cpkts), (btbbx_le_data_pkt *)(r.own + C.ppkts), d_msgs, T.msg_cap,
					     (uint32_t *)(d_counts + 1), d_bytes, T.byte_cap, d_counts, r.own + C.scratch, r.q);
		if (rc)
			return rc;
		HIP_TRY(hipMemcpyAsync(counts, d_counts, sizeof(counts), hipMemcpyDeviceToHost, r.q));
	}
	const LeHostOut outs[] = {{data, r.own + D.data, sizeof(btbbx_le_data), false}, {data_pkts, d_dpkts, sizeof(btbbx_le_data_pkt), true},
				  {crypt, r.own + C.crypt, sizeof(btbbx_le_crypt), false}, {crypt_pkts, r.own + C.cpkts, sizeof(btbbx_le_crypt_pkt), true},
				  {plain_pkts, r.own + C.ppkts, sizeof(btbbx_le_data_pkt), true}};
	return le_host_message_outs(le_host_finish(a, r, 0, outs, 5), r, counts, T.msg_cap, msgs, d_msgs, n_msgs_out, bytes, d_bytes, n_bytes_out);
}

// ---- following: the follow stage or the span stage behind the seed stage ---------------------------------------------------------

// the advertising scan's block: the counter, the hits, the ordering's scratch, the decoded records
struct LfAdvLayout {
	size_t hits, order, pkts, total;
};

static LfAdvLayout le_follow_adv_layout(uint32_t cap)
{
	LfAdvLayout A;
	A.hits = 256;
	A.order = A.hits + ld_up((size_t)cap * sizeof(btbbx_hit));
	A.pkts = A.order + (cap >= 2 ? ld_up(btbbx_order_hits_scratch_bytes(cap)) : 0);
	A.total = A.pkts + ld_up((size_t)cap * sizeof(btbbx_le_pkt));
	return A;
}

// The advertising scan over the device copy of the capture, repeated with room for every match when `ablock` (room for adv_cap
// hits) was too small -- in a block of its own then, *spill, which the caller frees behind its last synchronize --, ordered and
// decoded.  On return ablock begins with the count, adv_cap is what it holds and *d_adv its decoded records
static int le_follow_host_adv(const LeHostArgs &a, const LeHostRun &r, uint64_t pitch_words, int adv_errors, char *&ablock, uint32_t &adv_cap,
			      void **spill, btbbx_le_pkt **d_adv)
{
	uint32_t adv_count = 0;
	for (int pass = 0; pass < 2; pass++) {
		HIP_TRY(hipMemsetAsync(ablock, 0, sizeof(uint32_t), r.q));
		const int rc = le_launch_scan(r.d_words, a.n_words, pitch_words, a.n_streams, a.search_bits, BTBBX_LE_ADV_AA, adv_errors,
					      (btbbx_hit *)(ablock + le_follow_adv_layout(adv_cap).hits), adv_cap, (uint32_t *)ablock, r.q);
		if (rc)
			return rc;
		hipError_t e = hipMemcpyAsync(&adv_count, ablock, sizeof(adv_count), hipMemcpyDeviceToHost, r.q);
		if (e == hipSuccess)
			e = hipStreamSynchronize(r.q);
		if (e != hipSuccess)
			return hip_fail(e, "advertising scan");
		if (adv_count <= adv_cap || pass)
			break;
		adv_cap = adv_count;
		if (hipMalloc(spill, le_follow_adv_layout(adv_cap).total) != hipSuccess) {
			set_error("%s: advertising block of %zu bytes failed", a.who, le_follow_adv_layout(adv_cap).total);
			return BTBBX_E_NOMEM;
		}
		ablock = (char *)*spill;
	}
	const LfAdvLayout A = le_follow_adv_layout(adv_cap);
	*d_adv = (btbbx_le_pkt *)(ablock + A.pkts);
	if (std::min(adv_count, adv_cap) >= 2) {
		const int rc = btbbx_order_hits_device((btbbx_hit *)(ablock + A.hits), (uint32_t *)ablock, adv_cap, ablock + A.order, A.pkts - A.order, r.q);
		if (rc)
			return rc;
	}
	return btbbx_le_decode_hits_device(r.d_words, a.n_words, pitch_words, (btbbx_hit *)(ablock + A.hits), (uint32_t *)ablock, adv_cap, r.d_phys,
					   BTBBX_LE_ADV_CRC_INIT, *d_adv, r.q);
}

// the advertising hits le_follow_host_chain makes room for at first (a 40-bit pattern with up to four errors matches noise at one
// offset in ten million)
static uint32_t le_follow_adv_guess(const LeHostArgs &a)
{
	const uint64_t guess = a.search_bits / 16384 * a.n_streams + 4096;
	return guess > 0xfffffff0ull ? 0xfffffff0u : (uint32_t)guess;
}

// The chain of btbbx_le_epoch_host and btbbx_le_span_host: the advertising scan, the tracking, the seed stage and the wrapper's
// last stage -- last(r, pitch_words, d_seeds, d_scratch, d_out): its launches; r names the advertising block too --, whose scratch takes last_scratch(dev_cap, dev_conns)
// bytes.  outs: the last stage's outputs (at most five; src is not read): their device records stand behind the scratch in this
// order, dev_conns or dev_cap of them each (or `fixed` of them), and d_out[o] is where those of outs[o] begin.
// A failed launch does not end the call at once: the stream is synchronised and a spilled advertising block freed first
template <class Scratch, class Last>
static int64_t le_follow_host_chain(const LeHostArgs &a, int adv_errors, btbbx_le_seed *seeds, bool missing, Scratch last_scratch,
				    const LeHostOut *outs, int n_outs, Last last)
{
	int rc = le_host_check(a, &adv_errors, (!seeds && a.conn_cap) || missing);
	if (rc)
		return rc;
	const uint64_t pitch_words = a.n_streams == 1 ? a.n_words : a.pitch_words;
	CallScope scope;
	uint32_t adv_cap = le_follow_adv_guess(a);
	// behind the tracking's part: the seeds, the last stage's scratch and records, the advertising scan's block
	const auto records = [&](uint32_t cap, uint32_t conns, int upto) {
		size_t at = ld_up((size_t)conns * sizeof(btbbx_le_seed)) + ld_up(last_scratch(cap, conns));
		for (int o = 0; o < upto; o++)
			at += ld_up(outs[o].count(conns, cap) * outs[o].size);
		return at;
	};
	LeHostRun r;
	rc = le_host_begin(a, [&](uint32_t cap, uint32_t conns) { return records(cap, conns, n_outs) + le_follow_adv_layout(adv_cap).total; }, &r);
	if (rc)
		return rc;
	if (!r.have) {                                          // no candidate: nothing to copy, a fixed table is zeros
		for (int o = 0; o < n_outs; o++)
			if (outs[o].fixed >= 0 && outs[o].dst)
				memset(outs[o].dst, 0, (size_t)outs[o].fixed * outs[o].size);
		return BTBBX_OK;
	}
	void *spill = nullptr;                                  // a second advertising block, when the first was too small
	btbbx_le_seed *d_seeds = (btbbx_le_seed *)r.own;
	LeHostOut all[6] = {{seeds, d_seeds, sizeof(btbbx_le_seed), false}};
	char *d_out[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
	for (int o = 0; o < n_outs; o++) {
		d_out[o] = r.own + records(r.dev_cap, r.dev_conns, o);
		all[o + 1] = {outs[o].dst, d_out[o], outs[o].size, outs[o].per_cand, outs[o].fixed};
	}
	if (r.nc) {
		char *ablock = r.own + records(r.dev_cap, r.dev_conns, n_outs);
		btbbx_le_pkt *d_adv = nullptr;
		rc = le_follow_host_adv(a, r, pitch_words, adv_errors, ablock, adv_cap, &spill, &d_adv);
		if (!rc)
			rc = le_host_track(a, r);
		if (!rc)
			rc = btbbx_le_seed_device(d_adv, (uint32_t *)ablock, adv_cap, r.d_conns, r.d_conn_count, r.dev_conns, r.d_tracks, a.unit_bits,
						  d_seeds, r.q);
		r.d_adv = d_adv;
		r.d_adv_count = (const uint32_t *)ablock;
		r.adv_cap = adv_cap;
		if (!rc)
			rc = last(r, pitch_words, d_seeds, r.own + ld_up((size_t)r.dev_conns * sizeof(btbbx_le_seed)), d_out);
	}
	const int64_t ret = le_host_finish(a, r, rc, all, n_outs + 1);
	if (spill)
		(void)hipFree(spill);
	return ret;
}

extern "C" int64_t btbbx_le_epoch_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
					uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
					btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
					uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
					int adv_errors, btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_seed *seeds,
					btbbx_le_follow *follows, btbbx_le_follow_pkt *follow_pkts)
{
	const LeHostArgs a = LE_HOST_ARGS("btbbx_le_epoch_host");
	const LeHostOut outs[] = {{follows, nullptr, sizeof(btbbx_le_follow), false}, {follow_pkts, nullptr, sizeof(btbbx_le_follow_pkt), true}};
	return le_follow_host_chain(
		a, adv_errors, seeds, !follows && conn_cap, [](uint32_t cap, uint32_t k) { return le_follow_layout(cap, k).total; }, outs, 2,
		[&](const LeHostRun &r, uint64_t pitch, const btbbx_le_seed *d_seeds, char *d_scratch, char *const *d_out) {
			return le_follow_launch(r.d_words, n_words, pitch, n_streams, r.d_cands, r.d_count, r.dev_cap, r.d_conns, r.d_conn_count,
						r.dev_conns, r.d_pkts, d_seeds, unit_bits, jitter_bits, (btbbx_le_follow *)d_out[0],
						(btbbx_le_follow_pkt *)d_out[1], d_scratch, r.q);
		});
}

extern "C" int64_t btbbx_le_span_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				      uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
				      btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
				      uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
				      int adv_errors, btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_seed *seeds,
				      uint32_t max_updates, btbbx_le_span *spans, btbbx_le_span_pkt *span_pkts, btbbx_le_span_rec *span_recs)
{
	const LeHostArgs a = LE_HOST_ARGS("btbbx_le_span_host");
	if (max_updates > LS_MAX_UPDATES) {
		set_error("%s: max_updates must be 0..%u", a.who, LS_MAX_UPDATES);
		return BTBBX_E_ARG;
	}
	// (the device records of connection g stand at g * (max_updates + 1), whatever dev_conns is: the first nc of them are copied)
	const LeHostOut outs[] = {{spans, nullptr, sizeof(btbbx_le_span), false}, {span_pkts, nullptr, sizeof(btbbx_le_span_pkt), true},
				  {span_recs, nullptr, (max_updates + 1) * sizeof(btbbx_le_span_rec), false}};
	return le_follow_host_chain(
		a, adv_errors, seeds, (!spans || !span_recs) && conn_cap,
		[&](uint32_t cap, uint32_t k) { return le_span_layout(cap, k, max_updates).total; }, outs, 3,
		[&](const LeHostRun &r, uint64_t pitch, const btbbx_le_seed *d_seeds, char *d_scratch, char *const *d_out) {
			return le_span_launch(r.d_words, n_words, pitch, n_streams, r.d_cands, r.d_count, r.dev_cap, r.d_conns, r.d_conn_count,
					      r.dev_conns, r.d_pkts, d_seeds, unit_bits, jitter_bits, max_updates, (btbbx_le_span *)d_out[0],
					      (btbbx_le_span_pkt *)d_out[1], (btbbx_le_span_rec *)d_out[2], d_scratch, r.q);
		});
}

// the data stage, the decryption stage and the keyed span stage behind the seed stage
extern "C" int64_t btbbx_le_keyed_span_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
					    uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
					    btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
					    uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
					    int adv_errors, btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_seed *seeds,
					    const uint8_t *keys, uint32_t n_keys, uint32_t window, btbbx_le_crypt *crypt,
					    btbbx_le_crypt_pkt *crypt_pkts, uint32_t max_updates, btbbx_le_span *spans,
					    btbbx_le_span_pkt *span_pkts, btbbx_le_span_rec *span_recs)
{
	const LeHostArgs a = LE_HOST_ARGS("btbbx_le_keyed_span_host");
	if (max_updates > LS_MAX_UPDATES) {
		set_error("%s: max_updates must be 0..%u", a.who, LS_MAX_UPDATES);
		return BTBBX_E_ARG;
	}
	const int rc = le_crypt_check_keys(a.who, n_keys, window);
	if (rc)
		return rc;
	// the data stage's and the decryption stage's parts as btbbx_le_crypt_host lays them out (no message, no octet is kept; the
	// decryption stage's records are outputs here and stand with them), then the keyed span stage's scratch
	const auto crypt_tail = [&](uint32_t cap, uint32_t k) {
		return le_crypt_host_layout(cap, k, n_keys, le_data_host_layout(cap, k, 0, 0), false);
	};
	const LeHostOut outs[] = {{crypt, nullptr, sizeof(btbbx_le_crypt), false}, {crypt_pkts, nullptr, sizeof(btbbx_le_crypt_pkt), true},
				  {spans, nullptr, sizeof(btbbx_le_span), false}, {span_pkts, nullptr, sizeof(btbbx_le_span_pkt), true},
				  {span_recs, nullptr, (max_updates + 1) * sizeof(btbbx_le_span_rec), false}};
	return le_follow_host_chain(
		a, adv_errors, seeds, ((!spans || !span_recs || !crypt) && conn_cap) || !keys,
		[&](uint32_t cap, uint32_t k) { return ld_up(crypt_tail(cap, k).total) + btbbx_le_keyed_span_scratch_bytes(cap, k, max_updates); }, outs, 5,
		[&](const LeHostRun &r, uint64_t pitch, const btbbx_le_seed *d_seeds, char *d_scratch, char *const *d_out) {
			const LdtHostTail D = le_data_host_layout(r.dev_cap, r.dev_conns, 0, 0);
			const LxHostTail C = crypt_tail(r.dev_cap, r.dev_conns);
			const btbbx_le_data_pkt *d_dpkts = (const btbbx_le_data_pkt *)(d_scratch + D.dpkts);
			uint64_t *d_counts = (uint64_t *)(d_scratch + C.counts);
			uint8_t *d_keys = (uint8_t *)(d_scratch + C.keys);
			HIP_TRY(hipMemcpyAsync(d_keys, keys, 16 * (size_t)n_keys, hipMemcpyHostToDevice, r.q));
			int rc2 = le_host_data(r, n_words, pitch, n_streams, d_scratch, D);
			if (!rc2)
				rc2 = le_crypt_launch(r.d_words, n_words, pitch, n_streams, r.d_cands, r.d_count, r.dev_cap, r.d_conns, r.d_conn_count,
						      r.dev_conns, r.d_pkts, d_dpkts, d_keys, n_keys, window, (btbbx_le_crypt *)d_out[0],
						      (btbbx_le_crypt_pkt *)d_out[1], (btbbx_le_data_pkt *)(d_scratch + C.ppkts),
						      (btbbx_le_msg *)(d_scratch + C.msgs), 0, (uint32_t *)(d_counts + 1), (uint8_t *)(d_scratch + C.bytes), 0,
						      d_counts, d_scratch + C.scratch, r.q);
			if (!rc2)
				rc2 = le_keyed_launch_span(r.d_words, n_words, pitch, n_streams, r.d_cands, r.d_count, r.dev_cap, r.d_conns, r.d_conn_count,
							   r.dev_conns, r.d_pkts, d_seeds, d_dpkts, (const btbbx_le_crypt *)d_out[0],
							   (const btbbx_le_crypt_pkt *)d_out[1], unit_bits, jitter_bits, max_updates,
							   (btbbx_le_span *)d_out[2], (btbbx_le_span_pkt *)d_out[3], (btbbx_le_span_rec *)d_out[4],
							   d_scratch + ld_up(C.total), r.q);
			return rc2;
		});
}

// ---- pairing: the data stage and the pairing stage behind the seed stage ----------------------------------------------------------

extern "C" int64_t btbbx_le_pair_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				       uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
				       btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
				       uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
				       int adv_errors, btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_seed *seeds,
				       uint64_t msg_cap, uint64_t byte_cap, uint32_t tk_limit, btbbx_le_pair *pairs, uint8_t *keys,
				       uint32_t key_cap, uint32_t *n_keys_out)
{
	const LeHostArgs a = LE_HOST_ARGS("btbbx_le_pair_host");
	const int rc = le_pair_check_limits(a.who, tk_limit, key_cap);
	if (rc)
		return rc;
	uint32_t n_keys = 0;
	// the data stage's part (its scratch, records, messages and octets, none of them copied out), then this stage's scratch
	const auto caps = [&](uint32_t cap, uint32_t k) { return le_data_host_layout(cap, k, msg_cap, byte_cap); };
	const LeHostOut outs[] = {{pairs, nullptr, sizeof(btbbx_le_pair), false}, {keys, nullptr, 16, false, (int64_t)key_cap},
				  {&n_keys, nullptr, sizeof(uint32_t), false, 1}};
	const int64_t ret = le_follow_host_chain(
		a, adv_errors, seeds, (!pairs && conn_cap) || (!keys && key_cap),
		[&](uint32_t cap, uint32_t k) { return ld_up(caps(cap, k).total) + le_pair_layout(k).total; }, outs, 3,
		[&](const LeHostRun &r, uint64_t pitch, const btbbx_le_seed *d_seeds, char *d_scratch, char *const *d_out) {
			const LdtHostTail T = caps(r.dev_cap, r.dev_conns);
			btbbx_le_msg *d_msgs = (btbbx_le_msg *)(d_scratch + T.msgs);
			uint64_t *d_counts = (uint64_t *)(d_scratch + T.counts);
			uint8_t *d_bytes = (uint8_t *)(d_scratch + T.bytes);
			int rc2 = le_host_data(r, n_words, pitch, n_streams, d_scratch, T);
			if (!rc2)
				rc2 = le_pair_launch(r.d_conn_count, r.dev_conns, d_seeds, d_msgs, (uint32_t *)(d_counts + 1), T.msg_cap, d_bytes,
						     T.byte_cap, tk_limit, (btbbx_le_pair *)d_out[0], (uint8_t *)d_out[1], key_cap, (uint32_t *)d_out[2],
						     d_scratch + ld_up(T.total), r.q);
			return rc2;
		});
	if (ret >= 0 && n_keys_out)
		*n_keys_out = n_keys;
	return ret;
}

// ---- address resolution -----------------------------------------------------------------------------------------------------------

// the advertising channels alone: btbbx_le_scan_host's chain for the advertising AA, then the resolve stage under the caller's keys
extern "C" int64_t btbbx_le_resolve_adv_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
					     uint64_t search_bits, const uint16_t *phys_channel, int adv_errors, const uint8_t *given,
					     uint32_t n_given, btbbx_le_pkt *adv, uint64_t adv_cap, uint32_t *slot_addr, btbbx_le_addr *addrs,
					     uint32_t addr_cap, uint32_t *n_addrs_out, btbbx_le_irk *irks, uint32_t irk_cap, uint32_t *n_irks_out)
{
	const char *who = "btbbx_le_resolve_adv_host";
	int rc = le_check_args(who, n_words, pitch_words, n_streams, search_bits, adv_errors);
	if (!rc)
		rc = le_resolve_check_limits(who, adv_cap, n_given, irk_cap);
	if (rc)
		return rc;
	if (!words || !phys_channel || ((!adv || !slot_addr) && adv_cap) || (!addrs && addr_cap) || (!irks && irk_cap) || (!given && n_given)) {
		set_error("%s: null pointer", who);
		return BTBBX_E_ARG;
	}
	rc = ctx_require();
	if (rc)
		return rc;
	if (n_addrs_out)
		*n_addrs_out = 0;
	if (n_irks_out)
		*n_irks_out = 0;
	if (n_streams == 1)
		pitch_words = n_words;
	CallScope scope;
	hipStream_t q = scope_stream();
	const uint64_t cap_words = (uint64_t)(n_streams - 1) * pitch_words + n_words;
	const size_t words_bytes = ((size_t)(cap_words + 1) * 8 + 255) & ~(size_t)255;
	char *dblock = (char *)scope_device(words_bytes + 2 * (size_t)n_streams);
	if (!dblock)
		return BTBBX_E_NOMEM;
	const uint64_t *d_words = (const uint64_t *)dblock;
	uint16_t *d_phys = (uint16_t *)(dblock + words_bytes);
	HIP_TRY(hipMemcpyAsync(dblock, words, (size_t)cap_words * 8, hipMemcpyHostToDevice, q));
	HIP_TRY(hipMemcpyAsync(d_phys, phys_channel, 2 * (size_t)n_streams, hipMemcpyHostToDevice, q));
	// the scan as btbbx_le_scan_host runs it: a first guess, repeated with room for every match so that the prefix is the true one
	uint64_t guess = std::min<uint64_t>(search_bits / 1024 * n_streams + 4096, adv_cap);
	uint32_t dev_cap = (uint32_t)guess, count = 0, n = 0;
	char *block = nullptr;
	size_t at = 0;
	auto take = [&](size_t bytes) { const size_t here = at; at += ld_up(bytes); return here; };
	size_t hits = 0, order = 0, order_bytes = 0, pkts = 0, keys = 0, slots = 0, arecs = 0, irecs = 0, counts = 0, scratch = 0;
	for (int pass = 0; pass < 2; pass++) {
		n = (uint32_t)std::min<uint64_t>(dev_cap, adv_cap);     // the records that are decoded and resolved
		at = 256;
		hits = take((size_t)dev_cap * sizeof(btbbx_hit));
		order_bytes = dev_cap >= 2 ? btbbx_order_hits_scratch_bytes(dev_cap) : 0;
		order = take(order_bytes);
		pkts = take((size_t)n * sizeof(btbbx_le_pkt));
		keys = take(16 * (size_t)n_given);
		slots = take(8 * (size_t)n);
		arecs = take((size_t)addr_cap * sizeof(btbbx_le_addr));
		irecs = take((size_t)irk_cap * sizeof(btbbx_le_irk));
		counts = take(256);
		scratch = take(le_resolve_layout(n, 0, irk_cap).total);
		block = (char *)scope_hits(at);
		if (!block)
			return BTBBX_E_NOMEM;
		HIP_TRY(hipMemsetAsync(block, 0, sizeof(uint32_t), q));
		rc = le_launch_scan(d_words, n_words, pitch_words, n_streams, search_bits, BTBBX_LE_ADV_AA, adv_errors, (btbbx_hit *)(block + hits),
				    dev_cap, (uint32_t *)block, q);
		if (rc)
			return rc;
		HIP_TRY(hipMemcpyAsync(&count, block, sizeof(count), hipMemcpyDeviceToHost, q));
		HIP_TRY(hipStreamSynchronize(q));
		if (count <= dev_cap || adv_cap == 0)
			break;
		dev_cap = count;
	}
	uint32_t *d_count = (uint32_t *)block, *d_counts = (uint32_t *)(block + counts);
	btbbx_le_pkt *d_adv = (btbbx_le_pkt *)(block + pkts);
	if (std::min(count, dev_cap) >= 2) {
		rc = btbbx_order_hits_device((btbbx_hit *)(block + hits), d_count, dev_cap, block + order, ld_up(order_bytes), q);
		if (rc)
			return rc;
	}
	if (n) {
		rc = btbbx_le_decode_hits_device(d_words, n_words, pitch_words, (btbbx_hit *)(block + hits), d_count, n, d_phys, BTBBX_LE_ADV_CRC_INIT,
						 d_adv, q);
		if (rc)
			return rc;
	}
	if (n_given)
		HIP_TRY(hipMemcpyAsync(block + keys, given, 16 * (size_t)n_given, hipMemcpyHostToDevice, q));
	rc = le_resolve_launch(n ? d_adv : nullptr, d_count, n, nullptr, 0, nullptr, nullptr, nullptr, 0, nullptr, 0, (const uint8_t *)(block + keys),
			       n_given, (uint32_t *)(block + slots), (btbbx_le_addr *)(block + arecs), addr_cap, d_counts, (btbbx_le_irk *)(block + irecs),
			       irk_cap, d_counts + 1, nullptr, block + scratch, q);
	if (rc)
		return rc;
	uint32_t got[2] = {0, 0};
	HIP_TRY(hipMemcpyAsync(got, d_counts, sizeof(got), hipMemcpyDeviceToHost, q));
	HIP_TRY(hipStreamSynchronize(q));
	const uint32_t have = std::min(count, n), have_addrs = std::min(got[0], addr_cap);
	if (have) {
		HIP_TRY(hipMemcpyAsync(adv, d_adv, (size_t)have * sizeof(btbbx_le_pkt), hipMemcpyDeviceToHost, q));
		HIP_TRY(hipMemcpyAsync(slot_addr, block + slots, 8 * (size_t)have, hipMemcpyDeviceToHost, q));
	}
	if (have_addrs)
		HIP_TRY(hipMemcpyAsync(addrs, block + arecs, (size_t)have_addrs * sizeof(btbbx_le_addr), hipMemcpyDeviceToHost, q));
	if (irk_cap)
		HIP_TRY(hipMemcpyAsync(irks, block + irecs, (size_t)irk_cap * sizeof(btbbx_le_irk), hipMemcpyDeviceToHost, q));
	HIP_TRY(hipStreamSynchronize(q));
	if (n_addrs_out)
		*n_addrs_out = got[0];
	if (n_irks_out)
		*n_irks_out = got[1];
	return (int64_t)count;
}

// the data stage, the decryption stage and the resolve stage behind the seed stage
extern "C" int64_t btbbx_le_resolve_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
					 uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
					 btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
					 uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
					 int adv_errors, btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_seed *seeds,
					 const uint8_t *keys, uint32_t n_keys, uint32_t window, uint64_t msg_cap, uint64_t byte_cap,
					 const uint8_t *given, uint32_t n_given, btbbx_le_peer *peers, btbbx_le_irk *irks, uint32_t irk_cap,
					 uint32_t *n_irks_out, btbbx_le_addr *addrs, uint32_t addr_cap, uint32_t *n_addrs_out)
{
	const LeHostArgs a = LE_HOST_ARGS("btbbx_le_resolve_host");
	int rc = le_resolve_check_limits(a.who, 0, n_given, irk_cap);
	if (!rc)
		rc = le_crypt_check_keys(a.who, n_keys, window);
	if (rc)
		return rc;
	uint32_t n_irks = 0, n_addrs = 0;
	void *extra = nullptr;                                  // this stage's own blocks, when the advertising block had to grow
	const uint32_t guess = std::min(le_follow_adv_guess(a), 0x7fffffffu);
	// the data stage's and the decryption stage's parts as btbbx_le_crypt_host lays them out, then the caller's keys, the slot map and
	// this stage's scratch, the last two for `guess` advertising records
	const auto caps = [&](uint32_t cap, uint32_t k) { return le_data_host_layout(cap, k, msg_cap, byte_cap); };
	const auto crypt_tail = [&](uint32_t cap, uint32_t k) { return le_crypt_host_layout(cap, k, n_keys, caps(cap, k)); };
	const auto own_given = [&](uint32_t cap, uint32_t k) { return ld_up(crypt_tail(cap, k).total); };
	const auto own_slots = [&](uint32_t cap, uint32_t k) { return own_given(cap, k) + ld_up(16 * (size_t)n_given); };
	const auto own_scratch = [&](uint32_t cap, uint32_t k) { return own_slots(cap, k) + ld_up(8 * (size_t)guess); };
	const LeHostOut outs[] = {{peers, nullptr, sizeof(btbbx_le_peer), false}, {irks, nullptr, sizeof(btbbx_le_irk), false, (int64_t)irk_cap},
				  {addrs, nullptr, sizeof(btbbx_le_addr), false, (int64_t)addr_cap}, {&n_irks, nullptr, sizeof(uint32_t), false, 1},
				  {&n_addrs, nullptr, sizeof(uint32_t), false, 1}};
	const int64_t ret = le_follow_host_chain(
		a, adv_errors, seeds, (!peers && conn_cap) || (!irks && irk_cap) || (!addrs && addr_cap) || (!given && n_given) || !keys,
		[&](uint32_t cap, uint32_t k) { return own_scratch(cap, k) + le_resolve_layout(guess, k, irk_cap).total; }, outs, 5,
		[&](const LeHostRun &r, uint64_t pitch, const btbbx_le_seed *d_seeds, char *d_scratch, char *const *d_out) {
			const LdtHostTail D = le_data_host_layout(r.dev_cap, r.dev_conns, 0, 0), T = caps(r.dev_cap, r.dev_conns);
			const LxHostTail C = crypt_tail(r.dev_cap, r.dev_conns);
			const btbbx_le_data_pkt *d_dpkts = (const btbbx_le_data_pkt *)(d_scratch + D.dpkts);
			btbbx_le_msg *d_msgs = (btbbx_le_msg *)(d_scratch + C.msgs);
			uint64_t *d_counts = (uint64_t *)(d_scratch + C.counts);
			uint8_t *d_bytes = (uint8_t *)(d_scratch + C.bytes), *d_keys = (uint8_t *)(d_scratch + C.keys);
			uint8_t *d_given = (uint8_t *)(d_scratch + own_given(r.dev_cap, r.dev_conns));
			const uint32_t adv_cap = std::min(r.adv_cap, 0x7fffffffu);
			char *d_slots = d_scratch + own_slots(r.dev_cap, r.dev_conns), *d_own = d_scratch + own_scratch(r.dev_cap, r.dev_conns);
			if (adv_cap > guess) {
				const size_t slot_bytes = ld_up(8 * (size_t)adv_cap);
				if (hipMalloc(&extra, slot_bytes + le_resolve_layout(adv_cap, r.dev_conns, irk_cap).total) != hipSuccess) {
					set_error("%s: block for %u advertising records failed", a.who, adv_cap);
					return (int)BTBBX_E_NOMEM;
				}
				d_slots = (char *)extra;
				d_own = d_slots + slot_bytes;
			}
			HIP_TRY(hipMemcpyAsync(d_keys, keys, 16 * (size_t)n_keys, hipMemcpyHostToDevice, r.q));
			if (n_given)
				HIP_TRY(hipMemcpyAsync(d_given, given, 16 * (size_t)n_given, hipMemcpyHostToDevice, r.q));
			int rc2 = le_host_data(r, n_words, pitch, n_streams, d_scratch, D);
			if (!rc2)
				rc2 = le_crypt_launch(r.d_words, n_words, pitch, n_streams, r.d_cands, r.d_count, r.dev_cap, r.d_conns, r.d_conn_count,
						      r.dev_conns, r.d_pkts, d_dpkts, d_keys, n_keys, window, (btbbx_le_crypt *)(d_scratch + C.crypt),
						      (btbbx_le_crypt_pkt *)(d_scratch + C.cpkts), (btbbx_le_data_pkt *)(d_scratch + C.ppkts), d_msgs,
						      T.msg_cap, (uint32_t *)(d_counts + 1), d_bytes, T.byte_cap, d_counts, d_scratch + C.scratch, r.q);
			if (!rc2)
				rc2 = le_resolve_launch(r.d_adv, r.d_adv_count, adv_cap, r.d_conn_count, r.dev_conns, d_seeds, d_msgs,
							(const uint32_t *)(d_counts + 1), T.msg_cap, d_bytes, T.byte_cap, d_given, n_given,
							(uint32_t *)d_slots, (btbbx_le_addr *)d_out[2], addr_cap, (uint32_t *)d_out[4],
							(btbbx_le_irk *)d_out[1], irk_cap, (uint32_t *)d_out[3], (btbbx_le_peer *)d_out[0], d_own, r.q);
			return rc2;
		});
	if (extra)
		(void)hipFree(extra);
	if (ret >= 0 && n_irks_out)
		*n_irks_out = n_irks;
	if (ret >= 0 && n_addrs_out)
		*n_addrs_out = n_addrs;
	return ret;
}
