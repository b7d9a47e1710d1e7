// packet_dropin.h -- piece of packet.hip: the four single-packet kernels of the drop-in API: decode_bytes_kernel (btbb_decode), replay_kernel
// (single try_clock / crc_check calls) and trials_state_kernel + trials_merge_kernel (btbb_uap_from_header, bluetooth_piconet.c:648-750).
#pragma once

// 64 symbols, one per byte (bit 0 counts), -> one packed word
__device__ __forceinline__ uint64_t pack64(const uint8_t *sym)
{
	uint64_t v = 0;
	const uint4 *p = reinterpret_cast<const uint4 *>(sym);
	for (int q = 0; q < 4; q++) {
		const uint4 x = p[q];
		const uint32_t d[4] = {x.x, x.y, x.z, x.w};
		for (int k = 0; k < 4; k++) {
			const uint32_t b = d[k] & 0x01010101u;
			v |= (uint64_t)((b | (b >> 7) | (b >> 14) | (b >> 21)) & 0xfu) << (16 * q + 4 * k);
		}
	}
	return v;
}

// The drop-in's single-packet decode in ONE launch: the symbol bytes and the current payload bit
// bytes are packed by the workgroup, lane 0 decodes, and the payload bits are unpacked again --
// instead of pack + pack + decode + unpack launches around a one-lane kernel.
__global__ __launch_bounds__(64) void decode_bytes_kernel(const uint8_t *sym, uint8_t *pay, const btbbx_pkt_in *in,
							   btbbx_pkt_out *o, uint32_t mode, int with_payload)
{
	__shared__ uint64_t pkt[BTBBX_PKT_WORDS + 2];
	const uint32_t lane = threadIdx.x;
	if (lane < BTBBX_PKT_WORDS + 2)
		pkt[lane] = lane < BTBBX_PKT_WORDS ? pack64(sym + 64 * lane) : 0;      // 3200 staged bytes
	if (with_payload && lane < 43)
		o->payload[lane] = pack64(pay + 64 * lane);                            // 2752 staged bytes
	chain_lds_init();
	if (lane == 0)
		decode_one(pkt, in[0], o, mode);
	__syncthreads();
	if (with_payload && lane < 43) {
		const uint64_t v = o->payload[lane];
		for (int k = 0; k < 64; k += 4) {
			const uint32_t n = (uint32_t)(v >> k) & 0xf;
			*reinterpret_cast<uint32_t *>(pay + 64 * lane + k) = (n * 0x00204081u) & 0x01010101u;
		}
	}
}

// ---- "last writer wins" over the 64 trials of a packet, taken in lane order (replay_kernel, trials_merge_kernel) ----
// scalar fields: the highest lane that assigned them, -1 if none did
__device__ __forceinline__ int last_lane(bool mine)
{
	const uint64_t m = __ballot(mine);
	return m ? 63 - (int)__builtin_clzll(m) : -1;
}
// payload word j: from the highest trial down, the bits that trial's prefix (wrote[k] bits) covers; row(k) = word j of trial k's buffer
template <class Row>
__device__ __forceinline__ uint64_t merge_payload_word(uint64_t word, uint32_t j, const uint32_t *wrote, Row row)
{
	uint64_t undecided = ~0ULL;
	for (int k = 63; k >= 0 && undecided; k--) {
		const uint32_t w = wrote[k];
		if (w <= 64u * j)
			continue;
		const uint32_t nb = w - 64u * j;
		const uint64_t covers = (nb >= 64 ? ~0ULL : ((1ULL << nb) - 1)) & undecided;
		word = (word & ~covers) | (row(k) & covers);
		undecided &= ~covers;
	}
	return word;
}

// DEC_TRIALS for one packet, 64 trials at once: lane = candidate count, every lane starts from the
// entry state and writes into a private payload buffer; what the reference's sequential loop
// (bluetooth_piconet.c:675-690) leaves in the packet is then "last writer wins" per field and per
// payload bit, taken in lane order.  Valid because a trial never reads what an earlier trial
// wrote: try_clock + crc_check(c) depend on the entry UAP / type only when FEC 1/3 fails (then for
// every clock alike), the payload header merge is bitwise, and EV4's llid / flow read never
// decides anything (see the identities at the top of this file).
__global__ __launch_bounds__(64) void replay_kernel(const uint64_t *packet, const btbbx_pkt_in *in, btbbx_pkt_out *o,
						     TrialPlan plan)
{
	__shared__ uint64_t pay[64][44];
	__shared__ uint32_t wrote[64];
	chain_lds_init();
	const uint32_t lane = threadIdx.x;
	const btbbx_pkt_in pi = in[0];
	PState s;
	s.w = packet;
	s.length = (int)pi.length;
	pstate_enter(s, pi);
	pstate_from_head(s, o);
	s.out = pay[lane];
	for (int j = 0; j < 44; j++)
		pay[lane][j] = 0;
	const uint32_t entry_flags = s.flags;

	const bool do_try = (plan.try_mask >> lane) & 1, do_crc = (plan.crc_mask >> lane) & 1;
	const uint32_t clock = (lane + plan.clock_offset) & 63;
	uint32_t dis;
	const uint32_t hdr = header_fec13(s.w, dis);
	int header_rv = 0, payload_rv = 0;
	if (do_try)
		header_rv = (int)do_try_clock(s, clock, hdr, dis);
	if (do_crc)
		payload_rv = do_crc_check<true>(s, clock);
	wrote[lane] = s.written;
	__syncthreads();

	// scalar fields: the highest lane that assigned them
	const int l_ut = last_lane(s.dirty & D_UT), l_plen = last_lane(s.dirty & D_PLEN), l_phl = last_lane(s.dirty & D_PHL);
	const int l_lf = last_lane(s.dirty & D_LF), l_ph8 = last_lane(s.ph_mask & 0xff), l_ph16 = last_lane(s.ph_mask & 0xff00);
	const int l_try = last_lane(do_try), l_crc = last_lane(do_crc);
	const uint32_t f_uap = l_ut >= 0 ? (uint32_t)__shfl((int)s.uap, l_ut) : pi.uap;
	const uint32_t f_type = l_ut >= 0 ? (uint32_t)__shfl((int)s.type, l_ut) : pi.type;
	const int f_plen = l_plen >= 0 ? __shfl(s.plen, l_plen) : o->payload_length;
	const int f_phl = l_phl >= 0 ? __shfl(s.phl, l_phl) : o->payload_header_length;
	const uint32_t f_llid = l_lf >= 0 ? (uint32_t)__shfl((int)s.llid, l_lf) : pi.llid;
	const uint32_t f_flow = l_lf >= 0 ? (uint32_t)__shfl((int)s.flow, l_lf) : pi.flow;
	uint32_t f_ph = (uint32_t)o->payload_header;
	if (l_ph8 >= 0)
		f_ph = (f_ph & ~0xffu) | ((uint32_t)__shfl((int)s.ph16, l_ph8) & 0xffu);
	if (l_ph16 >= 0)
		f_ph = (f_ph & ~0xff00u) | ((uint32_t)__shfl((int)s.ph16, l_ph16) & 0xff00u);
	uint32_t f_flags = s.flags & ~entry_flags;                  // bits this trial added (HAS_PAYLOAD)
	for (int d = 32; d; d >>= 1)
		f_flags |= (uint32_t)__shfl_xor((int)f_flags, d);
	f_flags |= entry_flags;
	const int f_hrv = l_try >= 0 ? __shfl(header_rv, l_try) : 0;
	const int f_prv = l_crc >= 0 ? __shfl(payload_rv, l_crc) : 0;

	// payload: word j takes, from the highest lane down, the bits that lane's prefix covers
	if (lane < 43) {
		// (merge_payload_word written out: through the call this kernel's instructions come out in another order, profiles/r08_packet)
		uint64_t word = o->payload[lane], undecided = ~0ULL;
		for (int k = 63; k >= 0 && undecided; k--) {
			const uint32_t w = wrote[k];
			if (w <= 64u * lane)
				continue;
			const uint32_t nb = w - 64u * lane;
			const uint64_t covers = (nb >= 64 ? ~0ULL : ((1ULL << nb) - 1)) & undecided;
			word = (word & ~covers) | (pay[k][lane] & covers);
			undecided &= ~covers;
		}
		o->payload[lane] = word;
	}
	if (lane == 0) {
		o->header_present = (uint8_t)do_header_present(s);
		o->header_rv = f_hrv;
		o->payload_rv = f_prv;
		o->payload_length = f_plen;
		o->payload_header_length = f_phl;
		o->flags = f_flags;
		o->type = (uint8_t)f_type;
		o->llid = (uint8_t)f_llid;
		o->flow = (uint8_t)f_flow;
		o->uap = (uint8_t)f_uap;
		o->payload_header = f_ph;
	}
}

// The same for btbb_uap_from_header in two steps, so that the 64 trials run once: step 1 runs every
// trial with its writes captured per lane (TrialState in global memory) and returns the
// {try_clock, type, crc_check} table; the host then eliminates candidates exactly like the
// reference and hands back which trials the reference would have executed; step 2 merges those.
struct TrialState {
	uint32_t dirty, ph16, ph_mask, flags_added, written;
	int32_t plen, phl;
	uint8_t uap, type, llid, flow;
	uint64_t payload[44];
};

__global__ __launch_bounds__(64) void trials_state_kernel(const uint8_t *sym, const btbbx_pkt_in *in,
							   const btbbx_pkt_out *o, TrialState *st, btbbx_trial *trials)
{
	// every workgroup packs the 3200 staged symbol bytes for itself (LDS): no separate pack launch
	__shared__ uint64_t packet[BTBBX_PKT_WORDS + 2];
	if (threadIdx.x < BTBBX_PKT_WORDS + 2)
		packet[threadIdx.x] = threadIdx.x < BTBBX_PKT_WORDS ? pack64(sym + 64 * threadIdx.x) : 0;
	// one workgroup per candidate clock: 64 waves on 64 CUs each run ONE trial (no divergence between
	// packet types inside a wave), so the latency of the call is that of the longest single trial
	// instead of the sum over all types a 64-lane wave would have to serialise
	chain_lds_init();
	if (threadIdx.x)
		return;
	const uint32_t lane = blockIdx.x;
	const btbbx_pkt_in pi = in[0];
	TrialState *me = st + lane;
	PState s;
	s.w = packet;
	s.length = (int)pi.length;
	pstate_enter(s, pi);
	pstate_from_head(s, o);
	s.out = me->payload;
	for (int j = 0; j < 44; j++)
		me->payload[j] = 0;
	uint32_t dis;
	const uint32_t hdr = header_fec13(s.w, dis);
	const uint32_t uap = do_try_clock(s, lane, hdr, dis);
	const int rv = do_crc_check<true>(s, lane);
	btbbx_trial t;
	t.uap = (uint8_t)uap;
	t.type = (uint8_t)s.type;
	t.rv = (int16_t)rv;
	trials[lane] = t;
	me->dirty = s.dirty;
	me->ph16 = s.ph16;
	me->ph_mask = s.ph_mask;
	me->flags_added = s.flags & ~pi.flags;
	me->written = s.written;
	me->plen = s.plen;
	me->phl = s.phl;
	me->uap = (uint8_t)s.uap;
	me->type = (uint8_t)s.type;
	me->llid = (uint8_t)s.llid;
	me->flow = (uint8_t)s.flow;
}

// lane = candidate count; the trial it stands for ran with clock (count + clock_offset) & 63
__global__ __launch_bounds__(64) void trials_merge_kernel(const TrialState *st, const btbbx_pkt_in *in, btbbx_pkt_out *o,
							   uint8_t *pay, TrialPlan plan)
{
	__shared__ uint32_t wrote[64];
	__shared__ uint32_t src_of[64];
	const uint32_t lane = threadIdx.x;
	const btbbx_pkt_in pi = in[0];
	const TrialState *me = st + ((lane + plan.clock_offset) & 63);
	const bool did_try = (plan.try_mask >> lane) & 1, did_crc = (plan.crc_mask >> lane) & 1;
	const uint32_t dirty = (did_try ? me->dirty & D_UT : 0u) | (did_crc ? me->dirty & ~D_UT : 0u);
	const uint32_t ph_mask = did_crc ? me->ph_mask : 0u;
	wrote[lane] = did_crc ? me->written : 0u;
	src_of[lane] = (lane + plan.clock_offset) & 63;
	__syncthreads();
	const int l_ut = last_lane(dirty & D_UT), l_plen = last_lane(dirty & D_PLEN), l_phl = last_lane(dirty & D_PHL);
	const int l_lf = last_lane(dirty & D_LF), l_ph8 = last_lane(ph_mask & 0xff), l_ph16 = last_lane(ph_mask & 0xff00);
	uint32_t f_flags = did_crc ? me->flags_added : 0u;
	for (int d = 32; d; d >>= 1)
		f_flags |= (uint32_t)__shfl_xor((int)f_flags, d);
	if (lane < 43) {
		// entry payload bits come in, and the merged ones go out, one per byte (`pay`, 2752 bytes)
		const uint64_t word = merge_payload_word(pack64(pay + 64 * lane), lane, wrote, [&](int k) { return st[src_of[k]].payload[lane]; });
		o->payload[lane] = word;
		for (int k = 0; k < 64; k += 4)
			*reinterpret_cast<uint32_t *>(pay + 64 * lane + k) = (((uint32_t)(word >> k) & 0xf) * 0x00204081u) & 0x01010101u;
	}
	if (lane == 0) {
		auto at = [&](int l) { return st + ((l + plan.clock_offset) & 63); };
		if (l_ut >= 0) { o->uap = at(l_ut)->uap; o->type = at(l_ut)->type; } else { o->uap = pi.uap; o->type = pi.type; }
		if (l_plen >= 0) o->payload_length = at(l_plen)->plen;
		if (l_phl >= 0) o->payload_header_length = at(l_phl)->phl;
		if (l_lf >= 0) { o->llid = at(l_lf)->llid; o->flow = at(l_lf)->flow; } else { o->llid = pi.llid; o->flow = pi.flow; }
		uint32_t ph = (uint32_t)o->payload_header;
		if (l_ph8 >= 0) ph = (ph & ~0xffu) | (at(l_ph8)->ph16 & 0xffu);
		if (l_ph16 >= 0) ph = (ph & ~0xff00u) | (at(l_ph16)->ph16 & 0xff00u);
		o->payload_header = ph;
		o->flags = pi.flags | f_flags;
		o->header_rv = 0;
		o->payload_rv = 0;
	}
}
