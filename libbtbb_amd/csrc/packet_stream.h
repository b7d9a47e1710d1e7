// packet_stream.h -- piece of packet.hip: decode_view (btbb_decode_header :1198 + btbb_decode_payload :1223 of one packet), decode_kernel,
// and the stream decoder decode_hits_kernel with its lane-group payload phases (long_payloads, dh_payloads, ev_payloads).
#pragma once

// mode bits of decode_kernel (packet_obj.h):
//   DEC_HEADER   btbb_decode_header
//   DEC_PAYLOAD  btbb_decode_payload (after a successful header when DEC_HEADER is set)
// (DEC_TRIALS -- leave the packet as a set of try_clock / crc_check calls leaves it -- is
//  replay_kernel / trials_state_kernel + trials_merge_kernel below)

#ifdef DH_PROFILE
__device__ unsigned long long g_dh_prof[8];
#define DH_MARK(k) do { uint64_t now_; __builtin_amdgcn_sched_barrier(0); asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(now_) : : "memory"); \
	__builtin_amdgcn_sched_barrier(0); dh_acc[k] += (uint32_t)(now_ - dh_t); dh_t = now_; } while (0)
#define DH_PARAMS , uint32_t *dh_acc, uint64_t &dh_t
#define DH_PASS , dh_acc, dh_t
#else
#define DH_MARK(k) do { } while (0)
#define DH_PARAMS
#define DH_PASS
#endif
// header_present + decode_header / decode_payload of one packet (w = its 50 packed words)
// `s` arrives with its view of the packet set (w, length and, for a packet read straight from the stream, sh /
// wlimit / direct); everything else of the entry state comes from pi and *o
__device__ __forceinline__ void decode_view(PState &s, const btbbx_pkt_in &pi, btbbx_pkt_out *o, uint32_t mode,
					    OutRef pay_out, uint64_t *head_out, const uint64_t *head_in DH_PARAMS)
{
	pstate_enter(s, pi);
	// The fixed part of btbbx_pkt_out (40 bytes in front of the payload words) is read and written as FIVE 8-byte
	// words: a lane per packet means every vector memory instruction touches 64 different sectors, and the address
	// unit works those off one by one -- twenty field-sized accesses per packet were most of decode_hits_kernel's time.
	static_assert(offsetof(btbbx_pkt_out, payload) == 40 && offsetof(btbbx_pkt_out, payload_header) == 32, "head of btbbx_pkt_out");
	union Head {
		uint64_t q[5];
		struct {
			int32_t header_rv, payload_rv, payload_length, payload_header_length;
			uint32_t flags, header_packed;
			uint8_t header_present, type, lt_addr, hdr_flags, hec, llid, flow, uap;
			uint64_t payload_header;
		} f;
	} hd;
	{
		const uint64_t *src = head_in ? head_in : reinterpret_cast<const uint64_t *>(o);
#pragma unroll
		for (int k = 0; k < 5; k++)
			hd.q[k] = src[k];
	}
	pstate_from_head(s, hd.f.payload_length, hd.f.payload_header_length, (uint32_t)hd.f.payload_header, hd.f.lt_addr, hd.f.hdr_flags, hd.f.hec,
			 hd.f.header_packed);
	s.out = (pay_out.l || pay_out.g) ? pay_out : OutRef(o->payload);

	int header_rv = 0, payload_rv = 0;
	DH_MARK(3);
	uint32_t hraw, hdis;
	if (s.has_pre) {
		hraw = s.pre_hdr;
		hdis = s.pre_dis;
	} else {
		hraw = header_fec13(s, hdis);
	}
	hd.f.header_present = (uint8_t)do_header_present(s, hdis);
	DH_MARK(4);

	{
		bool go = true;
		if (mode & DEC_HEADER) {
			// btbb_decode_header (:1198-1221)
			const uint32_t dis = hdis, hdr = hraw;
			go = false;
			if ((s.flags & F_CLK6_VALID) && dis < 4) {
				uint32_t clear = hdr ^ (uint32_t)wh(s, wh_start(pi.clkn, 0), 18);
				s.header18 = clear;
				uint32_t hec = clear >> 10;
				if (uap_from_hec(clear & 0x3ff, hec) == s.uap) {
					s.lt_addr = clear & 7;
					s.type = (clear >> 3) & 0xf;
					s.hdr_flags = (clear >> 7) & 7;
					s.hec = hec;
					header_rv = 1;
					go = true;
				}
			}
		}
		DH_MARK(5);
		if ((mode & DEC_PAYLOAD) && go) {
			// btbb_decode_payload (:1223-1297)
			uint32_t clock = pi.clkn;
			s.phl = 0;
			switch (s.type) {
			case 0: case 1: s.plen = 0; payload_rv = 1; break;
			case 2:  payload_rv = do_fhs<true>(s, clock); break;
			case 3: case 8: case 10: case 14: payload_rv = do_DM<true>(s, clock); break;
			case 4: case 9: case 11: case 15: payload_rv = do_DH<true>(s, clock); break;
			case 5: case 6: payload_rv = do_HV<true>(s, clock); break;
			case 7:
				payload_rv = do_EV35<true>(s, clock, 32);
				if (payload_rv <= 1)
					payload_rv = do_HV<true>(s, clock);
				break;
			case 12: case 13: {
				// EV4 / EV5 into HBM: the lane-group phase (payload_length and the verdict come from ev_payloads)
				const uint32_t size = s.length - 122u, unit = s.type == 12 ? 15u : 8u;
				if (s.def_slot && !s.out.l && s.length >= 122u + unit) {
					const uint32_t most = s.type == 12 ? 98u : 182u, units = size / unit < most ? size / unit : most;
					defer_payload(s, clock, (s.type == 12 ? 10u : 8u) * units, s.type == 12 ? DHL_EV4 : DHL_EV5);
					payload_rv = 2;
				} else {
					payload_rv = s.type == 12 ? do_EV4<true>(s, clock) : do_EV35<true>(s, clock, 182);
				}
				break;
			}
			}
			s.flags |= F_HAS_PAYLOAD;
		}
	}
	DH_MARK(6);
	hd.f.header_rv = header_rv;
	hd.f.payload_rv = payload_rv;
	hd.f.payload_length = s.plen;
	hd.f.payload_header_length = s.phl;
	hd.f.flags = s.flags;
	hd.f.header_packed = s.header18;
	hd.f.type = (uint8_t)s.type;
	hd.f.lt_addr = (uint8_t)s.lt_addr;
	hd.f.hdr_flags = (uint8_t)s.hdr_flags;
	hd.f.hec = (uint8_t)s.hec;
	hd.f.llid = (uint8_t)s.llid;
	hd.f.flow = (uint8_t)s.flow;
	hd.f.uap = (uint8_t)s.uap;
	hd.f.payload_header = s.ph16;
	{
		uint64_t *dst = head_out ? head_out : reinterpret_cast<uint64_t *>(o);
#pragma unroll
		for (int k = 0; k < 5; k++)
			dst[k] = hd.q[k];
	}
}

__device__ void decode_one(const uint64_t *w, const btbbx_pkt_in &pi, btbbx_pkt_out *o, uint32_t mode)
{
	PState s;
	s.w = w;
	s.length = (int)pi.length;
#ifdef DH_PROFILE
	uint32_t dh_acc[8];
	uint64_t dh_t = 0;
#endif
	decode_view(s, pi, o, mode, OutRef(), nullptr, nullptr DH_PASS);
}

__global__ __launch_bounds__(64) void decode_kernel(const uint64_t *packets, const btbbx_pkt_in *in,
						     uint32_t n_packets, btbbx_pkt_out *outs, uint32_t mode)
{
	chain_lds_init();
	uint32_t pkt = blockIdx.x * blockDim.x + threadIdx.x;
	if (pkt >= n_packets)
		return;
	decode_one(packets + (uint64_t)pkt * BTBBX_PKT_WORDS, in[pkt], outs + pkt, mode);
}

// Decode straight from the packed streams: what gather_kernel + decode_kernel do, without the 400-byte row that
// the first writes and the second reads back (profiles/r02_v4/pmc_secondary.json: the two moved 2.0 GB per
// 1.29 M packets, of which the packets themselves are 0.5 GB).  One lane per hit; the captured length is the
// gather's: min(max_length, 3125, symbols left in the stream), and d_in[i].length is ignored.
//
// A lane walking its packet word by word from HBM fetched 753 B per packet for ~300 needed (every 8-byte read
// drags a 64-byte sector through the L2, profiles/traffic_secondary.json, round 2) and sat out a latency per step.
// The kernel's phases now (NOTEBOOK.md 3.4 has the numbers behind each):
//   A  every lane loads its hit and, in one batch, words 1 .. 4 of its packet; from those it decodes the header and
//      the payload header under its clock: the packet's type and EXACTLY how many symbols its decoder will read
//   B  the workgroup's 256 packets change hands (counting sort on decoder and length): one decoder per wave
//   C  the wave copies its 64 packets into LDS (global_load_lds, a dozen instructions in flight together)
//   D  one lane per packet decodes from LDS; payloads of up to 256 bits go to a per-lane LDS copy of the record
//   E  the wave stores head + payload of packet after packet as consecutive words (one 64-byte sector for most)
// s_bits() takes words the staging did not cover (DH_STAGE_WORDS per wave) from the stream as before, so the extents
// only decide where a word comes from, never what it is.
#define DH_STAGE_WORDS 384u                  // LDS words per wave for staged packets (3 KiB; 4 waves per workgroup)
__device__ __forceinline__ uint32_t symbols_of_type(uint32_t type)
{
	// 122 symbols of access code + trailer + header, then the longest payload of the type (FEC 2/3: 15 symbols per
	// 10 bits): bluetooth_packet.c:771-1196.  Single-slot types 366, three-slot 1626, five-slot the whole capture.
	if (type == 10 || type == 11 || type == 12 || type == 13)
		return 1626;
	if (type == 14 || type == 15)
		return BTBBX_MAX_SYMBOLS;
	return 366;
}

// which payload decoder a type runs (decode_view's switch)
__device__ __forceinline__ uint32_t decoder_of_type(uint32_t type)
{
	// 0 none, 1 FHS, 2 DM, 3 DH, 4 HV, 5 EV3 (+ HV), 6 EV4, 7 EV5: a nibble per type
	return (uint32_t)(0x3276323254432100ULL >> (4 * type)) & 0xf;
}
#define DH_OUT_WORDS 4u                      // payload words per lane that leave through LDS
#define DH_OUT_SECTOR 3u                     // ... of which these share the 64-byte sector of the record's head
// How many symbols of the packet the payload decoder of `type` will look at under this clock, and whether what it
// writes fits DH_OUT_WORDS words (small; wide: it needs the last of them, which lies in the record's second sector).
// DM / DH / AUX1 / DV carry their length in the payload header (do_payload_header, the
// decoders' own first step, on a scratch copy of the state): a DM3 with twelve bytes in it is 6 words of stream, not
// the 26 its type could have -- with the type's bound alone a wave with sixteen DM3 in it ran out of its LDS stage
// and half its lanes read their packets from HBM word by word.  An estimate that is too small only sends s_bits() to
// the stream for the rest; it never changes what is read.
__device__ __forceinline__ uint32_t payload_extent(const PState &s0, uint32_t type, uint32_t clock, bool &small, bool &wide)
{
	bool fec = false;
	int header_bytes = 2;
	uint32_t pos = 122;
	switch (type) {
	case 3:  fec = true; header_bytes = 1; break;
	case 8:  fec = true; header_bytes = 1; pos = 202; break;
	case 10: case 14: fec = true; break;
	case 4: case 9: header_bytes = 1; break;
	case 11: case 15: break;
	default: {
		// payload bits the other single-slot decoders write at most: nothing for NULL / POLL, FHS 160, HV1 80,
		// HV2 160, HV3 240 (type 7 tries EV3 first: 256); EV4 / EV5 run over several slots
		const uint32_t bits = (0x85300500u >> (4 * (type & 7)) & 0xf) * 32u;   // (rounded up to 32; types >= 8 never get here as small)
		small = type < 8 && bits <= 64 * DH_OUT_WORDS;
		wide = small && bits > 64 * DH_OUT_SECTOR;
		return symbols_of_type(type);
	}
	}
	PState s = s0;
	pstate_blank_out(s);
	s.type = type;
	small = true;
	wide = false;
	if (!do_payload_header<false>(s, pos, clock, header_bytes, s.length - (int)pos, fec))
		return pos + 30;
	const uint32_t nbits = (uint32_t)s.plen * 8;
	small = nbits <= 64 * DH_OUT_WORDS;
	wide = small && nbits > 64 * DH_OUT_SECTOR;
	return pos + (fec ? 15 * ((nbits + 9) / 10) : nbits);
}

// ---- long payloads: a group of lanes per packet ---------------------------------------------------------------------
// A lane that walks a DM3 / DH3 / DM5 / DH5 payload alone reads one stream word and writes one record word per step,
// each a sector of its own, one latency after the other: 1.4 - 3.5 ms per 1.29 M full-length packets against 0.13 - 0.15
// for the single-slot types (profiles/r03_chain/decode_by_type.txt).  do_DM / do_DH therefore stop after their checks
// when the payload has more than DHL_MIN_BITS bits, EV4 / EV5 before their loops (PState::def_nbits, defer_payload), and
// the wave works those packets off together, a group of G lanes per packet, 64 / G packets per round:
//   long_payloads   DM and DH, TWO payload words per lane, G = 8 / 16 / 32 (the workgroup sort keeps packets of one G
//                   together).  Per round, lane `sub` of a group
//     1. holds four stream words of its packet, requested one round ahead (a round's stores and loads all have a round's
//        worth of work to complete in: gfx9 counts both in one in-order counter);
//     2. DH (:962-1011): payload words 2 sub, 2 sub + 1 are funnel shifts of three of them.  DM (:898-958): the words go
//        to LDS (zeroed at and behind the captured length when a block reaches there: the reference reads zeros), FOUR
//        consecutive blocks of the (15,10) code per lane and step are decoded from LDS and their 40 bits ORed into the
//        packed payload in LDS (two ds_or: they start on a byte); one failing block anywhere in the packet and nothing
//        is written (rv 0), as in the reference;
//     3. unwhitens its words with the whitening bits from (start + 64 j) mod 127 and cuts at payload_length;
//     4. CRC (:671-690, :772-781): the register is GF(2)-linear; a seed is the same as its bits XORed onto the first
//        sixteen message bits; zero bits appended to a message advance the register by an invertible map, so "register
//        == 0" can be tested on the payload padded to whole words; and with A = "advance by one bit" the register after
//        n words is an invertible map applied to the XOR over the words of A^(-64 j) (register of word j alone).  So
//        every lane runs its own two words from a zero register (four four-byte steps), applies the FIXED matrix
//        A^(-128 sub) -- sixteen 16-bit columns per lane from g_adv64inv, loaded once per wave -- and the group XORs:
//        zero <=> the reference's compare of the computed with the received CRC succeeds.  No lane needs another lane's
//        word, whatever the payload length;
//     5. stores its words (344 contiguous bytes for a DH5; the last word keeps the record's bits behind the payload).
//   dh_payloads     a wave with DH payloads only: the same without step 2's LDS, THREE words per lane, G = 8 / 16.
//   ev_payloads     EV4 (:1044-1097) / EV5 (:1099-1128), one word per lane: the payload ends at the first byte count whose
//                   CRC register is zero -- a prefix of registers over the lanes.
// tests/_wave_model.py is the numpy model of the CRC steps (pinned against the oracle on the CPU).
// two LDS areas per wave (in decode_hits_kernel: its input stage and its result stage, both free by then):
#define DHL_STG_WORDS 288u                   // `stg`: the round's DM packets as they lie in the stream: 4 G (+ G / 4 + 1: LDS banks) words per group
#define DHL_LIST   0u                        // `lst`: 64 x 2 words: what the owner lanes know about their deferred packets
#define DHL_PB     128u                      //        128 words: decoded FEC 2/3 bits, packed, 2 G words per group
#define DHL_LST_WORDS 256u
struct __attribute__((packed, aligned(8))) dhl_pair_t { uint64_t a, b; };    // two payload words of a record: one 16-byte store
typedef __attribute__((address_space(3))) uint64_t dhl_u64_t;
typedef __attribute__((address_space(3))) uint32_t dhl_u32_t;
typedef const __attribute__((address_space(1))) uint64_t dhl_g64_t;

// XOR over the 2^logg lanes of a group (3 <= logg <= 6), every lane gets the result
__device__ __forceinline__ uint32_t group_xor(uint32_t x, uint32_t logg)
{
	x ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0xB1, 0xf, 0xf, true);      // quad_perm [1,0,3,2]
	x ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x4E, 0xf, 0xf, true);      // quad_perm [2,3,0,1]
	x ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x141, 0xf, 0xf, true);     // row_half_mirror: the other quad of eight
	if (logg > 3)
		x ^= (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x140, 0xf, 0xf, true); // row_mirror: the other eight of sixteen
	if (logg > 4)
		x ^= (uint32_t)__shfl_xor((int)x, 16);
	if (logg > 5)
		x ^= (uint32_t)__shfl_xor((int)x, 32);
	return x;
}

// the register after the matrix whose columns are the sixteen 16-bit halves of c[0..7]: per pair of register bits
// two sign-extending bit-field extracts, one byte permute that joins their low / high halves, one and-xor
__device__ __forceinline__ uint32_t apply_columns(const uint32_t (&c)[8], uint32_t reg)
{
	uint32_t x = 0;
#pragma unroll
	for (int k = 0; k < 8; k++) {
		const uint32_t m0 = (uint32_t)__builtin_amdgcn_sbfe((int)reg, 2 * k, 1), m1 = (uint32_t)__builtin_amdgcn_sbfe((int)reg, 2 * k + 1, 1);
		x ^= c[k] & __builtin_amdgcn_perm(m1, m0, 0x07060100u);
	}
	return (x ^ (x >> 16)) & 0xffffu;
}

// All 64 lanes of a wave; the wave's n_def DH / DM list entries are in LDS (lst[DHL_LIST ..]).  `stg` = DHL_STG_WORDS words
// of LDS of this wave, `lst` = DHL_LST_WORDS more; `outs` = the records of the workgroup of decode_hits_kernel that
// deferred the packets.
__device__ __forceinline__ void long_payloads(dhl_u64_t *stg, dhl_u64_t *lst, uint32_t n_def, uint32_t logg, btbbx_pkt_out *outs, uint32_t lane)
{
	dhl_u32_t *const stg32 = (dhl_u32_t *)stg, *const lst32 = (dhl_u32_t *)lst;
	const uint32_t G = 1u << logg, R = 64u >> logg;
	const uint32_t sub = lane & (G - 1), grp = lane >> logg, gbase = grp << logg;
	const uint64_t gmask = (1ULL << G) - 1;                     // (G <= 32: 43 words at two per lane)
	lst[DHL_PB + 2 * lane] = 0;
	lst[DHL_PB + 2 * lane + 1] = 0;
	// this lane's matrix: sixteen columns of A^(-128 sub)
	uint32_t col[8];
	{
		const uint4 *src = reinterpret_cast<const uint4 *>(g_adv64inv) + 4 * sub;
		const uint4 a = src[0], b = src[1];
		col[0] = a.x; col[1] = a.y; col[2] = a.z; col[3] = a.w; col[4] = b.x; col[5] = b.y; col[6] = b.z; col[7] = b.w;
	}
	// a group's staged words: 4 G + G / 4 + 1 words apart, so that the groups' 15-bit reads fall into different LDS banks
	// (4 G words = a multiple of 256 bytes: every group on the same banks)
	const uint32_t stg_base = grp * (4u * G + (G >> 2) + 1u);
	for (uint32_t i = lane; i < DHL_STG_WORDS; i += 64)
		stg[i] = 0;
	const uint32_t wh_lane = (128u * sub) % 127u;              // whitening phase of word 2 sub relative to the payload's first bit
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
	const uint32_t rounds = (n_def + R - 1) >> (6 - logg);
	// the words of round r on their way: four stream words of the group's packet -- DH: the three that hold payload words
	// 2 sub and 2 sub + 1; DM: words sub, sub + G, sub + 2 G, sub + 3 G of the packet
	auto request = [&](uint32_t r, uint64_t (&w)[4]) {
		const uint32_t e = r * R + grp;
#pragma unroll
		for (int k = 0; k < 4; k++)
			w[k] = 0;
		if (e < n_def) {
			const uint64_t pa = lst[DHL_LIST + 2 * e], pb = lst[DHL_LIST + 2 * e + 1];
			dhl_g64_t *const src = (dhl_g64_t *)(uintptr_t)DEFER_SRC(pa);
			const uint32_t p_nw = DEFER_NW(pa), p_sh = DEFER_SH(pa);
			const bool p_fec = DEFER_KIND(pb) == DHL_DM;
			const uint32_t i0 = p_fec ? sub : 2u * sub + ((p_sh + 122u) >> 6), step = p_fec ? G : 1u;
#pragma unroll
			for (int k = 0; k < 4; k++) {
				const uint32_t i = i0 + (uint32_t)k * step;
				if (i < p_nw && (p_fec || k < 3))
					w[k] = src[i];
			}
		}
	};
	uint64_t nw[4];
	request(0, nw);
	// a round's words are stored at the start of the next round
	uint64_t st_val0 = 0, st_val1 = 0;
	uint32_t st_pkt = 0, st_n = 0;
	for (uint32_t r = 0; r < rounds; r++) {
		const uint32_t e = r * R + grp;
		const bool has = e < n_def;
		uint64_t pa = 0, pb = 0;
		if (has) {
			pa = lst[DHL_LIST + 2 * e];
			pb = lst[DHL_LIST + 2 * e + 1];
		}
		const uint32_t p_sh = DEFER_SH(pa);
		const uint32_t p_pkt = DEFER_PKT(pb), p_len = DEFER_LEN(pb), nbits = DEFER_NBITS(pb);
		const uint32_t kind = DEFER_KIND(pb), p_widx = DEFER_WIDX(pb), p_uap = DEFER_UAP(pb);
		const bool p_fec = has && kind == DHL_DM, p_wht = DEFER_WHITENED(pb);
		const uint32_t nblocks = (nbits + 9u) / 10u;
		const uint32_t T = nbits >> 6, nwp = (nbits + 63u) >> 6;
		// 2a. DH: payload words 2 sub, 2 sub + 1 are funnel shifts of the lane's three stream words
		// (computed by every lane, wanted or not: the one wait for the words asked for a round ago then sits here, on every
		// path, and the compiler needs no second one in front of the next request)
		const uint32_t sft = (p_sh + 122u) & 63u;
		uint64_t word0 = sft ? (nw[0] >> sft) | (nw[1] << (64u - sft)) : nw[0];
		uint64_t word1 = sft ? (nw[1] >> sft) | (nw[2] << (64u - sft)) : nw[1];
		if (!(has && kind == DHL_DH)) {
			word0 = 0;
			word1 = 0;
		}
		const uint64_t any_fec = __ballot(p_fec);
		bool fail = false;
		if (any_fec) {
			// the DM packets of the round into LDS, cut at the captured length when a block reaches behind it
			if (__ballot(p_fec && 122u + 15u * nblocks > p_len)) {
				const uint32_t valid = p_sh + p_len;                        // stream bits of the packet's words that are symbols of the capture
#pragma unroll
				for (int k = 0; k < 4; k++) {
					const uint32_t first = 64u * (sub + (uint32_t)k * G), h = valid > first ? valid - first : 0u;
					if (h < 64)
						nw[k] &= (1ULL << h) - 1;
				}
			}
#pragma unroll
			for (int k = 0; k < 4; k++)
				stg[stg_base + (uint32_t)k * G + sub] = nw[k];
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
			__builtin_amdgcn_wave_barrier();
			// 2b. DM: the (15,10) blocks of the packet
			// FOUR consecutive blocks per lane and step: 60 stream bits from three staged dwords (every read unconditional:
			// a lane without blocks reads the group's first words), four parity and four correction look-ups in flight
			// together, and the 40 payload bits start on a byte of the packed payload -- two ds_or, no branch.  Blocks behind
			// the packet's last are zeroed before they are decoded (zeros decode to zeros); bits of the last block behind
			// payload_length end in the partial last word, which step 3 cuts, or in a word no lane keeps.  (Two blocks per
			// lane and step, one ds_or pair each: 37 instructions per block against 14.)
			for (uint32_t n0 = 0; ; n0 += G) {
				const uint32_t n = n0 + sub;
				const bool on = p_fec && 4u * n < nblocks;
				if (!__ballot(on))
					break;
				const uint32_t left = nblocks - 4u * n, have = on ? (left < 4u ? left : 4u) : 0u;
				const uint32_t q = p_sh + 122u + 60u * n, i = 2u * stg_base + (on ? q >> 5 : 0u);
				const uint32_t w0 = stg32[i], w1 = stg32[i + 1], w2 = stg32[i + 2];
				const uint64_t vm = (1ULL << (15u * have)) - 1;
				const uint32_t x0 = __builtin_amdgcn_alignbit(w1, w0, q & 31u) & (uint32_t)vm;
				const uint32_t x1 = __builtin_amdgcn_alignbit(w2, w1, q & 31u) & (uint32_t)(vm >> 32);
				const uint32_t b2 = __builtin_amdgcn_alignbit(x1, x0, 30);
				uint32_t d0 = x0 & 0x3ffu, d1 = (x0 >> 15) & 0x3ffu, d2 = b2 & 0x3ffu, d3 = (x1 >> 13) & 0x3ffu;
				const uint32_t m0 = g_lds.fixm23[((x0 >> 10) & 31u) ^ g_lds.par23[d0]], m1 = g_lds.fixm23[((x0 >> 25) & 31u) ^ g_lds.par23[d1]];
				const uint32_t m2 = g_lds.fixm23[((b2 >> 10) & 31u) ^ g_lds.par23[d2]], m3 = g_lds.fixm23[((x1 >> 23) & 31u) ^ g_lds.par23[d3]];
				if ((m0 | m1 | m2 | m3) >> 15)
					fail = true;
				d0 ^= m0 & 0x3ffu;
				d1 ^= m1 & 0x3ffu;
				d2 ^= m2 & 0x3ffu;
				d3 ^= m3 & 0x3ffu;
				if (on) {
					const uint32_t byte = 5u * n, d = 2u * DHL_PB + 4u * gbase + (byte >> 2);
					// Bits behind payload_length never leave the group's packed area: at 128 bytes (1024 bits = exactly the sixteen
					// words of a group of eight lanes) the six spare bits of block 102 would otherwise be ORed into word 0 of the next
					// group's packet -- non-zero whenever that block is mis-corrected or the packet is noise.
					const uint32_t room = nbits - 40u * n;                  // > 0: 4 n < nblocks = ceil(nbits / 10)
					uint64_t dv = (uint64_t)(d3 >> 2) << 32 | (d0 | d1 << 10 | d2 << 20 | d3 << 30);
					if (room < 40u)
						dv &= (1ULL << room) - 1;
					const uint64_t v = dv << (8u * (byte & 3u));
					__hip_atomic_fetch_or(lst32 + d, (uint32_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
					__hip_atomic_fetch_or(lst32 + d + 1, (uint32_t)(v >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
				}
			}
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
			__builtin_amdgcn_wave_barrier();
			if (p_fec) {
				word0 = lst[DHL_PB + 2 * lane];
				word1 = lst[DHL_PB + 2 * lane + 1];
			}
			lst[DHL_PB + 2 * lane] = 0;                                 // the packed bits are consumed: ready for the next round
			lst[DHL_PB + 2 * lane + 1] = 0;
		}
		// the stream words are used up: the previous round's words go out, the next round's words are asked for, and the
		// lane that writes a partial last word asks for what the record holds there (used at the end of the round) --
		// all of it behind the last wait of this round for memory, in front of ~200 instructions that need none
		if (st_n == 2) {
			*reinterpret_cast<dhl_pair_t *>(outs[st_pkt].payload + 2 * sub) = dhl_pair_t{st_val0, st_val1};
		} else if (st_n == 1) {
			outs[st_pkt].payload[2 * sub] = st_val0;
		}
		if (r + 1 < rounds)
			request(r + 1, nw);
		const uint32_t j0 = 2u * sub;
		const bool act0 = has && j0 < nwp, act1 = has && j0 + 1u < nwp;
		const bool part = has && (T >> 1) == sub && (nbits & 63u);  // this lane holds the partial last word
		uint64_t oldw = 0;
		if (part)
			oldw = outs[p_pkt].payload[T];
		const uint64_t fail_mask = __ballot(fail);
		const bool group_fail = ((fail_mask >> gbase) & gmask) != 0;
		// 3. unwhitened, cut at the payload length
		uint64_t out0 = 0, out1 = 0;
		const uint64_t keep = (1ULL << (nbits & 63u)) - 1;          // (of the partial last word)
		if (act0) {
			uint32_t idx = p_widx + wh_lane;
			idx = idx >= 127u ? idx - 127u : idx;
			out0 = word0 ^ (p_wht ? wh_bits(idx, 64) : 0ULL);
			if (part && !(T & 1u))
				out0 &= keep;
			if (act1) {
				idx += 64u;
				idx = idx >= 127u ? idx - 127u : idx;
				out1 = word1 ^ (p_wht ? wh_bits(idx, 64) : 0ULL);
				if (part && (T & 1u))
					out1 &= keep;
			}
		}
		// 4. CRC: the lane's two words from a zero register (the seed's bits on the first sixteen of the payload), carried back
		// over the words in front of them
		const uint64_t cw = out0 ^ (sub == 0 ? (uint64_t)crc_seed(p_uap) : 0ULL);
		uint32_t reg = crc_word(crc_word(0, (uint32_t)cw), (uint32_t)(cw >> 32));
		reg = crc_word(crc_word(reg, (uint32_t)out1), (uint32_t)(out1 >> 32));
		const uint32_t total = group_xor(apply_columns(col, reg), logg);
		int rv = total == 0 ? 10 : 2;
		if (p_fec && group_fail)
			rv = 0;
		// 5. out (DM: nothing when a block failed)
		st_n = rv == 0 ? 0u : act1 ? 2u : act0 ? 1u : 0u;
		st_val0 = part && !(T & 1u) ? out0 | (oldw & ~keep) : out0;
		st_val1 = part && (T & 1u) ? out1 | (oldw & ~keep) : out1;
		st_pkt = p_pkt;
		if (has && sub == 0)
			outs[p_pkt].payload_rv = rv;                            // (decode_hits_kernel left a placeholder)
	}
	if (st_n == 2) {
		*reinterpret_cast<dhl_pair_t *>(outs[st_pkt].payload + 2 * sub) = dhl_pair_t{st_val0, st_val1};
	} else if (st_n == 1) {
		outs[st_pkt].payload[2 * sub] = st_val0;
	}
}

// A wave whose deferred payloads are all DH (no FEC 2/3: nothing goes through LDS but the list): THREE payload words per lane,
// G = 8 / 16 lanes per packet -- a DH5 takes 15 lanes of 16 and four share a round (two words per lane: 22 of 32, two per round),
// a DH3 eight of eight.  The steps are long_payloads' 1, 2a, 3, 4, 5 with the matrix A^(-192 sub); the lane's four stream words are
// what a DM lane stages, so the prefetch costs the same registers.
__device__ __forceinline__ void dh_payloads(dhl_u64_t *lst, uint32_t n_def, uint32_t logg, btbbx_pkt_out *outs, uint32_t lane)
{
	const uint32_t G = 1u << logg, R = 64u >> logg;
	const uint32_t sub = lane & (G - 1), grp = lane >> logg;
	uint32_t col[8];
	{
		const uint4 *src = reinterpret_cast<const uint4 *>(g_adv64inv) + 6 * sub;
		const uint4 a = src[0], b = src[1];
		col[0] = a.x; col[1] = a.y; col[2] = a.z; col[3] = a.w; col[4] = b.x; col[5] = b.y; col[6] = b.z; col[7] = b.w;
	}
	const uint32_t wh_lane = (192u * sub) % 127u;              // whitening phase of word 3 sub relative to the payload's first bit
	const uint32_t rounds = (n_def + R - 1) >> (6 - logg);
	auto request = [&](uint32_t r, uint64_t (&w)[4]) {
		const uint32_t e = r * R + grp;
#pragma unroll
		for (int k = 0; k < 4; k++)
			w[k] = 0;
		if (e < n_def) {
			const uint64_t pa = lst[DHL_LIST + 2 * e];
			dhl_g64_t *const src = (dhl_g64_t *)(uintptr_t)DEFER_SRC(pa);
			const uint32_t p_nw = DEFER_NW(pa), p_sh = DEFER_SH(pa);
			const uint32_t i0 = 3u * sub + ((p_sh + 122u) >> 6);
#pragma unroll
			for (int k = 0; k < 4; k++)
				if (i0 + (uint32_t)k < p_nw)
					w[k] = src[i0 + (uint32_t)k];
		}
	};
	uint64_t nw[4];
	request(0, nw);
	uint64_t st_val[3] = {0, 0, 0};
	uint32_t st_pkt = 0, st_n = 0;
	auto store = [&]() {
		uint64_t *const dst = outs[st_pkt].payload + 3 * sub;
		if (st_n >= 2)
			*reinterpret_cast<dhl_pair_t *>(dst) = dhl_pair_t{st_val[0], st_val[1]};
		else if (st_n == 1)
			dst[0] = st_val[0];
		if (st_n == 3)
			dst[2] = st_val[2];
	};
	for (uint32_t r = 0; r < rounds; r++) {
		const uint32_t e = r * R + grp;
		const bool has = e < n_def;
		uint64_t pa = 0, pb = 0;
		if (has) {
			pa = lst[DHL_LIST + 2 * e];
			pb = lst[DHL_LIST + 2 * e + 1];
		}
		const uint32_t p_sh = DEFER_SH(pa);
		const uint32_t p_pkt = DEFER_PKT(pb), nbits = DEFER_NBITS(pb);
		const uint32_t p_widx = DEFER_WIDX(pb), p_uap = DEFER_UAP(pb);
		const bool p_wht = DEFER_WHITENED(pb);
		const uint32_t T = nbits >> 6, nwp = (nbits + 63u) >> 6;
		// the lane's three payload words: funnel shifts of its four stream words (by every lane, wanted or not: the round's one
		// wait for memory sits here)
		const uint32_t sft = (p_sh + 122u) & 63u;
		uint64_t word[3];
#pragma unroll
		for (int k = 0; k < 3; k++) {
			word[k] = sft ? (nw[k] >> sft) | (nw[k + 1] << (64u - sft)) : nw[k];
			if (!has)
				word[k] = 0;
		}
		store();
		if (r + 1 < rounds)
			request(r + 1, nw);
		const uint32_t j0 = 3u * sub, Tq = T / 3u, Tr = T - 3u * Tq;
		const bool part = has && Tq == sub && (nbits & 63u);        // this lane holds the partial last word
		uint64_t oldw = 0;
		if (part)
			oldw = outs[p_pkt].payload[T];
		const uint64_t keep = (1ULL << (nbits & 63u)) - 1;          // (of the partial last word)
		uint64_t out[3] = {0, 0, 0};
		uint32_t idx = p_widx + wh_lane;
		idx = idx >= 127u ? idx - 127u : idx;
		uint32_t n_act = 0;
#pragma unroll
		for (int k = 0; k < 3; k++) {
			if (has && j0 + (uint32_t)k < nwp) {
				out[k] = word[k] ^ (p_wht ? wh_bits(idx, 64) : 0ULL);
				if (part && Tr == (uint32_t)k)
					out[k] &= keep;
				n_act = (uint32_t)k + 1u;
			}
			idx += 64u;
			idx = idx >= 127u ? idx - 127u : idx;
		}
		const uint64_t cw = out[0] ^ (sub == 0 ? (uint64_t)crc_seed(p_uap) : 0ULL);
		uint32_t reg = crc_word(crc_word(0, (uint32_t)cw), (uint32_t)(cw >> 32));
		reg = crc_word(crc_word(reg, (uint32_t)out[1]), (uint32_t)(out[1] >> 32));
		reg = crc_word(crc_word(reg, (uint32_t)out[2]), (uint32_t)(out[2] >> 32));
		const uint32_t total = group_xor(apply_columns(col, reg), logg);
		st_n = n_act;
#pragma unroll
		for (int k = 0; k < 3; k++)
			st_val[k] = part && Tr == (uint32_t)k ? out[k] | (oldw & ~keep) : out[k];
		st_pkt = p_pkt;
		if (has && sub == 0)
			outs[p_pkt].payload_rv = total == 0 ? 10 : 2;           // (decode_hits_kernel left a placeholder)
	}
	store();
}

// EV4 (:1044-1097) and EV5 (:1099-1128) payloads of a wave, in a loop of their own (rare types; and what they keep in
// registers -- two more matrices, a prefix over the lanes, eight registers per word -- stays out of long_payloads, whose
// allocation decides the occupancy of decode_hits_kernel).  n_ev list entries from DHL_LIST + 2 first on; G = 8 .. 32 lanes
// per packet, one per payload word.  The first byte count L whose CRC register is zero ends the payload:
//   register in front of word `sub` = A^(64 sub) applied to the XOR over the words j in front of it of A^(-64 (j + 1))
//   (register of word j alone)  -- a per-lane matrix, a plain XOR prefix over the lanes, a per-lane matrix --,
// then the lane's eight bytes one by one, a zero register noted per byte; the lowest lane with a noted byte decides.
// A round's stream words are asked for one round ahead; the record's old last word is read where the length is known.
__device__ __forceinline__ void ev_payloads(dhl_u64_t *stg, dhl_u64_t *lst, uint32_t first, uint32_t n_ev, uint32_t logg, btbbx_pkt_out *outs, uint32_t lane)
{
	dhl_u32_t *const stg32 = (dhl_u32_t *)stg, *const lst32 = (dhl_u32_t *)lst;
	const uint32_t G = 1u << logg, R = 64u >> logg;
	const uint32_t sub = lane & (G - 1), grp = lane >> logg, gbase = grp << logg;
	const uint64_t gmask = (1ULL << G) - 1;                     // (G <= 32: an EV payload has at most 23 words)
	lst[DHL_PB + lane] = 0;
	if (lane < 2)
		stg[128 + lane] = 0;
	const uint32_t wh_lane = (64u * sub) % 127u;
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
	__builtin_amdgcn_wave_barrier();
	const uint32_t rounds = (n_ev + R - 1) >> (6 - logg);
	// this lane's two matrices: A^(-64 (sub + 1)) and A^(64 sub), sixteen 16-bit columns each
	uint32_t rinv[8], rfwd[8];
	{
		const uint4 *si = reinterpret_cast<const uint4 *>(g_adv64inv) + 2 * (sub + 1), *sf = reinterpret_cast<const uint4 *>(g_adv64fwd) + 2 * sub;
		const uint4 a = si[0], b = si[1], c = sf[0], d = sf[1];
		rinv[0] = a.x; rinv[1] = a.y; rinv[2] = a.z; rinv[3] = a.w; rinv[4] = b.x; rinv[5] = b.y; rinv[6] = b.z; rinv[7] = b.w;
		rfwd[0] = c.x; rfwd[1] = c.y; rfwd[2] = c.z; rfwd[3] = c.w; rfwd[4] = d.x; rfwd[5] = d.y; rfwd[6] = d.z; rfwd[7] = d.w;
	}
	// the stream words of round r: EV4 words sub and sub + G of the packet (its blocks all lie inside the capture:
	// min(98, size / 15)); EV5 reads ONE byte, every payload byte is the first one under the whitening of its place
	auto request = [&](uint32_t r, uint64_t &w0, uint64_t &w1) {
		const uint32_t e = r * R + grp;
		w0 = 0;
		w1 = 0;
		if (e < n_ev) {
			const uint64_t pa = lst[DHL_LIST + 2 * (first + e)], pb = lst[DHL_LIST + 2 * (first + e) + 1];
			dhl_g64_t *const src = (dhl_g64_t *)(uintptr_t)DEFER_SRC(pa);
			const uint32_t p_nw = DEFER_NW(pa), p_sh = DEFER_SH(pa);
			const bool is4 = DEFER_KIND(pb) == DHL_EV4;
			const uint32_t i0 = is4 ? sub : (p_sh + 122u) >> 6, i1 = is4 ? sub + G : i0 + 1u;
			if (is4 || sub == 0) {
				if (i0 < p_nw)
					w0 = src[i0];
				if (i1 < p_nw)
					w1 = src[i1];
			}
		}
	};
	uint64_t nw0, nw1;
	request(0, nw0, nw1);
#pragma unroll 1
	for (uint32_t r = 0; r < rounds; r++) {
		const uint32_t e = r * R + grp;
		const bool has = e < n_ev;
		uint64_t pa = 0, pb = 0;
		if (has) {
			pa = lst[DHL_LIST + 2 * (first + e)];
			pb = lst[DHL_LIST + 2 * (first + e) + 1];
		}
		const uint32_t p_sh = DEFER_SH(pa);
		const uint32_t p_pkt = DEFER_PKT(pb), nbits = DEFER_NBITS(pb);
		const uint32_t kind = DEFER_KIND(pb), p_widx = DEFER_WIDX(pb), p_uap = DEFER_UAP(pb);
		const bool p_wht = DEFER_WHITENED(pb), is4 = has && kind == DHL_EV4;
		const uint32_t nblocks = nbits / 10u;                   // (EV4)
		// 1. the stream words asked for a round ago
		const uint64_t w0 = nw0, w1 = nw1;
		const uint32_t sft = (p_sh + 122u) & 63u;
		const uint32_t low8 = (uint32_t)(sft ? (w0 >> sft) | (w1 << (64u - sft)) : w0) & 0xffu;
		const uint32_t first8 = (uint32_t)__shfl((int)low8, (int)gbase);
		uint64_t word = (uint64_t)(first8 * 0x01010101u) | (uint64_t)(first8 * 0x01010101u) << 32;
		// 2. EV4: the (15,10) blocks, as in long_payloads -- and which block is the first that does not decode
		uint32_t first_fail = nblocks;
		if (__ballot(is4)) {
			stg[2 * gbase + sub] = w0;
			stg[2 * gbase + G + sub] = w1;
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
			__builtin_amdgcn_wave_barrier();
			// (four consecutive blocks per lane and step, as in long_payloads)
			for (uint32_t n0 = 0; ; n0 += G) {
				const uint32_t n = n0 + sub;
				const bool on = is4 && 4u * n < nblocks;
				if (!__ballot(on))
					break;
				const uint32_t left = nblocks - 4u * n, have = on ? (left < 4u ? left : 4u) : 0u;
				const uint32_t q = p_sh + 122u + 60u * n, i = 4u * gbase + (on ? q >> 5 : 0u);
				const uint32_t v0 = stg32[i], v1 = stg32[i + 1], v2 = stg32[i + 2];
				const uint64_t vm = (1ULL << (15u * have)) - 1;
				const uint32_t x0 = __builtin_amdgcn_alignbit(v1, v0, q & 31u) & (uint32_t)vm;
				const uint32_t x1 = __builtin_amdgcn_alignbit(v2, v1, q & 31u) & (uint32_t)(vm >> 32);
				const uint32_t b2 = __builtin_amdgcn_alignbit(x1, x0, 30);
				uint32_t d0 = x0 & 0x3ffu, d1 = (x0 >> 15) & 0x3ffu, d2 = b2 & 0x3ffu, d3 = (x1 >> 13) & 0x3ffu;
				const uint32_t m0 = g_lds.fixm23[((x0 >> 10) & 31u) ^ g_lds.par23[d0]], m1 = g_lds.fixm23[((x0 >> 25) & 31u) ^ g_lds.par23[d1]];
				const uint32_t m2 = g_lds.fixm23[((b2 >> 10) & 31u) ^ g_lds.par23[d2]], m3 = g_lds.fixm23[((x1 >> 23) & 31u) ^ g_lds.par23[d3]];
				const uint32_t bad = (m0 >> 15) | (m1 >> 15) << 1 | (m2 >> 15) << 2 | (m3 >> 15) << 3;  // which of the four do not decode
				d0 ^= m0 & 0x3ffu;
				d1 ^= m1 & 0x3ffu;
				d2 ^= m2 & 0x3ffu;
				d3 ^= m3 & 0x3ffu;
				if (on) {
					const uint32_t byte = 5u * n, d = 2u * DHL_PB + 2u * gbase + (byte >> 2);
					const uint64_t v = ((uint64_t)(d3 >> 2) << 32 | (d0 | d1 << 10 | d2 << 20 | d3 << 30)) << (8u * (byte & 3u));
					__hip_atomic_fetch_or(lst32 + d, (uint32_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
					__hip_atomic_fetch_or(lst32 + d + 1, (uint32_t)(v >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
				}
				const uint64_t gm = (__ballot(bad != 0) >> gbase) & gmask;
				const uint32_t gl = gm ? (uint32_t)__builtin_ctzll(gm) : 0u;
				const uint32_t gb = (uint32_t)__shfl((int)bad, (int)(gbase + gl));
				if (gm && first_fail == nblocks)
					first_fail = 4u * (n0 + gl) + (uint32_t)__builtin_ctz(gb | 16u);
			}
			__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
			__builtin_amdgcn_wave_barrier();
			if (is4)
				word = lst[DHL_PB + lane];
			lst[DHL_PB + lane] = 0;
		}
		if (r + 1 < rounds)
			request(r + 1, nw0, nw1);
		// 3. unwhitened, cut at the bits the decoder may look at
		const uint32_t T = nbits >> 6;
		const bool active = has && 64u * sub < nbits;
		uint64_t out = 0;
		if (active) {
			uint32_t idx = p_widx + wh_lane;
			idx = idx >= 127u ? idx - 127u : idx;
			out = word ^ (p_wht ? wh_bits(idx, 64) : 0ULL);
			if (sub == T)
				out &= (1ULL << (nbits & 63u)) - 1;
		}
		// 4. the register in front of this lane's word
		uint32_t reg;
		{
			const uint64_t cw = out ^ (sub == 0 ? (uint64_t)crc_seed(p_uap) : 0ULL);
			const uint32_t reg0 = crc_word(crc_word(0, (uint32_t)cw), (uint32_t)(cw >> 32));
			const uint32_t q = apply_columns(rinv, reg0);
			uint32_t x = q, t;                                      // inclusive XOR prefix over the lanes of the group
			t = (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x111, 0xf, 0xf, true); x ^= sub >= 1 ? t : 0u;      // row_shr:1
			t = (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x112, 0xf, 0xf, true); x ^= sub >= 2 ? t : 0u;
			t = (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x114, 0xf, 0xf, true); x ^= sub >= 4 ? t : 0u;
			if (logg > 3) {
				t = (uint32_t)__builtin_amdgcn_mov_dpp((int)x, 0x118, 0xf, 0xf, true); x ^= sub >= 8 ? t : 0u;
			}
			if (logg > 4) {                                         // the second sixteen of a group of 32: + the first sixteen's total
				t = (uint32_t)__shfl((int)x, (int)(gbase + 15));
				x ^= sub >= 16 ? t : 0u;
			}
			reg = apply_columns(rfwd, x ^ q);
		}
		// 5. byte by byte; which byte counts may end the payload: EV4 2 .. 5 (blocks that decoded - 1) / 4 (byte L - 1 is looked
		// at by the loop's step b when 8 L <= 10 b), EV5 3 .. bytes - 1
		const uint32_t ok_blocks = first_fail < nblocks ? first_fail : nblocks;
		const uint32_t hi = is4 ? (ok_blocks ? 5u * (ok_blocks - 1u) / 4u : 0u) : (nbits >> 3) - 1u, lo = is4 ? 2u : 3u;
		uint32_t zero = 0;
#pragma unroll
		for (int i = 0; i < 8; i++) {
			uint32_t byte = (uint32_t)(out >> (8 * i)) & 0xffu;
			if (i == 1 && sub == 0)
				byte ^= crc_seed(p_uap) >> 8;                       // (the seed sits on bits 8 .. 15 of the first word)
			reg = crc_byte(reg, byte);
			const uint32_t L = 8u * sub + (uint32_t)i + 1u;
			if (reg == 0 && L >= lo && L <= hi)
				zero |= 1u << i;
		}
		const uint64_t hm = (__ballot(has && zero != 0) >> gbase) & gmask;
		const uint32_t hl = hm ? (uint32_t)__builtin_ctzll(hm) : 0u;
		const uint32_t hz = (uint32_t)__shfl((int)zero, (int)(gbase + hl));
		const uint32_t L_hit = hm ? 8u * hl + (uint32_t)__builtin_ctz(hz | 0x100u) + 1u : 0u;
		// 6. length, verdict, and the bits the decoder wrote before it stopped
		if (has) {
			uint32_t plen, wbits;
			int rv;
			if (is4) {
				if (L_hit) {
					rv = 10; plen = L_hit; wbits = 10u * ((8u * L_hit + 9u) / 10u + 1u);
				} else {
					plen = hi + 1u; wbits = 10u * ok_blocks;
					rv = ok_blocks == 98u ? 2 : first_fail < nblocks && first_fail < 3u ? 0 : 1;    // all 98 | stopped by an undecodable block in the first 45 symbols | later, or by the capture's end
				}
			} else {
				const uint32_t bytes = nbits >> 3;
				if (L_hit) {
					rv = 10; plen = L_hit; wbits = 8u * (L_hit + 1u);
				} else {
					plen = bytes; wbits = nbits; rv = bytes == 182u ? 2 : 1;
				}
			}
			const uint32_t wT = wbits >> 6, wrem = wbits & 63u;
			if (64u * sub < wbits) {
				uint64_t v = out;
				if (sub == wT) {                                        // (a partial last word keeps what the record held behind it)
					const uint64_t wm = (1ULL << wrem) - 1;
					v = (out & wm) | (outs[p_pkt].payload[sub] & ~wm);
				}
				outs[p_pkt].payload[sub] = v;
			}
			if (sub == 0) {
				outs[p_pkt].payload_length = (int32_t)plen;
				outs[p_pkt].payload_rv = rv;
			}
		}
	}
}

// The deferred payloads of one wave of decode_hits_kernel: dmask = which of its 64 list slots `slots` are filled
// (defer_payload).  DH / DM entries to the front of the LDS list, EV4 / EV5 behind them; lanes per packet = one per
// payload word of the longest payload of either kind (the sort of decode_hits_kernel keeps like with like).  `outs` = the
// records of that workgroup; all 64 lanes.
__device__ __forceinline__ void long_wave(dhl_u64_t *stg, dhl_u64_t *lst, const uint4 *slots, uint64_t dmask, btbbx_pkt_out *outs, uint32_t lane)
{
	const bool mine = (dmask >> lane) & 1;
	uint4 e = make_uint4(0, 0, 0, 0);
	if (mine)
		e = slots[lane];
	const bool ev = mine && DEFER_KIND_HI(e.w) >= DHL_EV4;
	const uint64_t ev_mask = __ballot(ev), dh_mask = dmask & ~ev_mask;
	const uint32_t n_dh = (uint32_t)__popcll(dh_mask), n_ev = (uint32_t)__popcll(ev_mask);
	const uint32_t own_words = mine ? (DEFER_NBITS_LO(e.z) + 63u) >> 6 : 0u;
	if (mine) {
		const uint64_t among = ev ? ev_mask : dh_mask;
		const uint32_t rank = (ev ? n_dh : 0u) + __builtin_amdgcn_mbcnt_hi((uint32_t)(among >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)among, 0u));
		lst[DHL_LIST + 2 * rank] = (uint64_t)e.x | (uint64_t)e.y << 32;
		lst[DHL_LIST + 2 * rank + 1] = (uint64_t)e.z | (uint64_t)e.w << 32;
	}
	if (n_dh) {
		const uint32_t w = ev ? 0u : own_words;
		if (__ballot(mine && !ev && DEFER_KIND_HI(e.w) == DHL_DM)) {    // (two payload words per lane)
			const uint32_t logg = __ballot(w > 32) ? 5u : __ballot(w > 16) ? 4u : 3u;
			long_payloads(stg, lst, n_dh, logg, outs, lane);
		} else {                                                // DH only: three
			dh_payloads(lst, n_dh, __ballot(w > 24) ? 4u : 3u, outs, lane);
		}
	}
	if (n_ev) {
		const uint32_t w = ev ? own_words : 0u;
		const uint32_t logg = __ballot(w > 16) ? 5u : __ballot(w > 8) ? 4u : 3u;
		ev_payloads(stg, lst, n_dh, n_ev, logg, outs, lane);
	}
}

#define DH_WAVES_PER_EU 6
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DH_WAVES_PER_EU, DH_WAVES_PER_EU)))
void decode_hits_kernel(const uint64_t *words, uint64_t n_words, uint64_t pitch_words,
							  const btbbx_hit *hits, const btbbx_pkt_in *in, uint32_t n_packets,
							  const uint32_t *d_count, uint32_t max_length, btbbx_pkt_out *outs,
							  uint32_t *lengths, uint32_t mode, btbbx_pkt_in one_in, uint32_t clk_div,
							  uint4 *long_list)
{
	__shared__ uint64_t stage[4][DH_STAGE_WORDS];
	__shared__ uint64_t ostage[4][64 * DH_OUT_WORDS];
	chain_lds_init();
	uint32_t pkt = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	if (d_count)                                        // the list's length lives in HBM (no host round trip): n_packets is its capacity
		n_packets = min(n_packets, *d_count);
	bool live = pkt < n_packets;
	if (blockIdx.x * blockDim.x >= n_packets)
		return;
#ifdef DH_PROFILE
	uint32_t dh_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	uint64_t dh_t;
	asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(dh_t) : : "memory");
#endif
	btbbx_hit h;
	h.offset = 0;
	h.stream = 0;
	if (live)
		h = hits[pkt];
	const uint64_t total_bits = n_words * 64;
	const uint64_t avail = h.offset < total_bits ? total_bits - h.offset : 0;
	uint32_t len = avail < max_length ? (uint32_t)avail : max_length;
	if (len > BTBBX_MAX_SYMBOLS)
		len = BTBBX_MAX_SYMBOLS;
	const uint64_t first_word = h.offset >> 6;
	PState s;
	s.w = words + (uint64_t)h.stream * pitch_words + first_word;
	s.sh = (uint32_t)(h.offset & 63);
	s.wlimit = first_word < n_words ? (uint32_t)(n_words - first_word < 64 ? n_words - first_word : 64) : 0;
	s.direct = true;
	s.length = live ? (int)len : 0;
	btbbx_pkt_in pi;
	pi.length = 0; pi.clkn = 0; pi.flags = 0; pi.uap = 0; pi.type = 0; pi.llid = 0; pi.flow = 0;
	if (live) {
		if (in) {
			pi = in[pkt];
		} else {
			// a capture of one piconet: every packet enters with the same state, its clock follows from where it was found
			// (CLK1-27 advances once per clk_div symbols: 625 at 1 Msym/s)
			// (one_in.length = the symbols of the current slot that had already passed at the buffer's first symbol)
			pi = one_in;
			const uint64_t since = h.offset + one_in.length;
			pi.clkn = one_in.clkn + (since >> 32 ? (uint32_t)(since / clk_div) : (uint32_t)since / clk_div);
		}
	}
	pi.length = len;

	asm volatile("" : "+v"(pi.clkn), "+v"(len));
	DH_MARK(0);                                         // hit + btbbx_pkt_in loaded
	// how much of the packet the decoders can want: the type the header yields under this packet's clock
	uint32_t want = 0, dtype = 0;
	bool small = false, wide = false;                   // its payload fits DH_OUT_WORDS words / needs more than DH_OUT_SECTOR
	uint32_t hdr = 0, dis = 0;
	typedef __attribute__((address_space(3))) uint64_t lds_u64_t;
	{
		// the header and the payload header (symbols 68 .. 232 of the packet) are in its words 1 .. 4: four loads in
		// flight together, parked in the input stage, instead of one s_bits() after the other going to the stream
		uint64_t hw[4];
#pragma unroll
		for (uint32_t k = 0; k < 4; k++)
			hw[k] = live && k + 1 < s.wlimit ? s.w[k + 1] : 0ULL;
#pragma unroll
		for (uint32_t k = 0; k < 4; k++)
			stage[wave][lane * 5 + k + 1] = hw[k];
		s.staged = s.wlimit < 5 ? s.wlimit : 5;
		s.stage_off = (uint32_t)(uintptr_t)(lds_u64_t *)(&stage[wave][lane * 5]);
	}
	if (live) {
		want = len < 126 ? len : 126;
		s.flags = pi.flags;
		hdr = header_fec13(s, dis);
		if ((mode & DEC_PAYLOAD) && len > 126) {
			uint32_t type = pi.type;
			if (mode & DEC_HEADER)
				type = ((hdr ^ (uint32_t)wh(s, wh_start(pi.clkn, 0), 18)) >> 3) & 0xf;
			const uint32_t bound = payload_extent(s, type, pi.clkn, small, wide);
			want = len < bound ? len : bound;
			dtype = type;
		}
	}
	asm volatile("" : "+v"(want));
	s.staged = 0;
	if (live && lengths)
		lengths[pkt] = len;
	// The workgroup's 256 packets change hands so that a wave decodes packets of one kind and about one length: a wave
	// with DM, DH and FHS packets in it runs the three decoders one after the other with a third of its lanes each,
	// and a loop over FEC blocks runs as long as its longest packet.  (With the stores, the staging and the exact
	// extents fixed the kernel issues vector instructions 68 % of the time, profiles/r03_chain/pmc_decode_mid.json;
	// while it sat in s_waitcnt the same sort gained nothing.)  Counting sort on (decoder, symbols wanted); what a
	// thread knows about its packet goes to the thread that takes it over through the input stage, which is still empty.
	{
		// (the counters and the permutation live in ostage, which nothing uses before the sort is over)
		uint32_t *const sort_cnt = reinterpret_cast<uint32_t *>(&ostage[0][0]);
		uint8_t *const perm = reinterpret_cast<uint8_t *>(&ostage[0][32]);
		uint64_t *const xch = &stage[0][0];
		const uint32_t tid = threadIdx.x;
		if (tid < 64)
			sort_cnt[tid] = 0;
		__syncthreads();
		uint32_t key = 63;
		if (live) {
			const uint32_t cls = want <= 126 ? 0 : decoder_of_type(dtype);
			const uint32_t lb = want <= 126 ? 0 : (want - 122) >> 5;
			key = cls * 8 + (lb < 7 ? lb : 7);
			// payloads that go to the wave phase (long_payloads): together, by the lanes a packet takes there (keys that
			// are all but unused otherwise: class 0 has one length, HV packets that are not cut short another)
			if (!small && want > 126 && (cls == 2 || cls == 3)) {
				const uint32_t pbits = cls == 2 ? (want - 122) / 15 * 10 : want - 122, words = (pbits + 63) >> 6;   // (about: the grouping only)
				key = cls == 2 ? 32u + (words > 32 ? 2u : words > 16 ? 1u : 0u)          // (DM, two words per lane: groups of 32 / 16 / 8)
					       : 1u + (words > 24 ? 1u : 0u);                                // (DH, three: 16 / 8)
			}
		}
		const uint32_t r = atomicAdd(&sort_cnt[key], 1u);
		xch[tid] = h.offset;
		xch[256 + tid] = (uint64_t)h.stream | (uint64_t)want << 16 | (uint64_t)wide << 28 | (uint64_t)small << 30 | (uint64_t)live << 31 | (uint64_t)pi.clkn << 32;
		xch[512 + tid] = (uint64_t)pi.flags | (uint64_t)pi.uap << 32 | (uint64_t)pi.type << 40 | (uint64_t)pi.llid << 48 | (uint64_t)pi.flow << 56;
		xch[768 + tid] = (uint64_t)hdr | (uint64_t)dtype << 24 | (uint64_t)dis << 32;
		__syncthreads();
		// (the scan of wave_scan.h, written out: as a call this kernel comes out with other code, profiles/r08_packet)
		uint32_t c = sort_cnt[lane], incl = c;
		for (int d = 1; d < 64; d <<= 1) {
			const uint32_t u = __shfl_up(incl, d);
			if (lane >= (uint32_t)d)
				incl += u;
		}
		perm[__shfl(incl - c, key) + r] = (uint8_t)tid;
		__syncthreads();
		const uint32_t q = perm[tid];
		const uint64_t x0 = xch[q], x1 = xch[256 + q], x2 = xch[512 + q], x3 = xch[768 + q];
		__syncthreads();                                // the stage is free again
		pkt = blockIdx.x * blockDim.x + q;
		h.offset = x0;
		h.stream = (uint16_t)x1;
		want = (uint32_t)(x1 >> 16) & 0xfff;            // <= 3125
		wide = (x1 >> 28) & 1;
		small = (x1 >> 30) & 1;
		live = (x1 >> 31) & 1;
		pi.clkn = (uint32_t)(x1 >> 32);
		pi.flags = (uint32_t)x2;
		pi.uap = (uint8_t)(x2 >> 32); pi.type = (uint8_t)(x2 >> 40); pi.llid = (uint8_t)(x2 >> 48); pi.flow = (uint8_t)(x2 >> 56);
		const uint64_t avail2 = h.offset < total_bits ? total_bits - h.offset : 0;
		len = avail2 < max_length ? (uint32_t)avail2 : max_length;
		if (len > BTBBX_MAX_SYMBOLS)
			len = BTBBX_MAX_SYMBOLS;
		const uint64_t fw = h.offset >> 6;
		s.w = words + (uint64_t)h.stream * pitch_words + fw;
		s.sh = (uint32_t)(h.offset & 63);
		s.wlimit = fw < n_words ? (uint32_t)(n_words - fw < 64 ? n_words - fw : 64) : 0;
		s.length = live ? (int)len : 0;
		pi.length = len;
		hdr = (uint32_t)x3 & 0x3ffffu;
		dtype = (uint32_t)(x3 >> 24) & 0xfu;
		dis = (uint32_t)(x3 >> 32);
	}
	s.has_pre = true;
	s.pre_hdr = hdr;
	s.pre_dis = dis;
	DH_MARK(1);                                         // header read from the stream, type known
	// Results leave through LDS.  A lane storing its own packet's words touches 64 different sectors per instruction
	// (the phase after the decoders was 29 % of the wave time, 6 % now).  The payload words of a packet that writes
	// <= 256 bits (FHS 160, DM1 / DH1 / AUX1 / DV <= 240, HV 240, EV3 256, short multi-slot packets) are collected in
	// ostage, the head in the input stage once every lane is done reading it, and the wave stores head + payload of
	// packet after packet as consecutive words.  ostage starts from what the record holds, so bits the decoders leave
	// alone stay.  Head + three payload words = the record's first 64-byte sector; the fourth word (`wide` packets
	// only) is in the second.
	const uint64_t small_mask = __ballot(small), wide_mask = __ballot(wide), live_mask = __ballot(live);
	// the record's head (entry state of the decoders): on its way while the packets are staged
	uint64_t head_in[5] = {0, 0, 0, 0, 0};
	if (live) {
#pragma unroll
		for (int k = 0; k < 5; k++)
			head_in[k] = reinterpret_cast<const uint64_t *>(outs + pkt)[k];
	}
	uint32_t nw = live ? (s.sh + want + 63) / 64 : 0;              // words of the stream that hold those symbols
	if (nw > s.wlimit)
		nw = s.wlimit;
	// a payload that will be left to the wave phase: its lane reads the header and the payload header, four words
	if (live && !small && want > 126 && nw > 4 && (decoder_of_type(dtype) == 2 || decoder_of_type(dtype) == 3))
		nw = 4;
	// LDS slots in lane order; a packet that does not fit the wave's budget any more stays in the stream
	// (the scan of wave_scan.h, written out: as a call this kernel comes out with other code, profiles/r08_packet)
	uint32_t before = nw;
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t t = __shfl_up(before, d);
		if (lane >= (uint32_t)d)
			before += t;
	}
	before -= nw;
	if (before + nw > DH_STAGE_WORDS)
		nw = 0;
	const uint32_t stage_base = (uint32_t)(uintptr_t)(lds_u64_t *)(&stage[wave][0]);
	// The words go from HBM to LDS without passing through registers (global_load_lds_dword: the wave's LDS base is
	// uniform, lane i fills dword i): packet j of the wave is one instruction -- lanes below twice its word count --
	// and all 64 packets' loads are in flight together, one HBM latency per wave.  (Round 3 first staged one packet at
	// a time through registers -- the wave sat out 64 latencies in a row, 80 % of its life in s_waitcnt,
	// profiles/r03_chain/pmc_decode_before.json -- then sixteen at a time, which cost 48 registers.)
	typedef __attribute__((address_space(3))) uint32_t lds_u32_t;
	typedef __attribute__((address_space(1))) const uint32_t glb_u32_t;
	{
		// what the records hold in the payload words the small packets will leave through ostage
		lds_u32_t *const obase = (lds_u32_t *)(lds_u64_t *)(&ostage[wave][0]);
#pragma unroll
		for (uint32_t t = 0; t < 2 * DH_OUT_WORDS; t++) {
			const uint32_t f = t * 64 + lane, p = f / (2 * DH_OUT_WORDS), k = f % (2 * DH_OUT_WORDS);
			const uint32_t pkt_p = __shfl(pkt, p);
			if (((small_mask >> p) & 1) && (k < 2 * DH_OUT_SECTOR || ((wide_mask >> p) & 1)))
				__builtin_amdgcn_global_load_lds((glb_u32_t *)(uintptr_t)(reinterpret_cast<const uint32_t *>(outs + pkt_p) + 10 + k),
								 obase + t * 64, 4, 0, 0);
		}
	}
	{
		// The staged packets lie back to back in the wave's stage, so the stage is one run of dwords and instruction
		// i fills dwords 64 i .. 64 i + 63 of it, whichever packets they belong to: every packet first writes its lane
		// number into the slots it will get, the lane that loads dword D reads the owner from there and takes the
		// owner's stream address.  (One instruction per packet was 64 rounds of readlanes and compares: 820 of the
		// kernel's 2 700 vector instructions per wave.)
		lds_u32_t *const sbase = (lds_u32_t *)(lds_u64_t *)(&stage[wave][0]);
		const uint64_t staged_mask = __ballot(nw > 0);
		const uint32_t last = staged_mask ? 63u - (uint32_t)__builtin_clzll(staged_mask) : 0u;
		const uint32_t total2 = staged_mask ? 2u * (uint32_t)__builtin_amdgcn_readlane(before + nw, last) : 0u;
		for (uint32_t k = 0; __ballot(k < nw); k++)
			if (k < nw)
				sbase[2 * (before + k)] = lane;
		const uint64_t adj = (uint64_t)(uintptr_t)s.w - 8ull * before;        // dword D of the stage is at adj + 4 D
		for (uint32_t d0 = 0; d0 < total2; d0 += 64) {
			const uint32_t d = d0 + lane;
			const uint32_t owner = d < total2 ? sbase[d & ~1u] : 0u;
			const uint64_t a = __shfl(adj, owner) + 4ull * d;            // (every lane takes part in the shuffle)
			if (d < total2)
				__builtin_amdgcn_global_load_lds((glb_u32_t *)(uintptr_t)a, sbase + d0, 4, 0, 0);
		}
	}
	asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
	__builtin_amdgcn_wave_barrier();
	s.staged = nw;
	s.stage_off = stage_base + 8u * before;
	DH_MARK(2);                                         // packets staged

	uint64_t head[5] = {0, 0, 0, 0, 0};
	if (long_list) {
		s.def_slot = long_list + ((size_t)(blockIdx.x * 4 + wave) * 64 + lane);
		s.def_pkt8 = pkt - blockIdx.x * blockDim.x;
	}
	if (live)
		decode_view(s, pi, outs + pkt, mode,
			    small ? OutRef::lds((uint32_t)(uintptr_t)(lds_u64_t *)(&ostage[wave][lane * DH_OUT_WORDS])) : OutRef(), head, head_in DH_PASS);
	__builtin_amdgcn_wave_barrier();                    // every lane is done with the staged packets
	// which of the wave's 64 list slots hold a payload that was left for later (do_DM / do_DH, defer_payload)
	const uint64_t long_mask = long_list ? __ballot(live && s.def_nbits != 0) : 0ULL;
	const uint64_t keep_mask = __ballot(small && !s.spoiled);
#pragma unroll
	for (int k = 0; k < 5; k++)
		stage[wave][lane * 5 + k] = head[k];
	__builtin_amdgcn_wave_barrier();
#pragma unroll
	for (uint32_t t = 0; t < 5 + DH_OUT_WORDS; t++) {
		const uint32_t f = t * 64 + lane, p = f / (5 + DH_OUT_WORDS), k = f % (5 + DH_OUT_WORDS);
		const uint32_t pkt_p = __shfl(pkt, p);
		if ((live_mask >> p) & 1) {
			uint64_t *dst = reinterpret_cast<uint64_t *>(outs + pkt_p);
			if (k < 5)
				dst[k] = stage[wave][p * 5 + k];
			else if (((keep_mask >> p) & 1) && (k - 5 < DH_OUT_SECTOR || ((wide_mask >> p) & 1)))
				dst[k] = ostage[wave][p * DH_OUT_WORDS + k - 5];
		}
	}
	DH_MARK(7);                                         // decoded, results stored
	if (__builtin_expect(long_mask != 0, 0)) {
		// The payloads the lanes left alone, a group of lanes per packet (long_payloads), in the wave's input stage: behind
		// the store phase, when nothing of the lanes' decoders is alive any more.  Fused into this kernel rather than run
		// as a kernel of its own behind it (round 4 measured both): the phase is bound by instruction issue, the lanes' phases by latency -- waves
		// in the one fill the gaps of waves in the other (DH5 at full length: 497 against 562 us per 1.29 M packets).  What
		// is known about a packet comes back from the list its lane wrote (defer_payload): 16 bytes, still in the L2.
		asm volatile("s_waitcnt vmcnt(0)" : : : "memory");            // the list entries are written
		__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
		__builtin_amdgcn_wave_barrier();
		// (nothing of the lanes' phase is handed over in vector registers: lane number and wave number are made afresh, so no
		// value computed for the long phase is kept alive through the decoders)
		uint32_t lane2 = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
		asm volatile("" : "+v"(lane2));
		uint32_t wave2 = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
		asm volatile("" : "+s"(wave2));
		long_wave((dhl_u64_t *)(lds_u64_t *)(&stage[wave2][0]), (dhl_u64_t *)(lds_u64_t *)(&ostage[wave2][0]), long_list + (size_t)(blockIdx.x * 4 + wave2) * 64, long_mask,
			  outs + (size_t)blockIdx.x * blockDim.x, lane2);
	}
#ifdef DH_PROFILE
	if (lane == 0)
		for (int k = 0; k < 8; k++)
			atomicAdd(&g_dh_prof[k], (unsigned long long)dh_acc[k]);
#endif
}
