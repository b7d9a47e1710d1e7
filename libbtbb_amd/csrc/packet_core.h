// packet_core.h -- piece of packet.hip: the device tables, the bit / FEC / CRC primitives, the decoder state (PState, Sink) and
// the per-type decoders.  Restates unfec13, unfec23, unwhiten, crcgen, uap_from_hec, try_clock, crc_check, fhs .. HV and
// btbb_header_present of lib/src/bluetooth_packet.c (lines at each function).
#pragma once
#include "defer_entry.h"

__constant__ ChainTables g_chain;

// Per-workgroup LDS copies of the small tables the decoders index with per-lane values inside
// their inner loops (whitening slice, CRC byte / word step, FEC 2/3 parity and correction): a DS read
// instead of a divergent constant-memory load or a 10-step loop.  4.6 KiB, copied by
// chain_lds_init() at kernel start from the image chain_upload() built on the host.
struct __attribute__((aligned(16))) ChainLds {
	uint32_t wh32[128];        // 32 whitening bits from phase idx (idx <= 126)
	uint16_t crc[256];         // crc_byte(0, x): one byte through the reflected CRC-CCITT register
	uint16_t crc_z[3][256];    // the same followed by 1, 2, 3 zero bytes (slicing: four bytes per step)
	uint8_t  par23[1024];      // FEC 2/3 parity of 10 data bits
	int8_t   fix23[32];
	uint16_t fixm23[32];       // the same as a mask: the data bit to flip, 0x8000 = undecodable (long_payloads)
	uint8_t  whiten_idx[64];
	uint16_t adv32[2][256];    // the CRC register 32 zero bytes later, by its low / high byte (linear: XOR the two)
};
// the image every workgroup copies (built once on the host in chain_upload)
__device__ __attribute__((aligned(16))) ChainLds g_chain_lds_image;

// Table of trials_linear_kernel.  The CRC register is GF(2)-linear in seed, data and whitening, the seed has
// eight free bits (the UAP, bits 8..15) and the whitening sequence from any phase is the GF(2) combination of
// seven basis sequences selected by its own first seven bits (a 7-stage LFSR).  Row L (payload length in
// bytes) holds what each of those fifteen bits contributes to the register after L bytes:
//   [0..7]  register after L zero bytes from the seed with only bit 8 + b set
//   [8..14] register after the first L bytes of the whitening sequence whose first seven bits are unit vector j
//   [15]    0
#define LIN_MAXLEN 344                      // payload lengths 0 .. 343 (DH5)
__device__ __attribute__((aligned(16))) uint16_t g_lin[LIN_MAXLEN * 16];
// g_advw[i - 1][h][x]: the CRC register 4 i zero bytes after holding x in its low (h = 0) / high (h = 1) byte,
// i = 1 .. 7 (linear: XOR the two halves) -- what carries a chunk's start register to a word inside the chunk
__device__ __attribute__((aligned(16))) uint16_t g_advw[7 * 2 * 256];
// g_adv64inv[j][k]: the CRC register that holds 1 << k after 64 j zero bits -- the matrix A^(-64 j) by columns (A = one
// zero bit through the register: invertible), what lane j of the long-payload phase of decode_hits_kernel applies to the
// register of payload word j alone
__device__ __attribute__((aligned(16))) uint16_t g_adv64inv[64 * 16];
// g_adv64fwd[j][k]: the register 64 j zero bits AFTER holding 1 << k -- A^(+64 j): carries the XOR the lanes of an EV4 / EV5
// payload have accumulated in front of word j back into the true register in front of that word
__device__ __attribute__((aligned(16))) uint16_t g_adv64fwd[64 * 16];

#define F_WHITENED    (1u << 0)
#define F_CLK6_VALID  (1u << 4)
#define F_HAS_PAYLOAD (1u << 7)
#define DHL_MIN_BITS  256              // payloads longer than this leave decode_hits_kernel's lanes for its wave phase (= 64 DH_OUT_WORDS)

// ---- bit helpers ----------------------------------------------------------------------------

// n (1..64) bits of the packet starting at symbol pos; pos + n <= 3200
__device__ __forceinline__ uint64_t pk_bits(const uint64_t *w, uint32_t pos, uint32_t n)
{
	uint32_t i = pos >> 6, s = pos & 63;
	uint64_t v = w[i] >> s;
	if (s + n > 64)
		v |= w[i + 1] << (64 - s);
	return n == 64 ? v : v & ((1ULL << n) - 1);
}

// the same for n <= 32 through two dword reads and one funnel shift (the 64-bit form costs two 8-byte reads, two
// 64-bit shifts and a 64-bit mask); pos + n <= 3200, so dword (pos >> 5) + 1 is still inside the 50-word row
__device__ __forceinline__ uint32_t pk_bits32(const uint64_t *w, uint32_t pos, uint32_t n)
{
	const uint32_t *d = reinterpret_cast<const uint32_t *>(w);
	const uint32_t i = pos >> 5;
	const uint32_t v = __builtin_amdgcn_alignbit(d[i + 1], d[i], pos & 31);
	return n == 32 ? v : v & ((1u << n) - 1);
}

// n (1..64) whitening bits starting at phase idx (0..126), straight from constant memory (used
// where a kernel needs a handful of them; the decoders below use the LDS copies)
__device__ __forceinline__ uint64_t wh_bits_const(uint32_t idx, uint32_t n)
{
	uint32_t i = idx >> 6, s = idx & 63;
	uint64_t v = g_chain.whiten2[i] >> s;
	if (s + n > 64)
		v |= g_chain.whiten2[i + 1] << (64 - s);
	return n == 64 ? v : v & ((1ULL << n) - 1);
}

__device__ __forceinline__ uint32_t wh_start_const(uint32_t clock, uint32_t skip)
{
	return (g_chain.whiten_idx[clock & 63] + skip) % 127u;
}

__shared__ ChainLds g_lds;

__device__ __forceinline__ uint64_t wh_bits(uint32_t idx, uint32_t n)
{
	uint64_t v = g_lds.wh32[idx];
	if (n > 32) {
		const uint32_t j = idx + 32;
		v |= (uint64_t)g_lds.wh32[j >= 127 ? j - 127 : j] << 32;
	}
	return n == 64 ? v : v & ((1ULL << n) - 1);
}

__device__ __forceinline__ uint32_t wh_start(uint32_t clock, uint32_t skip)
{
	return (g_lds.whiten_idx[clock & 63] + skip) % 127u;
}

__device__ __forceinline__ uint32_t rev8(uint32_t b) { return __brev(b) >> 24; }

// one byte through the reflected CRC-CCITT register of crcgen (:681-687)
__device__ __forceinline__ uint32_t crc_byte_calc(uint32_t crc, uint32_t byte)
{
	uint32_t x = (crc ^ byte) & 0xff;
	x ^= (x << 4) & 0xff;
	return ((crc >> 8) ^ (x << 8) ^ (x << 3) ^ (x >> 4)) & 0xffff;
}
// the same through the LDS table (the register update is linear: crc' = crc >> 8 ^ T[(crc ^ byte) & 0xff])
__device__ __forceinline__ uint32_t crc_byte(uint32_t crc, uint32_t byte)
{
	return (crc >> 8) ^ g_lds.crc[(crc ^ byte) & 0xff];
}

// Four bytes per step.  The register update is linear over GF(2) and the register is 16 bits wide, so
// after the bytes b0..b3 (b0 first) it holds
//     Z3[(crc ^ b0) & 0xff] ^ Z2[(crc >> 8) ^ b1] ^ Z1[b2] ^ Z0[b3],   Zk[x] = byte x followed by k zero bytes:
// four INDEPENDENT table reads instead of a chain of four dependent ones (the CRC over the 187 / 343 bytes
// of a DH3 / DH5 trial is what the brute force spends its time in, and it was bound by that latency).
__device__ __forceinline__ uint32_t crc_word(uint32_t crc, uint32_t w)
{
	const uint32_t x = crc ^ w;
	return g_lds.crc_z[2][x & 0xff] ^ g_lds.crc_z[1][(x >> 8) & 0xff] ^ g_lds.crc_z[0][(w >> 16) & 0xff] ^ g_lds.crc[w >> 24];
}

__device__ __forceinline__ uint32_t crc_seed(uint32_t uap) { return rev8(uap & 0xff) << 8; }

// uap_from_hec (:693-705)
__device__ __forceinline__ uint32_t uap_from_hec(uint32_t data, uint32_t hec)
{
#pragma unroll
	for (int i = 9; i >= 0; i--) {
		if (hec & 0x80)
			hec ^= 0x65;
		hec = ((hec << 1) | (((hec >> 7) ^ (data >> i)) & 1)) & 0xff;
	}
	return rev8(hec);
}

// FEC 1/3 of n <= 21 triples held in the low 3n bits of v: majority bits (compacted) and
// the number of triples that disagree (:552-568)
__device__ __forceinline__ uint32_t fec13(uint64_t v, uint32_t n, uint32_t &disagree)
{
	const uint64_t M = 0x9249249249249249ULL;          // every third bit
	uint64_t a = v & M, b = (v >> 1) & M, c = (v >> 2) & M;
	uint64_t maj = (a & b) | (b & c) | (c & a);
	uint64_t dis = (a ^ b) | (b ^ c) | (c ^ a);
	if (n < 21) {
		uint64_t keep = (1ULL << (3 * n)) - 1;
		maj &= keep;
		dis &= keep;
	}
	disagree = __popcll(dis);
	// bit 3 i -> bit i: pairs, nibbles, bytes, ... close ranks (five shift / or / and steps instead of n)
	uint64_t x = maj;
	x = (x | x >> 2) & 0x30c30c30c30c30c3ULL;
	x = (x | x >> 4) & 0xf00f00f00f00f00fULL;
	x = (x | x >> 8) & 0x00ff0000ff0000ffULL;
	x = (x | x >> 16) & 0xffff00000000ffffULL;
	x = (x | x >> 32) & 0xffffffffULL;
	return (uint32_t)x;
}

// one (15,10) block: 15 symbols in -> 10 corrected data bits, false if uncorrectable (:602-646)
__device__ __forceinline__ bool fec23_block(uint32_t blk, uint32_t &data)
{
	data = blk & 0x3ff;
	uint32_t diff = (blk >> 10) ^ g_lds.par23[data];
	int fix = g_lds.fix23[diff & 31];
	if (fix == -2)
		return false;
	if (fix >= 0)
		data ^= 1u << fix;
	return true;
}

// all threads of the workgroup; ends with a barrier
__device__ void chain_lds_init()
{
	static_assert(sizeof(ChainLds) % 16 == 0, "the image is copied 16 bytes at a time");
	const uint4 *src = reinterpret_cast<const uint4 *>(&g_chain_lds_image);
	uint4 *dst = reinterpret_cast<uint4 *>(&g_lds);
	for (uint32_t i = threadIdx.x; i < sizeof(ChainLds) / 16; i += blockDim.x)
		dst[i] = src[i];
	__syncthreads();
}

// ---- packet state -----------------------------------------------------------------------------

// Where a decoder's payload words go: HBM, or (decode_hits_kernel, small packets) the wave's LDS.  Two address spaces
// behind one generic pointer would make every access a FLAT instruction, which counts on both vmcnt and lgkmcnt: each
// table lookup behind a payload store then waits for the store to come back from the memory pipeline.
struct OutRef {
	uint64_t *g = nullptr;
	uint32_t l = 0;          // LDS byte address + 1, or 0
	__device__ OutRef() {}
	__device__ OutRef(uint64_t *p) : g(p) {}
	__device__ __forceinline__ static OutRef lds(uint32_t byte_address) { OutRef r; r.l = byte_address + 1; return r; }
	__device__ __forceinline__ uint64_t ld(uint32_t k) const
	{
		if (l)
			return *reinterpret_cast<const __attribute__((address_space(3))) uint64_t *>(l - 1 + 8u * k);
		return g[k];
	}
	__device__ __forceinline__ void st(uint32_t k, uint64_t v) const
	{
		if (l)
			*reinterpret_cast<__attribute__((address_space(3))) uint64_t *>(l - 1 + 8u * k) = v;
		else
			g[k] = v;
	}
};
struct PState {
	const uint64_t *w;       // 50 packed words (a gathered packet), or -- `direct` -- the stream word the packet starts in
	// direct mode (decode_hits_kernel): the packet is bits [sh, sh + length) of w[0 .. wlimit)
	uint32_t sh = 0;         // bit of w[0] the packet starts at
	uint32_t wlimit = 0;     // stream words that exist from w on
	uint32_t staged = 0;     // direct mode: w[0 .. staged) have a copy in LDS at LDS byte address `stage_off`
	uint32_t stage_off = 0;
	bool direct = false;
	// the FEC 1/3 decoded header and its disagreeing triples, when the caller has them already (decode_hits_kernel)
	bool has_pre = false;
	uint32_t pre_hdr = 0, pre_dis = 0;
	int length;              // pkt->length
	uint32_t flags;
	uint32_t uap, type;
	uint32_t lt_addr, hdr_flags, hec, header18;
	int plen;                // payload_length
	int phl;                 // payload_header_length
	uint32_t ph16;           // payload_header bits
	uint32_t ph_written;     // how many payload_header chars were written
	uint32_t llid, flow;
	// payload writer
	OutRef out;              // 43 words or nothing
	bool spoiled = false;    // out is the caller's scratch copy (LDS) and holds a payload the reference would not have written
	// decode_hits_kernel: a DM / DH payload of more than 256 bits is not walked by its lane; do_DM / do_DH return after
	// their checks with the bit count here and the wave works it off afterwards, a group of lanes per packet (long_payloads)
	// (long_wave, at the end of decode_hits_kernel); the sixteen bytes that phase needs to know go straight into def_slot from here
	uint4 *def_slot = nullptr;   // where (null: every payload is walked by its lane)
	uint32_t def_pkt8 = 0;       // the record's index in its workgroup's 256
	uint32_t def_nbits = 0;      // != 0: deferred
	uint32_t written;        // payload bits written (prefix)
	// which fields a trial assigned (replay_kernel merges 64 trials by "last writer wins")
	uint32_t dirty;          // D_* bits
	uint32_t ph_mask;        // payload-header bits assigned
};
#define D_UT    1u           // uap, type        (try_clock)
#define D_PLEN  2u           // payload_length
#define D_PHL   4u           // payload_header_length
#define D_LF    8u           // llid, flow

// The entry state of the decoders: the caller's fields of a btbbx_pkt_in, then what the packet object held before the call
// (the head of a btbbx_pkt_out; pstate_blank_out: nothing) with nothing assigned or written yet.  The view of the packet
// (w, length, sh, wlimit, direct, has_pre ...) and `out` are the caller's.
__device__ __forceinline__ void pstate_enter(PState &s, const btbbx_pkt_in &pi)
{
	s.flags = pi.flags;
	s.uap = pi.uap;
	s.type = pi.type;
	s.llid = pi.llid;
	s.flow = pi.flow;
}
__device__ __forceinline__ void pstate_from_head(PState &s, int plen, int phl, uint32_t ph16, uint32_t lt_addr, uint32_t hdr_flags,
						 uint32_t hec, uint32_t header18)
{
	s.plen = plen;
	s.phl = phl;
	s.ph16 = ph16;
	s.ph_written = 0;
	s.dirty = 0;
	s.ph_mask = 0;
	s.lt_addr = lt_addr; s.hdr_flags = hdr_flags; s.hec = hec; s.header18 = header18;
	s.written = 0;
}
__device__ __forceinline__ void pstate_from_head(PState &s, const btbbx_pkt_out *o)
{
	pstate_from_head(s, o->payload_length, o->payload_header_length, (uint32_t)o->payload_header, o->lt_addr, o->hdr_flags, o->hec, o->header_packed);
}
__device__ __forceinline__ void pstate_blank_out(PState &s) { pstate_from_head(s, 0, 0, 0, 0, 0, 0, 0); }

// n (1..64) symbols of the packet from symbol pos.  A gathered packet is 50 words with zeros behind the captured
// length; in direct mode the same view is taken of the stream itself: symbols at and behind `length` (which the
// reference's decoders do read, :898-958) and words behind the end of the stream read as 0.
__device__ __forceinline__ uint64_t s_bits(const PState &s, uint32_t pos, uint32_t n)
{
	if (!s.direct)
		return pk_bits(s.w, pos, n);
	if ((int)pos >= s.length)
		return 0;
	const uint32_t q = pos + s.sh, i = q >> 6, sft = q & 63;
	// words the wave staged through LDS (decode_hits_kernel) come from there, anything behind them from the stream
	auto word = [&](uint32_t k) -> uint64_t {
		if (k < s.staged)
			return *reinterpret_cast<const __attribute__((address_space(3))) uint64_t *>(s.stage_off + 8u * k);
		return k < s.wlimit ? ((const __attribute__((address_space(1))) uint64_t *)(uintptr_t)s.w)[k] : 0ULL;    // (direct mode: the stream in HBM)
	};
	uint64_t v = word(i) >> sft;
	if (sft + n > 64)
		v |= word(i + 1) << (64 - sft);
	const uint32_t have = (uint32_t)s.length - pos;         // symbols left in front of `length`
	const uint32_t keep = n < have ? n : have;
	return keep == 64 ? v : v & ((1ULL << keep) - 1);
}

// streams payload bits into the CRC (whole bytes) and, when WRITE, into the output words
template <bool WRITE>
struct Sink {
	uint64_t acc = 0;
	uint32_t nacc = 0;
	uint32_t crc;
	uint64_t oacc = 0;
	uint32_t onacc = 0, oword = 0;
	OutRef out;
	__device__ Sink(uint32_t seed, OutRef o) : crc(seed), out(o) {}
	__device__ __forceinline__ void push(uint64_t bits, uint32_t n)   // n <= 32
	{
		if (n == 32 && nacc == 0) {                                   // whole word on a byte boundary
			crc = crc_word(crc, (uint32_t)bits);
		} else {
			acc |= bits << nacc;
			nacc += n;
			while (nacc >= 8) {
				crc = crc_byte(crc, (uint32_t)acc & 0xff);
				acc >>= 8;
				nacc -= 8;
			}
		}
		if (WRITE) {
			oacc |= bits << onacc;
			onacc += n;
			if (onacc >= 64) {
				out.st(oword++, oacc);
				onacc -= 64;
				oacc = onacc ? bits >> (n - onacc) : 0;
			}
		}
	}
	// merge the unfinished word with what the output already holds
	__device__ __forceinline__ void flush()
	{
		if (WRITE && onacc) {
			uint64_t keep = ~0ULL << onacc;
			out.st(oword, (out.ld(oword) & keep) | oacc);
		}
	}
};

__device__ __forceinline__ bool whitened(const PState &s) { return s.flags & F_WHITENED; }

__device__ __forceinline__ uint64_t wh(const PState &s, uint32_t idx, uint32_t n)
{
	return whitened(s) ? wh_bits(idx, n) : 0ULL;
}

// Four consecutive (15,10) blocks from symbol `pos` on, their symbols and table reads issued together (a lane that decodes
// block after block waits for four dependent LDS round trips per block; decode_hits_kernel is bound by exactly those waits).
// ok bit j = block j decodes; blocks behind `count` are not looked at.
__device__ __forceinline__ uint32_t fec23_blocks4(const PState &s, uint32_t pos, uint32_t count, uint32_t (&data)[4])
{
	uint32_t blk[4], diff[4];
	const uint64_t sym60 = s_bits(s, pos, 60);             // (symbols behind `length` read as 0 either way)
#pragma unroll
	for (int j = 0; j < 4; j++)
		blk[j] = (uint32_t)j < count ? (uint32_t)(sym60 >> (15 * j)) & 0x7fff : 0;
#pragma unroll
	for (int j = 0; j < 4; j++) {
		data[j] = blk[j] & 0x3ff;
		diff[j] = (blk[j] >> 10) ^ g_lds.par23[data[j]];
	}
	uint32_t ok = 0;
#pragma unroll
	for (int j = 0; j < 4; j++) {
		const int fix = g_lds.fix23[diff[j] & 31];
		if (fix >= 0)
			data[j] ^= 1u << fix;
		if (fix != -2)
			ok |= 1u << j;
	}
	return ok;
}

// all FEC-2/3 blocks of `nblocks` decodable?
__device__ __forceinline__ bool fec23_ok(const PState &s, uint32_t pos, uint32_t nblocks)
{
	for (uint32_t k = 0; k < nblocks; k += 4) {
		uint32_t d[4];
		const uint32_t cnt = nblocks - k < 4 ? nblocks - k : 4;
		if ((fec23_blocks4(s, pos + 15 * k, cnt, d) & ((1u << cnt) - 1)) != (1u << cnt) - 1)
			return false;
	}
	return true;
}

// The payload of s is left to the lane-group phase (long_payloads): what that phase needs, sixteen bytes (defer_entry.h)
__device__ __forceinline__ void defer_payload(PState &s, uint32_t clock, uint32_t nbits, uint32_t kind)
{
	// stream words the decoder looks at: 122 symbols of access code and header, then the payload -- FEC 2/3 blocks may
	// lie behind the captured length (they read as zeros), never behind word 45; EV5 reads one byte; nothing
	// behind the stream's end is loaded
	const uint32_t ext = kind == DHL_DH ? nbits : kind == DHL_EV5 ? 8u : 15u * ((nbits + 9u) / 10u);
	const uint32_t nw = (s.sh + 122u + ext + 63u) >> 6;
	const uint64_t a = DEFER_PACK_A((uintptr_t)s.w, nw < s.wlimit ? nw : s.wlimit, s.sh);
	const uint64_t b = DEFER_PACK_B(s.def_pkt8, (uint32_t)s.length, nbits, kind, (s.flags & 1u) ? 1u : 0u, wh_start(clock, 18), s.uap & 0xffu);
	*s.def_slot = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
	s.def_nbits = nbits;
}

// The same for a caller that only looks at the register at the end (DM): bytes go through the CRC four at a time -- one
// step of four independent table reads instead of four dependent ones -- and finish() takes the last one to three.
template <bool WRITE>
struct SinkW : Sink<WRITE> {
	__device__ SinkW(uint32_t seed, OutRef o) : Sink<WRITE>(seed, o) {}
	__device__ __forceinline__ void push(uint64_t bits, uint32_t n)   // n <= 32
	{
		this->acc |= bits << this->nacc;
		this->nacc += n;
		if (this->nacc >= 32) {
			this->crc = crc_word(this->crc, (uint32_t)this->acc);
			this->acc >>= 32;
			this->nacc -= 32;
		}
		if (WRITE) {
			this->oacc |= bits << this->onacc;
			this->onacc += n;
			if (this->onacc >= 64) {
				this->out.st(this->oword++, this->oacc);
				this->onacc -= 64;
				this->oacc = this->onacc ? bits >> (n - this->onacc) : 0;
			}
		}
	}
	__device__ __forceinline__ void finish()
	{
		while (this->nacc >= 8) {
			this->crc = crc_byte(this->crc, (uint32_t)this->acc & 0xff);
			this->acc >>= 8;
			this->nacc -= 8;
		}
	}
};
// fhs (:783-818)
template <bool WRITE>
__device__ __forceinline__ int do_fhs(PState &s, uint32_t clock)
{
	int size = s.length - 122;
	s.plen = 20;
	s.dirty |= D_PLEN;
	if (size < 240)
		return 1;
	uint64_t corr[3] = {0, 0, 0};
#pragma unroll
	for (uint32_t k = 0; k < 16; k += 4) {
		uint32_t d4[4];
		const uint32_t ok = fec23_blocks4(s, 122 + 15 * k, 4, d4);
#pragma unroll
		for (uint32_t j = 0; j < 4; j++) {
			if (!((ok >> j) & 1))
				return 0;
			const uint32_t d = d4[j], bit = 10 * (k + j);
			corr[bit >> 6] |= (uint64_t)d << (bit & 63);
			if ((bit & 63) > 54)
				corr[(bit >> 6) + 1] |= (uint64_t)d >> (64 - (bit & 63));
		}
	}
	int rv = 0;
	uint32_t c = clock;
	for (int attempt = 0; attempt < 33; attempt++) {
		if (attempt)
			c = 31 + attempt;
		uint32_t idx = wh_start(c, 18);
		uint32_t crc = crc_seed(s.uap);
		uint64_t pl[3];
		for (int i = 0; i < 3; i++) {
			uint32_t n = i < 2 ? 64 : 32;
			pl[i] = corr[i] ^ wh(s, idx, n);
			idx = (idx + n) % 127u;
			for (uint32_t b = 0; b < n; b += 32)                  // 20 bytes = five words
				crc = crc_word(crc, (uint32_t)(pl[i] >> b));
		}
		if (WRITE) {
			s.out.st(0, pl[0]);
			s.out.st(1, pl[1]);
			s.out.st(2, (s.out.ld(2) & ~0xffffffffULL) | pl[2]);
			if (s.written < 160) s.written = 160;
		}
		if (crc == 0) {
			rv = 1000;
			break;
		}
	}
	return rv;
}

// decode_payload_header (:821-895)
template <bool WRITE>
__device__ __forceinline__ bool do_payload_header(PState &s, uint32_t pos, uint32_t clock, int header_bytes, int size, bool fec)
{
	uint32_t hbits = header_bytes == 2 ? 16 : 8;
	if (size < (int)hbits)
		return false;
	uint32_t raw;
	if (fec) {
		if (size < (header_bytes == 2 ? 30 : 15))
			return false;
		uint32_t d0, d1 = 0;
		if (!fec23_block((uint32_t)s_bits(s, pos, 15), d0))
			return false;
		if (header_bytes == 2 && !fec23_block((uint32_t)s_bits(s, pos + 15, 15), d1))
			return false;
		raw = (d0 | (d1 << 10)) & ((1u << hbits) - 1);
	} else {
		raw = (uint32_t)s_bits(s, pos, hbits);
	}
	uint32_t ph = raw ^ (uint32_t)wh(s, wh_start(clock, 18), hbits);
	s.ph16 = (s.ph16 & ~((1u << hbits) - 1)) | ph;
	s.ph_mask |= (1u << hbits) - 1;
	s.dirty |= D_PLEN | D_LF | D_PHL;
	if (s.ph_written < hbits) s.ph_written = hbits;
	int plen = header_bytes == 2 ? (int)((s.ph16 >> 3) & 0x3ff) + 4 : (int)((s.ph16 >> 3) & 0x1f) + 3;
	int cap;
	switch (s.type) {
	case 3:  cap = 20;  break;
	case 4:  cap = 30;  break;
	case 8:  cap = 12;  break;
	case 10: cap = 125; break;
	case 11: cap = 187; break;
	case 14: cap = 228; break;
	case 15: cap = 343; break;
	default: cap = 0;   break;
	}
	s.plen = plen < cap ? plen : cap;
	s.llid = s.ph16 & 3;
	s.flow = (s.ph16 >> 2) & 1;
	s.phl = header_bytes;
	return true;
}

// DM (:898-958)
template <bool WRITE>
__device__ __forceinline__ int do_DM(PState &s, uint32_t clock)
{
	uint32_t pos = 122;
	int size = s.length - 122;
	int header_bytes = 2, max_length;
	switch (s.type) {
	case 8:  pos += 80; size -= 80; header_bytes = 1; max_length = 12; break;
	case 3:  header_bytes = 1; max_length = 20; break;
	case 10: max_length = 125; break;
	case 14: max_length = 228; break;
	default: return 0;
	}
	if (!do_payload_header<WRITE>(s, pos, clock, header_bytes, size, true))
		return 0;
	if (s.plen > max_length)
		return 1;
	int nbits = s.plen * 8;
	if (nbits > size)
		return 1;
	uint32_t nblocks = (nbits + 9) / 10;
	if (WRITE && s.def_slot && !s.out.l && nbits > DHL_MIN_BITS) {
		defer_payload(s, clock, (uint32_t)nbits, DHL_DM);
		return 2;                                           // (replaced by the lane-group phase's verdict)
	}
	// The reference writes nothing when a block fails.  Into HBM that takes a pass over all blocks first; a scratch copy
	// is written as the blocks decode and marked as not to be kept when one fails.
	if (WRITE && !s.out.l && !fec23_ok(s, pos, nblocks))
		return 0;
	SinkW<WRITE> sink(crc_seed(s.uap), s.out);
	uint32_t idx = wh_start(clock, 18);
	int left = nbits;
	for (uint32_t k = 0; k < nblocks; k += 4) {             // four blocks = 40 data bits per step
		uint32_t d[4];
		const uint32_t cnt = nblocks - k < 4 ? nblocks - k : 4;
		const uint32_t ok = fec23_blocks4(s, pos + 15 * k, cnt, d);
		const uint64_t w40 = wh(s, idx, 40);
		idx = idx + 40 >= 127 ? idx + 40 - 127 : idx + 40;
#pragma unroll
		for (uint32_t j = 0; j < 4; j++) {
			if (j >= cnt)
				break;
			if (!((ok >> j) & 1)) {
				if (WRITE)
					s.spoiled = true;
				return 0;
			}
			const uint32_t n = left < 10 ? left : 10;
			sink.push((d[j] ^ (uint32_t)(w40 >> (10 * j))) & ((1u << n) - 1), n);
			left -= n;
		}
	}
	sink.finish();
	sink.flush();
	if (WRITE && s.written < (uint32_t)nbits) s.written = nbits;
	return sink.crc == 0 ? 10 : 2;
}

// DH (:962-1011)
template <bool WRITE>
__device__ __forceinline__ int do_DH(PState &s, uint32_t clock)
{
	const uint32_t pos = 122;
	int size = s.length - 122;
	int header_bytes = 2, max_length;
	switch (s.type) {
	case 9:
	case 4:  header_bytes = 1; max_length = 30; break;
	case 11: max_length = 187; break;
	case 15: max_length = 343; break;
	default: return 0;
	}
	if (!do_payload_header<WRITE>(s, pos, clock, header_bytes, size, false))
		return 0;
	if (s.plen > max_length)
		return 1;
	int nbits = s.plen * 8;
	if (nbits > size)
		return 1;
	if (WRITE && s.def_slot && !s.out.l && nbits > DHL_MIN_BITS) {
		defer_payload(s, clock, (uint32_t)nbits, DHL_DH);
		return 2;                                           // (replaced by the lane-group phase's verdict)
	}
	Sink<WRITE> sink(crc_seed(s.uap), s.out);
	uint32_t idx = wh_start(clock, 18);
	for (int done = 0; done < nbits; done += 32) {
		uint32_t n = nbits - done < 32 ? nbits - done : 32;
		sink.push(s_bits(s, pos + done, n) ^ wh(s, idx, n), n);
		idx = (idx + n) % 127u;
	}
	sink.flush();
	if (WRITE && s.written < (uint32_t)nbits) s.written = nbits;
	if (s.type == 9)
		return 2;
	return sink.crc == 0 ? 10 : 2;
}

// EV3 (:1013-1042) / EV5 (:1099-1128)
template <bool WRITE>
__device__ __forceinline__ int do_EV35(PState &s, uint32_t clock, int maxlength)
{
	int size = s.length - 122;
	uint32_t first8 = (uint32_t)s_bits(s, 122, 8);
	Sink<WRITE> sink(crc_seed(s.uap), s.out);
	uint32_t idx = wh_start(clock, 18);
	int rv = 2;
	int L;
	for (L = 0; L < maxlength; L++) {
		if (8 * L + 8 > size) {
			rv = 1;
			break;
		}
		// the reference writes byte L, then tests the CRC over bytes 0..L-1
		uint32_t byte = first8 ^ (uint32_t)wh(s, idx, 8);
		idx = (idx + 8) % 127u;
		bool match = L > 2 && sink.crc == 0;     // CRC over bytes 0..L-1 == 0
		sink.push(byte, 8);
		if (WRITE && s.written < (uint32_t)(8 * L + 8)) s.written = 8 * L + 8;
		if (match) {
			rv = 10;
			break;
		}
	}
	sink.flush();
	s.plen = L;
	s.dirty |= D_PLEN;
	return rv;
}

// EV4 (:1044-1097)
template <bool WRITE>
__device__ __forceinline__ int do_EV4(PState &s, uint32_t clock)
{
	int size = s.length - 122;
	uint32_t crc = crc_seed(s.uap);
	uint64_t acc = 0;           // payload bits produced but not yet consumed by the CRC
	uint32_t nacc = 0;
	uint64_t oacc = 0;
	uint32_t onacc = 0, oword = 0;
	int L = 1;
	int rv = 2;
	for (int b = 0; b < 98; b++) {
		int syms = 15 * b, bits = 10 * b;
		if (syms + 15 > size) { rv = 1; break; }
		uint32_t d;
		if (!fec23_block((uint32_t)s_bits(s, 122 + syms, 15), d)) { rv = syms < 45 ? 0 : 1; break; }
		uint64_t ten = d ^ (uint32_t)wh(s, wh_start(clock, 18 + bits), 10);
		acc |= ten << nacc;
		nacc += 10;
		if (WRITE) {
			oacc |= ten << onacc;
			onacc += 10;
			if (onacc >= 64) {
				s.out.st(oword++, oacc);
				onacc -= 64;
				oacc = onacc ? ten >> (10 - onacc) : 0;
			}
			if (s.written < (uint32_t)(bits + 10)) s.written = bits + 10;
		}
		bool hit = false;
		while (L * 8 <= bits) {
			crc = crc_byte(crc, (uint32_t)acc & 0xff);      // byte L-1
			acc >>= 8;
			nacc -= 8;
			if (L >= 2 && crc == 0) { hit = true; break; }
			L++;
		}
		if (hit) { rv = 10; break; }
	}
	if (WRITE && onacc) {
		uint64_t keep = ~0ULL << onacc;
		s.out.st(oword, (s.out.ld(oword) & keep) | oacc);
	}
	s.plen = L;
	s.dirty |= D_PLEN;
	return rv;
}

// HV (:1131-1174)
template <bool WRITE>
__device__ __forceinline__ int do_HV(PState &s, uint32_t clock)
{
	int size = s.length - 122;
	s.phl = 0;
	s.dirty |= D_PHL;
	if (size < 240) {
		s.plen = 0;
		s.dirty |= D_PLEN;
		return 1;
	}
	uint32_t idx = wh_start(clock, 18);
	if (s.type == 5) {
		uint32_t data[4], total = 0;
		for (int i = 0; i < 4; i++) {       // 80 triples = 4 x 20
			uint32_t dis;
			data[i] = fec13(s_bits(s, 122 + 60 * i, 60), 20, dis);
			total += dis;
		}
		if (!(total < 20))
			return 0;
		s.plen = 10;
		s.dirty |= D_PLEN;
		s.flags |= F_HAS_PAYLOAD;
		if (WRITE) {
			Sink<true> sink(0, s.out);
			for (int i = 0; i < 4; i++) {
				sink.push(data[i] ^ (uint32_t)wh(s, idx, 20), 20);
				idx = (idx + 20) % 127u;
			}
			sink.flush();
			if (s.written < 80) s.written = 80;
		}
	} else if (s.type == 6) {
		if (!fec23_ok(s, 122, 16))
			return 0;
		s.plen = 20;
		s.dirty |= D_PLEN;
		s.flags |= F_HAS_PAYLOAD;
		if (WRITE) {
			Sink<true> sink(0, s.out);
			for (uint32_t k = 0; k < 16; k++) {
				uint32_t d;
				fec23_block((uint32_t)s_bits(s, 122 + 15 * k, 15), d);
				sink.push(d ^ (uint32_t)wh(s, idx, 10), 10);
				idx = (idx + 10) % 127u;
			}
			sink.flush();
			if (s.written < 160) s.written = 160;
		}
	} else if (s.type == 7) {
		s.plen = 30;
		s.dirty |= D_PLEN;
		s.flags |= F_HAS_PAYLOAD;
		if (WRITE) {
			Sink<true> sink(0, s.out);
			for (int done = 0; done < 240; done += 30) {
				sink.push(s_bits(s, 122 + done, 30) ^ wh(s, idx, 30), 30);
				idx = (idx + 30) % 127u;
			}
			sink.flush();
			if (s.written < 240) s.written = 240;
		}
	}
	return 2;
}

// crc_check (:708-769)
template <bool WRITE>
__device__ int do_crc_check(PState &s, uint32_t clock)
{
	int rv = 1;
	switch (s.type) {
	case 2:  rv = do_fhs<WRITE>(s, clock); break;
	case 8: case 3: case 10: case 14: rv = do_DM<WRITE>(s, clock); break;
	case 4: case 11: case 15: rv = do_DH<WRITE>(s, clock); break;
	case 7:  rv = WRITE ? do_EV35<WRITE>(s, clock, 32) : 1; break;     // always mapped to 1 below
	case 12: rv = do_EV4<WRITE>(s, clock); break;
	case 13: rv = WRITE ? do_EV35<WRITE>(s, clock, 182) : 1; break;
	case 5:  rv = do_HV<WRITE>(s, clock); break;
	default: break;
	}
	if (rv == 0 && s.type != 2 && s.type != 3 && s.type != 5)
		return 1;
	if (rv > 1 && (s.type == 7 || s.type == 13))
		return 1;
	return rv;
}

// FEC-1/3 decoded header bits and the number of disagreeing triples
__device__ __forceinline__ uint32_t header_fec13(const uint64_t *w, uint32_t &disagree)
{
	return fec13(pk_bits(w, 68, 54), 18, disagree);
}
__device__ __forceinline__ uint32_t header_fec13(const PState &s, uint32_t &disagree)
{
	return fec13(s_bits(s, 68, 54), 18, disagree);
}

// try_clock (:1178-1195); returns the reference's return value
__device__ __forceinline__ uint32_t do_try_clock(PState &s, uint32_t clock, uint32_t hdr, uint32_t disagree)
{
	if (!(disagree < 4))
		return 0;
	uint32_t clear = hdr ^ (uint32_t)wh(s, wh_start(clock, 0), 18);
	s.uap = uap_from_hec(clear & 0x3ff, clear >> 10);
	s.type = (clear >> 3) & 0xf;
	s.dirty |= D_UT;
	return s.uap;
}

// btbb_header_present (:1371-1408)
// (dis: the disagreeing triples of the header, header_fec13)
__device__ __forceinline__ int do_header_present(const PState &s, uint32_t dis)
{
	if (s.length < 122)
		return 0;
	const uint32_t five = (uint32_t)s_bits(s, 63, 5);
	uint32_t msb = five & 1;
	uint32_t tr = five >> 1;
	uint32_t want = msb ? 0xAu : 0x5u;          // !m, m, !m, m  (LSB first)
	uint32_t errs = __popc(tr ^ want);
	return (errs + dis) < 5;
}
__device__ __forceinline__ int do_header_present(const PState &s)
{
	uint32_t dis;
	(void)fec13(s_bits(s, 68, 54), 18, dis);
	return do_header_present(s, dis);
}
