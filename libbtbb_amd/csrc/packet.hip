// packet.hip -- the bit chain behind an access code, on packed symbols, for gfx950.
//
// Restates, one lane per (packet, clock) trial or per packet, the reference's
//   unfec13 (lib/src/bluetooth_packet.c:552)    unfec23 / fec23 (:571-649)
//   unwhiten (:653)   crcgen / payload_crc (:671, :772)   uap_from_hec (:693)
//   try_clock (:1178) crc_check (:708) fhs/DM/DH/EV3/EV4/EV5/HV (:783-1174)
//   btbb_header_present (:1371) btbb_decode_header (:1198) btbb_decode_payload (:1223)
// Symbols are bits of 64-bit words (bit i of the packet = symbol i), so FEC 1/3 is three
// masked ANDs, whitening is an XOR with a slice of the 127-bit sequence, and the CRC runs
// a byte at a time.  Identities used (all exact):
//   * crcgen over n bytes followed by its own 16 check bits leaves the register at 0, so
//     payload_crc() == (CRC over all payload_length bytes == 0) for payload_length >= 2;
//   * with payload_length == 1 payload_crc() can never succeed (the check word read from
//     in front of payload[] has bit 4 set by payload_length itself, the seed's low byte
//     is 0), which removes the llid/flow dependency of EV4;
//   * crc_check() maps every EV3/EV5 result to 1 (:760-766).
// Reference quirks kept: FEC-2/3 reads past pkt->length (DM), EV3/EV5 re-use the first
// payload byte (:1036, :1122), DV whitening restarts at 18 (:913-937), a failed FEC 1/3
// leaves UAP/type from the previous trial (:1186-1187).
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <type_traits>
#include "packet_launch.h"
#include "packet_core.h"

static uint32_t host_crc_byte(uint32_t crc, uint32_t byte)
{
	uint32_t x = (crc ^ byte) & 0xff;
	x ^= (x << 4) & 0xff;
	return ((crc >> 8) ^ (x << 8) ^ (x << 3) ^ (x >> 4)) & 0xffff;
}

int chain_upload(const HostTables &t)
{
	// trials_linear_kernel puts the trials of a batch into type order by arithmetic (its step 1b), which rests on one property of
	// the whitening sequence: the four bits that whiten the header's type field (header bits 3 .. 6) take every value for
	// exactly four of the 64 CLK1-6 candidates.  Checked here, once, on the table the kernels are built from.
	{
		int seen[16] = {0};
		for (int clk = 0; clk < 64; clk++) {
			uint32_t v = 0;
			for (int j = 0; j < 4; j++)
				v |= (uint32_t)t.whiten[(t.whiten_idx[clk] + 3 + j) % 127] << j;
			seen[v]++;
		}
		for (int v = 0; v < 16; v++)
			if (seen[v] != 4) {
				set_error("btbbx_init: internal: the type-field whitening is not four clocks per value");
				return BTBBX_E_ARG;
			}
	}
	// the LDS image of the decoders
	{
		static ChainLds img;
		memset(&img, 0, sizeof(img));
		for (int i = 0; i < 128; i++)
			for (int j = 0; j < 32; j++)
				img.wh32[i] |= (uint32_t)t.whiten[((i < 127 ? i : 0) + j) % 127] << j;
		for (int i = 0; i < 256; i++) {
			uint32_t c = host_crc_byte(0, (uint32_t)i);
			img.crc[i] = (uint16_t)c;
			for (int k = 0; k < 3; k++) {
				c = host_crc_byte(c, 0);
				img.crc_z[k][i] = (uint16_t)c;
			}
		}
		for (int i = 0; i < 1024; i++) {
			uint32_t par = 0;
			for (int bit = 0; bit < 10; bit++)
				if ((i >> bit) & 1)
					par ^= t.fec23_par[bit];
			img.par23[i] = (uint8_t)par;
		}
		memcpy(img.fix23, t.fec23_fix, 32);
		for (int i = 0; i < 32; i++)
			img.fixm23[i] = t.fec23_fix[i] == -2 ? 0x8000u : t.fec23_fix[i] >= 0 ? (uint16_t)(1u << t.fec23_fix[i]) : 0u;
		memcpy(img.whiten_idx, t.whiten_idx, 64);
		for (int h = 0; h < 2; h++)
			for (int i = 0; i < 256; i++) {
				uint32_t c = (uint32_t)i << (8 * h);
				for (int k = 0; k < 32; k++)
					c = host_crc_byte(c, 0);
				img.adv32[h][i] = (uint16_t)c;
			}
		HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_chain_lds_image), &img, sizeof(img)));
	}
	// the rows of trials_linear_kernel
	{
		static uint16_t lin[LIN_MAXLEN * 16];
		memset(lin, 0, sizeof(lin));
		for (int bit = 0; bit < 8; bit++) {
			uint32_t crc = 1u << (8 + bit);
			for (int L = 0; L < LIN_MAXLEN; L++) {
				lin[L * 16 + bit] = (uint16_t)crc;
				crc = host_crc_byte(crc, 0);
			}
		}
		// the recurrence of the whitening sequence: w[k + 7] = XOR of the w[k + j] picked by `taps` (found, not assumed)
		uint32_t taps = 0;
		for (uint32_t m = 1; m < 128 && !taps; m++) {
			bool ok = true;
			for (int k = 0; k < 127 && ok; k++) {
				uint32_t x = 0;
				for (int j = 0; j < 7; j++)
					if ((m >> j) & 1)
						x ^= t.whiten[(k + j) % 127];
				ok = x == t.whiten[(k + 7) % 127];
			}
			if (ok)
				taps = m;
		}
		if (!taps) {
			set_error("chain_upload: the whitening sequence is not a 7-stage LFSR sequence");
			return BTBBX_E_ARG;
		}
		for (int e = 0; e < 7; e++) {
			static uint8_t seq[8 * LIN_MAXLEN + 8];
			for (int k = 0; k < 7; k++)
				seq[k] = k == e;
			for (int k = 7; k < 8 * LIN_MAXLEN; k++) {
				uint32_t x = 0;
				for (int j = 0; j < 7; j++)
					if ((taps >> j) & 1)
						x ^= seq[k - 7 + j];
				seq[k] = (uint8_t)x;
			}
			uint32_t crc = 0;
			for (int L = 1; L < LIN_MAXLEN; L++) {
				uint32_t byte = 0;
				for (int j = 0; j < 8; j++)
					byte |= (uint32_t)seq[8 * (L - 1) + j] << j;
				crc = host_crc_byte(crc, byte);
				lin[L * 16 + 8 + e] = (uint16_t)crc;
			}
		}
		HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_lin), lin, sizeof(lin)));
		static uint16_t advw[7 * 2 * 256];
		for (int i = 1; i <= 7; i++)
			for (int h = 0; h < 2; h++)
				for (int x = 0; x < 256; x++) {
					uint32_t c = (uint32_t)x << (8 * h);
					for (int k = 0; k < 4 * i; k++)
						c = host_crc_byte(c, 0);
					advw[((i - 1) * 2 + h) * 256 + x] = (uint16_t)c;
				}
		HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_advw), advw, sizeof(advw)));
		// A^(-64): the register u that holds 1 << k 64 zero bits later, found by running every u forward (nothing assumed
		// about the polynomial beyond "the step is invertible", which the search checks)
		static uint16_t adv64inv[64 * 16];
		{
			static uint16_t back[65536];
			static uint8_t hit[65536];
			memset(hit, 0, sizeof(hit));
			for (uint32_t u = 0; u < 65536; u++) {
				uint32_t c = u;
				for (int b = 0; b < 8; b++)
					c = host_crc_byte(c, 0);
				back[c] = (uint16_t)u;
				hit[c] = 1;
			}
			for (uint32_t v = 0; v < 65536; v++)
				if (!hit[v]) {
					set_error("chain_upload: the CRC register's zero-byte step is not invertible");
					return BTBBX_E_ARG;
				}
			for (int k = 0; k < 16; k++) {
				uint32_t c = 1u << k;
				for (int j = 0; j < 64; j++) {
					adv64inv[j * 16 + k] = (uint16_t)c;
					c = back[c];
				}
			}
		}
		HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_adv64inv), adv64inv, sizeof(adv64inv)));
		static uint16_t adv64fwd[64 * 16];
		for (int k = 0; k < 16; k++) {
			uint32_t c = 1u << k;
			for (int j = 0; j < 64; j++) {
				adv64fwd[j * 16 + k] = (uint16_t)c;
				for (int b = 0; b < 8; b++)
					c = host_crc_byte(c, 0);
			}
		}
		HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_adv64fwd), adv64fwd, sizeof(adv64fwd)));
	}
	ChainTables c;
	memset(&c, 0, sizeof(c));
	for (int j = 0; j < 256; j++)
		if (t.whiten[j % 127])
			c.whiten2[j >> 6] |= 1ULL << (j & 63);
	memcpy(c.whiten_idx, t.whiten_idx, 64);
	memcpy(c.fec23_par, t.fec23_par, 10);
	memcpy(c.fec23_fix, t.fec23_fix, 32);
	HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_chain), &c, sizeof(c)));
	return BTBBX_OK;
}

// the kernels, in one translation unit: they share the static LDS image and the tables of packet_core.h
#include "packet_trials.h"
#include "packet_stream.h"
#include "packet_dropin.h"

// cut packets out of the packed streams
// five packets per 256-thread workgroup: thread -> (packet, output word); the output rows of a workgroup are
// contiguous (5 x 400 bytes), so its stores coalesce across packets
#define GATHER_PACKETS (256 / BTBBX_PKT_WORDS)
__global__ __launch_bounds__(256) void gather_kernel(const uint64_t *words, uint64_t n_words, uint64_t pitch_words,
						      const btbbx_hit *hits, uint32_t n_packets, uint32_t max_length,
						      uint64_t *packets, uint32_t *lengths, const uint32_t *d_count)
{
	if (d_count)
		n_packets = min(n_packets, *d_count);
	uint32_t pkt = blockIdx.x * GATHER_PACKETS + threadIdx.x / BTBBX_PKT_WORDS;
	uint32_t i = threadIdx.x % BTBBX_PKT_WORDS;          // output word
	if (pkt >= n_packets || threadIdx.x >= GATHER_PACKETS * BTBBX_PKT_WORDS)
		return;
	const btbbx_hit h = hits[pkt];
	const uint64_t *base = words + (uint64_t)h.stream * pitch_words;
	uint64_t total_bits = n_words * 64;
	uint64_t avail = h.offset < total_bits ? total_bits - h.offset : 0;
	uint32_t len = avail < max_length ? (uint32_t)avail : max_length;
	if (len > BTBBX_MAX_SYMBOLS)
		len = BTBBX_MAX_SYMBOLS;
	uint64_t bit = h.offset + 64ULL * i;
	uint64_t j = bit >> 6;
	uint32_t sh = (uint32_t)(bit & 63);
	uint64_t lo = j < n_words ? base[j] : 0, hi = (j + 1) < n_words ? base[j + 1] : 0;
	uint64_t v = sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
	// zero everything at and beyond `len`
	uint32_t first = 64 * i;
	if (first >= len)
		v = 0;
	else if (len - first < 64)
		v &= (1ULL << (len - first)) - 1;
	packets[(uint64_t)pkt * BTBBX_PKT_WORDS + i] = v;
	if (i == 0)
		lengths[pkt] = len;
}

// btbb_header_present of gathered packets, one byte each (the survey walks only packets that carry a header)
__global__ __launch_bounds__(256) void header_flags_kernel(const uint64_t *packets, const uint32_t *lengths, uint32_t n_packets,
							    uint8_t *present, const uint32_t *d_count)
{
	const uint32_t i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n_packets || (d_count && i >= *d_count))
		return;
	PState s;
	s.w = packets + (uint64_t)i * BTBBX_PKT_WORDS;
	s.length = (int)lengths[i];
	present[i] = (uint8_t)do_header_present(s);
}

// ---- launchers --------------------------------------------------------------------------------
int launch_trials_state(const uint8_t *d_sym, const btbbx_pkt_in *d_in, const btbbx_pkt_out *d_out, void *d_state,
			btbbx_trial *d_trials, hipStream_t stream)
{
	int rc = ctx_require();
	if (rc)
		return rc;
	hipLaunchKernelGGL(trials_state_kernel, dim3(64), dim3(64), 0, stream, d_sym, d_in, d_out, (TrialState *)d_state, d_trials);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

int launch_trials_merge(const void *d_state, const btbbx_pkt_in *d_in, btbbx_pkt_out *d_out, uint8_t *d_pay,
			const TrialPlan *plan, hipStream_t stream)
{
	hipLaunchKernelGGL(trials_merge_kernel, dim3(1), dim3(64), 0, stream, (const TrialState *)d_state, d_in, d_out, d_pay,
			   *plan);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

size_t trials_state_bytes() { return 64 * sizeof(TrialState); }

int launch_gather(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, const btbbx_hit *d_hits, uint32_t n_packets,
		  const uint32_t *d_count, uint32_t max_length, uint64_t *d_packets, uint32_t *d_lengths, hipStream_t hip_stream)
{
	int rc = ctx_require();
	if (rc)
		return rc;
	if (!n_packets)
		return BTBBX_OK;
	hipLaunchKernelGGL(gather_kernel, dim3((n_packets + GATHER_PACKETS - 1) / GATHER_PACKETS), dim3(256), 0,
			   hip_stream, d_words, n_words, pitch_words, d_hits, n_packets, max_length, d_packets, d_lengths, d_count);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

extern "C" int btbbx_gather_packets_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
					   const btbbx_hit *d_hits, uint32_t n_packets, uint32_t max_length,
					   uint64_t *d_packets, uint32_t *d_lengths, void *hip_stream)
{
	return launch_gather(d_words, n_words, pitch_words, d_hits, n_packets, nullptr, max_length, d_packets, d_lengths, (hipStream_t)hip_stream);
}

extern "C" int btbbx_trials_device(const uint64_t *d_packets, const btbbx_pkt_in *d_in, uint32_t n_packets,
				   btbbx_trial *d_trials, void *hip_stream)
{
	return launch_trials(d_packets, d_in, n_packets, nullptr, d_trials, (hipStream_t)hip_stream);
}

int launch_trials(const uint64_t *d_packets, const btbbx_pkt_in *d_in, uint32_t n_packets, const uint32_t *d_count,
		  btbbx_trial *d_trials, hipStream_t hip_stream)
{
	int rc = ctx_require();
	if (rc)
		return rc;
	if (!n_packets)
		return BTBBX_OK;
	if (n_packets <= 256) {      // latency shape while 64 n waves are only a few rounds over the chip
		hipLaunchKernelGGL(trials_wide_kernel, dim3(n_packets * 64), dim3(64), 0, (hipStream_t)hip_stream,
				   d_packets, d_in, n_packets, d_trials, d_count);
	} else {                     // per-packet FEC / CRC prefix work once, O(1) per DM / DH / FHS trial
		const uint32_t batches = (n_packets + TL_PACKETS - 1) / TL_PACKETS;
		const uint32_t resident = (uint32_t)ctx().num_cus * TL_WGS_PER_CU;
		hipLaunchKernelGGL(trials_linear_kernel, dim3(batches < resident ? batches : resident), dim3(TL_THREADS), 0,
				   (hipStream_t)hip_stream, d_packets, d_in, n_packets, d_trials, d_count);
	}
#ifdef TL_PROFILE
	if (n_packets > 256) {
		unsigned long long prof[16], tot = 0;
		(void)hipDeviceSynchronize();
		(void)hipMemcpyFromSymbol(prof, HIP_SYMBOL(g_tl_prof), sizeof(prof));
		for (int k = 0; k < 16; k++) tot += prof[k];
		fprintf(stderr, "trials profile:");
		for (int k = 0; k < 10; k++) fprintf(stderr, " %d:%.1f%%", k, 100.0 * (double)prof[k] / (double)(tot ? tot : 1));
		fprintf(stderr, "\n");
		static unsigned long long z[16];
		(void)hipMemcpyToSymbol(HIP_SYMBOL(g_tl_prof), z, sizeof(z));
	}
#endif
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

extern "C" int btbbx_uap_table_device(const uint64_t *d_packets, const btbbx_pkt_in *d_in, uint32_t n_packets,
				      uint16_t *d_table, void *hip_stream)
{
	int rc = ctx_require();
	if (rc)
		return rc;
	if (!n_packets)
		return BTBBX_OK;
	if ((uintptr_t)d_table & 15) {
		set_error("btbbx_uap_table_device: table must be 16-byte aligned");
		return BTBBX_E_ARG;
	}
	hipLaunchKernelGGL(uap_table_kernel, dim3((n_packets + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream,
			   d_packets, d_in, n_packets, (uint4 *)d_table);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

int launch_header_flags(const uint64_t *d_packets, const uint32_t *d_lengths, uint32_t n_packets, const uint32_t *d_count,
			uint8_t *d_present, hipStream_t stream)
{
	if (!n_packets)
		return BTBBX_OK;
	hipLaunchKernelGGL(header_flags_kernel, dim3((n_packets + 255) / 256), dim3(256), 0, stream, d_packets, d_lengths, n_packets, d_present, d_count);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

int launch_decode_bytes(const uint8_t *d_sym, uint8_t *d_pay, const btbbx_pkt_in *d_in, btbbx_pkt_out *d_out,
			uint32_t mode, bool with_payload, hipStream_t stream)
{
	int rc = ctx_require();
	if (rc)
		return rc;
	hipLaunchKernelGGL(decode_bytes_kernel, dim3(1), dim3(64), 0, stream, d_sym, d_pay, d_in, d_out, mode,
			   with_payload ? 1 : 0);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

int launch_decode(const uint64_t *d_packets, const btbbx_pkt_in *d_in, uint32_t n_packets,
		  btbbx_pkt_out *d_out, uint32_t mode, const TrialPlan *plan, hipStream_t stream)
{
	int rc = ctx_require();
	if (rc)
		return rc;
	if (!n_packets)
		return BTBBX_OK;
	TrialPlan p = {0, 0, 0};
	if (plan)
		p = *plan;
	if (mode & DEC_TRIALS) {                 // single try_clock / crc_check calls of the drop-in API
		if (mode != DEC_TRIALS || n_packets != 1) {
			set_error("decode: trial replay is a one-packet mode");
			return BTBBX_E_ARG;
		}
		hipLaunchKernelGGL(replay_kernel, dim3(1), dim3(64), 0, stream, d_packets, d_in, d_out, p);
		HIP_TRY(hipGetLastError());
		return BTBBX_OK;
	}
	hipLaunchKernelGGL(decode_kernel, dim3((n_packets + 63) / 64), dim3(64), 0, stream,
			   d_packets, d_in, n_packets, d_out, mode);
	HIP_TRY(hipGetLastError());
	return BTBBX_OK;
}

extern "C" int btbbx_decode_device(const uint64_t *d_packets, const btbbx_pkt_in *d_in, uint32_t n_packets,
				   btbbx_pkt_out *d_out, void *hip_stream)
{
	return launch_decode(d_packets, d_in, n_packets, d_out, DEC_HEADER | DEC_PAYLOAD, nullptr, (hipStream_t)hip_stream);
}

// decode_hits_kernel with the list its lanes leave for its own lane-group phase (DM / DH / EV payloads beyond 256 bits, sixteen
// bytes per packet).  The list lives in a block from the device's stream-ordered pool -- asked for and given back on the
// caller's stream, so concurrent callers on other streams share nothing and nothing is synchronised; the pool keeps what it has
// (release threshold raised once).  A runtime or device without such a pool still decodes: the kernel takes a null list, and
// every lane then walks its payload itself as in round 3 (slower for multi-slot packets, same results).
// *block = a block for the list from the device's stream-ordered pool, or null (see above); the pool's release threshold is
// raised once per device
static int decode_hits_list_alloc(size_t bytes, hipStream_t stream, void **block)
{
	static std::atomic<uint64_t> pool_ready{0}, pool_absent{0};
	*block = nullptr;
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	const bool tracked = dev >= 0 && dev < 64;
	if (tracked && ((pool_absent.load() >> dev) & 1))
		return BTBBX_OK;
	if (tracked && !((pool_ready.load() >> dev) & 1)) {
		hipMemPool_t pool;
		uint64_t keep = UINT64_MAX;
		if (hipDeviceGetDefaultMemPool(&pool, dev) != hipSuccess ||
		    hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep) != hipSuccess) {
			(void)hipGetLastError();
			pool_absent.fetch_or(1ULL << dev);
			return BTBBX_OK;
		}
		pool_ready.fetch_or(1ULL << dev);
	}
	if (hipMallocAsync(block, bytes, stream) != hipSuccess) {
		(void)hipGetLastError();
		*block = nullptr;
	}
	return BTBBX_OK;
}

static int launch_decode_hits(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, const btbbx_hit *d_hits,
			      const btbbx_pkt_in *d_in, uint32_t n_packets, const uint32_t *d_count, uint32_t max_length,
			      btbbx_pkt_out *d_out, uint32_t *d_lengths, const btbbx_pkt_in &one_in, uint32_t clk_div, hipStream_t stream)
{
	const uint32_t groups = (uint32_t)(((uint64_t)n_packets + 255) / 256);
	void *block;
	const int rc = decode_hits_list_alloc((size_t)groups * 4 * 64 * sizeof(uint4), stream, &block);
	if (rc)
		return rc;
	hipLaunchKernelGGL(decode_hits_kernel, dim3(groups), dim3(256), 0, stream, d_words, n_words, pitch_words, d_hits, d_in, n_packets,
			   d_count, max_length, d_out, d_lengths, DEC_HEADER | DEC_PAYLOAD, one_in, clk_div, (uint4 *)block);
	hipError_t e = hipGetLastError();
	if (block) {
		const hipError_t f = hipFreeAsync(block, stream);
		if (e == hipSuccess)
			e = f;
	}
	HIP_TRY(e);
	return BTBBX_OK;
}

extern "C" int btbbx_decode_hits_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
					const btbbx_hit *d_hits, const btbbx_pkt_in *d_in, uint32_t n_packets,
					uint32_t max_length, btbbx_pkt_out *d_out, uint32_t *d_lengths, void *hip_stream)
{
	int rc = ctx_require();
	if (rc)
		return rc;
	if (!n_packets)
		return BTBBX_OK;
	if (!d_words || !d_hits || !d_in || !d_out) {
		set_error("btbbx_decode_hits_device: null pointer");
		return BTBBX_E_ARG;
	}
	return launch_decode_hits(d_words, n_words, pitch_words, d_hits, d_in, n_packets, nullptr, max_length, d_out, d_lengths, btbbx_pkt_in{}, 1u,
				  (hipStream_t)hip_stream);
}

// The same with the number of hits still on the device (the counter btbbx_scan_device filled): decodes
// min(*d_count, cap) packets, launches for `cap`.  With btbbx_order_hits_device in front of it the chain
// scan -> order -> decode runs without a host round trip.
extern "C" int btbbx_decode_hits_counted_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
						const btbbx_hit *d_hits, const btbbx_pkt_in *d_in, const uint32_t *d_count,
						uint32_t cap, uint32_t max_length, btbbx_pkt_out *d_out, uint32_t *d_lengths,
						void *hip_stream)
{
	int rc = ctx_require();
	if (rc)
		return rc;
	if (!cap)
		return BTBBX_OK;
	if (!d_words || !d_hits || !d_in || !d_out || !d_count) {
		set_error("btbbx_decode_hits_counted_device: null pointer");
		return BTBBX_E_ARG;
	}
	rc = launch_decode_hits(d_words, n_words, pitch_words, d_hits, d_in, cap, d_count, max_length, d_out, d_lengths, btbbx_pkt_in{}, 1u,
				(hipStream_t)hip_stream);
	if (rc)
		return rc;
#ifdef DH_PROFILE
	{
		unsigned long long prof[8], total = 0;
		HIP_TRY(hipDeviceSynchronize());
		HIP_TRY(hipMemcpyFromSymbol(prof, HIP_SYMBOL(g_dh_prof), sizeof(prof)));
		for (int k = 0; k < 8; k++) total += prof[k];
		fprintf(stderr, "decode_hits profile (%% of wave time): loads %.1f type %.1f staging %.1f head-load %.1f present %.1f header %.1f payload %.1f store %.1f; s_memtime ticks per wave %.0f\n",
			100.0 * prof[0] / total, 100.0 * prof[1] / total, 100.0 * prof[2] / total, 100.0 * prof[3] / total,
			100.0 * prof[4] / total, 100.0 * prof[5] / total, 100.0 * prof[6] / total, 100.0 * prof[7] / total,
			(double)total / ((cap + 63) / 64));
		unsigned long long zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
		HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_dh_prof), zero, sizeof(zero)));
	}
#endif
	return BTBBX_OK;
}

// A capture of ONE piconet, decoded without a btbbx_pkt_in per packet: every packet enters with the state *entry
// describes (flags, UAP, ...; its length field is ignored) and the clock entry->clkn + offset / clk_div -- CLK1-27
// advances once per 625 symbols at 1 Msym/s, so a receiver that knows the clock at the first symbol of its buffer knows
// it for every access code the scan found in it.  The list's length is read from HBM as above (d_count may be NULL:
// then `cap` records are decoded).
extern "C" int btbbx_decode_hits_piconet_phase_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
						      const btbbx_hit *d_hits, const uint32_t *d_count, uint32_t cap,
						      const btbbx_pkt_in *entry, uint32_t clk_div, uint32_t clk_phase, uint32_t max_length,
						      btbbx_pkt_out *d_out, uint32_t *d_lengths, void *hip_stream)
{
	int rc = ctx_require();
	if (rc)
		return rc;
	if (!cap)
		return BTBBX_OK;
	if (!d_words || !d_hits || !entry || !d_out || !clk_div || clk_phase >= clk_div) {
		set_error("btbbx_decode_hits_piconet_device: null pointer, clk_div = 0 or clk_phase >= clk_div");
		return BTBBX_E_ARG;
	}
	btbbx_pkt_in one = *entry;
	one.length = clk_phase;                     // (the kernel takes the captured length from the stream, the field carries the phase)
	return launch_decode_hits(d_words, n_words, pitch_words, d_hits, nullptr, cap, d_count, max_length, d_out, d_lengths, one, clk_div,
				  (hipStream_t)hip_stream);
}

// ... for a buffer whose first symbol is the first symbol of a slot (clk_phase 0)
extern "C" int btbbx_decode_hits_piconet_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
						const btbbx_hit *d_hits, const uint32_t *d_count, uint32_t cap,
						const btbbx_pkt_in *entry, uint32_t clk_div, uint32_t max_length,
						btbbx_pkt_out *d_out, uint32_t *d_lengths, void *hip_stream)
{
	return btbbx_decode_hits_piconet_phase_device(d_words, n_words, pitch_words, d_hits, d_count, cap, entry, clk_div, 0, max_length,
						      d_out, d_lengths, hip_stream);
}
