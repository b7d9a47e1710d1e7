// le_record.h -- from dewhitened octets to a btbbx_le_pkt: what the 1M decoder (le.hip le_decode_kernel) and the coded-PHY
// decoder (le_coded.h le_coded_decode_kernel) share.  The channel mapping and the access-address rules of the reference
// (lib/src/bluetooth_le_packet.c), the two LDS tables (byte-wise CRC-24 of the reflected register, the whitening register
// advanced eight bits at a time) and le_record, which dewhitens octet by octet, runs the CRC, and forms every field of the
// record.  The callers differ in where a whitened octet comes from (the stream; a trellis path) and in who decides the
// PDU's length and whether the packet is complete.
#pragma once
#include "common.h"

// le_channel_index of the reference (bluetooth_le_packet.c:266-280), its integer arithmetic included: an odd or
// out-of-range MHz value gives what the reference's unsigned-char conversion gives
__host__ __device__ inline uint8_t le_channel_index(uint16_t mhz)
{
	const int f = mhz;
	if (f == 2402)
		return 37;
	if (f < 2426)
		return (uint8_t)((f - 2404) / 2);
	if (f == 2426)
		return 38;
	if (f < 2480)
		return (uint8_t)(11 + (f - 2428) / 2);
	return 39;
}

// a 12-bit window of the AA with a run of seven or more equal bits, as the reference's enumeration counts such windows
// (bluetooth_le_packet.c:184-238): its case list leaves out 38 of the 224 windows that hold such a run -- seven ones at
// bits 0..6 or 5..11 unless the rest of the window is zero, seven ones at 4..10 with bit 2 clear, nine zeros at 0..8
// unless bits 9..11 are all ones, and 0x401 -- and the offense count follows the reference, not the rule
__host__ __device__ inline bool le_run_window(uint32_t v)
{
	uint32_t ones = v, zeros = ~v & 0xfffu;
	for (int k = 0; k < 6; k++) {                       // x & x >> 1 ... six times: bit i survives iff bits i..i+6 are all set
		ones &= ones >> 1;
		zeros &= zeros >> 1;
	}
	if (!(ones | zeros))
		return false;
	if ((v & 0xffu) == 0x7fu && (v >> 8) != 0)
		return false;
	if ((v & 0xff0u) == 0xfe0u && (v & 0xfu) != 0)
		return false;
	if ((v & 0xffcu) == 0x7f0u)
		return false;
	if ((v & 0x3ffu) == 0x200u && (v >> 10) != 3)
		return false;
	return v != 0x401u;
}

// aa_data_channel_offenses (bluetooth_le_packet.c:100-242), restated: transitions beyond 24, fewer than two transitions
// in the six most significant bits, four equal octets, the advertising AA or one of its one-bit neighbours, and one
// per nibble-aligned 12-bit window with a long run (le_run_window)
__host__ __device__ inline uint32_t le_data_offenses(uint32_t aa)
{
	uint32_t n = 0;
	const uint32_t transitions = (uint32_t)__builtin_popcount((aa ^ (aa >> 1)) & 0x7fffffffu);
	if (transitions > 24)
		n += transitions - 24;
	const uint32_t top6 = aa >> 26;
	if (__builtin_popcount((top6 ^ (top6 >> 1)) & 0x1fu) < 2)
		n++;
	const uint32_t b0 = aa & 0xff;
	if (b0 == ((aa >> 8) & 0xff) && b0 == ((aa >> 16) & 0xff) && b0 == (aa >> 24))
		n++;
	if (aa == BTBBX_LE_ADV_AA)
		n++;
	if (__builtin_popcount(aa ^ BTBBX_LE_ADV_AA) == 1)
		n++;
	for (int shift = 0; shift <= 20; shift += 4)
		n += le_run_window((aa >> shift) & 0xfffu) ? 1u : 0u;
	return n;
}

__host__ __device__ inline uint32_t le_reverse24(uint32_t x)
{
	uint32_t r = 0;
	for (int i = 0; i < 24; i++)
		r |= ((x >> i) & 1u) << (23 - i);
	return r;
}

// entry i of the byte-wise CRC table of the reflected register: state = state >> 8 ^ T[(state ^ octet) & 0xff]
__device__ __forceinline__ uint32_t le_crc_tab_entry(uint32_t i)
{
	uint32_t s = i;
	for (int k = 0; k < 8; k++)
		s = (s >> 1) ^ ((s & 1u) ? 0xda6000u : 0u);     // x^24 + x^10 + x^9 + x^6 + x^4 + x^3 + x + 1, reflected
	return s;
}

// entry i < 128 of the whitening table (127-state LFSR): low byte = the eight output bits from state i, high byte = the next state
__device__ __forceinline__ uint16_t le_wh_tab_entry(uint32_t i)
{
	uint32_t w = i, o = 0;
	for (int k = 0; k < 8; k++) {
		o |= (w & 1u) << k;
		if (w & 1u)
			w ^= 0x88u;
		w >>= 1;
	}
	return (uint16_t)(o | (w << 8));
}

// The record of one hit.  raw(k) = the k-th octet behind the access address as received, still whitened; `forced_pdu` < 0:
// the PDU has 2 + header octet 1 octets (the 1M rule), else that many, whatever the header says, and 0 = no PDU at all (every
// octet, both CRCs and the header-derived fields as for zeros); is_truncated(pdu) = the stream ended before the last CRC bit.
template <class Raw, class Trunc>
__device__ __forceinline__ void le_record(Raw raw, Trunc is_truncated, int forced_pdu, const uint32_t *crc_tab, const uint16_t *wh_tab,
					  uint16_t mhz, uint32_t crc_init_reflected, uint32_t aa, const btbbx_hit &h, btbbx_le_pkt &o)
{
	const uint8_t ch_idx = le_channel_index(mhz);
	const uint8_t ch_k = (uint8_t)(((int)mhz - 2402) / 2);
	uint32_t ws = (ch_idx & 0x3fu) | 0x40u;            // whitening register: position 0 = 1, positions 1..6 = channel index
	uint32_t crc = crc_init_reflected;
	uint32_t *ob = reinterpret_cast<uint32_t *>(o.bytes);
	ob[0] = aa;
	uint32_t h0 = 0, h1 = 0, pdu = 0, crc_rx = 0;
	uint32_t dw = 1;                                    // next dword of `bytes` to store
	if (forced_pdu != 0) {
		// header
		uint32_t wt = wh_tab[ws];
		h0 = raw(0u) ^ (wt & 0xffu);
		ws = wt >> 8;
		wt = wh_tab[ws];
		h1 = raw(1u) ^ (wt & 0xffu);
		ws = wt >> 8;
		pdu = forced_pdu < 0 ? 2 + h1 : (uint32_t)forced_pdu;
		crc = (crc >> 8) ^ crc_tab[(crc ^ h0) & 0xffu];
		crc = (crc >> 8) ^ crc_tab[(crc ^ h1) & 0xffu];
		uint32_t acc = h0 | (h1 << 8);
		for (uint32_t k = 2; k < pdu + 3; k++) {
			wt = wh_tab[ws];
			const uint32_t d = raw(k) ^ (wt & 0xffu);
			ws = wt >> 8;
			if (k < pdu)
				crc = (crc >> 8) ^ crc_tab[(crc ^ d) & 0xffu];
			else
				crc_rx |= d << (8 * (k - pdu));
			if (dw < 16) {
				acc |= d << (8 * (k & 3));
				if ((k & 3) == 3) {
					ob[dw++] = acc;
					acc = 0;
				}
			}
		}
		if (dw < 16 && ((pdu + 3) & 3))
			ob[dw++] = acc;
	} else {
		crc = 0;
	}
	while (dw < 16)
		ob[dw++] = 0;
	ob[16] = 0;                                         // (the record's tail padding: records are compared as bytes)
	const bool truncated = is_truncated(pdu);
	o.offset = h.offset;
	o.stream = h.stream;
	o.aa_errors = h.ac_errors;
	o.crc_rx = crc_rx;
	o.crc_calc = crc;
	o.crc_ok = (forced_pdu != 0 && !truncated && crc == crc_rx) ? 1 : 0;
	o.pdu_bytes = (uint16_t)pdu;
	o.truncated = truncated ? 1 : 0;
	o.channel_idx = ch_idx;
	o.channel_k = ch_k;
	const bool data = ch_idx < 37;
	o.is_data = data ? 1 : 0;
	o.access_address = aa;
	if (data) {
		o.length = (uint8_t)(h1 & 0x1f);
		o.adv_type = o.adv_tx_add = o.adv_rx_add = 0;
		const uint32_t off = le_data_offenses(aa);
		o.access_address_offenses = (uint8_t)off;
		o.access_address_ok = off ? 0 : 1;
	} else {
		o.length = (uint8_t)(h1 & 0x3f);
		o.adv_type = (uint8_t)(h0 & 0xf);
		o.adv_tx_add = (h0 & 0x40) ? 1 : 0;
		o.adv_rx_add = (h0 & 0x80) ? 1 : 0;
		const bool ok = aa == BTBBX_LE_ADV_AA;
		o.access_address_ok = ok ? 1 : 0;
		o.access_address_offenses = ok ? 0 : (__builtin_popcount(aa ^ BTBBX_LE_ADV_AA) == 1 ? 1 : 32);
	}
}
