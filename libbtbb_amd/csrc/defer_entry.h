// defer_entry.h -- the sixteen bytes a lane of decode_hits_kernel leaves for a payload it does not walk itself
// (defer_payload, packet_core.h) and the lane-group phases take apart again (packet_stream.h).  Host and device, no HIP
// headers needed: tests/c/defer_entry_check.cpp pins every field's place.
//   a: stream word the packet starts in (address, 48 bits) | stream words to load << 48 (7) | bit the packet starts at << 55 (6)
//   b: record index in its workgroup (8) | captured length << 8 (12) | bits << 20 (12) | kind << 32 (2) | whitened << 34 |
//      whitening phase of the payload's first bit << 35 (7) | UAP << 42 (8)
// kind / bits: DHL_DH, DHL_DM: payload_length * 8; DHL_EV4: ten per block its loop may look at (min(98, size / 15));
// DHL_EV5: eight per byte its loop may write (min(182, size / 8))
#pragma once
#include <stdint.h>

#define DHL_DH  0u
#define DHL_DM  1u
#define DHL_EV4 2u
#define DHL_EV5 3u

// Macros, not inline functions: decode_hits_kernel comes out with another register allocation when its lane-group phases
// take the entry apart through calls, however small, and with another instruction order when defer_payload packs through one
// (profiles/r08_packet).  As macros the expressions reach the compiler as they were written at each place.
#define DEFER_PACK_A(src, nw, sh) ((uint64_t)(src) | (uint64_t)(nw) << 48 | (uint64_t)(sh) << 55)
#define DEFER_PACK_B(pkt, len, nbits, kind, whitened, widx, uap) \
	((uint64_t)(pkt) | (uint64_t)(len) << 8 | (uint64_t)(nbits) << 20 | (uint64_t)(kind) << 32 | (uint64_t)(whitened) << 34 | \
	 (uint64_t)(widx) << 35 | (uint64_t)(uap) << 42)
// the fields of word a
#define DEFER_SRC(a)      ((a) & 0xffffffffffffULL)
#define DEFER_NW(a)       ((uint32_t)((a) >> 48) & 127u)
#define DEFER_SH(a)       ((uint32_t)((a) >> 55) & 63u)
// ... of word b
#define DEFER_PKT(b)      ((uint32_t)(b) & 0xffu)
#define DEFER_LEN(b)      ((uint32_t)((b) >> 8) & 0xfffu)
#define DEFER_NBITS(b)    ((uint32_t)((b) >> 20) & 0xfffu)
#define DEFER_KIND(b)     ((uint32_t)((b) >> 32) & 3u)
#define DEFER_WHITENED(b) (((b) >> 34) & 1u)
#define DEFER_WIDX(b)     ((uint32_t)((b) >> 35) & 127u)
#define DEFER_UAP(b)      ((uint32_t)((b) >> 42) & 0xffu)
// ... of the low / high dword of b (long_wave holds the entry as the four dwords its lane loaded)
#define DEFER_NBITS_LO(b_lo) (((b_lo) >> 20) & 0xfffu)
#define DEFER_KIND_HI(b_hi)  ((b_hi) & 3u)
