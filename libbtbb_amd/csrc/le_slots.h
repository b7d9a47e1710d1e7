// le_slots.h -- what the tracking's slot passes (le_track.h, included by le.hip) and the coded tracking's stand-in flag pass
// (le_ctrack.h, a translation unit of its own) both read: the candidate as it is moved, the membership rule, the
// layout of info[] and the host-side description of the flag pass.  No kernel lives here: a unit that includes this
// header compiles no kernel of another.
#pragma once
#include "le_record.h"

#define LT_THREADS     256u                // lanes of a slot pass's workgroup (LE_THREADS of le.hip)
#define LT_INFO_EVENT  0x100u              // info[j]: the channel index in the low byte, this bit where slot j opens an event

struct LdCand { uint2 a, b, c; };           // a btbbx_le_cand as the three 8-byte words it is moved in

__device__ __forceinline__ LdCand ld_load(const btbbx_le_cand *c, uint32_t i)
{
	const uint2 *p = reinterpret_cast<const uint2 *>(c + i);
	LdCand r;
	r.a = p[0];
	r.b = p[1];
	r.c = p[2];
	return r;
}

// rule 1: the connection a candidate is a member of, K for none
__device__ __forceinline__ uint32_t lt_member_of(uint2 c, const uint16_t *phys, uint32_t n_streams, uint32_t k, uint32_t &ch)
{
	const uint32_t stream = c.x & 0xffffu;
	ch = 0xff;
	if (c.y >= k || stream >= n_streams)
		return k;
	ch = le_channel_index(phys[stream]);
	return ch < 37 ? c.y : k;
}

// What the flag pass of a tracking run reads and writes, and where it is enqueued: slot j of n = params[0] holds candidate vals[j]
// of connection (uint32_t)keys[j]; info[j] and the tile counts tiles[0 .. n_tiles), one per tile_slots slots, are what it leaves.  A stand-in (le_track_launch)
// is a function that enqueues one kernel with the grid (n_tiles) x LT_THREADS that does exactly that.
struct LtFlagPass {
	const btbbx_le_cand *cands;
	const uint64_t *keys;
	const uint32_t *vals;
	const uint32_t *params;
	const uint16_t *phys;
	uint32_t n_streams, ifs_bits;
	uint32_t *info, *tiles;
	uint32_t n_tiles, tile_slots;                  // the grid; the slots a workgroup scans (LT_TILE of le_track.h, a multiple of LT_THREADS)
	hipStream_t q;
};
struct LtFlagStandIn {
	void (*enqueue)(const LtFlagPass &pass, const void *user);
	const void *user;
};
