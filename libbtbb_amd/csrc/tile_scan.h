// tile_scan.h -- what the two-words-per-lane pattern scans share (scan_known.h scan_known_lap_kernel, le.hip le_scan_kernel:
// 256-lane workgroups stride over 512-word tiles of one stream at a time): the fetch of a lane's run, the launchers' tile
// arithmetic (their argument checks: check_scan_args, common.h).  NOT shared, on purpose: the (stream, tile) cursor, the cut of a ragged tile's masks
// and the hit ring.  As functions they change the generated code of kernels that were tuned by measurement (selects for
// the masks' branches, another loop rotation, ring cursors in other registers: profiles/r07_frame), so each kernel keeps them.
#pragma once
#include "common.h"

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// nw[0..1] = the lane's words of tile ft of stream fstream (lane byte offset lw_bytes inside the tile), nw[2] = the word
// behind them, through a buffer descriptor over the tile (as scan_slide_kernel's load_pair: the hardware's range check
// returns zero for the words behind the stream's end): no zero-initialised registers, no exec masks.
template <uint32_t TILE_WORDS, class Args>
__device__ __forceinline__ void fetch_run(const Args &a, uint32_t ft, uint32_t fstream, uint32_t lw_bytes, uint64_t (&nw)[3])
{
	uint32_t bytes = 0;                             // wave-uniform
	const uint64_t *tp = a.words;
	if (fstream < a.n_streams) {
		tp = a.words + (uint64_t)fstream * a.pitch_words + (uint64_t)ft * TILE_WORDS;
		bytes = (TILE_WORDS + 1u) * 8u;             // (a full tile: every word and the halo word are in range)
		if (ft >= a.full_tiles) {
			asm volatile("" ::: "memory");              // (a real branch: flattened, its 64-bit compares are vector instructions of every tile)
			const uint64_t first = (uint64_t)ft * TILE_WORDS;
			const uint64_t left = first < a.n_words ? a.n_words - first : 0;
			bytes = (uint32_t)(left < TILE_WORDS + 1u ? left : TILE_WORDS + 1u) * 8u;
		}
	}
	const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint64_t *>(tp), 0, (int)bytes, 0x00020000);
	const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)lw_bytes, 0, 0);
	const u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)lw_bytes, 16, 0);
	nw[0] = ((uint64_t)v.y << 32) | v.x;
	nw[1] = ((uint64_t)v.w << 32) | v.z;
	nw[2] = ((uint64_t)w.y << 32) | w.x;
}

// tiles and grid of one launch: eight workgroups per CU stride over the tiles of all streams
struct TileGrid {
	uint64_t tiles_per_stream, n_tiles;
	uint32_t full_tiles;         // leading tiles of a stream whose words, halo word and offsets are all in range
	uint32_t grid;
};
inline int tile_grid(const char *who, uint64_t search_bits, uint64_t n_words, uint32_t n_streams, uint32_t tile_words, int num_cus, TileGrid *g)
{
	const uint64_t search_words = (search_bits + 63) / 64;
	g->tiles_per_stream = (search_words + tile_words - 1) / tile_words;
	g->n_tiles = g->tiles_per_stream * n_streams;
	// tile t is full iff (t + 1) * tile_words + 1 <= n_words and (t + 1) * tile_words * 64 <= search_bits
	const uint64_t by_words = n_words ? (n_words - 1) / tile_words : 0, by_bits = search_bits / (tile_words * 64ull);
	const uint64_t full = by_words < by_bits ? by_words : by_bits;
	g->full_tiles = full > 0xffffffffull ? 0xffffffffu : (uint32_t)full;
	const uint64_t cap = (uint64_t)num_cus * 8;
	const uint64_t grid = g->n_tiles < cap ? g->n_tiles : cap;
	if (g->tiles_per_stream + grid >= (1ull << 32)) {     // the kernels' cursors are 32-bit
		set_error("%s: stream too long for one launch (split it)", who);
		return BTBBX_E_ARG;
	}
	g->grid = (uint32_t)grid;
	return BTBBX_OK;
}
