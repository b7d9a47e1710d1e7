// radix_sort.h -- the stable LSD radix passes of survey.hip (survey_hist / rows / scatter_kernel: eight bits per pass over an array
// of 64-bit keys that travels with an array of record indices), for every list that is ordered on the device: the survey's hits
// by (LAP, offset, stream), the LE discovery's candidates by (AA, CRCInit, stream, offset) (le_discover.h) and the LE tracking's
// slots by (connection, offset, stream) (le_track.h).
#pragma once
#include "common.h"

#define RADIX_SORT_TILE 4096u              // keys a workgroup ranks per pass (16 rounds of 256)

struct RadixPass {
	int by_stream;                         // the digit comes from hits[vals[i]].stream, not from keys[i]
	uint32_t shift;
};

// keys[0] / vals[0] hold the list, params[0] its length (<= cap); hist: 256 words per tile of RADIX_SORT_TILE keys, tot: 256 words
struct RadixBufs {
	uint64_t *keys[2];
	uint32_t *vals[2];
	uint32_t *hist, *tot;
	const uint32_t *params;
	uint32_t cap;
};

inline uint32_t radix_sort_blocks(size_t cap) { return (uint32_t)(((cap ? cap : 1) + RADIX_SORT_TILE - 1) / RADIX_SORT_TILE); }

// n_passes passes from side `cur` of the buffers, least significant digit first; returns the side the list ends in.
// hits: only read by a by_stream pass.  Launches only: nothing is synchronised or read back.
int radix_sort_passes(const RadixBufs &b, const btbbx_hit *hits, const RadixPass *passes, int n_passes, int cur, hipStream_t q);
