// scan_launch.h -- the launcher of the access-code scans and the geometry of its segment slots: not part of the exported ABI
// (defined in scan.hip; called from there and from the ordered scan of sort.hip).
#pragma once
#include "common.h"

// one launch of the scan kernel that fits (lap, the tables in force, max_ac_errors).  d_first: first-match mode; bucket_*: every
// record is also counted in the bucket the ordering will put it in; slots: the hits leave through the segment slots; gate: the
// launch returns at once unless *gate != 0.  Nothing is synchronised.
int launch_scan(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
		uint32_t n_streams, uint64_t search_bits, uint32_t lap, int max_ac_errors,
		btbbx_hit *d_hits, uint32_t hit_cap, uint32_t *d_hit_count,
		unsigned long long *d_first, hipStream_t stream, uint32_t *bucket_cnt = nullptr, uint64_t bucket_mul = 0,
		uint32_t bucket_shift = 0, bool msb = false, const ScanSlots *slots = nullptr, const uint32_t *gate = nullptr);
// geometry of the segment slots for a scan of these streams (sort.hip sizes its scratch from it); false: this scan has no slot form
// (LAP_ANY with tables for more than two errors) or more segments than the slots' 31-bit numbers hold
bool scan_slot_geometry(uint64_t search_bits, uint32_t n_streams, uint32_t lap, uint32_t *segs_per_stream, uint64_t *n_segs);
