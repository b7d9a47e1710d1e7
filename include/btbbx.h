/*
 * btbbx.h -- batch (GPU-resident) entry points of the MI355X baseband scanner.
 *
 * Additive to the drop-in API in btbb.h.  Plain C ABI: pointers and sizes only.
 * Everything here runs on the GPU through hand-written gfx950 HIP kernels; there
 * is no CPU fallback -- every entry point fails with BTBBX_E_NODEVICE when no HIP
 * device is usable.
 *
 * Data layout ("packed stream"): LSB-first 64-bit words, stream bit i is bit
 * (i % 64) of word (i / 64), so that the 64-symbol window starting at bit c has
 * the value the reference obtains from air_to_host64(&stream[c], 64)
 * (lib/src/bluetooth_packet.c:235-242).
 *
 * Reference interfaces replaced (relative to /root/reference):
 *   btbbx_scan_*      <- the caller loop around btbb_find_ac, lib/src/btbb.h:82-94,
 *                        lib/src/bluetooth_packet.c:368-464 (all matches, not first)
 *   btbbx_pack_*      <- the one-symbol-per-byte convention of btbb.h:90,116
 *   btbbx_trials_*    <- try_clock + crc_check over the 64 CLK1-6 candidates,
 *                        lib/src/bluetooth_piconet.c:675-690,
 *                        lib/src/bluetooth_packet.c:708-769, 1178-1195
 *   btbbx_decode_*    <- btbb_header_present / btbb_decode_header / btbb_decode_payload,
 *                        lib/src/bluetooth_packet.c:1198-1297, 1371-1408
 *   btbbx_hop_*       <- gen_hops / hop / init_candidates / channel_winnow / btbb_winnow,
 *                        lib/src/bluetooth_piconet.c:311-362, 443-446, 455-498, 575-645
 *   btbbx_hop_reversal_batch_*
 *                     <- btbb_init_hop_reversal + btbb_winnow for many piconets in one call,
 *                        lib/src/bluetooth_piconet.c:455-498, 575-645
 *   btbbx_le_*        <- the LE search in front of lell_allocate_and_decode (the reference
 *                        expects found, dewhitened bytes), lib/src/bluetooth_le_packet.c:282-312
 *   btbbx_survey_*    <- btbb_uap_from_header under the survey mode of btbb_process_packet,
 *                        lib/src/bluetooth_piconet.c:648-750, 807-858
 *   btbbx_survey_clock_jobs_device, btbbx_acquire_host
 *                     <- the step from a settled piconet to its hop reversal in btbb_process_packet / try_hop,
 *                        lib/src/bluetooth_piconet.c:489-490, 510-515, 528-531
 */
#ifndef INCLUDED_BTBBX_H
#define INCLUDED_BTBBX_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the names declared here are exported */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define BTBBX_OK            0
#define BTBBX_E_NODEVICE   -2   /* no usable HIP device / runtime error (see btbbx_last_error) */
#define BTBBX_E_ARG        -3   /* bad argument */
#define BTBBX_E_NOTINIT    -4   /* btbbx_init / btbb_init not called */
#define BTBBX_E_NOMEM      -5

#define BTBBX_LAP_ANY 0xffffffffu
#define BTBBX_MAX_SYMBOLS 3125            /* bluetooth_packet.h:27 */
#define BTBBX_PKT_WORDS 50                /* 3200 bits >= 3125 symbols, one packed packet */

/* one detected access code */
typedef struct btbbx_hit {
	uint64_t offset;      /* symbol index of the first sync-word bit inside its stream */
	uint32_t lap;         /* LAP recovered (LAP_ANY) or searched for */
	uint8_t  ac_errors;   /* as btbb_packet_get_ac_errors() would report */
	uint8_t  reserved;
	uint16_t stream;      /* stream (channel) index of the launch */
} btbbx_hit;

/* result of one (packet, clock) trial: what try_clock + crc_check leave behind */
typedef struct btbbx_trial {
	uint8_t uap;          /* try_clock() return value / pkt->UAP */
	uint8_t type;         /* pkt->packet_type after try_clock */
	int16_t rv;           /* crc_check() return value: 0, 1, 2, 10 or 1000 */
} btbbx_trial;

/* one packet to decode: where it is and what is known about it */
typedef struct btbbx_pkt_in {
	uint32_t length;      /* symbols captured, <= 3125 (btbb_packet_set_data clamps) */
	uint32_t clkn;        /* CLK1-27 as stored by set_data (caller's clkn >> 1) */
	uint32_t flags;       /* packet flags (BTBB_WHITENED etc., btbb.h:27-35) */
	uint8_t  uap;         /* pkt->UAP on entry */
	uint8_t  type;        /* pkt->packet_type on entry (state left by earlier calls) */
	uint8_t  llid;        /* pkt->payload_llid on entry */
	uint8_t  flow;        /* pkt->payload_flow on entry */
} btbbx_pkt_in;

/* everything btbb_decode_header + btbb_decode_payload write into a packet */
typedef struct btbbx_pkt_out {
	int32_t  header_rv;          /* btbb_decode_header() */
	int32_t  payload_rv;         /* btbb_decode_payload() (0 if header failed) */
	int32_t  payload_length;
	int32_t  payload_header_length;
	uint32_t flags;              /* packet flags afterwards */
	uint32_t header_packed;      /* 18 unwhitened header bits */
	uint8_t  header_present;     /* btbb_header_present() */
	uint8_t  type, lt_addr, hdr_flags, hec;
	uint8_t  llid, flow, uap;
	uint64_t payload_header;     /* 16 payload-header bits, LSB first */
	uint64_t payload[43];        /* 2744 payload bits, LSB first */
} btbbx_pkt_out;

/* ---- context ---------------------------------------------------------------- */
/* Build the device tables for searches correcting up to max_ac_errors (0..5) bit
 * errors on the CURRENT HIP device.  Like btbb_init() the first non-zero value wins
 * (bluetooth_packet.c:288-289).  Returns 0 or a negative BTBBX_E_*. */
int btbbx_init(int max_ac_errors);
/* The same for every device of `devices[0..n_devices)` (HIP ordinals); the calling thread's current
 * device is restored.  Needed before btbbx_scan_host_multi; one-process-per-GPU callers just select
 * their device and call btbbx_init / btbb_init.  The tables are the same on every device: the first
 * non-zero max_ac_errors of the PROCESS wins, as with the reference's one global map. */
int btbbx_init_devices(const int *devices, int n_devices, int max_ac_errors);
void btbbx_shutdown(void);
const char *btbbx_last_error(void);
int btbbx_device_count(void);
int btbbx_table_errors(void);          /* the max_ac_errors the tables were built with */
/* Host-only diagnostic, no device needed: the candidate set the LAP_ANY scan probes for every offset that passes
 * the barker filter -- all values of nineteen sliding parity checks of the (64,30) code (gen_syndrome's generator,
 * bluetooth_packet.c:147-159) that a window within max_ac_errors of a sync word can take, as a 2^19-bit set in
 * 16384 words.  *taps (may be NULL) receives the check's tap pattern: check b of a window w is the parity of
 * w & (taps << b), b = 0..18.  Returns the number of members or a negative BTBBX_E_*. */
int btbbx_slide_set(int max_ac_errors, uint32_t *bitmap_words, uint64_t *taps);
/* The same for tables built for THREE or FOUR errors (max_ac_errors = 3 or 4), whose scan tests a survivor in two
 * levels, as the kernel reads them: first_words = a 2^20-bit set (32768 words) over twenty positions of the check
 * taps[0], indexed by the COMPLEMENT of the checks' value (index i, bit i & 31 of word i >> 5); second_words = a
 * 2^24-bit set (524288 words) over twenty-four positions of the check taps[1], index i at bit 31 - (i & 31) of word
 * i >> 5.  A window within max_ac_errors of a sync word is a member of both.  Returns 0 or a negative BTBBX_E_*.
 * max_ac_errors = 5 (first_words may be NULL and is not written): second_words alone = the front set the five-error scan
 * probes before its exact check, the same size and bit order; taps[0] = 0, taps[1] = its check. */
int btbbx_slide_sets_two_level(int max_ac_errors, uint32_t *first_words, uint32_t *second_words, uint64_t *taps);

/* ---- device memory helpers (so C callers need not link HIP themselves) -------- */
void *btbbx_malloc(size_t bytes);
void btbbx_free(void *dptr);
int btbbx_memcpy_h2d(void *dst, const void *src, size_t bytes);
int btbbx_memcpy_d2h(void *dst, const void *src, size_t bytes);
int btbbx_memset(void *dptr, int value, size_t bytes);
int btbbx_sync(void *hip_stream);

/* ---- access-code scan -------------------------------------------------------- */
/* All pointers are DEVICE pointers.  n_streams packed streams of n_words words each
 * lie pitch_words apart; offsets [0, search_bits) of every stream are tested, which
 * needs search_bits + 63 <= 64 * n_words.  Hits are appended (unordered) to d_hits (16-byte aligned),
 * *d_hit_count counts ALL hits even beyond hit_cap.  If the count exceeds hit_cap the hit_cap records
 * that were stored are an UNSPECIFIED subset of the matches (whichever wavefronts came first), not the
 * first ones: size the buffer from the count and scan again, use btbbx_scan_first_device for
 * first-match semantics, or use the host wrappers below, which do this themselves.  The caller zeroes
 * *d_hit_count.  Asynchronous on hip_stream (NULL = the null stream). */
int btbbx_scan_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
		      uint32_t n_streams, uint64_t search_bits,
		      uint32_t lap, int max_ac_errors,
		      btbbx_hit *d_hits, uint32_t hit_cap, uint32_t *d_hit_count,
		      void *hip_stream);

/* The two packed layouts a capture can have in HBM.  BTBBX_FMT_PACKED: LSB-first words (above).  BTBBX_FMT_PACKED_MSB: 8 symbols
 * per byte with the FIRST symbol in bit 7 -- what a dongle's bit-packed dumps look like.  The scan kernels take
 * either: MSB-first dwords are turned round in registers as they are loaded, the capture is not rewritten.  (The packet
 * decoders read LSB-first words: convert once with btbbx_msb_to_lsb_device before handing hits of an MSB capture to them.) */
#define BTBBX_FMT_PACKED  0      /* LSB-first packed words (const uint64_t *) */
#define BTBBX_FMT_SYMBOLS 1      /* one 0/1 symbol per byte (const char *), packed on the GPU (streaming ingest only) */
#define BTBBX_FMT_PACKED_MSB 2   /* 8 symbols per byte, first symbol in bit 7 */
int btbbx_scan_device_fmt(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
			  uint32_t n_streams, uint64_t search_bits,
			  uint32_t lap, int max_ac_errors, int format,
			  btbbx_hit *d_hits, uint32_t hit_cap, uint32_t *d_hit_count,
			  void *hip_stream);

/* First match only (btbb_find_ac semantics) of ONE stream: *d_first receives
 * (offset << 32 | lap << 8 | ac_errors) of the smallest matching offset, or
 * UINT64_MAX.  search_bits < 2^32.  The caller presets *d_first to UINT64_MAX. */
int btbbx_scan_first_device(const uint64_t *d_words, uint64_t n_words, uint64_t search_bits,
			    uint32_t lap, int max_ac_errors, uint64_t *d_first,
			    void *hip_stream);

/* Host convenience wrappers (copy in, scan on the GPU, copy out, sort by
 * (stream, offset)).  Return the number of hits found or a negative BTBBX_E_*.  The count may exceed
 * cap; then the cap records written are the cap SMALLEST (stream, offset) ones -- cap = 1 is the
 * first match of btbb_find_ac (lib/src/bluetooth_packet.c:444-464).  Safe to call from several host
 * threads at once (each call leases its own scratch memory and stream). */
int64_t btbbx_scan_host(const uint64_t *words, uint64_t n_words, uint64_t search_bits,
			uint32_t lap, int max_ac_errors, btbbx_hit *hits, uint64_t cap);
int64_t btbbx_scan_symbols(const char *symbols, uint64_t n_symbols, uint64_t search_length,
			   uint32_t lap, int max_ac_errors, btbbx_hit *hits, uint64_t cap);
/* First match only, from host memory: *first_hit = the match with the smallest offset in
 * [0, search_length) -- what btbb_find_ac returns (lib/src/bluetooth_packet.c:444-464).  Returns 1
 * (found), 0 (none) or a negative BTBBX_E_*.  search_length + 63 <= n_symbols, search_length < 2^32. */
int btbbx_find_first_symbols(const char *symbols, uint64_t n_symbols, uint64_t search_length,
			     uint32_t lap, int max_ac_errors, btbbx_hit *first_hit);

/* Time sharding over several GPUs of one node (no data-path collective): shard k of n
 * owns offsets [first_offset, first_offset + search_bits) of the capture and must be given words
 * [first_word, first_word + n_words) -- its slice plus a 63-symbol halo.  Offsets a shard reports are
 * local; global = first_offset + local.  One-process-per-GPU callers (MPI-style ranks) use
 * the plan directly; btbbx_scan_host_multi applies it over the listed devices with one host thread
 * per device, sorts per device and concatenates.  Every listed device must have been initialised
 * (btbbx_init_devices); a device may be listed more than once. */
typedef struct btbbx_shard {
	uint64_t first_word;      /* first word of the capture this shard reads */
	uint64_t n_words;         /* words it reads (slice + halo), 0 for an empty shard */
	uint64_t search_bits;     /* offsets it tests */
	uint64_t first_offset;    /* = 64 * first_word */
} btbbx_shard;
int btbbx_shard_plan(uint64_t search_bits, uint32_t n_shards, uint32_t shard, btbbx_shard *out);
int64_t btbbx_scan_host_multi(const uint64_t *words, uint64_t n_words, uint64_t search_bits,
			      uint32_t lap, int max_ac_errors, btbbx_hit *hits, uint64_t cap,
			      const int *devices, int n_devices);
void btbbx_sort_hits(btbbx_hit *hits, size_t n);
/* the same order for a hit list still in device memory (the host wrappers and the streaming ingest
 * sort here before copying out); synchronises hip_stream */
int btbbx_sort_hits_device(btbbx_hit *d_hits, uint32_t n, void *hip_stream);
/* The same order with the list's length still in device memory (the counter btbbx_scan_device filled): orders the
 * first min(*d_count, cap) records of d_hits in place -- no host round trip, no synchronisation, all work on
 * hip_stream.  d_scratch: btbbx_order_hits_scratch_bytes(cap) bytes of device memory owned by the caller (16-byte
 * aligned), so callers on different streams share nothing.  Offsets must stay below 2^47. */
size_t btbbx_order_hits_scratch_bytes(uint32_t cap);
int btbbx_order_hits_device(btbbx_hit *d_hits, const uint32_t *d_count, uint32_t cap, void *d_scratch,
			    size_t scratch_bytes, void *hip_stream);
/* ... for the hit list of a btbbx_scan_device call over n_streams streams and search_bits offsets: the same without the
 * pass that looks for the list's largest stream number and offset */
int btbbx_order_scan_hits_device(btbbx_hit *d_hits, const uint32_t *d_count, uint32_t cap, uint32_t n_streams,
				 uint64_t search_bits, void *d_scratch, size_t scratch_bytes, void *hip_stream);
/* btbbx_scan_device with the list coming back in (stream, offset) order: the scan kernels count every record they write in
 * the bucket the ordering will put it in, so the list is not read again for a histogram.  Arguments as btbbx_scan_device plus
 * the ordering scratch (btbbx_order_hits_scratch_bytes(cap)); cap >= 2; nothing is synchronised.  The call zeroes
 * *d_count itself (on hip_stream): the list is built from this call's matches only, records an earlier scan appended
 * are not carried over -- chain scans with btbbx_scan_device and order the whole list once with btbbx_order_hits_device. */
/* Scratch for btbbx_scan_ordered_device over n_streams streams of search_bits offsets each (round 6).  Where the scan has its
 * segment-slot form -- every known-LAP scan, and LAP_ANY with tables for up to two errors -- every wave leaves its hits, ranked,
 * in slots of the segment they lie in (4096 offsets for a known LAP, 4032 for LAP_ANY), and the ordered list is one compaction of
 * those slots: no bucket counters, no scatter, no ranking pass.  The slots take about 22 bytes per segment (two 8-byte slots, a
 * 2-byte count, a 4-byte start index) plus 24 bytes per record of cap for the hits ranked beyond a segment's slots.  The size
 * returned covers that and the general ordering, which stays the fallback for a stream the slots cannot rank (one made of sync
 * words); for LAP_ANY with tables for more errors it equals btbbx_order_hits_scratch_bytes(cap).  A call that is handed
 * btbbx_order_hits_scratch_bytes(cap) bytes only runs the general ordering.  Needs btbb_init / btbbx_init first (the answer
 * depends on the tables). */
size_t btbbx_scan_ordered_scratch_bytes(uint64_t search_bits, uint32_t n_streams, uint32_t lap, uint32_t cap);
int btbbx_scan_ordered_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			      uint64_t search_bits, uint32_t lap, int max_ac_errors, btbbx_hit *d_hits, uint32_t cap,
			      uint32_t *d_count, void *d_scratch, size_t scratch_bytes, void *hip_stream);
int btbbx_scan_ordered_device_fmt(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				  uint64_t search_bits, uint32_t lap, int max_ac_errors, int format, btbbx_hit *d_hits, uint32_t cap,
				  uint32_t *d_count, void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* symbols (one 0/1 byte each, bit 0 is used) -> packed words; n_words_out =
 * ceil(n_symbols / 64), the tail of the last word is zero */
int btbbx_pack_device(const uint8_t *d_symbols, uint64_t n_symbols, uint64_t *d_words,
		      void *hip_stream);
int btbbx_unpack_device(const uint64_t *d_words, uint64_t n_symbols, uint8_t *d_symbols,
			void *hip_stream);
/* bytes holding 8 symbols MSB first (first received symbol in bit 7) -> LSB-first words, in place (for the packet decoders;
 * the scans take BTBBX_FMT_PACKED_MSB directly) */
int btbbx_msb_to_lsb_device(uint64_t *d_words, uint64_t n_words, void *hip_stream);

/* ---- streaming ingest (live captures) ------------------------------ */
/* Feeds a capture to the GPU chunk by chunk: pinned double buffers, asynchronous host->device
 * copies overlapped with the scan of the previous chunk, a one-word carry so that access codes
 * straddling chunk boundaries are found exactly once.  Offsets in the returned hits are global
 * (symbols since btbbx_stream_open).  Every chunk except the last must be a multiple of 64
 * symbols.  feed() returns the hits of the chunk fed BEFORE this one (the current one is still
 * in flight); flush() waits for and returns the rest. */
typedef struct btbbx_stream btbbx_stream;
/* format: BTBBX_FMT_PACKED, BTBBX_FMT_SYMBOLS (packed on the GPU) or BTBBX_FMT_PACKED_MSB (scanned as it is), see above */
btbbx_stream *btbbx_stream_open(uint32_t lap, int max_ac_errors, uint64_t max_chunk_symbols, int format);
int64_t btbbx_stream_feed(btbbx_stream *s, const void *data, uint64_t n_symbols, btbbx_hit *hits, uint64_t cap);
/* zero-copy variant: write the next chunk straight into the pinned staging buffer returned by
 * acquire() (max_chunk_symbols bytes for SYMBOLS, /8 for PACKED), then submit() = feed() minus
 * the memcpy */
void *btbbx_stream_acquire(btbbx_stream *s);
int64_t btbbx_stream_submit(btbbx_stream *s, uint64_t n_symbols, btbbx_hit *hits, uint64_t cap);
int64_t btbbx_stream_flush(btbbx_stream *s, btbbx_hit *hits, uint64_t cap);
void btbbx_stream_close(btbbx_stream *s);

/* ---- synthetic traffic (same generator as libbtbb_amd/synth.py) --------------- */
/* words [first_word, first_word + n_words) of the infinite stream `seed`:
 * iid noise plus one sync word per `stride` symbols (stride >= 512), LAP random or
 * fixed_lap (>= 0), k % err_cycle bit errors in sync-word bits 0..56. */
int btbbx_synth_device(uint64_t *d_words, uint64_t first_word, uint64_t n_words,
		       uint64_t seed, uint32_t stride, int64_t fixed_lap, uint32_t err_cycle,
		       void *hip_stream);

/* ---- packet chain ------------------------------------------------------------ */
/* Cut packets out of packed streams: packet i = bits [offset, offset + length) of
 * stream hits[i].stream, zero padded to BTBBX_PKT_WORDS words. */
int btbbx_gather_packets_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
				const btbbx_hit *d_hits, uint32_t n_packets, uint32_t max_length,
				uint64_t *d_packets, uint32_t *d_lengths, void *hip_stream);

/* 64 clock trials per packet: d_trials[i * 64 + c] = state after try_clock(c) and
 * crc_check(c) run in clock order c = 0..63 on packet i (bluetooth_piconet.c:675-690
 * with GOT_FIRST_PACKET clear).  d_in[i] gives each packet's entry state. */
int btbbx_trials_device(const uint64_t *d_packets, const btbbx_pkt_in *d_in, uint32_t n_packets,
			btbbx_trial *d_trials, void *hip_stream);

/* The HEC-only half of the brute force: d_table[i * 64 + c] = try_clock(c)'s return value (the UAP
 * candidate for CLK1-6 = c, bluetooth_packet.c:1178-1195 / uap_from_hec :693-705) in the low byte
 * and the packet type that clock yields in the high byte; 0 when the header's FEC 1/3 fails.
 * Reads 8 bytes and writes 128 bytes per packet.  d_in may be NULL (all packets whitened);
 * d_table 16-byte aligned. */
int btbbx_uap_table_device(const uint64_t *d_packets, const btbbx_pkt_in *d_in, uint32_t n_packets,
			   uint16_t *d_table, void *hip_stream);

/* header_present + decode_header + decode_payload with the clock / UAP in d_in */
int btbbx_decode_device(const uint64_t *d_packets, const btbbx_pkt_in *d_in, uint32_t n_packets,
			btbbx_pkt_out *d_out, void *hip_stream);

/* The same for packets that still lie in the packed streams: packet i is what
 * btbbx_gather_packets_device would cut out for d_hits[i] (same max_length, same captured
 * length, zeros behind it), decoded without the intermediate 400-byte row.  d_in[i].length is
 * ignored; d_lengths (may be NULL) receives the captured lengths. */
int btbbx_decode_hits_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
			     const btbbx_hit *d_hits, const btbbx_pkt_in *d_in, uint32_t n_packets,
			     uint32_t max_length, btbbx_pkt_out *d_out, uint32_t *d_lengths, void *hip_stream);
/* ... with the number of hits still in device memory: decodes the first min(*d_count, cap) hits (launched for cap);
 * scan -> btbbx_order_hits_device -> this call is the known-LAP chain without a host round trip */
int btbbx_decode_hits_counted_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
				     const btbbx_hit *d_hits, const btbbx_pkt_in *d_in, const uint32_t *d_count,
				     uint32_t cap, uint32_t max_length, btbbx_pkt_out *d_out, uint32_t *d_lengths,
				     void *hip_stream);
/* ... for a capture of ONE piconet, without a btbbx_pkt_in per packet: every packet enters with the state of *entry
 * (a HOST pointer; flags, UAP, type, llid, flow -- what btbb_packet_set_data / btbb_packet_set_uap / the flag setters leave,
 * lib/src/bluetooth_packet.c:467-480; its length is ignored) and the clock entry->clkn + offset / clk_div: CLK1-27 advances
 * once per 625 symbols at 1 Msym/s, so a receiver that knows its clock at the first symbol of the buffer knows it for
 * every access code found in it (the clkn argument of btbb_packet_set_data, lib/src/btbb.h:116).  d_count may be NULL
 * (then cap records are decoded). */
int btbbx_decode_hits_piconet_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
				     const btbbx_hit *d_hits, const uint32_t *d_count, uint32_t cap,
				     const btbbx_pkt_in *entry, uint32_t clk_div, uint32_t max_length,
				     btbbx_pkt_out *d_out, uint32_t *d_lengths, void *hip_stream);
/* The call above takes symbol 0 of the buffer for the FIRST symbol of a slot.  A buffer that starts clk_phase symbols
 * into a slot (0 <= clk_phase < clk_div) is decoded with the clock entry->clkn + (offset + clk_phase) / clk_div: without the
 * phase, every access code behind the next slot boundary would get a clock one too low and fail its header check. */
int btbbx_decode_hits_piconet_phase_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
					   const btbbx_hit *d_hits, const uint32_t *d_count, uint32_t cap,
					   const btbbx_pkt_in *entry, uint32_t clk_div, uint32_t clk_phase, uint32_t max_length,
					   btbbx_pkt_out *d_out, uint32_t *d_lengths, void *hip_stream);

/* ---- piconet survey: UAP and CLK1-6 for every LAP of a hit list -------------------------------- */
/* What the reference's survey mode (btbb_init_survey / btbb_process_packet / btbb_next_survey_result,
 * bluetooth_piconet.c:807-858) leaves in one piconet after it has seen every packet of a list.  The packets of a LAP
 * are taken in ascending (offset, stream), whatever the order of the list; for each one, on a piconet that starts as
 * btbb_piconet_new + btbb_init_piconet(lap) leave it,
 *     btbb_piconet_set_channel_seen(pn, channel);
 *     if (btbb_header_present(pkt) && !flag(pn, BTBB_UAP_VALID)) btbb_uap_from_header(pkt, pn);
 * with every branch of btbb_uap_from_header (:648-750): the walk over 64 or the live candidates, the first CRC success
 * ending it (candidates above it keep their value), settling by elimination, the reset when none is left and the reset
 * after MAX_PATTERN_LENGTH packets.  What the reference prints is in the record instead. */
typedef struct btbbx_survey_rec {      /* 64 bytes */
	uint32_t lap;
	uint32_t flags;                  /* piconet flags as the reference leaves them (LAP_VALID, GOT_FIRST_PACKET, UAP_VALID, CLK6_VALID) */
	uint8_t  uap, clk_offset, used_channels;
	uint8_t  settled_by;             /* 0 not settled, 1 elimination ("UAP = ..."), 2 CRC ("Correct CRC! ...") */
	uint8_t  afh_map[10];            /* channels seen, over ALL packets of the LAP */
	uint16_t first_stream;           /* first packet of the LAP in time order: its stream ... */
	uint32_t n_packets;              /* hits with this LAP */
	uint32_t n_walked;               /* calls of btbb_uap_from_header the loop above makes */
	uint32_t n_resets;               /* remaining == 0 resets + "Oops" resets */
	uint32_t settled_after;          /* total_packets_observed as the reference prints it, 0 if not settled */
	uint32_t settled_hit;            /* index into d_hits of the settling packet, UINT32_MAX if none */
	int32_t  packets_observed, total_packets_observed;
	uint32_t first_pkt_time;
	uint64_t first_offset;           /* ... and its offset */
} btbbx_survey_rec;

/* Device scratch the survey of a list of up to cap hits needs (about 760 bytes per hit: sort keys, the gathered packets and
 * their 64-clock trial tables).  Host only, no device needed. */
size_t btbbx_survey_scratch_bytes(uint32_t cap);
/* Surveys the first min(*d_count, cap) records of d_hits (d_count may be NULL: then cap records), in any order.  A packet is a
 * hit: LAP = hit.lap (24 bits), channel = channels[hit.stream] (the stream index when channels is NULL), clock
 * entry->clkn + (offset + clk_phase) / clk_div as in btbbx_decode_hits_piconet_phase_device (uint32_t arithmetic), symbols and
 * captured length as btbbx_gather_packets_device cuts them out with the same max_length, entry state *entry.  channels and entry
 * are HOST pointers; a channel table covers at most 256 streams.  The list must come from a scan of the same geometry:
 * offsets below 64 * n_words <= 2^40, streams below n_streams.  (A hit outside it is not a fault -- it is surveyed as an empty
 * packet that marks no channel -- but where it falls among the packets of its LAP, and so first_offset / first_stream of that
 * record, is unspecified.)  The gather, trial and walk stages work on the list's length, not on cap; scratch and launch sizes
 * follow cap.
 * Records come in ASCENDING LAP order -- btbb_next_survey_result hands piconets out in order of first appearance; sort by
 * (first_offset, first_stream) to restore that.  *d_rec_count counts all piconets; when it exceeds rec_cap the rec_cap smallest
 * LAPs are stored.  d_candidates (may be NULL) receives the 64 clock6_candidates of every stored record.  d_scratch:
 * btbbx_survey_scratch_bytes(cap) bytes, 16-byte aligned, owned by the caller.  Asynchronous on hip_stream, no host round trip.
 * BTBBX_E_ARG before any launch for: a channel above 78, more than 79 streams without a channel table, clk_div = 0,
 * clk_phase >= clk_div, scratch too small, misaligned pointers. */
int btbbx_survey_hits_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			     const btbbx_hit *d_hits, const uint32_t *d_count, uint32_t cap,
			     const uint8_t *channels, const btbbx_pkt_in *entry, uint32_t clk_div, uint32_t clk_phase, uint32_t max_length,
			     btbbx_survey_rec *d_recs, uint32_t rec_cap, uint32_t *d_rec_count, int16_t *d_candidates,
			     void *d_scratch, size_t scratch_bytes, void *hip_stream);
/* Host wrapper: copy in, btbbx_scan_ordered_device with LAP_ANY (repeated with room for every match when its first buffer was
 * too small, as btbbx_scan_host does), survey with scratch sized from the number of hits found, copy out.  Every packet enters as btbb_find_ac +
 * btbb_packet_set_data leave it (BTBB_WHITENED set, nothing else known), with the stored clock (CLK1-27, what
 * btbb_packet_set_data keeps of its clkn argument) clkn0 + (offset + clk_phase) / clk_div.  Returns the number of piconets
 * or a negative BTBBX_E_*; when that exceeds rec_cap the rec_cap smallest LAPs are returned.  candidates may be NULL.
 * Safe to call from several host threads at once. */
int64_t btbbx_survey_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			  uint64_t search_bits, int max_ac_errors, const uint8_t *channels,
			  uint32_t clkn0, uint32_t clk_div, uint32_t clk_phase,
			  btbbx_survey_rec *recs, uint64_t rec_cap, int16_t *candidates);

/* ---- Bluetooth LE 1M scan (Core v5.x Vol 6 Part B 2.1, 3.1.1, 3.2) ------------------------- */
/* Finds preamble + access address (AA) in demodulated LE captures (packed streams as above, one per RF channel),
 * dewhitens with the channel's LFSR, reads the PDU length from the header, checks the CRC-24 and derives what
 * lell_allocate_and_decode (lib/src/bluetooth_le_packet.c:282-312) derives from the dewhitened bytes.  The lell_*
 * entry points themselves still abort: this is the batch path in front of them. */
#define BTBBX_LE_ADV_AA       0x8e89bed6u
#define BTBBX_LE_ADV_CRC_INIT 0x555555u
#define BTBBX_LE_MAX_BYTES    64          /* lell_packet.symbols, bluetooth_le_packet.h:30 */
#define BTBBX_LE_MAX_ERRORS   4

/* Stage 1: the pattern search.  Arguments as btbbx_scan_device, except:
 *   - offsets [0, search_bits) are tested for the first PREAMBLE bit, which needs search_bits + 39 <= 64 * n_words;
 *   - a match is <= max_errors (0..4) mismatches over the 40 bits preamble + AA;
 *   - the records are btbbx_hit with offset = first preamble bit, lap = the 32 AA bits AS RECEIVED,
 *     ac_errors = mismatches over the 40 bits, stream = stream index.
 * btbbx_order_hits_device / btbbx_sort_hits order them unchanged. */
int btbbx_le_scan_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			 uint64_t search_bits, uint32_t aa, int max_errors,
			 btbbx_hit *d_hits, uint32_t hit_cap, uint32_t *d_hit_count, void *hip_stream);

/* one decoded LE packet (104 bytes) */
typedef struct btbbx_le_pkt {
	uint64_t offset;            /* first preamble bit in its stream */
	uint16_t stream;
	uint8_t  aa_errors;         /* mismatches over preamble + AA */
	uint8_t  crc_ok;            /* 1 iff complete and crc_calc == crc_rx */
	uint32_t crc_rx;            /* the 24 CRC bits as received: bit i = the i-th CRC bit on air (register position 23 - i) */
	uint32_t crc_calc;          /* the CRC over the PDU in the same orientation */
	uint16_t pdu_bytes;         /* 2 + L: the octets the CRC covered (L = header octet 1, all 8 bits) */
	uint8_t  truncated;         /* the stream ended before the last CRC bit (bits past it read as 0); crc_ok = 0 */
	/* what lell_allocate_and_decode(bytes, phys_channel, 0, &p) derives (bluetooth_le_packet.c:282-312) */
	uint8_t  channel_idx;
	uint8_t  channel_k;
	uint8_t  is_data;
	uint8_t  length;            /* header octet 1 masked as the reference does: 0x3f advertising, 0x1f data */
	uint8_t  adv_type;
	uint8_t  adv_tx_add;
	uint8_t  adv_rx_add;
	uint8_t  access_address_ok;
	uint8_t  access_address_offenses;
	uint32_t access_address;    /* as received */
	uint8_t  bytes[BTBBX_LE_MAX_BYTES]; /* the received AA (4 octets), then the dewhitened header, payload and CRC; zero past the end */
} btbbx_le_pkt;

/* Stage 2: dewhiten + CRC + decode the first min(*d_count, cap) hits; the count stays in device memory.
 * d_phys_channel: one uint16 per stream, the RF frequency in MHz (lell_allocate_and_decode's phys_channel).
 * crc_init: CRCInit, 24 bits (BTBBX_LE_ADV_CRC_INIT on the advertising channels). */
int btbbx_le_decode_hits_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
				const btbbx_hit *d_hits, const uint32_t *d_count, uint32_t cap,
				const uint16_t *d_phys_channel, uint32_t crc_init,
				btbbx_le_pkt *d_out, void *hip_stream);

/* Host wrapper: copy in, scan, order by (stream, offset), decode, copy out.  Returns the number of matches found
 * or a negative BTBBX_E_*.  When that exceeds cap, the cap SMALLEST (stream, offset) records are returned, as
 * btbbx_scan_host does.  Safe to call from several host threads at once. */
int64_t btbbx_le_scan_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			   uint64_t search_bits, const uint16_t *phys_channel, uint32_t aa, uint32_t crc_init,
			   int max_errors, btbbx_le_pkt *pkts, uint64_t cap);

/* ---- promiscuous LE connection discovery: access address and CRCInit ------------------------- */
/* On the 37 data channels every connection has an AA and a CRCInit of its own; these entries find both without being
 * told either.  Offset o of stream s is a CANDIDATE iff
 *   1. le_channel_index(phys_channel[s]) < 37 (an advertising channel yields no candidates);
 *   2. bits o .. o+7 alternate and bit o equals bit o+8 (the preamble of the AA behind it), no error allowed;
 *   3. the AA = bits o+8 .. o+39 has no data-channel offense (aa_data_channel_offenses, bluetooth_le_packet.c:100-242);
 *   4. the two dewhitened header octets have (h0 & 3) != 0, (h0 & 0xe0) == 0 and h1 <= max_len;
 *   5. the packet lies in the stream: o + 40 + 8 * (2 + h1 + 3) <= 64 * n_words;
 *   6. o < search_bits.
 * Its CRCInit is the one 24-bit preset with which the CRC over the 2 + h1 PDU octets equals the received CRC: the value to
 * hand to btbbx_le_decode_hits_device.  Noise yields candidates as well (2.7e-5 of the offsets at max_len 27); a connection
 * shows as the same (AA, CRCInit) again and again, on several channels. */
typedef struct btbbx_le_cand {   /* 24 bytes */
	uint64_t offset;         /* first preamble bit */
	uint32_t access_address;
	uint32_t crc_init;       /* as btbbx_le_decode_hits_device takes it */
	uint16_t stream;
	uint8_t  header0, length; /* dewhitened h0, h1 */
	uint32_t conn;           /* from the scan: the data channel index (0..36); after grouping: index into the connection
	                          * list, 0xffffffff = none */
} btbbx_le_cand;
typedef struct btbbx_le_conn {   /* 32 bytes */
	uint32_t access_address, crc_init;
	uint32_t n_packets, n_empty; /* members; members with length 0 */
	uint64_t channel_mask;   /* bit ch set iff a member lies on data channel index ch (a shifted alias of a connection shows the
	                          * same mask: btbbx_le_track_device ranks aliases away by the hop check) */
	uint64_t first;          /* index of its first member in the sorted candidate list */
} btbbx_le_conn;

/* Stage 1: every candidate of offsets [0, search_bits) of every stream, in no particular order.  Arguments and their check as
 * btbbx_le_scan_device (search_bits + 39 <= 64 * n_words); d_phys_channel: one uint16 per stream, the RF frequency in MHz;
 * max_len 0..255 (27: the 4.0 / 4.1 maximum, 0: empty PDUs only).  *d_cand_count (zeroed by the caller) counts every candidate,
 * also those past cand_cap, which are dropped.  d_cands: 8-byte aligned. */
int btbbx_le_discover_scan_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				  uint64_t search_bits, const uint16_t *d_phys_channel, uint32_t max_len,
				  btbbx_le_cand *d_cands, uint32_t cand_cap, uint32_t *d_cand_count, void *hip_stream);

/* Stage 2: the first min(*d_cand_count, cand_cap) candidates are sorted stably by (AA << 24 | CRCInit, stream, offset) in
 * place; every group of equal (AA, CRCInit) with at least min_count members becomes one btbbx_le_conn, in ascending (AA, CRCInit)
 * order; every candidate's conn (on entry its channel index) becomes the index of its connection or 0xffffffff.
 * *d_conn_count counts every such group; the conn_cap smallest are stored.  Nothing is read back: both counts stay in device
 * memory.  d_scratch: btbbx_le_discover_scratch_bytes(cand_cap) bytes, 16-byte aligned.
 * A list that does not come from the scan must keep the scan's promises: conn = the data channel index of the candidate's
 * stream (only its low six bits are read, nothing is validated: a wrong value gives a wrong channel_mask), and offsets
 * below 2^48 (the sort keys carry 48 offset bits; the scan's argument check keeps its own offsets below 2^46). */
size_t btbbx_le_discover_scratch_bytes(uint32_t cand_cap);
int btbbx_le_discover_group_device(btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap, uint32_t min_count,
				   btbbx_le_conn *d_conns, uint32_t conn_cap, uint32_t *d_conn_count,
				   void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* Host wrapper: copy in, scan (repeated with room for every candidate when the first buffer was too small, as
 * btbbx_scan_host does), group, copy out.  Returns the number of connections or a negative BTBBX_E_*; when that exceeds
 * conn_cap the conn_cap smallest (AA, CRCInit) are returned.  cands may be NULL (cand_cap 0); otherwise it receives the first
 * cand_cap candidates of the sorted list.  *n_cands_out (may be NULL) = all candidates found.  Safe to call from several host
 * threads at once. */
int64_t btbbx_le_discover_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			       uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
			       btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
			       uint64_t *n_cands_out);

/* ---- LE connection tracking: interval, event counters, hop increment and hop check ----------- */
/* Behind the grouping, for every stored connection: its packets in time order, its connection events, the connection interval,
 * the event counter of every event, the hop increment of channel selection algorithm #1, and for every packet whether it lies
 * on the channel that selection predicts -- the check that tells a connection from its shifted aliases, whose groups hop with
 * it only by accident.  All arithmetic is integer arithmetic.  With N = min(*d_cand_count, cand_cap), K = min(*d_conn_count,
 * conn_cap), and bit o of every stream received at the same instant (the survey's premise), unit_bits bits being 1.25 ms (1250
 * at one sample per symbol):
 *   1. MEMBERS.  Candidate i < N is a member of connection g < K iff conn == g, stream < n_streams and
 *      ch = le_channel_index(d_phys_channel[stream]) < 37; any other candidate gets sixteen 0xff bytes as its record.
 *   2. TIME ORDER.  The members of g by ascending (offset, stream), ties by list index; rank = the position in that order.
 *   3. EVENTS.  end_m = offset_m + 80 + 8 * length_m.  In time order member m opens a new event iff it is the first member, or
 *      ch_m != ch_(m-1), or offset_m > end_(m-1) + ifs_bits.  Event e has the anchor A_e (the offset of its first member) and the
 *      channel C_e; first_anchor = A_0, map_mask = OR of 1 << C_e, n_used its popcount.
 *   4. INTERVAL.  D_e = A_(e+1) - A_e, q_e = (D_e + unit_bits / 2) / unit_bits; the pair FITS iff q_e >= 1 and
 *      |D_e - q_e * unit_bits| <= jitter_bits; n_fit counts the fitting pairs, interval = the gcd of their q_e (64 bits; 0 when
 *      none fits).  TIMED iff 6 <= interval <= 3200.
 *   5. COUNTERS (TIMED).  P = interval * unit_bits, k_e = (D_e + P / 2) / P, n_0 = 0, n_(e+1) = n_e + k_e in 64 bits.
 *   6. HOP INCREMENT (TIMED).  used[] = the channels of map_mask, ascending.  V(c) = {c}; with BTBBX_LE_TRACK_REMAP also every v
 *      in 0..36 outside map_mask with used[v mod n_used] == c (the remapping, with the observed map taken as the connection's).
 *      S(h, u), h in 5..16, u in 0..36 = the number of events with (u + h * n_e) mod 37 in V(C_e).  The pair with the largest S
 *      wins, ties to the smallest h, then the smallest u; n_second = the largest S of any other pair; HOPPING iff
 *      S(winner) > n_second.
 *   7. PREDICTION (TIMED).  unmapped_e = (first_unmapped + hop_increment * n_e) mod 37; expected_e = unmapped_e if map_mask
 *      holds it, else with REMAP used[unmapped_e mod n_used], else 0xff; on_hop = expected_e == C_e.  n_on_hop and n_off_hop
 *      count EVENTS (an unknown prediction in neither), so n_on_hop == S(winner).  Every packet carries its event's values.
 * Not TIMED: hop_increment, first_unmapped, n_on_hop, n_off_hop, n_second and every packet's counter and on_hop are 0, unmapped
 * and expected 0xff; everything else is written all the same.  A connection without a member: a record of zeros.
 * LIMITS, which follow from the rules: the counter is relative to the first event SEEN; an interval whose visible event spacings
 * are all multiples of k comes out k times too large (two events two intervals apart: doubled); a used channel that never shows
 * makes the remapping wrong; a parameter or channel map update inside the capture is not followed by this stage (with the
 * CONNECT_IND in the capture, btbbx_le_seed_device and btbbx_le_epoch_device lift all three). */
#define BTBBX_LE_TRACK_REMAP   1u   /* flags: score and predict through the remapping of the observed channel map */
#define BTBBX_LE_TRACK_TIMED   1u   /* btbbx_le_track.flags: 6 <= interval <= 3200 */
#define BTBBX_LE_TRACK_HOPPING 2u   /* btbbx_le_track.flags: TIMED and n_on_hop > n_second */

typedef struct btbbx_le_track {      /* 48 bytes, one per stored connection */
	uint64_t first_anchor;       /* offset of the first event's first packet */
	uint64_t map_mask;           /* bit c: some event lies on data channel index c */
	uint32_t n_events, n_fit;    /* events; consecutive event pairs that fit the 1.25 ms grid */
	uint32_t interval;           /* in units of 1.25 ms; 0: no fitting pair; a gcd >= 2^32 is stored as 0xffffffff */
	uint32_t n_on_hop, n_off_hop;/* TIMED: events whose channel is / is not the predicted one (unknown predictions count in neither) */
	uint32_t n_second;           /* TIMED: the best score of any other (hop increment, first unmapped channel) pair */
	uint8_t  hop_increment, first_unmapped, n_used, flags;
	uint32_t reserved;           /* written as 0 */
} btbbx_le_track;

typedef struct btbbx_le_track_pkt {  /* 16 bytes, one per candidate, parallel to the sorted candidate list */
	uint32_t rank;               /* position among its connection's members in time order */
	uint32_t event;              /* index of its event within the connection */
	uint32_t counter;            /* low 32 bits of the event counter relative to the first event seen; 0 unless TIMED */
	uint8_t  channel;            /* data channel index of its stream */
	uint8_t  unmapped, expected; /* TIMED: unmappedChannel of its event, the channel predicted for it; else 0xff */
	uint8_t  on_hop;             /* expected == channel */
} btbbx_le_track_pkt;              /* a candidate that is no member of a stored connection: sixteen 0xff bytes */

/* The input is what btbbx_le_discover_group_device leaves: the sorted list, every candidate's conn, the connection count.  A
 * list from elsewhere must keep its promises: the members of g are exactly the candidates [conns[g].first, first + n_packets),
 * and offsets lie below 2^48 (the sort keys carry 48 offset bits).  d_tracks[0 .. K) and d_pkts[0 .. N) are written, every byte
 * of them, nothing behind them; nothing is read back and the call is asynchronous on hip_stream.  d_scratch:
 * btbbx_le_track_scratch_bytes(cand_cap, conn_cap) bytes (about 48 per candidate and 1.8 KiB per connection).  BTBBX_E_ARG,
 * before any launch: a null pointer, a record or scratch pointer that is not 8-byte aligned (the counters: 4, the channels: 2),
 * n_streams == 0, unit_bits < 2, jitter_bits >= unit_bits / 2, a scratch that is too small.  cand_cap == 0 or conn_cap == 0
 * succeeds and writes nothing. */
size_t btbbx_le_track_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap);
int btbbx_le_track_device(const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
			  const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
			  const uint16_t *d_phys_channel, uint32_t n_streams,
			  uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
			  btbbx_le_track *d_tracks, btbbx_le_track_pkt *d_pkts,
			  void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* Host wrapper: btbbx_le_discover_host, then the tracking on the same stream, copy out.  The discovery's arguments and return
 * value; tracks: conn_cap records, parallel to conns; pkts (may be NULL): cand_cap records, parallel to cands.  Safe to call from
 * several host threads at once. */
int64_t btbbx_le_track_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			    uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
			    btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
			    uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
			    btbbx_le_track *tracks, btbbx_le_track_pkt *pkts);

/* ---- LE channel selection algorithm #2: event counter recovery and hop check ----------------- */
/* Two Bluetooth 5 devices hop by channel selection algorithm #2 (Core Vol 6 Part B 4.5.8.3), which the tracking above reports as
 * TIMED but not HOPPING.  #2 has no increment to fit: the channel of an event is a function of the absolute 16-bit
 * connEventCounter, the channel identifier chId = (AA >> 16) ^ (AA & 0xffff) and the channel map.  The tracking gives every
 * event a counter relative to the first event seen, so one unknown is left, the absolute counter of that first event; this stage
 * tries all 65 536 and reports the one that explains most events, the prediction for every packet, and which of the two
 * algorithms explains the connection.  It runs behind the tracking, on what the tracking wrote.  All arithmetic is integer
 * arithmetic.  With N = min(*d_cand_count, cand_cap), K = min(*d_conn_count, conn_cap), and cands, tracks and pkts exactly what
 * btbbx_le_discover_group_device and btbbx_le_track_device left:
 *   1. MEMBERS.  Candidate i < N is a member of g < K iff cands[i].conn == g and pkts[i].rank != 0xffffffff; every other
 *      candidate gets eight 0xff bytes as its record.  A member's event is pkts[i].event, its channel C_e = pkts[i].channel, its
 *      relative counter n_e = pkts[i].counter mod 2^16 (the stored low 32 bits suffice: 2^16 divides 2^32); all members of an
 *      event carry the same values.  The map is tracks[g].map_mask, n_used its popcount (tracks[g].n_used), used[] its channels
 *      in ascending order.
 *   2. EVALUATED iff the track is TIMED.  Otherwise the record is channel_id with every other field 0, and the members get
 *      counter 0, prn 0, unmapped = expected = 0xff, on_hop 0.
 *   3. PRN.  prn_e(c): x = c ^ chId; three times: reverse the bits within each of the two bytes of x, then
 *      x = (17 * x + chId) mod 2^16; prn_e = x ^ chId.
 *   4. PREDICTION.  unmapped(c) = prn_e(c) mod 37; expected(c) = unmapped(c) if the map holds it, else with BTBBX_LE_CSA2_REMAP
 *      used[(n_used * prn_e(c)) >> 16], else 0xff (unknown).
 *   5. SCORE.  For c0 in 0..65535, S(c0) = the number of EVENTS with expected((c0 + n_e) mod 2^16) == C_e.  The largest S wins,
 *      ties to the smallest c0: counter0 = the winner, n_on = S(winner), n_second = the largest S of any other c0, n_off = the
 *      events whose prediction under the winner is known and differs.
 *   6. PACKETS.  A member packet of an EVALUATED connection gets counter = (counter0 + n_e) mod 2^16, that counter's prn,
 *      unmapped and expected, and on_hop = (expected == channel).
 * LIMITS, which follow from the rules: the observed map stands in for the connection's, so a used channel that never shows makes
 * the remapping wrong; with few events, or a map of one or two channels, many hypotheses tie (full map, REMAP, 200 random draws:
 * the winner was unique and right in 22 of them at 6 events, 197 at 8, 200 at 12); a channel map update inside the capture is not
 * followed by this stage (btbbx_le_epoch_device does, from the CONNECT_IND); the tracking's limits on the relative counters carry
 * over. */
#define BTBBX_LE_CSA2_REMAP     1u  /* flags argument: as BTBBX_LE_TRACK_REMAP */
#define BTBBX_LE_CSA2_EVALUATED 1u  /* btbbx_le_csa2.flags: the connection's track is TIMED */
#define BTBBX_LE_CSA2_UNIQUE    2u  /* EVALUATED and n_on > n_second */
#define BTBBX_LE_CSA2_PREFERRED 4u  /* UNIQUE and n_on > the track's n_on_hop: algorithm #2 explains more events than #1 */

typedef struct btbbx_le_csa2 {       /* 24 bytes, one per stored connection, parallel to conns / tracks */
	uint32_t n_on, n_off;        /* events on / off the predicted channel (unknown predictions in neither) */
	uint32_t n_second;           /* the best score of any other counter hypothesis */
	uint16_t channel_id;         /* (AA >> 16) ^ (AA & 0xffff) */
	uint16_t counter0;           /* connEventCounter of the first event seen */
	uint32_t flags;
	uint32_t reserved;           /* written as 0 */
} btbbx_le_csa2;

typedef struct btbbx_le_csa2_pkt {   /* 8 bytes, one per candidate, parallel to the sorted candidate list */
	uint16_t counter;            /* connEventCounter of its event */
	uint16_t prn;                /* prn_e of that counter */
	uint8_t  unmapped, expected, on_hop, reserved;  /* reserved written as 0 */
} btbbx_le_csa2_pkt;                 /* a candidate that is no member of a stored connection: eight 0xff bytes */

/* d_sel[0 .. K) and d_sel_pkts[0 .. N) are written, every byte of them, nothing behind them; nothing is read back and the call is
 * asynchronous on hip_stream.  Only bit 0 of flags is read.  d_scratch: btbbx_le_csa2_scratch_bytes(cand_cap, conn_cap) bytes =
 * 256 + 4 * (conn_cap + 1) + 4 * cand_cap + 1024 * conn_cap, each term rounded up to a multiple of 256 (a cap of 0 counts as 1):
 * the counts, the event bases, the event table and 64 partial results per connection.  BTBBX_E_ARG, before any launch: a null
 * pointer, a record or scratch pointer that is not 8-byte aligned (the counters: 4), a scratch that is too small.  cand_cap == 0
 * or conn_cap == 0 succeeds and writes nothing. */
size_t btbbx_le_csa2_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap);
int btbbx_le_csa2_device(const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
			 const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
			 const btbbx_le_track *d_tracks, const btbbx_le_track_pkt *d_pkts, uint32_t flags,
			 btbbx_le_csa2 *d_sel, btbbx_le_csa2_pkt *d_sel_pkts,
			 void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* Host wrapper: btbbx_le_track_host's chain with this stage queued behind the tracking on the same stream, copy out.  Its
 * arguments (flags & 1 serves both stages) and return value; sel: conn_cap records, parallel to conns; sel_pkts (may be NULL):
 * cand_cap records, parallel to cands.  Safe to call from several host threads at once. */
int64_t btbbx_le_csa2_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			   uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
			   btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
			   uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
			   btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_csa2 *sel, btbbx_le_csa2_pkt *sel_pkts);

/* ---- LE following from CONNECT_IND: absolute event counters, channel map updates -------------- */
/* The three limits the tracking and algorithm #2 share -- the observed map stands in for the connection's, the counter is
 * relative to the first event seen, an update inside the capture is not followed -- go away when the capture holds what a sniffer
 * follows: the CONNECT_IND on an advertising channel (AA, CRCInit, the true map, hop increment, interval, transmit window, ChSel;
 * the fields lell_print decodes, bluetooth_le_packet.c:627-647) and the LL_CHANNEL_MAP_IND / LL_CONNECTION_UPDATE_IND control
 * PDUs inside the connection, each with an absolute instant.  Two stages behind the tracking; a third beside the second,
 * btbbx_le_span_device further below, goes on through the parameter updates at which the second stops.  All arithmetic is
 * integer arithmetic, 64 bits wide where a sum can leave 32.
 *
 * SEED.  With M = min(*d_adv_count, adv_cap) records as btbbx_le_decode_hits_device leaves them for a scan with BTBBX_LE_ADV_AA /
 * BTBBX_LE_ADV_CRC_INIT, K = min(*d_conn_count, conn_cap), and bytes[] counted from the first AA octet (the payload starts at 6):
 *   1. REQUEST.  Record j is a request iff crc_ok == 1, truncated == 0, is_data == 0, adv_type == 5 and length == 34.  InitA =
 *      bytes 6..11, AdvA = 12..17, AA = LE32 at 18, CRCInit = LE24 at 22 (the integer btbbx_le_conn.crc_init holds), WinSize =
 *      [25], WinOffset = LE16 at 26, Interval = LE16 at 28, Latency = LE16 at 30, Timeout = LE16 at 32, map = the low 37 bits of
 *      the LE40 at 34, Hop = [39] & 0x1f, SCA = [39] >> 5, ChSel = (bytes[4] >> 5) & 1, TxAdd / RxAdd = bits 6 / 7 of bytes[4].
 *   2. VALID iff 5 <= Hop <= 16, 6 <= Interval <= 3200, popcount(map) >= 2, 1 <= WinSize <= min(8, Interval - 1) and
 *      WinOffset <= Interval.  Any other request is ignored.
 *   3. JOIN.  R = offset + 352, the request's last CRC bit + 1.  Connection g takes, among the valid requests with its (AA,
 *      CRCInit) and R <= tracks[g].first_anchor, the one with the largest (offset, stream), ties to the largest j.  None: the
 *      record is all zero, the connection is not SEEDED.
 *   4. RECORD.  flags = SEEDED, t0 = R + unit_bits * (1 + WinOffset) -- the start of the transmit window, transmitWindowDelay
 *      being 1.25 ms --, the fields of rule 1, request = j.
 * A caller may write seeds itself, from a CONNECT_IND seen elsewhere: the follow stage reads flags, t0, map, interval, hop and
 * chsel, nothing else.  LIMIT: a request whose connection never shows seeds nothing. */
#define BTBBX_LE_SEED_SEEDED 1u      /* btbbx_le_seed.flags */

typedef struct btbbx_le_seed {       /* 56 bytes, one per stored connection, parallel to conns / tracks */
	uint64_t t0;                 /* first bit of the transmit window */
	uint64_t map;                /* ChM, 37 bits */
	uint32_t access_address, crc_init;
	uint32_t request;            /* index of the request among the advertising records */
	uint16_t interval, win_offset, latency, timeout;
	uint8_t  win_size, hop, sca, chsel;
	uint8_t  init_a[6], adv_a[6];
	uint8_t  tx_add, rx_add;     /* the address types of InitA / AdvA */
	uint8_t  flags;
	uint8_t  reserved;           /* written as 0 */
} btbbx_le_seed;

/* d_seeds[0 .. K) is written, every byte of it, nothing behind it; one launch, asynchronous on hip_stream, nothing read back.
 * BTBBX_E_ARG, before any launch: a null pointer (d_adv may be NULL with adv_cap == 0), a record pointer that is not 8-byte
 * aligned (the counters: 4), unit_bits < 2.  conn_cap == 0 succeeds and writes nothing; adv_cap == 0 seeds nothing. */
int btbbx_le_seed_device(const btbbx_le_pkt *d_adv, const uint32_t *d_adv_count, uint32_t adv_cap,
			 const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
			 const btbbx_le_track *d_tracks, uint32_t unit_bits, btbbx_le_seed *d_seeds, void *hip_stream);

/* FOLLOW.  N, K, members, time order, events, anchors A_e and channels C_e are the tracking's (its rules 1-3), read from
 * pkts[i].rank / event / channel, the candidates' offsets and conns[g].first: candidate i < N is a member of g < K iff
 * cands[i].conn == g and pkts[i].rank != 0xffffffff; the event's anchor is the offset of its member of the smallest rank.  A
 * candidate that is no member gets twelve 0xff bytes.  A connection that is not SEEDED gets a zero record; its members get counter
 * 0, epoch 0, expected 0xff, on_hop 0, state 0, and kind and opcode as rule 3 gives them.  For a SEEDED connection, with
 * P = interval * unit_bits:
 *   1. FIRST.  Event e is BEFORE iff A_e + jitter_bits < t0.  f = the first event that is not BEFORE;
 *      c_f = (A_f + jitter_bits - t0) / P, by floor.  Every event BEFORE: nothing is counted.
 *   2. COUNTERS.  For e >= f, c_(e+1) = c_e + (A_(e+1) - A_e + P / 2) / P in 64 bits: the tracking's rule 5 with the seed's
 *      interval, not the fitted one.
 *   3. CONTROL PDUs.  Member m is CONTROL iff (header0 & 3) == 3 and length >= 1.  Its payload octets (the first 12 at most)
 *      are read from its stream behind the header, bits beyond the stream's end as 0, and dewhitened with the channel's sequence
 *      continued behind the two header octets; opcode = payload octet 0.  In time order the first CONTROL member with opcode 5
 *      and length 1 (LL_START_ENC_REQ) is ENC_START and sets ENCRYPTED; CONTROL members of larger rank are OPAQUE (opcode 0xff,
 *      never parsed).  Otherwise: MAP UPDATE iff opcode 1 and length 8 (map' = the low 37 bits of octets 1..5, instant = LE16 of
 *      octets 6..7); PARAM UPDATE iff opcode 0 and length 12 (instant = LE16 of octets 10..11); TERMINATE iff opcode 2 and
 *      length 2 (it sets TERMINATED).  An update PDU in a counted (not BEFORE) event with counter c has delta = (instant - c) mod
 *      2^16; it is VALID iff delta < 32767 and, for a map update, popcount(map') >= 2; its absolute instant is I = c + delta.  An
 *      update in a BEFORE event is ignored.
 *   4. STOP.  stop = the smallest I of any valid PARAM UPDATE, 2^64 - 1 without one.  Event e is BEYOND iff c_e >= stop.  A MAP
 *      UPDATE whose own event is BEYOND is ignored.
 *   5. MAP IN FORCE.  M_e = map' of the valid, unignored MAP UPDATE with the largest (I, rank) among those with I <= c_e, the
 *      seed's map without one.  epoch_e = the number of such update PDUs with I <= c_e (retransmissions count), stored
 *      saturating at 65535; 0 for a BEFORE event.
 *   6. PREDICTION, for counted events that are not BEYOND.  used_e[] = the channels of M_e, ascending, n_used_e their number.
 *      #1: u = (hop * ((c_e + 1) mod 37)) mod 37, expected = u if M_e holds it, else used_e[u mod n_used_e].  #2: rules 3-4 of
 *      btbbx_le_csa2_* with c_e mod 2^16, the map M_e and always the remapping.  chsel 0: #1.  chsel 1: both are scored over the
 *      events; the one with more events on its prediction is the connection's algorithm, a tie goes to #2.  BEFORE and BEYOND
 *      events have expected 0xff and on_hop 0.
 *   7. RECORDS.  n_before, n_on, n_off and n_beyond count EVENTS and add up to the connection's events; n_control counts
 *      CONTROL members, OPAQUE ones included; n_map_updates the valid, unignored map update PDUs.  A packet's kind is
 *      MAP_UPDATE / PARAM_UPDATE only for a VALID update that is not ignored; any other update stays CONTROL.
 * LIMITS: the interval after a parameter update is not followed by this stage (btbbx_le_span_device below finds the new window's anchor and goes on);
 * LL_PAUSE_ENC is not tracked; a first event seen only through a packet longer than unit_bits - jitter_bits - 230 bits behind
 * its missed anchor may get c_f one too large; a request whose connection never shows seeds nothing; an update behind
 * LL_START_ENC_REQ is OPAQUE here and read only by btbbx_le_keyed_epoch_device below, behind the decryption stage. */
#define BTBBX_LE_FOLLOW_SEEDED     1u   /* btbbx_le_follow.flags */
#define BTBBX_LE_FOLLOW_COUNTED    2u   /* some event is not BEFORE */
#define BTBBX_LE_FOLLOW_STOPPED    4u   /* stop is finite */
#define BTBBX_LE_FOLLOW_TERMINATED 8u
#define BTBBX_LE_FOLLOW_ENCRYPTED  16u
#define BTBBX_LE_FOLLOW_DECRYPTED  128u /* the keyed entries alone: a control PDU behind LL_START_ENC_REQ was read as plaintext */
#define BTBBX_LE_STATE_COUNTED 0u       /* btbbx_le_follow_pkt.state */
#define BTBBX_LE_STATE_BEFORE  1u
#define BTBBX_LE_STATE_BEYOND  2u
#define BTBBX_LE_PDU_DATA         0u    /* btbbx_le_follow_pkt.kind */
#define BTBBX_LE_PDU_CONTROL      1u
#define BTBBX_LE_PDU_MAP_UPDATE   2u
#define BTBBX_LE_PDU_PARAM_UPDATE 3u
#define BTBBX_LE_PDU_TERMINATE    4u
#define BTBBX_LE_PDU_ENC_START    5u
#define BTBBX_LE_PDU_OPAQUE       6u

typedef struct btbbx_le_follow {     /* 48 bytes, one per stored connection, parallel to conns / tracks / seeds */
	uint64_t map;                /* the map in force at the last predicted event; the seed's map without one */
	uint32_t counter_first;      /* low 32 bits of c_f; 0 unless COUNTED */
	uint32_t stop;               /* low 32 bits of stop */
	uint32_t n_before, n_on, n_off, n_beyond;   /* events */
	uint32_t n_control, n_map_updates;          /* members */
	uint8_t  algorithm;          /* 1 or 2 */
	uint8_t  flags;
	uint8_t  reserved[6];        /* written as 0 */
} btbbx_le_follow;                   /* a connection that is not SEEDED: 48 zero bytes */

typedef struct btbbx_le_follow_pkt { /* 12 bytes, one per candidate, parallel to the sorted candidate list */
	uint32_t counter;            /* low 32 bits of its event's connEventCounter; 0 for a BEFORE event */
	uint16_t epoch;
	uint8_t  kind, opcode;       /* opcode: 0xff unless CONTROL and parsed */
	uint8_t  expected, on_hop, state;
	uint8_t  reserved;           /* written as 0 */
} btbbx_le_follow_pkt;               /* a candidate that is no member of a stored connection: twelve 0xff bytes */

/* The input is what btbbx_le_discover_group_device, btbbx_le_track_device and btbbx_le_seed_device left, with the streams the
 * candidates came from.  A list from elsewhere must keep the grouping's promise -- the members of g are candidates of
 * [conns[g].first, first + n_packets) -- and the tracking's: ranks and events number a connection's members and events without
 * gaps; a member whose first + rank or first + event lies beyond N is treated as no member.  d_tracks and d_phys_channel are
 * taken for the chain's sake and not read: everything the stage needs of them stands in d_pkts.  d_follows[0 .. K) and
 * d_follow_pkts[0 .. N) are written, every byte of them, nothing behind them; nothing is read back and the call is asynchronous on
 * hip_stream.  d_scratch: btbbx_le_epoch_scratch_bytes(cand_cap, conn_cap) bytes (about 130 per candidate and 64 per
 * connection).  The count of launches depends on conn_cap only through one radix pass per byte of it.  BTBBX_E_ARG, before any
 * launch: a null pointer, n_streams == 0, unit_bits < 2, jitter_bits >= unit_bits / 2, n_words == 0 or above 2^42, pitch_words <
 * n_words with more than one stream, a scratch that is too small or not 16-byte aligned, words or records that are not 8-byte
 * aligned (d_pkts included; d_follow_pkts, whose records are 12 bytes, and the counters: 4; the channels: 2).  cand_cap == 0 or conn_cap == 0 succeeds and writes
 * nothing. */
size_t btbbx_le_epoch_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap);
int btbbx_le_epoch_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			   const uint16_t *d_phys_channel,
			   const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
			   const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
			   const btbbx_le_track *d_tracks, const btbbx_le_track_pkt *d_pkts, const btbbx_le_seed *d_seeds,
			   uint32_t unit_bits, uint32_t jitter_bits,
			   btbbx_le_follow *d_follows, btbbx_le_follow_pkt *d_follow_pkts,
			   void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* Host wrapper: btbbx_le_track_host's chain with three additions on the same stream.  In front of the seed stage: the advertising
 * scan over all streams of the same device copy of the capture (BTBBX_LE_ADV_AA, adv_errors 0..4 mismatches allowed), ordered by
 * (stream, offset) and decoded with BTBBX_LE_ADV_CRC_INIT; it is repeated with room for every match when its first buffer was too
 * small, as btbbx_le_scan_host does.  Behind the tracking: the seed stage, then the follow stage.  The tracking's arguments and
 * return value; tracks, seeds and follows: conn_cap records, parallel to conns; pkts and follow_pkts (either may be NULL):
 * cand_cap records, parallel to cands.  seeds[g].request indexes the advertising records in (stream, offset) order, which
 * btbbx_le_scan_host returns for the same capture and adv_errors.  BTBBX_E_ARG: the tracking wrapper's conditions, adv_errors
 * outside 0..4, seeds or follows NULL with conn_cap != 0.  Safe to call from several host threads at once. */
int64_t btbbx_le_epoch_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			     uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
			     btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
			     uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
			     int adv_errors, btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_seed *seeds,
			     btbbx_le_follow *follows, btbbx_le_follow_pkt *follow_pkts);

/* Names.  The entries of this stage are btbbx_le_epoch_* ("epoch": the stretch of events one channel map is in force for), not
 * btbbx_le_follow_*: the exported names that contain "follow" are, and stay, the two of the BR/EDR follow stage below.  The
 * records keep the stage's name.  For source that would rather say what the stage does: */
#define btbbx_le_follow_scratch_bytes btbbx_le_epoch_scratch_bytes
#define btbbx_le_follow_device        btbbx_le_epoch_device
#define btbbx_le_follow_host          btbbx_le_epoch_host

/* ---- LE following through connection parameter updates: spans ------------------------------
 * The follow stage above ends at the instant of an LL_CONNECTION_UPDATE_IND.  The SPAN stage goes on: a span is the stretch of
 * events that one set of connection parameters times; at the instant the new transmit window's anchor is found on the old grid,
 * the counting restarts there with the new interval, and counters, map updates and the hop check run through.  It stands beside
 * the follow stage, takes the same input and changes nothing of it.
 *
 * Members, time order, events, A_e and C_e; CONTROL parsing (12 octets, dewhitening, zeros beyond the stream's end), ENC_START and
 * OPAQUE, TERMINATE, the validity of a map update, and delta = (instant - c) mod 2^16, VALID iff delta < 32767, I = c + delta are
 * the follow stage's (its rules 1 to 3).  A candidate that is no member gets sixteen 0xff bytes; a connection that is not SEEDED
 * gets 56 zero bytes, zero span records, and its members counter 0, epoch 0, span 0, expected 0xff, on_hop 0, state 0, applied 0.
 * For a SEEDED connection, in integer arithmetic that is 64 bits wide:
 *   1. SPAN 0.  Int_0 = seed.interval, T_0 = seed.t0, B_0 = 0, allowance a_0 = jitter_bits, start_0 = event 0.
 *   2. COUNTING in span s.  P_s = Int_s * unit_bits.  Event e >= start_s is EARLY iff A_e + a_s < T_s: its state is BEFORE in
 *      span 0 and GAP in a later span, it is not counted (counter 0, epoch 0, expected 0xff), and a PDU in it is ignored.  f_s =
 *      the first event >= start_s that is not EARLY; c_(f_s) = B_s + (A_f + a_s - T_s) / P_s, by floor;
 *      c_(e+1) = c_e + (A_(e+1) - A_e + P_s / 2) / P_s.
 *   3. PARAM UPDATE.  Opcode 0 and length 12: WinSize' = octet 1, WinOffset' = LE16 at octets 2..3, Interval' = LE16 at 4..5,
 *      Latency' = LE16 at 6..7, Timeout' = LE16 at 8..9, instant = LE16 at 10..11.
 *   4. END of span s.  I_s = the smallest I of a VALID param update in any event e >= f_s, under span s's counting.  Without one,
 *      span s is the last and stop = 2^64 - 1.  Span s's events are those with c_e < I_s; L is the last of them.
 *   5. APPLY.  Among the VALID param updates with I == I_s whose own event has c_e < I_s, take the one of the largest rank.  It
 *      applies iff it exists, s < max_updates, 6 <= Interval' <= 3200, 1 <= WinSize' <= min(8, Interval' - 1) and WinOffset' <=
 *      Interval'.  Then G = A_L + (I_s - c_L) * P_s -- where event I_s would lie on the old grid; Core Vol 6 Part B 5.1.1 gives no
 *      transmitWindowDelay here --, T_(s+1) = G + WinOffset' * unit_bits, B_(s+1) = I_s, Int_(s+1) = Interval', a_(s+1) = 2 *
 *      jitter_bits (both ends of the measured distance deviate), start_(s+1) = L + 1; go on with rule 2.  The applied PDU has
 *      applied = 1.
 *   6. STOP.  Otherwise stop = I_s and the connection is STOPPED: CAPPED when s == max_updates, REFUSED otherwise (there is no
 *      such PDU, or its parameters are invalid).  Events with c_e >= I_s keep span s's counters and are BEYOND.  A map update
 *      whose own event is BEYOND is ignored.
 *   7. MAP, PREDICTION, ALGORITHM, TALLIES: the follow stage's rules 5 to 7 over the final counters, which rise across spans
 *      (B_(s+1) = I_s); tallies and the #1 / #2 choice run over all spans.  n_gap counts GAP events; n_before + n_gap + n_on +
 *      n_off + n_beyond is the connection's events, and the n_events of its spans sum to n_on + n_off.  A packet's span is the
 *      span whose counting gave its counter; for an EARLY event the span it lies in front of.  kind is PARAM_UPDATE for every
 *      VALID param update in a counted event, and n_param_updates counts those.
 * With max_updates == 0 every field a record shares with the follow stage's equals it (flags but for CAPPED and REFUSED); for any
 * max_updates, an event of span 0 that the follow stage leaves COUNTED carries the same values.
 * LIMITS: the first counter of a later span is exact while WinSize' * unit_bits + 4 * jitter_bits < P_(s+1) and the events
 * deviate by at most jitter_bits; it also inherits A_L's deviation, and any drift over I_s - c_L intervals when the events just
 * before the instant are missed.  An update whose PDU is seen only behind LL_START_ENC_REQ is never read (but by
 * btbbx_le_keyed_span_device below, behind the decryption stage); LL_PAUSE_ENC is not tracked; more than 16 updates are not
 * followed. */
#define BTBBX_LE_SPAN_CAPPED   32u      /* btbbx_le_span.flags, beside the BTBBX_LE_FOLLOW_* values */
#define BTBBX_LE_SPAN_REFUSED  64u
#define BTBBX_LE_STATE_GAP     3u       /* btbbx_le_span_pkt.state, beside COUNTED / BEFORE / BEYOND */

typedef struct btbbx_le_span {       /* 56 bytes, one per stored connection, parallel to conns / tracks / seeds */
	uint64_t map;                /* the map in force at the last predicted event; the seed's map without one */
	uint32_t counter_first;      /* low 32 bits of c_(f_0); 0 unless COUNTED */
	uint32_t stop;               /* low 32 bits of stop */
	uint32_t n_before, n_on, n_off, n_beyond, n_gap;   /* events */
	uint32_t n_control, n_map_updates, n_param_updates; /* members */
	uint32_t n_spans;
	uint16_t interval;           /* of the last span */
	uint8_t  algorithm;          /* 1 or 2 */
	uint8_t  flags;
} btbbx_le_span;                     /* a connection that is not SEEDED: 56 zero bytes */

typedef struct btbbx_le_span_pkt {   /* 16 bytes, one per candidate, parallel to the sorted candidate list */
	uint32_t counter;            /* low 32 bits of its event's connEventCounter; 0 for a BEFORE or GAP event */
	uint16_t epoch, span;
	uint8_t  kind, opcode;       /* opcode: 0xff unless CONTROL and parsed */
	uint8_t  expected, on_hop, state;
	uint8_t  applied;            /* 1: the parameter update that opened a span */
	uint8_t  reserved[2];        /* written as 0 */
} btbbx_le_span_pkt;                 /* a candidate that is no member of a stored connection: sixteen 0xff bytes */

typedef struct btbbx_le_span_rec {   /* 40 bytes; span s of connection g at index g * (max_updates + 1) + s */
	uint64_t origin;             /* T_s */
	uint32_t base;               /* low 32 bits of B_s */
	uint32_t first_event;        /* f_s within the connection, 0xffffffff without one */
	uint32_t n_events;           /* the span's events that are COUNTED and not BEYOND */
	uint32_t pdu;                /* list index of the applied PDU, 0xffffffff for span 0 */
	uint16_t interval, win_offset, latency, timeout;   /* span 0: the seed's */
	uint8_t  win_size;
	uint8_t  flags;              /* bit 0: the span exists */
	uint8_t  reserved[6];        /* written as 0 */
} btbbx_le_span_rec;                 /* a span that does not exist: 40 zero bytes */

/* The arguments of btbbx_le_epoch_device up to jitter_bits, and its promises about them.  max_updates: 0..16.  d_spans[0 .. K),
 * d_span_pkts[0 .. N) and d_span_recs[0 .. K * (max_updates + 1)) are written, every byte of them, nothing behind them; nothing is
 * read back and the call is asynchronous on hip_stream.  d_scratch: btbbx_le_span_scratch_bytes(cand_cap, conn_cap, max_updates)
 * bytes (the follow stage's and about 16 per candidate, 96 + 4 * (max_updates + 1) per connection).  The count of launches
 * depends on max_updates -- six per round, max_updates + 1 rounds -- and on conn_cap through one radix pass per byte of it, never
 * on the data.  BTBBX_E_ARG, before any launch: max_updates above 16, the follow stage's conditions, a record pointer that is not
 * 8-byte aligned.  cand_cap == 0 or conn_cap == 0 succeeds and writes nothing. */
size_t btbbx_le_span_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap, uint32_t max_updates);
int btbbx_le_span_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			 const uint16_t *d_phys_channel,
			 const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
			 const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
			 const btbbx_le_track *d_tracks, const btbbx_le_track_pkt *d_pkts, const btbbx_le_seed *d_seeds,
			 uint32_t unit_bits, uint32_t jitter_bits, uint32_t max_updates,
			 btbbx_le_span *d_spans, btbbx_le_span_pkt *d_span_pkts, btbbx_le_span_rec *d_span_recs,
			 void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* Host wrapper: btbbx_le_epoch_host's chain -- the advertising scan, discovery, tracking and seed -- with the span stage behind
 * the seed stage.  Its arguments up to seeds and its return value; spans: conn_cap records, span_recs: conn_cap * (max_updates +
 * 1), span_pkts (may be NULL): cand_cap.  BTBBX_E_ARG: max_updates above 16, the follow wrapper's conditions, spans or span_recs
 * NULL with conn_cap != 0. */
int64_t btbbx_le_span_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			   uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
			   btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
			   uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
			   int adv_errors, btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_seed *seeds,
			   uint32_t max_updates, btbbx_le_span *spans, btbbx_le_span_pkt *span_pkts, btbbx_le_span_rec *span_recs);

/* ---- LE data extraction: roles, retransmission filter, L2CAP reassembly --------------------
 * Every stage above ends in a verdict about a connection; this one hands out what the connection carried.  Behind the tracking, on
 * the device, for every packet the role of its sender, its SN / NESN / MD bits and whether it is new or a retransmission; for every
 * direction of every connection the L2CAP messages reassembled from their fragments, their dewhitened octets packed into one
 * buffer and a record per message.  It needs no CONNECT_IND, so it serves promiscuously discovered and encrypted connections as
 * well (encrypted octets come out as ciphertext), and it changes nothing of its input.
 *
 * The input is what btbbx_le_discover_group_device and btbbx_le_track_device left, plus the streams.  N = min(*d_cand_count,
 * cand_cap), K = min(*d_conn_count, conn_cap).  Membership is the follow stage's, promises and guards included: candidate i < N is a
 * member of g < K iff cands[i].conn == g and pkts[i].rank != 0xffffffff (and first + rank, first + event lie within N).  Time order
 * is rank, events are pkts[i].event, an event's counter is the tracking's stored counter.  A list from elsewhere keeps, besides the
 * follow stage's promises, the grouping's order: conns[g].first ascends with g.  All arithmetic is integer arithmetic; offsets and
 * octet counts are 64 bits wide.
 *   1. HEADER.  h0 = cands[i].header0, L = cands[i].length; llid = h0 & 3, nesn = (h0 >> 2) & 1, sn = (h0 >> 3) & 1, md = (h0 >> 4) & 1.
 *   2. HEAD events.  Event e of a connection is HEAD iff e == 0 or its stored counter differs from that of event e - 1.  (By the
 *      tracking's rule 3 a packet lost inside an event splits the event, by its rule 5 the tail then carries the same counter: such a
 *      tail is not HEAD.  A connection that is not TIMED has every counter 0: only its event 0 is HEAD.)
 *   3. ROLE.  A member of a HEAD event has role = (its rank - the rank of the event's first member) & 1: 0 CENTRAL, 1 PERIPHERAL
 *      (inside an event the tracking admits no gap beyond ifs_bits, so packets alternate).  A member of any other event is UNKNOWN
 *      (role 2) and takes no part in rules 4 to 6.
 *   4. NEW / RETRANSMIT.  Per (connection, role in {0, 1}) in time order a member is NEW iff it is the first of its role or its sn
 *      differs from the sn of the previous member of the SAME role; otherwise it is RETRANSMIT.
 *   5. MESSAGES, over NEW members only, per (connection, role).  START iff llid == 2 and L >= 1.  CONTINUATION iff llid == 1 and
 *      L >= 1: it belongs to the message of the latest START of its (connection, role) before it in time order; without one it is
 *      ORPHAN.  EMPTY iff llid == 1 and L == 0.  CONTROL iff llid == 3.  Everything else (llid 0, or llid 2 with L == 0) is IGNORED.
 *      EMPTY, CONTROL and IGNORED members lie between fragments without breaking a message.  A message has n_fragments = 1 + its
 *      continuations and bytes = the sum of their L; a fragment's pos = the sum of L of the message's earlier fragments.  If the START
 *      has L >= 4, l2cap_len = LE16 of its dewhitened payload octets 0..1 and cid = LE16 of octets 2..3; otherwise the message is RUNT
 *      and both are 0xffff.  COMPLETE iff not RUNT and bytes == 4 + l2cap_len; OVERRUN iff not RUNT and bytes > 4 + l2cap_len.
 *   6. ORDER and BYTES.  Messages are numbered M = 0, 1, ... by (connection, rank of the START) ascending: a connection's messages
 *      lie next to each other, both roles interleaved in time order.  byte_offset(M) = the sum of bytes of all earlier messages.
 *      Message M is STORED iff M < msg_cap and byte_offset + bytes <= byte_cap; offsets only grow, so the stored messages are a
 *      prefix.  For a stored message d_bytes[byte_offset + pos + k] = payload octet k of each fragment: stream bits offset + 56 + 8k
 *      .. + 7, least significant first, dewhitened with the channel's sequence continued behind the two header octets; bits beyond
 *      the stream's end read as 0, as in the follow stage's rule 3.  d_msgs[M] is written for M < msg_cap, stored or not.
 *      *d_msg_count = all messages and *d_byte_count (64 bits) = all their octets: the stage WRITES both, it does not add to them.
 *      Nothing behind the stored prefix of d_bytes and nothing behind min(count, msg_cap) records of d_msgs is touched.
 *   7. RECORDS.  Every byte of d_data[0 .. K) and d_data_pkts[0 .. N) is written, nothing behind them.  first_msg of a connection
 *      without messages is the number of messages of the connections before it; the n_msgs of all connections add up to the count.
 * LIMITS, which follow from the rules: when the central's packet of an event was not received, the peripheral's first packet is
 * taken for it; two lost packets of one role in a row make a new packet look like a retransmission; the first event seen may be the
 * tail of one; connections that are not TIMED yield data only from their first event; an L2CAP header split over fragments (START
 * with L < 4) is not parsed. */
#define BTBBX_LE_DATA_START        0u   /* btbbx_le_data_pkt.kind */
#define BTBBX_LE_DATA_CONTINUATION 1u
#define BTBBX_LE_DATA_ORPHAN       2u
#define BTBBX_LE_DATA_EMPTY        3u
#define BTBBX_LE_DATA_CONTROL      4u
#define BTBBX_LE_DATA_IGNORED      5u
#define BTBBX_LE_DATA_RETRANSMIT   6u
#define BTBBX_LE_DATA_UNKNOWN      7u
#define BTBBX_LE_ROLE_CENTRAL      0u   /* btbbx_le_data_pkt.role, btbbx_le_msg.role */
#define BTBBX_LE_ROLE_PERIPHERAL   1u
#define BTBBX_LE_ROLE_UNKNOWN      2u
#define BTBBX_LE_MSG_COMPLETE      1u   /* btbbx_le_msg.flags */
#define BTBBX_LE_MSG_OVERRUN       2u
#define BTBBX_LE_MSG_RUNT          4u
#define BTBBX_LE_MSG_STORED        8u

typedef struct btbbx_le_data_pkt {   /* 12 bytes, parallel to the sorted candidate list; no member: twelve 0xff bytes */
	uint32_t msg;                /* its message, 0xffffffff unless START or CONTINUATION */
	uint32_t pos;                /* its first octet within the message; 0 without one */
	uint8_t  role;               /* 0 central, 1 peripheral, 2 unknown */
	uint8_t  kind;               /* START, CONTINUATION, ORPHAN, EMPTY, CONTROL, IGNORED, RETRANSMIT, UNKNOWN */
	uint8_t  bits;               /* sn | nesn << 1 | md << 2 */
	uint8_t  reserved;           /* 0 */
} btbbx_le_data_pkt;
typedef struct btbbx_le_data {       /* 48 bytes, parallel to conns; a connection without a member: zeros */
	uint64_t bytes;              /* of its messages */
	uint32_t first_msg, n_msgs, n_complete;
	uint32_t n_central, n_peripheral, n_unknown;     /* members by role */
	uint32_t n_retransmit, n_orphan, n_control, n_empty;
} btbbx_le_data;
typedef struct btbbx_le_msg {        /* 32 bytes */
	uint64_t byte_offset;
	uint32_t conn, start;        /* start: list index of the START */
	uint32_t n_fragments, bytes;
	uint16_t l2cap_len, cid;
	uint8_t  role, flags;        /* COMPLETE 1, OVERRUN 2, RUNT 4, STORED 8 */
	uint8_t  reserved[2];        /* written as 0 */
} btbbx_le_msg;

/* d_tracks and d_phys_channel are taken for the chain's sake and not read: everything the stage needs of them stands in d_pkts.
 * Nothing is read back and the call is asynchronous on hip_stream.  d_scratch: btbbx_le_data_scratch_bytes(cand_cap, conn_cap)
 * bytes (about 52 per candidate, 32 per 2048 candidates and 96 per connection), 16-byte aligned.  The count of launches, 18, depends on nothing.
 * BTBBX_E_ARG, before any launch: a null pointer (d_msgs may be null with msg_cap 0, d_bytes with byte_cap 0), n_streams == 0,
 * n_words == 0 or above 2^42, pitch_words < n_words with more than one stream, a scratch that is too small or not 16-byte aligned,
 * words, records, d_bytes or d_byte_count that are not 8-byte aligned (d_data_pkts, whose records are 12 bytes, and the counters:
 * 4; the channels: 2).  cand_cap == 0 or conn_cap == 0 succeeds and writes only the two counts, as 0. */
size_t btbbx_le_data_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap);
int btbbx_le_data_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			 const uint16_t *d_phys_channel,
			 const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
			 const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
			 const btbbx_le_track *d_tracks, const btbbx_le_track_pkt *d_pkts,
			 btbbx_le_data *d_data, btbbx_le_data_pkt *d_data_pkts, btbbx_le_msg *d_msgs, uint32_t msg_cap,
			 uint32_t *d_msg_count, uint8_t *d_bytes, uint64_t byte_cap, uint64_t *d_byte_count,
			 void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* Host wrapper: btbbx_le_track_host's chain with this stage behind the tracking on the same stream.  The tracking wrapper's
 * arguments and return value; data: conn_cap records, parallel to conns; data_pkts (may be NULL): cand_cap records, parallel to
 * cands; msgs: msg_cap records, bytes: byte_cap octets (either may be NULL with its cap 0); *n_msgs_out and *n_bytes_out (either may
 * be NULL) = all messages and all their octets.  Of msgs the first min(*n_msgs_out, msg_cap) records are written, of bytes the
 * stored prefix.  BTBBX_E_ARG: the tracking wrapper's conditions, data NULL with conn_cap != 0, msgs or bytes NULL with a cap. */
int64_t btbbx_le_data_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			   uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
			   btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
			   uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
			   btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_data *data, btbbx_le_data_pkt *data_pkts,
			   btbbx_le_msg *msgs, uint64_t msg_cap, uint64_t *n_msgs_out, uint8_t *bytes, uint64_t byte_cap,
			   uint64_t *n_bytes_out);

/* ---- LE decryption: session keys, packet counters, AES-CCM, plain L2CAP ----------------------
 * Behind the data stage, on the device: for every connection whose encryption start procedure is in the capture the session key
 * under one of the caller's long-term keys, for every encrypted packet its packet counter, and the data stage's messages once more,
 * over plaintext.  It changes nothing of its input.
 *
 * The input is the data stage's (streams, d_cands, d_conns, d_pkts and the counters), the data stage's d_data_pkts, read for role,
 * kind and bits, and the keys: key k is the 16 octets at d_keys + 16k in AES key byte order, that is the LTK most significant octet
 * first, as the Core Specification prints it.  Membership, time order, slot order first + rank, the payload octet rule (data stage
 * rule 6: dewhitening continued behind the header, zeros beyond the stream's end) and all guards for a list from elsewhere are the
 * data stage's.  "Octet j" below is payload octet j.  All arithmetic is integer arithmetic; counters are 64 bits wide.
 *   1. COUNTING members.  A member COUNTS iff its data-stage role is CENTRAL or PERIPHERAL and its data-stage kind is neither
 *      RETRANSMIT nor UNKNOWN.  Every other member never gets a counter.
 *   2. PROCEDURE PDUs, among COUNTING members with llid == 3.  ENC_REQ: role CENTRAL, L == 23, octet 0 == 0x03; SKDm = octets
 *      11..18, IVm = octets 19..22.  ENC_RSP: role PERIPHERAL, L == 13, octet 0 == 0x04; SKDs = octets 1..8, IVs = octets 9..12.
 *      START: role PERIPHERAL, L == 1, octet 0 == 0x05.  The connection's REQ is the ENC_REQ of the smallest rank, its RSP the
 *      ENC_RSP of the smallest rank above REQ's, its START the START of the smallest rank above RSP's.  It is ARMED iff all three
 *      exist.
 *   3. SESSION KEY.  skd[0..7] = SKDm as received, skd[8..15] = SKDs as received; the AES input block is block[j] = skd[15 - j];
 *      SK_k = AES-128(key_k, block), and the output block, octet 0 first, is the CCM key.  iv[0..3] = IVm as received, iv[4..7] = IVs.
 *   4. ENCRYPTED members.  In an ARMED connection a COUNTING member of rank above START's with llid != 0 is ENCRYPTED iff L >= 5
 *      and SHORT iff 1 <= L <= 4; a member of rank above START's that does not COUNT and has L >= 1 is SKIPPED.  Everything else is
 *      CLEAR: empty PDUs, everything up to START, every member of a connection that is not ARMED.  The ordinal n of an ENCRYPTED
 *      member is the number of ENCRYPTED members of the same (connection, role) of smaller rank.  SHORT, SKIPPED and CLEAR members
 *      take no ordinal.
 *   5. TRIAL of an ENCRYPTED member under key K and skew d.  c = n + d; dir = 1 for CENTRAL, 0 for PERIPHERAL.  nonce[0..3] = LE32 of
 *      c's low 32 bits, nonce[4] = ((c >> 32) & 0x7f) | dir << 7, nonce[5..12] = iv.  m = L - 4.  B0 = 0x49 | nonce | BE16(m);
 *      B1 = 00 01 (header0 & 0xE3) and 13 zero octets; S_i = AES(K, 0x01 | nonce | BE16(i)).  Plaintext octet j = octet j ^
 *      S_(1 + j/16)[j % 16] for j < m.  X = AES(K, B0); X = AES(K, X ^ B1); X = AES(K, X ^ P) for every 16-octet plaintext block P,
 *      the last one padded with zeros.  The trial VERIFIES iff X[0..3] ^ S_0[0..3] equals octets m .. m + 3.
 *   6. KEY.  The probes are the first min(4, .) ENCRYPTED members of the connection in time order, either role.  score_k = the number
 *      of probes that verify under SK_k at some d < window.  The connection's key is the smallest k of the largest score, if that
 *      score is >= 1: the connection is KEYED.  Otherwise every ENCRYPTED member of it is FAILED with skew 0xff.
 *   7. SKEW, in a KEYED connection.  An ENCRYPTED member is VERIFIED at the smallest d < window that verifies under the connection's
 *      key, and its counter is n + d; without one it is FAILED, its skew 0xff and its counter n.  Each member is searched on its
 *      own: no member's result depends on another's.
 *   8. MESSAGES: the data stage's rules 5 to 7 once more, over EFFECTIVE members.  A VERIFIED member has L' = L - 4, its own llid
 *      (START iff llid == 2, CONTINUATION or ORPHAN iff llid == 1, CONTROL iff llid == 3) and its plaintext as octets.  A CLEAR member
 *      is as in the data stage.  FAILED, SKIPPED and SHORT members have kind IGNORED: they are no fragment and break nothing.  The
 *      outputs have the data stage's shapes: d_msgs, d_plain_pkts (role and bits as in d_data_pkts, kind, msg and pos under the
 *      effective members), d_bytes and both counts, which the stage WRITES; msg_cap and byte_cap cut a prefix as there.  If no
 *      connection is ARMED, every message record, every octet, every d_plain_pkts record and both counts equal
 *      btbbx_le_data_device's on the same input, byte for byte.
 *   9. RECORDS.  Every byte of d_crypt[0 .. K) and d_crypt_pkts[0 .. N) is written, nothing behind them.  btbbx_le_crypt of a
 *      connection without a member: zeros; otherwise session_key = the connection's key's SK (zeros unless KEYED), iv (zeros
 *      unless ARMED), req / rsp / start = list indices, 0xffffffff if none, n_encrypted = n_verified + n_failed, n_skipped,
 *      key (0xff: none), max_skew = the largest skew of a VERIFIED member.  btbbx_le_crypt_pkt of a candidate that is no member:
 *      sixteen 0xff; of a VERIFIED or FAILED member counter (low 32 bits), counter_hi (bits 32..38), ordinal and skew; of every
 *      other member these are 0.  opcode = plaintext octet 0 of a VERIFIED member with llid == 3, else 0xff.
 * LIMITS: a connection whose LL_ENC_REQ / LL_ENC_RSP are not in the capture stays unarmed; LL_PAUSE_ENC and a second encryption
 * start are not tracked; a lost packet shows as skew and is found only within window; the roles' limits are the data stage's; an
 * update PDU decrypted here is not fed back to the follow or span stage (btbbx_le_keyed_epoch_device and
 * btbbx_le_keyed_span_device below read it from this stage's records). */
#define BTBBX_LE_CRYPT_CLEAR    0u   /* btbbx_le_crypt_pkt.state */
#define BTBBX_LE_CRYPT_VERIFIED 1u
#define BTBBX_LE_CRYPT_FAILED   2u
#define BTBBX_LE_CRYPT_SKIPPED  3u
#define BTBBX_LE_CRYPT_SHORT    4u
#define BTBBX_LE_CRYPT_REQ      1u   /* btbbx_le_crypt.flags */
#define BTBBX_LE_CRYPT_RSP      2u
#define BTBBX_LE_CRYPT_START    4u
#define BTBBX_LE_CRYPT_ARMED    8u
#define BTBBX_LE_CRYPT_KEYED    16u

typedef struct btbbx_le_crypt {      /* 56 bytes, parallel to conns; a connection without a member: zeros */
	uint8_t  session_key[16];
	uint8_t  iv[8];
	uint32_t req, rsp, start;    /* list indices, 0xffffffff if none */
	uint32_t n_encrypted, n_verified, n_failed, n_skipped;
	uint8_t  key;                /* index of the connection's key, 0xff: none */
	uint8_t  max_skew;
	uint8_t  flags;              /* REQ 1, RSP 2, START 4, ARMED 8, KEYED 16 */
	uint8_t  reserved;           /* 0 */
} btbbx_le_crypt;
typedef struct btbbx_le_crypt_pkt {  /* 16 bytes, parallel to the sorted candidate list; no member: sixteen 0xff bytes */
	uint32_t counter;            /* low 32 bits of the packet counter */
	uint32_t ordinal;
	uint8_t  state;              /* CLEAR, VERIFIED, FAILED, SKIPPED, SHORT */
	uint8_t  skew;               /* 0xff: FAILED */
	uint8_t  opcode;             /* of a VERIFIED control PDU, else 0xff */
	uint8_t  counter_hi;         /* bits 32..38 of the packet counter */
	uint8_t  reserved[4];        /* written as 0 */
} btbbx_le_crypt_pkt;

/* d_tracks and d_phys_channel are taken for the chain's sake and not read.  n_keys: 1..64, window: 1..32.  Nothing is read back and
 * the call is asynchronous on hip_stream.  d_scratch: btbbx_le_crypt_scratch_bytes(cand_cap, conn_cap, n_keys) bytes (about 76 per
 * candidate and 180 per connection and key), 16-byte aligned.  The count of launches, 24, depends on nothing.
 * BTBBX_E_ARG, before any launch: btbbx_le_data_device's conditions, n_keys or window out of range, a null pointer (d_msgs may be null
 * with msg_cap 0, d_bytes with byte_cap 0), d_crypt_pkts not 16-byte aligned, d_crypt not 8-byte, d_data_pkts or d_plain_pkts not
 * 4-byte aligned.  cand_cap == 0 or conn_cap == 0 succeeds and writes only the two counts, as 0. */
size_t btbbx_le_crypt_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap, uint32_t n_keys);
int btbbx_le_crypt_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			  const uint16_t *d_phys_channel,
			  const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
			  const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
			  const btbbx_le_track *d_tracks, const btbbx_le_track_pkt *d_pkts, const btbbx_le_data_pkt *d_data_pkts,
			  const uint8_t *d_keys, uint32_t n_keys, uint32_t window,
			  btbbx_le_crypt *d_crypt, btbbx_le_crypt_pkt *d_crypt_pkts, btbbx_le_data_pkt *d_plain_pkts,
			  btbbx_le_msg *d_msgs, uint32_t msg_cap, uint32_t *d_msg_count, uint8_t *d_bytes, uint64_t byte_cap,
			  uint64_t *d_byte_count, void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* Host wrapper: btbbx_le_data_host's chain with this stage behind the data stage on the same stream.  The data wrapper's arguments
 * and return value, with keys (16 * n_keys octets), n_keys and window behind data_pkts; data and data_pkts are the data stage's
 * records; crypt: conn_cap records; crypt_pkts and plain_pkts (either may be NULL): cand_cap records; msgs, bytes and the two
 * counts are rule 8's.  max_len is not raised: an encrypted PDU is 4 octets longer than its plaintext, so a 27-octet connection
 * needs max_len >= 31 and data length extension 255.  BTBBX_E_ARG: the data wrapper's conditions, keys NULL, crypt NULL with
 * conn_cap != 0, n_keys outside 1..64, window outside 1..32. */
int64_t btbbx_le_crypt_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			    uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
			    btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
			    uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
			    btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_data *data, btbbx_le_data_pkt *data_pkts,
			    const uint8_t *keys, uint32_t n_keys, uint32_t window, btbbx_le_crypt *crypt, btbbx_le_crypt_pkt *crypt_pkts,
			    btbbx_le_data_pkt *plain_pkts, btbbx_le_msg *msgs, uint64_t msg_cap, uint64_t *n_msgs_out, uint8_t *bytes,
			    uint64_t byte_cap, uint64_t *n_bytes_out);

/* ---- Keyed LE following: map and parameter updates sent encrypted ---------------------------
 * The follow stage and the span stage stop reading control PDUs at the first LL_START_ENC_REQ: every CONTROL member behind it is
 * OPAQUE, and a paired connection sends nearly all its LL_CHANNEL_MAP_IND and LL_CONNECTION_UPDATE_IND PDUs there.  The KEYED form
 * of either stage has the same rules and the same output records, with the control PDUs the decryption stage VERIFIED read as
 * plaintext.  It changes nothing of its input.
 *
 * The input is btbbx_le_epoch_device's / btbbx_le_span_device's plus three arrays: d_data_pkts, the data stage's, read for role;
 * d_crypt, the decryption stage's, read for session_key, iv and flags; d_crypt_pkts, read for state, counter and counter_hi.
 * d_data_pkts and d_crypt_pkts are parallel to the sorted candidate list, d_crypt to conns.  Members, ranks, events, slots and
 * ENC_START -- the first CONTROL member in time order that reads in the clear as opcode 5 and length 1 -- are the follow stage's.
 *   1. READABLE.  Member i of connection g with header length L is READABLE iff d_crypt[g].flags has KEYED,
 *      d_crypt_pkts[i].state == BTBBX_LE_CRYPT_VERIFIED, (header0 & 3) == 3 and L >= 5, d_data_pkts[i].role is CENTRAL or
 *      PERIPHERAL, and g has an ENC_START and i's rank is above its rank.  (The decryption stage gives VERIFIED to no other kind of
 *      control member; the other conditions guard a list from elsewhere.)  A member that fails one of them is treated as in the
 *      unkeyed stage.
 *   2. PLAINTEXT.  The nonce is the decryption stage's rule 5's with c = counter | (uint64_t)counter_hi << 32, dir = 1 for
 *      CENTRAL and 0 for PERIPHERAL, iv = d_crypt[g].iv.  S_1 = AES-128(session_key, 0x01 | nonce | 00 01).  L' = L - 4.  Plain
 *      octet j = (payload octet j as follow rule 3 reads it: dewhitening continued behind the header, zeros beyond the stream's
 *      end) ^ S_1[j] for j < min(L', 12).  The MIC's octets are never read as payload, and the MIC is not checked again.
 *   3. PARSING.  A READABLE member is CONTROL with length L' and those octets; follow rule 3 and span rule 3 parse it with L' in
 *      the length's place (map update: opcode 1 and L' 8; parameter update: opcode 0 and L' 12; TERMINATE: opcode 2 and L' 2).  It
 *      is never ENC_START, whatever its opcode.  A CONTROL member above ENC_START that is not READABLE stays OPAQUE with opcode
 *      0xff: FAILED, SKIPPED and SHORT members, the CLEAR members of a connection that is not ARMED, retransmissions.
 *   4. REST.  Everything else is follow rules 1-7 and span rules 1-7: n_control, stop, instants, epochs, spans, gaps, tallies,
 *      the algorithm.  BTBBX_LE_FOLLOW_DECRYPTED (128, the free bit of btbbx_le_follow.flags and btbbx_le_span.flags beside CAPPED
 *      and REFUSED) is set iff the connection is SEEDED and has a READABLE member.  The records are btbbx_le_follow, _follow_pkt,
 *      _span, _span_pkt and _span_rec; every byte of them is written, nothing behind them.
 *   5. EQUALITIES.  (a) If no member is READABLE, every output byte equals the unkeyed entry's on the same input.  (b) The keyed
 *      span stage with max_updates == 0 relates to the keyed follow stage as the unkeyed ones relate.
 * LIMITS: LL_PAUSE_ENC and a second encryption start are not tracked; a PDU the decryption stage did not VERIFY is not read -- a
 * lost packet beyond window, a role UNKNOWN in a split event's tail, a key that is not in the table.
 *
 * Each _device entry takes the unkeyed entry's arguments with d_data_pkts, d_crypt, d_crypt_pkts behind d_seeds, and makes its
 * promises.  d_scratch: the unkeyed stage's bytes, 16 per candidate and 2 bits per candidate.  The count of launches equals the
 * unkeyed entry's: the kernels that read a payload or say a PDU's kind are replaced by keyed ones and none is added, so the count
 * depends on conn_cap and max_updates as there and never on the data.  BTBBX_E_ARG, before any launch: the unkeyed entry's
 * conditions, a new pointer that is null or misaligned (d_crypt 8 bytes, d_crypt_pkts 16, d_data_pkts 4).  cand_cap == 0 or
 * conn_cap == 0 succeeds and writes nothing.  Asynchronous on hip_stream; nothing is read back. */
size_t btbbx_le_keyed_epoch_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap);
int btbbx_le_keyed_epoch_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				const uint16_t *d_phys_channel,
				const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
				const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
				const btbbx_le_track *d_tracks, const btbbx_le_track_pkt *d_pkts, const btbbx_le_seed *d_seeds,
				const btbbx_le_data_pkt *d_data_pkts, const btbbx_le_crypt *d_crypt, const btbbx_le_crypt_pkt *d_crypt_pkts,
				uint32_t unit_bits, uint32_t jitter_bits,
				btbbx_le_follow *d_follows, btbbx_le_follow_pkt *d_follow_pkts,
				void *d_scratch, size_t scratch_bytes, void *hip_stream);
size_t btbbx_le_keyed_span_scratch_bytes(uint32_t cand_cap, uint32_t conn_cap, uint32_t max_updates);
int btbbx_le_keyed_span_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			       const uint16_t *d_phys_channel,
			       const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
			       const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
			       const btbbx_le_track *d_tracks, const btbbx_le_track_pkt *d_pkts, const btbbx_le_seed *d_seeds,
			       const btbbx_le_data_pkt *d_data_pkts, const btbbx_le_crypt *d_crypt, const btbbx_le_crypt_pkt *d_crypt_pkts,
			       uint32_t unit_bits, uint32_t jitter_bits, uint32_t max_updates,
			       btbbx_le_span *d_spans, btbbx_le_span_pkt *d_span_pkts, btbbx_le_span_rec *d_span_recs,
			       void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* Host wrapper: btbbx_le_epoch_host's chain -- the advertising scan, discovery, tracking and seed -- then the data stage, the
 * decryption stage under keys / n_keys / window (as btbbx_le_crypt_host takes them) and the keyed span stage, all on one stream.
 * btbbx_le_span_host's arguments and return value, with keys, n_keys, window, crypt and crypt_pkts behind seeds; crypt: conn_cap
 * records; crypt_pkts and span_pkts (either may be NULL): cand_cap records.  The data stage's and the decryption stage's messages
 * and octets are not kept.  BTBBX_E_ARG: the span wrapper's conditions and the decryption wrapper's: keys NULL, crypt NULL with
 * conn_cap != 0, n_keys outside 1..64, window outside 1..32. */
int64_t btbbx_le_keyed_span_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				 uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
				 btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
				 uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
				 int adv_errors, btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_seed *seeds,
				 const uint8_t *keys, uint32_t n_keys, uint32_t window, btbbx_le_crypt *crypt,
				 btbbx_le_crypt_pkt *crypt_pkts, uint32_t max_updates, btbbx_le_span *spans,
				 btbbx_le_span_pkt *span_pkts, btbbx_le_span_rec *span_recs);

/* ---- LE legacy pairing key recovery: SMP exchange, TK search, STK --------------------------
 * Behind the data stage or the decryption stage, on the device: for every connection the Security Manager exchange among its
 * L2CAP messages (CID 0x0006), the temporary key (TK) of an LE legacy pairing -- 0 for Just Works or a six-digit passkey -- by
 * trying every value below tk_limit against the Confirm values, the short-term key (STK) under it as a key table that
 * btbbx_le_crypt_device takes as it is, and the long-term keys the peers distribute.  It changes nothing of its input.
 *
 * The input is the data stage's message outputs, or the decryption stage's, which have the same shapes (d_msgs, d_msg_count,
 * msg_cap, d_bytes, byte_cap), the connection count (d_conn_count, conn_cap; K = the smaller of the two) and the seed stage's
 * d_seeds, parallel to the connections.  A caller may write the seeds itself: the stage reads flags, init_a, adv_a, tx_add and
 * rx_add, nothing else.  The first W = min(*d_msg_count, msg_cap) message records are looked at.  A record is skipped if its
 * conn >= K, its byte_offset + bytes > byte_cap, or its bytes < 4 + l2cap_len: this guards a list from elsewhere (the data stage
 * writes none of these).  All arithmetic is integer arithmetic.
 *   1. SMP MESSAGE.  Record M is an SMP message iff its flags have COMPLETE and STORED, cid == 0x0006 and l2cap_len >= 1.  Its
 *      octets are v[k] = d_bytes[byte_offset + 4 + k], its code is v[0].
 *   2. PROCEDURE, per connection, by ascending M (the data stage's rule 6 makes that the time order within a connection):
 *        PREQ   role CENTRAL     code 0x01  l2cap_len 7    the first such SMP message
 *        PRSP   role PERIPHERAL  code 0x02  l2cap_len 7    the first above PREQ
 *        MCONF  role CENTRAL     code 0x03  l2cap_len 17   the first above PRSP
 *        SCONF  role PERIPHERAL  code 0x03  l2cap_len 17   the first above MCONF
 *        MRAND  role CENTRAL     code 0x04  l2cap_len 17   the first above SCONF if SCONF exists, else above MCONF
 *        SRAND  role PERIPHERAL  code 0x04  l2cap_len 17   the first above MRAND
 *      A missing message leaves everything that is defined "above" it missing too, except where the table says otherwise.
 *   3. METHOD.  Without PREQ and PRSP: NONE.  preq[j] and pres[j] are the octets v[j] of PREQ and PRSP.  ks = min(preq[4],
 *      pres[4]); INVALID iff ks < 7 or ks > 16; otherwise SECURE iff both preq[3] and pres[3] have bit 3 set (LE Secure
 *      Connections: there is no TK and nothing is searched); otherwise OOB iff preq[2] == 1 and pres[2] == 1 (the TK is 128 bits
 *      and is not searched); otherwise LEGACY.
 *   4. CHECKS.  The central's check exists iff MCONF and MRAND do, the peripheral's iff SCONF and SRAND do.  A connection is
 *      ARMED iff its method is LEGACY, its seed is SEEDED, at least one check exists and tk_limit >= 1.  With 16-octet arrays
 *      written least significant octet first: a = iat, rat, preq[0..6], pres[0..6] with iat = seed.tx_add & 1 and rat =
 *      seed.rx_add & 1; b = adv_a[0..5], init_a[0..5], 0, 0, 0, 0; r = the octets 1..16 of the check's Random message; conf = the
 *      octets 1..16 of its Confirm message.  The AES input of an array x is block[j] = x[15 - j], and an output block o reads
 *      back as x[i] = o[15 - i].  Key octets, most significant first: 0..11 are zero and 12..15 are BE32(tk).  A check HOLDS
 *      under tk iff AES(key(tk), AES(key(tk), r ^ a) ^ b) == conf.
 *   5. SEARCH.  The connection's TK is the smallest tk < tk_limit under which every check that exists holds; if there is one the
 *      connection is CRACKED, otherwise tk = 0xffffffff.  tk_limit is 0..1000000: 1 tries Just Works only, 0 searches nothing.
 *   6. STK.  Iff CRACKED and both MRAND and SRAND exist: c = mrand[0..7], srand[0..7], least significant first, the octets 1..8
 *      of each Random message.  The STK is AES(key(tk), block(c)), output octet 0 first, with its octets 0 .. 15 - ks set to
 *      zero.  Output octet 0 first is the byte order btbbx_le_crypt_device takes for d_keys.
 *   7. KEY TABLE.  The connections that have an STK take, by ascending connection index, the slots 0, 1, ... of d_keys; key_cap
 *      is 0..64.  *d_key_count = the number of all connections with an STK: the stage WRITES it, it does not add to it.  The slots
 *      from min(count, key_cap) to key_cap are written as zeros, so the table can go to the decryption stage as it is, with
 *      n_keys = key_cap.  A connection beyond key_cap keeps its STK in its record and gets key = 0xff.
 *   8. DISTRIBUTED KEYS.  Per (connection, role) the first SMP message with code 0x06 and l2cap_len 17: ltk[role][j] = v[16 - j],
 *      which is AES key byte order, and the keys flag LTK_CENTRAL or LTK_PERIPHERAL is set.  This is found wherever the messages
 *      are readable, in practice when the stage runs over the decryption stage's output.  With tk_limit == 0 the stage does
 *      rules 1 to 3, 8 and 9 only.
 *   9. RECORDS.  Every byte of d_pairs[0 .. K) is written, nothing behind it.  A connection without any of the above gets zeros,
 *      the six message indices and tk as 0xffffffff and key as 0xff.
 * LIMITS: only the first pairing of a connection is recognised, a failed pairing followed by a second one is not followed; a
 * connection that is not SEEDED is never ARMED, its procedure is still reported; SECURE and OOB pairings are named, not broken;
 * EDIV / Rand, IRK and CSRK are not extracted; SMP messages that the data stage left unstored (msg_cap, byte_cap) or incomplete
 * (a lost fragment) do not count. */
#define BTBBX_LE_PAIR_NONE     0u    /* btbbx_le_pair.method */
#define BTBBX_LE_PAIR_LEGACY   1u
#define BTBBX_LE_PAIR_SECURE   2u
#define BTBBX_LE_PAIR_OOB      3u
#define BTBBX_LE_PAIR_INVALID  4u
#define BTBBX_LE_PAIR_PREQ     1u    /* btbbx_le_pair.flags */
#define BTBBX_LE_PAIR_PRSP     2u
#define BTBBX_LE_PAIR_MCONF    4u
#define BTBBX_LE_PAIR_SCONF    8u
#define BTBBX_LE_PAIR_MRAND    16u
#define BTBBX_LE_PAIR_SRAND    32u
#define BTBBX_LE_PAIR_ARMED    64u
#define BTBBX_LE_PAIR_CRACKED  128u
#define BTBBX_LE_PAIR_KEY_STK            1u   /* btbbx_le_pair.keys */
#define BTBBX_LE_PAIR_KEY_LTK_CENTRAL    2u
#define BTBBX_LE_PAIR_KEY_LTK_PERIPHERAL 4u

typedef struct btbbx_le_pair {       /* 88 bytes, parallel to conns */
	uint8_t  stk[16];            /* the STK, rule 6 */
	uint8_t  ltk[2][16];         /* distributed LTKs, CENTRAL then PERIPHERAL, rule 8 */
	uint32_t preq, prsp, mconf, sconf, mrand, srand;   /* message indices, 0xffffffff if none */
	uint32_t tk;                 /* rule 5 */
	uint8_t  method;             /* NONE 0, LEGACY 1, SECURE 2, OOB 3, INVALID 4 */
	uint8_t  flags;              /* PREQ 1, PRSP 2, MCONF 4, SCONF 8, MRAND 16, SRAND 32, ARMED 64, CRACKED 128 */
	uint8_t  keys;               /* STK 1, LTK_CENTRAL 2, LTK_PERIPHERAL 4 */
	uint8_t  key_size;           /* ks, rule 3 */
	uint8_t  key;                /* slot in the key table, 0xff if none */
	uint8_t  reserved[7];        /* written as 0 */
} btbbx_le_pair;

/* Nothing is read back and the call is asynchronous on hip_stream.  d_scratch: btbbx_le_pair_scratch_bytes(conn_cap) bytes (about
 * 150 per connection), 16-byte aligned.  The count of launches, 12, depends on nothing.
 * BTBBX_E_ARG, before any launch: a null pointer (d_msgs may be null with msg_cap 0, d_bytes with byte_cap 0, d_keys with key_cap
 * 0), tk_limit > 1000000, key_cap > 64, d_seeds, d_msgs or d_pairs not 8-byte aligned (the counters: 4), a scratch that is too small
 * or not 16-byte aligned.  conn_cap == 0 succeeds and writes only the key count, as 0, and the zeroed key table. */
size_t btbbx_le_pair_scratch_bytes(uint32_t conn_cap);
int btbbx_le_pair_device(const uint32_t *d_conn_count, uint32_t conn_cap, const btbbx_le_seed *d_seeds,
			 const btbbx_le_msg *d_msgs, const uint32_t *d_msg_count, uint32_t msg_cap,
			 const uint8_t *d_bytes, uint64_t byte_cap, uint32_t tk_limit,
			 btbbx_le_pair *d_pairs, uint8_t *d_keys, uint32_t key_cap, uint32_t *d_key_count,
			 void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* Host wrapper: btbbx_le_epoch_host's chain (advertising scan, tracking, seed stage) with the data stage and this stage as its
 * last stage on the same stream.  btbbx_le_epoch_host's arguments up to and including seeds and its return value; msg_cap and
 * byte_cap: the device-side room for the data stage's messages, which are not copied out; pairs: conn_cap records, parallel to
 * conns; keys: 16 * key_cap octets (may be NULL with key_cap 0), the key table of rule 7; *n_keys_out (may be NULL) =
 * *d_key_count.  A capture without a candidate or without a stored connection gives a zeroed table and the count 0.
 * BTBBX_E_ARG: btbbx_le_epoch_host's conditions, pairs NULL with conn_cap != 0, keys NULL with key_cap != 0, tk_limit > 1000000,
 * key_cap > 64. */
int64_t btbbx_le_pair_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			   uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
			   btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
			   uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
			   int adv_errors, btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_seed *seeds,
			   uint64_t msg_cap, uint64_t byte_cap, uint32_t tk_limit, btbbx_le_pair *pairs, uint8_t *keys,
			   uint32_t key_cap, uint32_t *n_keys_out);

/* ---- LE address resolution: IRKs from SMP, RPAs resolved, identities ------------------------
 * Behind the advertising scan and -- for the keys the peers distribute -- behind the decryption stage, on the device: the distinct
 * device addresses of the advertising records, a table of identity resolving keys (IRKs: the caller's, then those the SMP
 * messages carry), every resolvable private address (RPA) tried against every key of the table, and per connection which
 * address and which key its two ends have.  It changes nothing of its input.
 *
 * The input is the decoded advertising records (d_adv, d_adv_count, adv_cap, as btbbx_le_seed_device takes them; A = the smaller
 * of count and cap), the message outputs of the data stage or the decryption stage exactly as btbbx_le_pair_device takes them
 * (d_msgs may be NULL with msg_cap 0: nothing is harvested then; the same three skip guards apply: conn >= K, octets outside
 * byte_cap, bytes < 4 + l2cap_len; an SMP message is what that stage's rule 1 says, sent by role CENTRAL or PERIPHERAL), the
 * connections (d_conn_count, conn_cap, d_seeds; K = the smaller of count and cap; conn_cap 0 is allowed: no peers, no harvest)
 * and the caller's keys (d_given, n_given keys of 16 octets in AES key order, most significant octet first: the byte order
 * btbbx_le_crypt_device takes).  All arithmetic is integer arithmetic.  An address is six octets a[0..5] as they lie in the PDU
 * (least significant first), like seed.init_a, with its random bit t.
 *   1. KIND.  PUBLIC 0 iff t == 0.  Otherwise by a[5] >> 6: 0 NONRESOLVABLE 1, 1 RESOLVABLE 2, 2 RESERVED 3, 3 STATIC 4.
 *   2. SLOTS.  Record i < A has the address slots 2i and 2i + 1.  A record with crc_ok == 0, is_data != 0 or channel_idx < 37
 *      has none.  Otherwise, with bytes[6..11] the first and bytes[12..17] the second address of the PDU, by adv_type:
 *        0, 2, 4, 6  ADV_IND, ADV_NONCONN_IND, SCAN_RSP, ADV_SCAN_IND   length >= 6: slot 0 = the first address, t = adv_tx_add,
 *                    role ADVERTISER 1; no slot 1
 *        1           ADV_DIRECT_IND   length >= 12: slot 0 ADVERTISER 1 (adv_tx_add), slot 1 TARGET 8 (adv_rx_add)
 *        3           SCAN_REQ         length >= 12: slot 0 SCANNER 2 (adv_tx_add), slot 1 ADVERTISER 1 (adv_rx_add)
 *        5           CONNECT_IND      length >= 12: slot 0 INITIATOR 4 (adv_tx_add), slot 1 ADVERTISER 1 (adv_rx_add)
 *      Every other type has none: extended advertising is not read.
 *   3. DISTINCT LIST.  key = t << 48 | a[5] << 40 | ... | a[0].  The distinct keys in ascending order are the address list;
 *      *d_addr_count = their number N: the stage WRITES it, it does not add to it.  d_slot_addr[s] (2 * adv_cap entries, every
 *      one written) = the rank of slot s's key in that list, 0xffffffff for a slot that holds no address.  The first
 *      min(N, addr_cap) records are written to d_addrs, every byte of them and nothing behind them.
 *   4. IRK TABLE.  Slots 0 .. n_given - 1 are the caller's keys, flag GIVEN 1, conn = 0xffffffff, role 0.  Behind them the
 *      harvested keys by ascending (connection, role), CENTRAL before PERIPHERAL, flag HARVESTED 2, conn and role set.  A
 *      (connection, role) has a key iff it has an SMP message with code 0x08 and l2cap_len 17; the first such counts:
 *      key[j] = v[16 - j], the byte order of the pairing stage's rule 8.  If it also has one with code 0x09 and l2cap_len 8, the
 *      first counts: id_random = v[1] & 1, id_addr[j] = v[2 + j], flag HAS_ADDR 4.  A slot whose sixteen octets are all zero
 *      gets flag NULLKEY 8 and is never tried (the specification's "no IRK" is one such).  *d_irk_count = n_given + the number
 *      of harvested keys, written, not added to; it may exceed irk_cap: the keys beyond the cap are neither stored nor tried.
 *      Duplicates are kept as they come.  Every byte of d_irks[0 .. irk_cap) is written, behind the count as zeros with
 *      conn = 0xffffffff.  irk_cap is 0..BTBBX_LE_RESOLVE_MAX_IRKS, n_given <= irk_cap.
 *   5. RESOLVE.  Over all N distinct addresses, whatever addr_cap is, and the min(*d_irk_count, irk_cap) slots without NULLKEY:
 *      only RESOLVABLE addresses are tried.  block[0..12] = 0, block[13] = a[5], block[14] = a[4], block[15] = a[3]; address
 *      and slot MATCH iff o = AES(key, block) has o[13] == a[2], o[14] == a[1], o[15] == a[0] (ah of Core Vol 3 Part H 2.2.2:
 *      prand = a[5..3], hash = a[2..0]).  The address's irk is the smallest matching slot, 0xffff if none.  A wrong key matches
 *      with probability 2^-24 per trial: against 4096 keys one unrelated RPA in 4096 resolves by accident, 256 of 2^20.
 *   6. ADDRESS RECORDS.  first_offset / last_offset: the smallest and the largest offset of a record that holds the address in a
 *      slot; n_slots: how many slots hold it; first_rec: the smallest such record index; addr, random (t), kind (rule 1), irk
 *      (rule 5), roles: the OR of the slot roles; channels: bit channel_idx - 37 of every such record.
 *   7. IRK RECORDS.  key, id_addr, id_random, flags, conn, role (rule 4); n_addrs: the distinct addresses whose irk is this
 *      slot; n_slots: the slots they fill.  All N addresses count, not only the stored ones.
 *   8. PEERS.  Parallel to the connections, every byte of d_peers[0 .. K) written, nothing behind it.  For a SEEDED connection
 *      whose seed.request < A: init_addr = d_slot_addr[2 * request], adv_addr = d_slot_addr[2 * request + 1], init_irk /
 *      adv_irk = those addresses' irk; otherwise 0xffffffff / 0xffff.  irk[role] = the table slot of the key harvested from
 *      that (connection, role), 0xffff if there is none or it lies beyond irk_cap.  The stage reads flags and request of a seed,
 *      nothing else.
 * LIMITS: extended advertising (type 7 and what AuxPtr points to) and addresses inside AdvData are not read; CSRK and
 * EDIV / Rand are not extracted; a second pairing's keys do not replace the first's; the Identity messages of an LE Secure
 * Connections pairing are read like any others once a key decrypts them. */
#define BTBBX_LE_RESOLVE_MAX_IRKS 4096u
#define BTBBX_LE_ADDR_PUBLIC        0u   /* btbbx_le_addr.kind */
#define BTBBX_LE_ADDR_NONRESOLVABLE 1u
#define BTBBX_LE_ADDR_RESOLVABLE    2u
#define BTBBX_LE_ADDR_RESERVED      3u
#define BTBBX_LE_ADDR_STATIC        4u
#define BTBBX_LE_ADDR_ADVERTISER    1u   /* btbbx_le_addr.roles */
#define BTBBX_LE_ADDR_SCANNER       2u
#define BTBBX_LE_ADDR_INITIATOR     4u
#define BTBBX_LE_ADDR_TARGET        8u
#define BTBBX_LE_IRK_GIVEN          1u   /* btbbx_le_irk.flags */
#define BTBBX_LE_IRK_HARVESTED      2u
#define BTBBX_LE_IRK_HAS_ADDR       4u
#define BTBBX_LE_IRK_NULLKEY        8u

typedef struct btbbx_le_addr {       /* 40 bytes, one per distinct address, ascending by key */
	uint64_t first_offset, last_offset;
	uint32_t n_slots, first_rec;
	uint8_t  addr[6], random, kind;
	uint16_t irk;                /* table slot, 0xffff if none */
	uint8_t  roles;              /* ADVERTISER 1, SCANNER 2, INITIATOR 4, TARGET 8 */
	uint8_t  channels;           /* bit channel_idx - 37 */
	uint8_t  reserved[4];        /* written as 0 */
} btbbx_le_addr;
typedef struct btbbx_le_irk {        /* 40 bytes, one per table slot */
	uint8_t  key[16], id_addr[6], id_random, flags;
	uint32_t conn;               /* 0xffffffff unless HARVESTED */
	uint32_t n_addrs, n_slots;
	uint8_t  role, reserved[3];  /* reserved: written as 0 */
} btbbx_le_irk;
typedef struct btbbx_le_peer {       /* 16 bytes, parallel to conns */
	uint32_t init_addr, adv_addr; /* ranks in the address list, 0xffffffff if none */
	uint16_t init_irk, adv_irk, irk[2];
} btbbx_le_peer;

/* Nothing is read back and the call is asynchronous on hip_stream.  d_scratch: btbbx_le_resolve_scratch_bytes(adv_cap, conn_cap,
 * irk_cap) bytes, 16-byte aligned: the keys and vals of both sides of the sort, its histogram, the per-address words, 44 words of
 * schedule per table slot, the round table and the counts, about 120 bytes per advertising record.  The count of launches, 32,
 * depends on no count and no cap.
 * BTBBX_E_ARG, before any launch: a null pointer (d_adv and d_slot_addr may be null with adv_cap 0, d_msgs with msg_cap 0, d_bytes
 * with byte_cap 0, d_given with n_given 0, d_addrs with addr_cap 0, d_irks with irk_cap 0, d_conn_count, d_seeds and d_peers with
 * conn_cap 0), irk_cap > 4096, n_given > irk_cap, adv_cap >= 2^31, a record pointer that is not 8-byte aligned (the slot map and
 * the counters: 4), a scratch that is too small or not 16-byte aligned. */
size_t btbbx_le_resolve_scratch_bytes(uint32_t adv_cap, uint32_t conn_cap, uint32_t irk_cap);
int btbbx_le_resolve_device(const btbbx_le_pkt *d_adv, const uint32_t *d_adv_count, uint32_t adv_cap,
			    const uint32_t *d_conn_count, uint32_t conn_cap, const btbbx_le_seed *d_seeds,
			    const btbbx_le_msg *d_msgs, const uint32_t *d_msg_count, uint32_t msg_cap,
			    const uint8_t *d_bytes, uint64_t byte_cap, const uint8_t *d_given, uint32_t n_given,
			    uint32_t *d_slot_addr, btbbx_le_addr *d_addrs, uint32_t addr_cap, uint32_t *d_addr_count,
			    btbbx_le_irk *d_irks, uint32_t irk_cap, uint32_t *d_irk_count, btbbx_le_peer *d_peers,
			    void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* Host wrapper over the advertising channels alone: capture in, advertising scan (BTBBX_LE_ADV_AA, adv_errors), order, decode,
 * then this stage with the caller's keys and no connection; it works on a capture without any data channel.  adv: adv_cap
 * decoded records in (stream, offset) order; slot_addr: 2 * adv_cap entries; addrs: addr_cap records; irks: irk_cap records.  Returns the
 * number of advertising records found; when it, *n_addrs_out or *n_irks_out exceeds its cap the prefix is returned and the count
 * says so (slot_addr then names ranks beyond addr_cap too).  The n_*_out pointers may be NULL.
 * BTBBX_E_ARG: btbbx_le_scan_host's conditions, a null array with a cap != 0, keys NULL with n_given != 0, irk_cap > 4096,
 * n_given > irk_cap, adv_cap >= 2^31. */
int64_t btbbx_le_resolve_adv_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				  uint64_t search_bits, const uint16_t *phys_channel, int adv_errors,
				  const uint8_t *given, uint32_t n_given, btbbx_le_pkt *adv, uint64_t adv_cap,
				  uint32_t *slot_addr, btbbx_le_addr *addrs, uint32_t addr_cap, uint32_t *n_addrs_out,
				  btbbx_le_irk *irks, uint32_t irk_cap, uint32_t *n_irks_out);

/* Host wrapper: btbbx_le_keyed_span_host's chain up to and including the decryption stage (keys, n_keys >= 1, window; msg_cap and
 * byte_cap: the device-side room for the decrypted messages, which are not copied out), then this stage over the decrypted
 * messages, the chain's own advertising records and the caller's keys (given, n_given, which may be 0).  btbbx_le_epoch_host's
 * arguments up to and including seeds and its return value; peers: conn_cap records parallel to conns; irks: irk_cap records;
 * addrs: addr_cap records; *n_irks_out and *n_addrs_out (may be NULL): the counts, which may exceed the caps.  A capture without
 * a candidate or without a stored connection gives zeroed tables and the counts 0.
 * BTBBX_E_ARG: btbbx_le_keyed_span_host's conditions on what it shares, peers NULL with conn_cap != 0, irks NULL with irk_cap
 * != 0, addrs NULL with addr_cap != 0, given NULL with n_given != 0, irk_cap > 4096, n_given > irk_cap. */
int64_t btbbx_le_resolve_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			      uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, uint32_t min_count,
			      btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
			      uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
			      int adv_errors, btbbx_le_track *tracks, btbbx_le_track_pkt *pkts, btbbx_le_seed *seeds,
			      const uint8_t *keys, uint32_t n_keys, uint32_t window, uint64_t msg_cap, uint64_t byte_cap,
			      const uint8_t *given, uint32_t n_given, btbbx_le_peer *peers, btbbx_le_irk *irks, uint32_t irk_cap,
			      uint32_t *n_irks_out, btbbx_le_addr *addrs, uint32_t addr_cap, uint32_t *n_addrs_out);

/* ---- LE Coded PHY scan: coded access address search, Viterbi decode ------------------------
 * The LE Coded PHY (Core v5.x Vol 6 Part B 2.2, 3.1, 3.2, 3.3) runs at the 1 Msym/s of the streams above.  AIR FORMAT, from the
 * first preamble symbol: 80 uncoded preamble symbols, ten times 0 0 1 1 1 1 0 0; FEC block 1 = access address (32 bits, LSB
 * first), CI (2 bits, LSB first), TERM1 (3 zero bits), always at S = 8 symbols per bit: 296 symbols; FEC block 2 = PDU (2 + L
 * octets), CRC-24, TERM2 (3 zero bits): N = 8 * (L + 5) + 3 bits at S = 8 (CI 0) or S = 2 (CI 1); CI 2 and 3 are RFU.  CRC,
 * then whitening, then FEC, then the pattern mapper; CRC and whitening are the 1M ones and cover PDU (whitening: and CRC) only.
 * The encoder is rate 1/2, K = 4, starts each block in state 0, a0 = b ^ b1 ^ b2 ^ b3, a1 = b ^ b2 ^ b3, a0 sent first; at S = 8 a
 * coded 0 is sent as 0 0 1 1 and a coded 1 as 1 1 0 0, at S = 2 coded bits are sent as they are.  A packet is 376 + S * N
 * symbols, 17040 at most.  Hard decisions only.
 *
 *  1. MATCH.  Offset o < search_bits of a stream matches iff the 336 symbols from o differ from preamble + mapped, coded AA
 *     (encoder from state 0, no CI) in at most max_errors places, max_errors 0 .. BTBBX_LE_CODED_MAX_ERRORS.  The record is a
 *     btbbx_hit: offset = first preamble symbol, lap = the AA SEARCHED FOR, ac_errors = the mismatch count, stream.  Every matching
 *     offset is reported, nothing is suppressed; an AA whose pattern is periodic (all zeros is one) matches at shifts too.  63 keeps
 *     the count in a uint8_t and below the side lobes of a true packet (smallest count at a wrong offset within +-400 symbols:
 *     104 for the advertising AA, 84 over 200 random AAs).  The records leave in no order; btbbx_order_hits_device orders them.
 *  2. TRELLIS.  State s = b1 | b2 << 1 | b3 << 2, next state (s << 1 | b) & 7.  A step reads S symbols; its branch metric is the
 *     Hamming distance between them and the mapped (a0, a1) of the transition.  Symbols past the stream's end read as 0.  State
 *     s' has the predecessors (s' >> 1) | x << 2, x = 0 or 1; the one with the smaller sum survives, x = 0 on equal sums.  A block
 *     starts with state 0 at metric 0, the other states unreachable.
 *  3. BLOCK 1.  37 steps of 8 symbols from o + 80, traced back from state 0.  Bits 0..31 = access_address (the DECODED one, which
 *     may differ from the one searched for), bits 32..33 = ci, metric1 = the path's metric.
 *  4. S.  ci 0: 8.  ci 1: 2.  ci 2 or 3: s = 0, there is no block 2: pdu_bytes = 0, crc_ok = 0, truncated = 0, symbols = 376,
 *     metric2 = 0, header_moved = 0, crc_rx = crc_calc = 0, bytes = the four AA octets and zeros, and the fields derived from the
 *     header are those of a zero header.
 *  5. LENGTH.  Block 2 starts at o + 376 and is ONE forward pass.  After step 16 + BTBBX_LE_CODED_LAG = 40 the path is traced back
 *     from the state with the smallest metric (smallest state index on ties); its first 16 bits, dewhitened, are the provisional
 *     header, L its octet 1 (all 8 bits), N = 8 * (L + 5) + 3 (>= 43 > 40: the lag step always exists).
 *  6. BODY.  The forward pass goes on to step N; the path is traced back from state 0.  Its first N - 3 bits are header, payload
 *     and CRC as sent, metric2 its metric; header_moved = 1 iff its 16 header bits differ from rule 5's.  L is not revised.
 *  7. RECORD.  The bits of rule 6 are dewhitened with the channel's register, the CRC-24 runs under crc_init over 2 + L octets;
 *     crc_rx, crc_calc, pdu_bytes, crc_ok, bytes[64] (decoded AA, then the dewhitened octets, zero past the end) and every lell
 *     field are formed exactly as btbbx_le_decode_hits_device forms them from its octets (one device function serves both).
 *     truncated = 1 and crc_ok = 0 iff o + symbols > 64 * n_words.  aa_errors = the hit's ac_errors; offset and stream the hit's.
 *  8. WRITES.  Records [0, min(*d_count, cap)) of both arrays are written whole, the reserved bytes as 0; nothing else is
 *     written; the count stays on the device.
 * LIMITS: the promiscuous discovery of coded connections (unknown AA) is the stage behind this one ("promiscuous LE Coded
 * connection discovery" below); not in here are reading ADV_EXT_IND / AuxPtr (extended
 * advertising), feeding coded records to the seed, follow or resolve stages, the 2M PHY, soft decisions, and bytes beyond 64
 * octets.  The lell_* entries still abort. */
#define BTBBX_LE_CODED_PATTERN    336   /* preamble 80 + coded AA 256 symbols */
#define BTBBX_LE_CODED_MAX_ERRORS 63
#define BTBBX_LE_CODED_LAG        24

typedef struct btbbx_le_coded_info {   /* 16 bytes, parallel to the btbbx_le_pkt of the same hit */
	uint32_t symbols;      /* 376 + S * N, from the first preamble symbol; 376 when s == 0 */
	uint32_t metric2;      /* symbol mismatches along block 2's chosen path */
	uint16_t metric1;      /* the same for block 1 (296 symbols) */
	uint8_t  ci, s;        /* CI as decoded; 8, 2, or 0 for an RFU CI */
	uint8_t  header_moved; /* the final path's 16 header bits differ from the lag decision's (rule 5) */
	uint8_t  reserved[3];
} btbbx_le_coded_info;

/* Stage 1 (rule 1).  Arguments as btbbx_le_scan_device; BTBBX_E_ARG: max_errors outside 0..63, search_bits + 335 > 64 * n_words,
 * n_streams outside 1..65535, pitch_words < n_words, a null pointer, d_words not 8-, d_hits not 16-, d_hit_count not 4-byte
 * aligned.  The counter is added to, not cleared. */
int btbbx_le_coded_scan_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			       uint64_t search_bits, uint32_t aa, int max_errors,
			       btbbx_hit *d_hits, uint32_t hit_cap, uint32_t *d_hit_count, void *hip_stream);

/* Stage 2 (rules 2..8) for the first min(*d_count, cap) hits.  The decoder keeps its survivor decisions in LDS (2112 bytes per
 * hit) and needs NO caller scratch: btbbx_le_coded_scratch_bytes returns 0 for every cap, d_scratch may be NULL and is never
 * touched, so no scratch is too short.  BTBBX_E_ARG: a null pointer with cap != 0, d_words, d_hits or d_out not 8-, d_count or
 * d_info not 4-, d_phys_channel not 2-byte aligned, n_words > 2^40. */
size_t btbbx_le_coded_scratch_bytes(uint32_t cap);
int btbbx_le_coded_decode_hits_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words,
				      const btbbx_hit *d_hits, const uint32_t *d_count, uint32_t cap,
				      const uint16_t *d_phys_channel, uint32_t crc_init,
				      btbbx_le_pkt *d_out, btbbx_le_coded_info *d_info,
				      void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* Host wrapper, btbbx_le_scan_host's chain: copy in, scan, scan again with room for every hit when the first guess was short,
 * order by (stream, offset), decode, copy out.  Returns the number of matches or a negative BTBBX_E_*; when it exceeds cap the
 * cap SMALLEST (stream, offset) records are returned.  Safe to call from several host threads at once. */
int64_t btbbx_le_coded_scan_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				 uint64_t search_bits, const uint16_t *phys_channel, uint32_t aa, uint32_t crc_init,
				 int max_errors, btbbx_le_pkt *pkts, btbbx_le_coded_info *info, uint64_t cap);

/* ---- promiscuous LE Coded connection discovery: access address and CRCInit ------------------
 * The coded scan above finds a packet whose access address it is told.  On the 37 data channels every connection has an AA and a
 * CRCInit of its own; this stage finds both in a capture that names neither, and hands them to the grouping of the 1M discovery
 * (btbbx_le_discover_group_device) unchanged.  Air format, trellis, tie rule, lag and whitening are rules 2 to 7 of the coded
 * decoder above ("the decoder's rule n" below); nothing of them is restated.  The contract is exact, without tolerances.
 * Offset o of stream s is a CANDIDATE iff
 *  1. CHANNEL.  ch = le_channel_index(phys_channel[s]) < 37 (an advertising channel yields no candidate).
 *  2. RANGE.  o < search_bits; the argument check is btbbx_le_coded_scan_device's, search_bits + 335 <= 64 * n_words.
 *  3. BLOCK 1.  The decoder's rule 3 from o + 80: 37 steps, traced back from state 0, give AA' (bits 0..31), ci (bits 32..33) and
 *     metric1.
 *  4. MATCH.  The 336 symbols from o differ from preamble + mapped, coded AA' in at most max_errors (0..63) places: rule 1 of the
 *     coded scan with the DECODED address.  Not "some address exists": addresses that differ in their last bits lie 8 symbols
 *     apart, so only the decoded one is determinate.  errors = that count.
 *  5. ADDRESS.  AA' has no data-channel offense (aa_data_channel_offenses, as rule 3 of the 1M discovery).
 *  6. S.  ci 0: S = 8.  ci 1: S = 2.  An RFU ci (2, 3) is no candidate.
 *  7. HEADER.  The decoder's rule 5 (block 2 from o + 376, the lag decision behind step 40 from the best state) gives the
 *     provisional dewhitened header h0, h1: (h0 & 3) != 0, (h0 & 0xe0) == 0 and h1 <= max_len (0..255).  L = h1.
 *  8. FIT.  The packet lies in the stream: o + 376 + S * (8 * (L + 5) + 3) <= 64 * n_words.
 *  9. BODY.  The decoder's rule 6: the forward pass goes on to step N = 8 * (L + 5) + 3, the path is traced back from state 0,
 *     metric2 its metric.  header_moved must be 0: a path that disowns the length it was cut to is no candidate.
 * 10. CRCINIT.  The one 24-bit preset, in the orientation btbbx_le_decode_hits_device takes, with which the CRC over the 2 + L
 *     dewhitened octets of rule 9's path equals its 24 received CRC bits: the register run backwards, last octet first.
 * 11. RECORD.  A btbbx_le_cand: offset = first preamble symbol, access_address = AA', crc_init, stream, header0 = h0, length = h1,
 *     conn = ch -- what btbbx_le_discover_group_device asks of a list that is not the 1M scan's.  When d_info is not NULL a
 *     btbbx_le_coded_cand_info is written at the same index.  The info records are parallel to THIS list only: the grouping
 *     reorders the candidates in place and knows nothing of them.
 * 12. WRITES.  Records [0, min(*d_cand_count, cand_cap)) are written whole, the reserved bytes as 0, and nothing else is written;
 *     *d_cand_count counts every candidate, also those past cand_cap.  The records leave in no order.
 * A true packet is a candidate when block 1 decodes to the address sent; symbol errors that make it decode to another address
 * give a candidate of that other address or none (rule 4 decides), never one of the address sent.  Noise: a window passes rule
 * 4 at max_errors 63 at about 1e-8 of the offsets before rules 5..9 apply.
 * LIMITS, each one out of scope here: tracking coded candidates (btbbx_le_track_device closes an event by the 1M duration 80 + 8
 * * length and needs the coded duration 376 + S * N first), ADV_EXT_IND / AuxPtr / AUX_CONNECT_REQ (extended advertising), soft
 * decisions, the 2M PHY, and the lell_* entries, which still abort.  (The first of these is lifted by the stage behind this one,
 * "LE Coded connection tracking" below: btbbx_le_ctrack_symbols_device and btbbx_le_ctrack_device.) */
typedef struct btbbx_le_coded_cand_info {   /* 16 bytes, parallel to the btbbx_le_cand of the same index of the SCAN's list */
	uint32_t symbols;      /* 376 + S * N, from the first preamble symbol */
	uint32_t metric2;      /* symbol mismatches along block 2's path */
	uint16_t metric1;      /* the same for block 1 */
	uint8_t  errors;       /* rule 4's count */
	uint8_t  ci, s;        /* CI as decoded (0, 1); 8 or 2 */
	uint8_t  reserved[3];
} btbbx_le_coded_cand_info;

/* Rules 1..12 for offsets [0, search_bits) of every stream, two kernels on hip_stream: an address-free scan leaves pre-records
 * (offset, stream, a lower bound of rule 4's count) in d_scratch, a decoder turns them into candidates.  d_scratch holds
 * pre_cap = scratch_bytes / 16 pre-records, btbbx_le_cfind_scratch_bytes(pre_cap) = 16 * pre_cap bytes; *d_pre_count is cleared
 * by the call and counts every pre-record: when it exceeds pre_cap the surplus was dropped and candidates may be missing -- call
 * again with room.  *d_cand_count (zeroed by the caller) is added to.  Nothing is read back.  BTBBX_E_ARG: max_errors outside
 * 0..63, max_len above 255, search_bits + 335 > 64 * n_words, n_streams outside 1..65535, pitch_words < n_words, a null pointer
 * (d_cands may be NULL when cand_cap is 0, d_info always), scratch_bytes < 16, d_words or d_cands not 8-, d_info or d_scratch not
 * 16-, a counter not 4-, d_phys_channel not 2-byte aligned.  (The entries are named le_cfind, "coded find".) */
size_t btbbx_le_cfind_scratch_bytes(uint32_t pre_cap);
int btbbx_le_cfind_scan_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			       uint64_t search_bits, const uint16_t *d_phys_channel, uint32_t max_len, int max_errors,
			       btbbx_le_cand *d_cands, btbbx_le_coded_cand_info *d_info, uint32_t cand_cap, uint32_t *d_cand_count,
			       uint32_t *d_pre_count, void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* Host wrapper, btbbx_le_discover_host's chain with this scan in it: copy in, scan (repeated with room when the pre-record list or
 * the candidate list was short), btbbx_le_discover_group_device, copy out.  Returns, and fills conns, cands and *n_cands_out, as
 * btbbx_le_discover_host does.  Safe to call from several host threads at once. */
int64_t btbbx_le_cfind_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			    uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, int max_errors, uint32_t min_count,
			    btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands, uint64_t cand_cap,
			    uint64_t *n_cands_out);

/* ---- LE Coded connection tracking: coded durations, events, hop check ------------------------
 * btbbx_le_track_device closes a connection event by the 1M duration 80 + 8 * length.  A coded packet lasts 376 + S * N symbols,
 * 8 to 70 times as long (an empty PDU: 720 symbols at S = 8; 255 octets: 17040), so on coded candidates every reply opens an
 * event of its own, the event spacings leave the 1.25 ms grid, the connection is not TIMED and btbbx_le_csa2_device evaluates
 * nothing.  Only the tracking's rule 3 reads a duration.  This stage computes the duration of every candidate of a list AS IT
 * STANDS -- behind the grouping, which reorders the list in place and leaves the discovery's info records behind -- and runs the
 * tracking with rule 3 taking it.  Trellis and tie rule are the coded decoder's rules 2 and 3 ("LE Coded PHY scan" above); nothing
 * of them is restated.  With N = min(*d_cand_count, cand_cap), for every i < N:
 *  1. STREAM.  cands[i].stream >= n_streams: symbols_i = 0.
 *  2. CI.  Otherwise the decoder's rule 3 at o = cands[i].offset: 37 steps of 8 symbols from o + 80, symbols past the stream's end
 *     read as 0 (an offset beyond the stream reads nothing but zeros), predecessor x = 0 on equal sums, traced back from state 0;
 *     ci = bits 32..33.  Block 1 is not whitened: no channel is needed, and an advertising stream is decoded like any other.
 *  3. S.  ci 0: S = 8.  ci 1: S = 2.  With L = cands[i].length, symbols_i = 376 + S * (8 * (L + 5) + 3).  An RFU ci (2, 3):
 *     symbols_i = 376, the decoder's rule 4.
 *  4. WRITES.  d_symbols[0 .. N) is written and nothing else; the count stays on the device, nothing is read back.
 * For a candidate that btbbx_le_cfind_scan_device produced, symbols_i equals the symbols of its btbbx_le_coded_cand_info.
 * Offsets lie below 2^48 (the grouping's promise); all address arithmetic is 64 bits wide.
 * TRACKING.  btbbx_le_ctrack_device is btbbx_le_track_device -- its rules 1, 2 and 4 to 7 word for word, its records, its flags,
 * btbbx_le_track_scratch_bytes, its launch count -- with rule 3 changed to end_m = offset_m + d_symbols[m] (a 64-bit sum; m = the
 * candidate's index in the list).  With d_symbols[i] = 80 + 8 * cands[i].length every output byte equals btbbx_le_track_device's.
 * LIMITS, each one out of scope here: feeding coded connections to the seed, follow, span, data, decryption or pairing stages
 * (they read payloads as 1M bits from the streams); LL_PHY_UPDATE_IND and connections that change PHY inside the capture (one
 * list, one kind of duration); ADV_EXT_IND, AuxPtr and AUX_CONNECT_REQ; soft decisions; the 2M PHY; the lell_* entries, which
 * still abort.  (The entries are named le_ctrack, "coded track".) */

/* Rules 1..4, one kernel on hip_stream.  BTBBX_E_ARG, before any launch: a null pointer with cand_cap != 0, d_words or d_cands
 * not 8-, d_symbols or the counter not 4-byte aligned, n_streams outside 1..65535, pitch_words < n_words, n_words > 2^40.
 * cand_cap == 0 succeeds and writes nothing. */
int btbbx_le_ctrack_symbols_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
				   const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
				   uint32_t *d_symbols, void *hip_stream);

/* The tracking with per-candidate durations.  Arguments, promises, writes and BTBBX_E_ARG as btbbx_le_track_device; in addition
 * d_symbols (N dwords, parallel to d_cands) must not be NULL and must be 4-byte aligned. */
int btbbx_le_ctrack_device(const btbbx_le_cand *d_cands, const uint32_t *d_cand_count, uint32_t cand_cap,
			   const btbbx_le_conn *d_conns, const uint32_t *d_conn_count, uint32_t conn_cap,
			   const uint16_t *d_phys_channel, uint32_t n_streams, const uint32_t *d_symbols,
			   uint32_t unit_bits, uint32_t ifs_bits, uint32_t jitter_bits, uint32_t flags,
			   btbbx_le_track *d_tracks, btbbx_le_track_pkt *d_pkts,
			   void *d_scratch, size_t scratch_bytes, void *hip_stream);

/* Host wrapper, btbbx_le_cfind_host's chain -- copy in, the coded scan repeated with room, the grouping -- with the durations of
 * the sorted list, the tracking that takes them and btbbx_le_csa2_device behind it on the same stream, then the copy-out.  Returns,
 * and fills conns, cands and *n_cands_out, as btbbx_le_cfind_host does; tracks and sel are parallel to conns, pkts, sel_pkts and
 * symbols to cands, as in btbbx_le_csa2_host.  pkts, sel_pkts and symbols may be NULL; when sel is NULL channel selection #2 is
 * not queued (and sel_pkts not touched).  When no connection was stored, pkts and sel_pkts get the 0xff fill of the 1M wrappers
 * (no candidate is a member); symbols holds the durations all the same.  Safe to call from several host threads at once. */
int64_t btbbx_le_ctrack_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			     uint64_t search_bits, const uint16_t *phys_channel, uint32_t max_len, int max_errors,
			     uint32_t min_count, btbbx_le_conn *conns, uint64_t conn_cap, btbbx_le_cand *cands,
			     uint64_t cand_cap, uint64_t *n_cands_out, uint32_t unit_bits, uint32_t ifs_bits,
			     uint32_t jitter_bits, uint32_t flags, btbbx_le_track *tracks, btbbx_le_track_pkt *pkts,
			     btbbx_le_csa2 *sel, btbbx_le_csa2_pkt *sel_pkts, uint32_t *symbols);

/* ---- hop selection and CLK1-27 reversal ------------------------- */
#define BTBBX_SEQUENCE_LENGTH 134217728u   /* values of CLK1-27, bluetooth_piconet.h:102 */

/* the inputs of the hop selection kernel for one piconet (precalc + address_precalc,
 * bluetooth_piconet.c:171-217) */
typedef struct btbbx_hop_cfg {
	uint32_t address;        /* (UAP << 24 | LAP) & 0xfffffff */
	uint8_t  afh;            /* BTBB_IS_AFH: index the bank modulo used_channels */
	uint8_t  used_channels;
	uint8_t  reserved[2];
	uint8_t  bank[80];       /* frequency register bank; entries past the filled part are 0 */
} btbbx_hop_cfg;

/* afh_map == NULL: basic hopping over all 79 channels; otherwise the 10-byte AFH channel map */
void btbbx_hop_cfg_init(btbbx_hop_cfg *cfg, uint32_t address, const uint8_t *afh_map);

/* channels of CLK1-27 values [first, first + count) -- what gen_hops stores in
 * sequence[first .. first+count); first and count multiples of 64; d_sequence receives count
 * bytes.  The whole 2^27-entry pattern is 128 MiB. */
int btbbx_hop_sequence_device(const btbbx_hop_cfg *cfg, uint64_t first, uint64_t count,
			      uint8_t *d_sequence, void *hip_stream);
/* hop(clock) for arbitrary CLK1-27 values (taken modulo 2^27) */
int btbbx_hop_channels_device(const btbbx_hop_cfg *cfg, const uint32_t *d_clocks, uint32_t n,
			      uint8_t *d_channels, void *hip_stream);

/* CLK1-27 reversal: the candidate list lives in HBM.  open() = init_candidates
 * (bluetooth_piconet.c:455-472): all clocks congruent clk6 mod 64 whose hop is `channel`
 * (a value > 127 matches nothing, as the reference compares signed chars);
 * aliased != 0 compares ((ch + 24) % 25) + 26 instead (:449-452). */
typedef struct btbbx_hop_reversal btbbx_hop_reversal;
btbbx_hop_reversal *btbbx_hop_reversal_open(const btbbx_hop_cfg *cfg, uint32_t clk6, uint8_t channel,
					    int aliased, int *n_candidates);
/* channel_winnow over n_obs observed hops in order (index offset relative to the first packet,
 * channel), stopping after the first one that leaves <= 1 candidate (btbb_winnow, :614-645).
 * *stop = how many observations were applied before that one (n_obs if none did), *count =
 * candidates left, *cand0 = the first of them.  Returns 0 or a negative BTBBX_E_*. */
int btbbx_hop_reversal_winnow(btbbx_hop_reversal *h, const int32_t *index_offsets, const uint8_t *channels,
			      uint32_t n_obs, uint32_t *stop, uint32_t *count, uint32_t *cand0);
int64_t btbbx_hop_reversal_candidates(btbbx_hop_reversal *h, uint32_t *dst, uint64_t cap);  /* ascending */
void btbbx_hop_reversal_close(btbbx_hop_reversal *h);

/* ---- batch reversal: CLK1-27 of many piconets in one chain ---------------------------- */
/* One job = one piconet with its observed hops.  Job j, with observations off[0..n) / ch[0..n) =
 * [obs_first, obs_first + n_obs) of the two shared arrays, leaves exactly what
 *     r = btbbx_hop_reversal_open(&cfg, clk6, ch[0], aliased, &n_initial);
 *     btbbx_hop_reversal_winnow(r, off, ch, n, &stop, &count, &cand0);
 *     btbbx_hop_reversal_candidates(r, dst, cand_cap);
 * leave: observation 0 is applied by the winnow as well, a channel above 127 matches nothing, an empty
 * initial list gives stop = 0 / count = 0, stop = n_obs when no observation leaves at most one candidate,
 * cand0 = the smallest surviving clock (0 when count = 0). */
typedef struct btbbx_clock_job {        /* 104 bytes */
	btbbx_hop_cfg cfg;              /* as btbbx_hop_cfg_init leaves it */
	uint32_t clk6;                  /* known CLK1-6 of the first observation, 0..63 */
	uint32_t aliased;               /* != 0: compare ((ch + 24) % 25) + 26 */
	uint32_t obs_first, n_obs;      /* this job's observations: [obs_first, obs_first + n_obs) of the shared arrays */
} btbbx_clock_job;

typedef struct btbbx_clock_result {     /* 24 bytes */
	uint32_t status;                /* 0 done, 1 job rejected (every other field is 0 then) */
	uint32_t n_initial;             /* what btbbx_hop_reversal_open reports in *n_candidates */
	uint32_t stop, count, cand0;    /* what btbbx_hop_reversal_winnow reports for the job's observations */
	uint32_t n_stored;              /* min(count, cand_cap) candidates written for this job (0 when d_candidates is NULL) */
} btbbx_clock_result;

/* Device scratch of a batch of up to job_cap jobs: job_cap * (2 * 1028 + 1) * 4 bytes, rounded up to 256 -- per job a
 * histogram over the number of observations a candidate agrees with (1025 bins, padded), the smallest clock of every bin,
 * and one threshold.  It depends neither on cand_cap nor on how many candidates a job has: no candidate list is kept, the
 * candidates that are asked for are found a second time and go straight to d_candidates.  Host only, no device needed. */
size_t btbbx_hop_reversal_batch_scratch_bytes(uint32_t job_cap, uint32_t cand_cap);
/* Works the first min(*d_n_jobs, job_cap) jobs of d_jobs (d_n_jobs == NULL: job_cap jobs); records behind them are not
 * written.  All pointers are DEVICE pointers; d_index_offsets / d_channels hold n_obs_total observations shared by all jobs
 * (ranges may overlap).  The ascending first min(count, cand_cap) candidates of job j go to d_candidates[j * cand_cap ..];
 * the rest of its slots is not written.  d_candidates == NULL or cand_cap == 0: records only.  Three kernels and one memset
 * (two kernels without candidates) whatever the job count; asynchronous on hip_stream, nothing is synchronised and the job
 * count never comes to the host.
 * BTBBX_E_ARG before any launch for: d_jobs, d_results or d_scratch NULL, the observation arrays NULL with n_obs_total != 0,
 * job_cap == 0 or >= 2^31, scratch too small, a pointer that is not 4-byte aligned (the scratch: 16; the channels: any).
 * The jobs are checked on the device.  A job with clk6 > 63, n_obs == 0 or n_obs > 1024, obs_first + n_obs > n_obs_total
 * (computed without wrapping), or cfg.afh != 0 with cfg.used_channels 0 or above 79 gets status = 1 and zeros in its
 * record; none of its candidate slots is written and its neighbours are not disturbed. */
int btbbx_hop_reversal_batch_device(const btbbx_clock_job *d_jobs, const uint32_t *d_n_jobs, uint32_t job_cap,
				    const int32_t *d_index_offsets, const uint8_t *d_channels, uint32_t n_obs_total,
				    btbbx_clock_result *d_results, uint32_t *d_candidates, uint32_t cand_cap,
				    void *d_scratch, size_t scratch_bytes, void *hip_stream);
/* Host wrapper: copy in, the call above with scratch of its own, copy out.  candidates (n_jobs * cand_cap words, may be
 * NULL) keeps the caller's values in the slots no job writes.  Returns n_jobs or a negative BTBBX_E_*.  Safe to call from
 * several host threads at once. */
int64_t btbbx_hop_reversal_batch_host(const btbbx_clock_job *jobs, uint32_t n_jobs,
				      const int32_t *index_offsets, const uint8_t *channels, uint32_t n_obs_total,
				      btbbx_clock_result *results, uint32_t *candidates, uint32_t cand_cap);

/* ---- clock acquisition from a capture: survey records -> jobs of the batch reversal ------------- */
/* Builds, on the device, the job table and the two observation arrays btbbx_hop_reversal_batch_device takes from the
 * records of a survey and the survey's own scratch, so that scan -> survey -> this call -> batch reversal is one chain on one
 * stream with no synchronisation between the calls.
 * Record g (g < min(*d_rec_count, rec_cap); d_rec_count == NULL: rec_cap records) gets a job iff it is settled (settled_by != 0),
 * in record order, that is ascending LAP.  Its observations: with W = the header-bearing packets of the LAP in ascending (offset,
 * stream), the survey's walk stopped at W[n_walked - 1] with packets_observed packets remembered since the last reset, so the
 * run btbb_init_hop_reversal + btbb_winnow see when the piconet settles (bluetooth_piconet.c:528-531) is W[n_walked -
 * packets_observed .. n_walked), and every later packet of W is what try_hop appends (:510-515): the job gets W[n_walked -
 * packets_observed .. end), cut to its first max_obs.  Observation: index_offset = (int32_t)(clock - first_pkt_time) (:511, :664),
 * channel = channels[stream] (the stream index when channels is NULL).  Job: clk6 = (clk_offset + first_pkt_time) & 0x3f (:489);
 * cfg as btbbx_hop_cfg_init(&cfg, (uap << 24 | lap) & 0xfffffff, NULL) leaves it -- with BTBBX_JOBS_AFH as
 * btbbx_hop_cfg_init(&cfg, address, rec.afh_map) leaves it: AFH over the channels the survey saw; aliased = 1 with
 * BTBBX_JOBS_ALIASED; obs_first = the exclusive prefix of n_obs over the jobs, so the ranges are disjoint and in job order.
 *
 * d_survey_scratch: the scratch of the btbbx_survey_hits_device call that wrote d_recs -- the same cap, not modified since,
 * this call ordered after that one.  It is READ, never written: several calls (other flags, other max_obs) may follow one
 * survey.  channels (a HOST pointer, may be NULL) and n_streams as given to the survey.
 * *d_n_jobs counts ALL settled records; when it exceeds job_cap the first job_cap jobs in record order are stored with their
 * observations and nothing behind them is written.  d_job_rec (may be NULL): the record index of every stored job.
 * d_obs_hits (may be NULL): per observation, the index into the survey's d_hits.  *d_n_obs (may be NULL): observations
 * written.  A packet belongs to one LAP, so obs_cap >= cap entries always suffice.  Two kernels, asynchronous on hip_stream,
 * nothing is read back; the output with d_n_jobs as its count is a valid input of btbbx_hop_reversal_batch_device
 * (n_obs_total = obs_cap).
 * BTBBX_E_ARG before any launch for: d_recs, d_jobs, d_n_jobs, the scratch or one of the two observation arrays NULL,
 * survey_scratch_bytes < btbbx_survey_scratch_bytes(cap), obs_cap < cap, max_obs 0 or above 1024 (the batch reversal's limit),
 * job_cap == 0, unknown flag bits, a channel above 78, more than 79 streams without a table (256 with one), a pointer that
 * is not 4-byte aligned (the scratch: 16; the channels: any). */
#define BTBBX_JOBS_AFH     1u
#define BTBBX_JOBS_ALIASED 2u
int btbbx_survey_clock_jobs_device(const btbbx_survey_rec *d_recs, const uint32_t *d_rec_count, uint32_t rec_cap,
				   const void *d_survey_scratch, size_t survey_scratch_bytes, uint32_t cap,
				   const uint8_t *channels, uint32_t n_streams, uint32_t flags, uint32_t max_obs,
				   btbbx_clock_job *d_jobs, uint32_t job_cap, uint32_t *d_n_jobs, uint32_t *d_job_rec,
				   int32_t *d_index_offsets, uint8_t *d_channels, uint32_t *d_obs_hits,
				   uint32_t obs_cap, uint32_t *d_n_obs, void *hip_stream);
/* Host wrapper: "capture in, (LAP, UAP, CLK1-27) of every piconet out".  Copy in, scan (ordered, repeated with room when the
 * first buffer was too small, as btbbx_survey_host does), survey, job builder and batch reversal on one stream, copy out.
 * The first thirteen arguments and the return value are those of btbbx_survey_host (clk6_candidates = its candidates).
 * job_rec[j] = the record of job j, results[j] its btbbx_clock_result, jobs (may be NULL) the job table itself; *n_jobs counts
 * all settled piconets among the stored records, min(*n_jobs, job_cap) jobs are written.  candidates (job_cap * cand_cap
 * words, may be NULL) as in btbbx_hop_reversal_batch_host.  The batch reversal's scratch is about 8 KiB per job, so the wrapper
 * reads the number of jobs back before it -- in the same transfer and wait in which btbbx_survey_host reads the number of
 * piconets; that is the only point between the scan and the results where the host waits.  The device entries stay fully
 * asynchronous.  Safe to call from several host threads at once.
 * A result with count == 1 gives CLK1-27 of the run's first packet: cand0.  The reference's CLKN offset (what
 * btbb_piconet_get_clk_offset reports once BTBB_CLK27_VALID is set, bluetooth_piconet.c:598) follows as
 *     (cand0 << 1) - (first_pkt_time << 1)
 * with first_pkt_time of the job's record. */
int64_t btbbx_acquire_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			   uint64_t search_bits, int max_ac_errors, const uint8_t *channels,
			   uint32_t clkn0, uint32_t clk_div, uint32_t clk_phase,
			   btbbx_survey_rec *recs, uint64_t rec_cap, int16_t *clk6_candidates,
			   uint32_t flags, uint32_t max_obs,
			   btbbx_clock_job *jobs, uint32_t *job_rec, btbbx_clock_result *results, uint64_t job_cap,
			   uint64_t *n_jobs, uint32_t *candidates, uint32_t cand_cap);

/* ---- following: every packet of every acquired piconet with its own UAP and clock ------------------- */
/* The last stage of btbb_process_packet (bluetooth_piconet.c:851-899: LAP -> UAP/CLK1-6 -> CLK1-27 -> FOLLOWING), for a whole
 * hit list behind the acquisition chain: every packet of a piconet gets the piconet's UAP and the piconet-aligned clock
 * (:872-881), is decoded with them, and is checked against the channel the piconet's hop selection gives for that clock --
 * which tells a real packet from a stray access code and shows lost sync. */
typedef struct btbbx_follow_pkt {   /* 16 bytes, one per hit */
	uint32_t piconet;     /* index into d_recs of the hit's LAP, UINT32_MAX when no stored record has it */
	uint32_t clkn;        /* the clock the packet was decoded with (see the stages below) */
	uint8_t  stage;       /* 0 LAP only, 1 UAP + CLK1-6, 2 UAP + CLK1-27 */
	uint8_t  channel;     /* channels[hit.stream] (the stream index without a table) */
	uint8_t  hop_channel; /* stage 2: the channel the job's hop selection gives for clkn, in aliased form when job.aliased; else 0xff */
	uint8_t  on_hop;      /* stage 2 and hop_channel == channel */
	uint32_t job;         /* index into d_jobs / d_results, UINT32_MAX when the record has no stored job */
} btbbx_follow_pkt;

typedef struct btbbx_follow_sum {   /* 32 bytes, one per survey record */
	uint32_t stage, job;              /* as in the packets of this record */
	uint32_t n_hits;                  /* hits of the list with this LAP */
	uint32_t n_header;                /* ... whose header_rv != 0 */
	uint32_t n_payload;               /* ... whose payload_rv > 0 */
	uint32_t n_on_hop, n_off_hop;     /* stage 2 only: on_hop / not on_hop */
	uint32_t lt_addr_mask;            /* bit a: some hit with header_rv != 0 had LT_ADDR a */
} btbbx_follow_sum;

/* Follows the first N = min(*d_count, cap) hits of d_hits through the R = min(*d_rec_count, rec_cap) records of a survey and
 * the J = min(*d_n_jobs, job_cap) jobs and results of btbbx_survey_clock_jobs_device + btbbx_hop_reversal_batch_device; a NULL
 * count pointer means its cap.  All pointers are DEVICE pointers except channels and entry (HOST pointers, as in the survey).
 * For hit i < N:
 *   c = entry->clkn + (offset + clk_phase) / clk_div in uint32_t arithmetic, the stored clock of btbbx_survey_hits_device;
 *   g = the record with lap == hit.lap among d_recs[0 .. R) (the records are in ASCENDING LAP order: they are searched);
 *       none: piconet = UINT32_MAX and the hit is stage 0;
 *   j = the job with d_job_rec[j] == g, j < J (jobs are in record order: d_job_rec ascends); none: job = UINT32_MAX.
 *   stage 2 iff j exists and d_results[j].status == 0 && d_results[j].count == 1:
 *       clkn = (cand0 + c - recs[g].first_pkt_time) & 0x7ffffff -- the receiver's clock plus the reference's CLKN offset
 *       (cand0 << 1) - (first_pkt_time << 1) (:598), halved; a hit before the run's first packet gets a smaller clock through
 *       the wrap (2^32 is a multiple of 2^27); uap = recs[g].uap; flags = entry->flags | UAP_VALID | CLK6_VALID | CLK27_VALID;
 *   stage 1 iff not stage 2 and recs[g].settled_by != 0:
 *       clkn = (recs[g].clk_offset + c) & 0x3f (:489); uap = recs[g].uap; flags = entry->flags | UAP_VALID | CLK6_VALID;
 *   stage 0 otherwise: clkn = c, uap and flags those of *entry -- the hit comes out exactly as
 *       btbbx_decode_hits_piconet_phase_device leaves it.
 *   d_in[i] = {length 0, clkn, flags, uap, entry->type, entry->llid, entry->flow}; d_out[i] and d_lengths[i] (d_lengths may be
 *   NULL) are what btbbx_decode_hits_counted_device writes for d_in[i] with the same max_length: the decoder is that call's.
 *   channel = channels[hit.stream], the stream index when channels is NULL (0xff for a stream >= n_streams: the list must come
 *   from a scan of the same geometry).  hop_channel, stage 2 only, comes from the job's own cfg -- the bank modulo used_channels
 *   when cfg.afh -- by the device code the reversal's agreement walk uses, so follow and reversal cannot disagree; when
 *   job.aliased it is ((ch + 24) % 25) + 26.  (0xff, never on hop, for a cfg the batch reversal rejects.)
 * Every d_sums[g], g < R, is written whole: a record none of whose hits are in the list gets its stage, its job and zeros.
 * Records and sums behind R are not written; d_in, d_follow, d_out and d_lengths behind N are not written.
 * job_cap == 0 means no jobs (stages 0 and 1 only); d_jobs, d_job_rec and d_results may be NULL then.
 * Asynchronous on hip_stream: nothing is synchronised, nothing is read back and no scratch is needed -- d_in is the only
 * intermediate and belongs to the caller.  Three launches besides the decoder's.
 * BTBBX_E_ARG before any launch for: d_words, d_hits, d_recs, d_in, d_follow, d_out, d_sums or entry NULL; d_jobs, d_job_rec or
 * d_results NULL while job_cap != 0; clk_div == 0 or clk_phase >= clk_div; cap == 0 or rec_cap == 0; a channel above 78, no or
 * more than 79 streams without a table, more than 256 with one; a pointer that is not 4-byte aligned (8 bytes where the
 * records hold 64-bit fields: d_words, d_hits, d_out). */
int btbbx_follow_hits_device(const uint64_t *d_words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			     const btbbx_hit *d_hits, const uint32_t *d_count, uint32_t cap,
			     const btbbx_survey_rec *d_recs, const uint32_t *d_rec_count, uint32_t rec_cap,
			     const btbbx_clock_job *d_jobs, const uint32_t *d_job_rec, const btbbx_clock_result *d_results,
			     const uint32_t *d_n_jobs, uint32_t job_cap,
			     const uint8_t *channels, const btbbx_pkt_in *entry, uint32_t clk_div, uint32_t clk_phase, uint32_t max_length,
			     btbbx_pkt_in *d_in, btbbx_follow_pkt *d_follow, btbbx_pkt_out *d_out, uint32_t *d_lengths,
			     btbbx_follow_sum *d_sums, void *hip_stream);
/* Host wrapper: btbbx_acquire_host with the follow stage appended on the same stream, over the same ordered hit list, the same
 * entry state (whitened, nothing else known) and max_length = BTBBX_MAX_SYMBOLS.  The return value and recs / job_rec /
 * results / n_jobs are as in btbbx_acquire_host (every stored record's job is worked, min(*n_jobs, job_cap) of them are
 * copied out).  *n_hits counts all hits; the first hit_cap of them in (stream, offset) order are copied to hits / follow /
 * pkts, while the survey and sums (one per stored record) always cover all hits.  pkts, job_rec and results may be NULL: then
 * they are not copied.  rec_cap == 0, or recs, hits (with hit_cap != 0), follow (with hit_cap != 0), sums, n_jobs or n_hits
 * NULL: BTBBX_E_ARG.  The only host wait between copy-in and copy-out is the one btbbx_acquire_host already has, where it
 * reads the counts to size scratch.  Safe to call from several host threads at once. */
int64_t btbbx_follow_host(const uint64_t *words, uint64_t n_words, uint64_t pitch_words, uint32_t n_streams,
			  uint64_t search_bits, int max_ac_errors, const uint8_t *channels,
			  uint32_t clkn0, uint32_t clk_div, uint32_t clk_phase,
			  btbbx_survey_rec *recs, uint64_t rec_cap, uint32_t flags, uint32_t max_obs,
			  uint32_t *job_rec, btbbx_clock_result *results, uint64_t job_cap, uint64_t *n_jobs,
			  btbbx_hit *hits, btbbx_follow_pkt *follow, btbbx_pkt_out *pkts, uint64_t hit_cap, uint64_t *n_hits,
			  btbbx_follow_sum *sums);

/* piconet introspection for tests and tools: what the reference keeps in struct btbb_piconet
 * (bluetooth_piconet.h:59-85).  field: 0 num_candidates, 1 winnowed, 2 packets_observed,
 * 3 total_packets_observed, 4 first_pkt_time, 5 flags, 6 used_channels */
int64_t btbbx_piconet_state(const void *piconet, int field);
int64_t btbbx_piconet_candidates(const void *piconet, uint32_t *dst, uint64_t cap);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* INCLUDED_BTBBX_H */
